"""The references, the two rules and the tables of tests/helpers/dense_product_cases.py pinned before
tests/test_gpu_dense_product_edges.py leans on them.  No GPU.

  * the reference: on `integers` numpy's own complex128 / fp64 product and a plain numpy emulation of the three-product scheme equal the
    int64 reference bit for bit; on `rough` and `graded` both stay inside the derived per-element bound at EVERY case of the tables
    (worst over all of them: 0.097 of the bound for numpy's complex product, 0.172 for the three-product emulation, 0.167 for the real
    product) -- the reference alone never needs the bar moved;
  * the checker: each of a list of defects a kernel of this kind can have -- a k-step dropped, a pad row or pad column of B let in, half
    a tile's rows zero, rows swapped, the tiles of two super-tiles exchanged, a neighbour's offset, the scales of the real and the imaginary
    column exchanged, a double of C's pitch gap overwritten -- applied to a correct result makes check() raise, on every kind of input
    and every form;
  * the tables: every edge the kernels switch at occurs in the sweeps, the cases of the tile map have the super-tile counts they are
    there for, and the block -> tile map of the kernels, replayed in numpy, gives every tile of every tabled shape exactly one block."""
import numpy as np
import pytest

from tests.helpers import dense_product_cases as dp

LD_EPS = float(np.finfo(np.longdouble).eps)
pytestmark = pytest.mark.skipif(LD_EPS > 2e-19, reason="np.longdouble carries no more than fp64 on this platform")

ALL_SWEEPS = [c for form in (dp.COMPLEX, dp.COMPLEX_4M, dp.REAL) for c in dp.sweep_cases(form)]


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("case", ALL_SWEEPS, ids=dp.case_id)
def test_integers_have_one_fp64_result(case):
    """numpy's product (BLAS: its own blocking and summation order, fused or not) and the three-product emulation land on the int64
    reference bit for bit: the equal-bits rule asks nothing of a kernel that a correct fp64 product in any order does not give"""
    o = dp.build(case.form, case.M, case.N, case.K, "integers", case.pitch, case.epilogue, case.seed)
    E = dp.exact(o)
    assert E.dtype == np.float64 and E.shape == (o.M, o.per * o.N)
    for three in (False, True):
        got = dp.fp64_result(o, three=three)
        assert np.array_equal(got.view(np.uint64), E.view(np.uint64)), three
    assert dp.check(o, o.place(dp.fp64_result(o, three=True))) == 0.0


@pytest.mark.parametrize("kind", ["rough", "graded"])
@pytest.mark.parametrize("case", ALL_SWEEPS, ids=dp.case_id)
def test_fp64_products_stay_inside_the_derived_bound(case, kind):
    o = dp.build(case.form, case.M, case.N, case.K, kind, case.pitch, case.epilogue, case.seed)
    assert dp.exact(o).dtype == np.longdouble and dp.bound(o).shape == (o.M, o.per * o.N) and (dp.bound(o) > 0).all()
    worst = max(dp.check(o, o.place(dp.fp64_result(o, three=three)), f"numpy three={three} " + o.label()) for three in (False, True))
    assert worst <= 0.5, worst  # (the bound has room: a reference at its edge could not tell a kernel's error from its own)


def test_the_bound_is_far_below_a_dropped_term():
    """a single missing k-step or a neighbour's column is of the size of S: many orders above the bar, on the graded columns too"""
    for kind in ("rough", "graded"):
        o = dp.build(dp.COMPLEX, 70, 70, 9, kind, "tight", "none", 1)
        good = dp.fp64_result(o)
        dropped = dp.fp64_result(o, A=o.A[:, :-1], B=o.B[:-1])
        ratio = np.abs(good - dropped) / dp.bound(o)
        assert np.median(ratio) > 1e12, np.median(ratio)


# ------------------------------------------------------------------------------------------------ the checker
def _swap_pairs(v):
    w = v.copy()
    w[0::2], w[1::2] = v[1::2], v[0::2]
    return w


def _tiles_exchanged(o, D):
    """the first row tile's leading columns and those of the first tile of the NEXT super-tile (two panels on) change places"""
    _, bm, bn, _ = dp.shape_of(o.form)
    start = 2 * bn
    w = min(bn, o.N - start)
    assert w > 0 and dp.tiling(o.form, o.M, o.N).super_cols >= 2
    D = D.copy()
    a, b = slice(0, o.per * w), slice(o.per * start, o.per * (start + w))
    rows = slice(0, min(bm, o.M))
    D[rows, a], D[rows, b] = D[rows, b].copy(), D[rows, a].copy()
    return D


def _rows_zero(o):
    A = o.A.copy()
    A[32:64] = 0
    return dp.fp64_result(o, A=A)


def _pad_row_in(o):
    return dp.fp64_result(o, A=np.hstack([o.A, np.ones((o.M, 1), dtype=o.A.dtype)]), B=o.B_pad[: o.K + 1, : o.N])


def _pad_column_in(o):
    B = o.B.copy()
    B[:, o.N - 1] = o.B_pad[: o.K, o.N]
    return dp.fp64_result(o, B=B)


def _rows_swapped(o):
    D = dp.fp64_result(o)
    D[[5, 38]] = D[[38, 5]]
    return D


def _gap_overwritten(o):
    c = o.place(dp.fp64_result(o))
    c[o.c_at + 3 * o.ldc + o.per * o.N + 1] = 0.0
    return c


DEFECTS = {
    "the last k-step dropped": lambda o: dp.fp64_result(o, A=o.A[:, :-1], B=o.B[:-1]),
    "one pad row of B let in (k = K taken with A = 1)": _pad_row_in,
    "column N - 1 taken from column N of the padded B": _pad_column_in,
    "rows 32 .. 63 of a tile zero": _rows_zero,
    "two rows swapped": _rows_swapped,
    "the tiles of one super-tile exchanged with the next": lambda o: _tiles_exchanged(o, dp.fp64_result(o)),
    "col_off of column j + 1 used for column j": lambda o: dp.fp64_result(o, off=np.concatenate([o.off[o.per:], o.off[-o.per:]])),
    "real and imaginary scale exchanged": lambda o: dp.fp64_result(o, scale=_swap_pairs(o.scale)),
    "one double of the pitch gap of C overwritten": _gap_overwritten,
}
# a shape per form at which every defect can occur: a K tail (pad rows), a ragged last panel (pad columns), more than one row
# tile, two super-tile columns, wide pitches and both epilogue arrays.  (For the real form "real and imaginary scale" are the scales of
# two neighbouring columns.)
DEFECT_SHAPES = {dp.COMPLEX: (70, 197, 9), dp.COMPLEX_4M: (70, 197, 9), dp.REAL: (140, 300, 18)}


@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("form", list(DEFECT_SHAPES), ids=lambda f: dp.FORM_NAMES[f])
def test_a_correct_result_passes_and_every_seeded_defect_is_caught(form, kind):
    M, N, K = DEFECT_SHAPES[form]
    o = dp.build(form, M, N, K, kind, "wide", "both", 77)
    assert o.k_pad > K and o.n_pad > N and o.ldc > o.per * N
    for three in (False, True):
        dp.check(o, o.place(dp.fp64_result(o, three=three)))
    for name, make in DEFECTS.items():
        bad = make(o)
        bad = bad if bad.ndim == 1 else o.place(bad)
        with pytest.raises(AssertionError):
            dp.check(o, bad, name)


def test_the_checker_sees_guards_nans_and_single_bits():
    o = dp.build(dp.COMPLEX, 17, 33, 5, "integers", "wide", "scale", 3)
    good = o.place(dp.fp64_result(o))
    dp.check(o, good)
    for at, value in ((0, 0.0), (o.c_at - 1, 0.0), (good.size - 1, -dp.SENTINEL), (o.c_at + o.ldc - 1, np.nan)):
        bad = good.copy()
        bad[at] = value
        with pytest.raises(AssertionError, match="outside the results"):
            dp.check(o, bad)
    bad = good.copy()
    bad[o.c_at + 2 * o.ldc + 7] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        dp.check(o, bad)
    bad = good.copy()
    bad[o.c_at + 2 * o.ldc + 7] = np.nextafter(bad[o.c_at + 2 * o.ldc + 7], np.inf)
    with pytest.raises(AssertionError, match="integer reference"):
        dp.check(o, bad)
    # a result left at the sentinel (a tile nobody computed) is a wrong value, not a pass
    bad = good.copy()
    bad[o.c_at + 16 * o.ldc : o.c_at + 16 * o.ldc + 2 * o.N] = dp.SENTINEL
    with pytest.raises(AssertionError):
        dp.check(o, bad)


def test_operands_are_laid_out_as_the_contract_says():
    for form, (M, N, K) in ((dp.COMPLEX, (5, 7, 3)), (dp.REAL, (5, 7, 4))):
        per, _, panel, turn = dp.shape_of(form)
        for pitch in dp.PITCHES:
            o = dp.build(form, M, N, K, "rough", pitch, "both", 0)
            a = o.a_buf[o.a_at : o.a_at + (M - 1) * o.lda + per * K]
            rows = np.stack([o.a_buf[o.a_at + i * o.lda : o.a_at + i * o.lda + per * K] for i in range(M)])
            assert np.array_equal(rows, dp._doubles(o.A, o.real)) and np.isnan(o.a_buf).sum() == o.a_buf.size - M * K * per
            assert np.isnan(a).sum() == (M - 1) * (o.lda - per * K) and o.a_at % 2 == 0 and o.lda % 2 == 0
            assert (o.k_pad, o.n_pad, o.ldb) == (turn, panel, per * panel)
            block = o.b_buf[o.b_at : o.b_at + o.k_pad * o.ldb].reshape(o.k_pad, o.ldb)
            assert np.isfinite(block).all() and np.isnan(o.b_buf[: o.b_at]).all() and np.isnan(o.b_buf[o.b_at + block.size :]).all()
            pad = np.ones(block.shape, dtype=bool)
            pad[:K, : per * N] = False
            assert (np.abs(block[pad]) >= 1e3).all() and (np.abs(block[pad]) <= 1e4).all()
            assert (o.c_buf == dp.SENTINEL).all() and o.c_buf.size == 4 * dp.GUARD + M * o.ldc
            assert o.off.size == o.scale.size == per * N and np.isnan(o.off_buf[o.off_at + per * N])


# ------------------------------------------------------------------------------------------------ the tables
def test_every_edge_occurs_in_the_sweeps():
    for form, edges in dp.EDGES.items():
        (m0, n0, k0), Ms, Ns, Ks, _ = dp.SWEEPS[form]
        for axis, values in (("M", Ms), ("N", Ns), ("K", Ks)):
            for e in edges[axis]:
                ends_on = e in values
                crosses = (e + 1 in values) if not (form == dp.REAL and axis == "K") else (e + 2 in values)  # (the real form takes even K only)
                assert ends_on and crosses, (dp.FORM_NAMES[form], axis, e)
    Ks = dp.SWEEPS[dp.COMPLEX][3]
    assert {k % 8 for k in Ks} == set(range(8))  # full turns and every tail of 1 .. 7 k-steps
    assert 1 in Ks and {k for k in Ks if 8 < k <= 16} and {k for k in Ks if 16 < k <= 24} and {k for k in Ks if k > 24}  # 1 .. 4+ turns: both LDS buffers
    assert {k % 16 for k in dp.SWEEPS[dp.REAL][3]} >= {0, 2, 14} and all(k % 2 == 0 for k in dp.SWEEPS[dp.REAL][3])
    assert 33 in dp.SWEEPS[dp.COMPLEX][2] and 32 in dp.SWEEPS[dp.COMPLEX][2]  # wave_has_columns changes between them
    assert dp.tiling(dp.COMPLEX, 70, 197).nbn == 4 and 197 - 3 * 64 == 5  # three panels and one of 5
    for form in dp.SWEEPS:
        cases = dp.sweep_cases(form)
        assert {(c.pitch, c.epilogue) for c in cases} == {(p, e) for p in dp.PITCHES for e in dp.EPILOGUES}
        assert all(c.K <= 1024 for c in cases)


def test_the_map_cases_have_the_super_tiles_they_are_there_for():
    seen = set()
    for (form, M, N, K), (r, rows, cols) in dp.MAP_CASES.items():
        t = dp.tiling(form, M, N)
        assert (t.st_rows_log2, t.super_rows, t.super_cols) == (r, rows, cols) and t.n_super == rows * cols, (form, M, N, t)
        owners, q_hi = dp.tile_owners(form, M, N)
        assert q_hi == -(-t.n_super // 8) - 1 and (q_hi >= 1) == (t.n_super > 8)  # q >> 6 counts the octets of super-tiles
        seen.add((form, r, t.n_super > 8))
        print(f"MAP {dp.FORM_NAMES[form]} {M} x {N} x {K}: {t}")
    assert seen >= {(dp.COMPLEX, 5, False), (dp.COMPLEX, 5, True), (dp.COMPLEX, 6, True), (dp.REAL, 5, False), (dp.REAL, 5, True)}
    assert all(dp.tiling(c.form, c.M, c.N).n_super <= 2 for c in ALL_SWEEPS)  # (the sweeps stay inside one or two super-tiles)


@pytest.mark.parametrize("shape", [(c.form, c.M, c.N) for c in ALL_SWEEPS] + [k[:3] for k in dp.MAP_CASES] +
                         [(dp.COMPLEX, 64 * 40, 64 * 3), (dp.COMPLEX, 64 * 600, 64 * 3 + 1), (dp.REAL, 128 * 70, 128 * 7)],
                         ids=lambda s: f"{dp.FORM_NAMES[s[0]]}-{s[1]}x{s[2]}")
def test_the_block_map_gives_every_tile_exactly_one_block(shape):
    """`S / nsn`, `S % nsn` with nbn no multiple of the super-tile's columns, super-tiles that hang over either edge, the second
    octet of super-tiles: the kernels' arithmetic, replayed for every block of the launcher's grid"""
    form, M, N = shape
    t = dp.tiling(form, M, N)
    owners, _ = dp.tile_owners(form, M, N)
    assert set(owners) == {(i, j) for i in range(t.nbm) for j in range(t.nbn)}
    assert all(len(v) == 1 for v in owners.values())
