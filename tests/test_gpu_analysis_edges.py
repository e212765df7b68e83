"""GPU parity of the analysis kernels (grid -> modes: scri_amd/csrc/kernels_analysis.hip and the dense quadrature product) at every
template instance and edge of their launchers, against the quadrature of oracle/spinsfast_ref.py carried in extended precision
(tests/helpers/analysis_cases.py exact_map2salm, pinned by tests/test_oracle_analysis_exact.py).  The counterpart of
tests/test_gpu_synthesis_edges.py.

One rule serves group A: with E_got = max|got - exact|, E_ref = max|fp64 oracle - exact| and scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured,
with F and G per family in analysis_cases.RULE.  Three kinds of rows: white noise (exact: exact_map2salm); one-hot pixel rows (row r = a
single 1 at pixel r: the result is the analysis matrix entry by entry -- a single wrong pixel weight, which white noise dilutes by
1 / sqrt(n_pix), stands alone; exact: exact_matrix, no sum); band-limited rows (exact syntheses of random modes on a grid that
resolves them: the modes come back, no analysis reference needed).  Every call also asserts that the result is finite, that the
route was the one the launchers' arithmetic names (the timing tags of the context) and that a repeated call gives the same bits.
The comparison is against the oracle and its own fp64 distance, never against another route of the library.

Group A -- engine.map2salm (bms_map2salm), default route and each of SCRI_AMD_NO_SPLIT_ANALYSIS, SCRI_AMD_NO_LARGE_ANALYSIS,
SCRI_AMD_NO_FUSED_ANALYSIS; analysis_cases.route_of restates build_analysis / run_analysis / launch_analysis_fused and names the family.
  A_SMALL_*      analysis_split_kernel, and analysis_fused_kernel with the split switched off: n_theta = 3 .. 40 at the edges of NT and
                 of the front waves, n_phi = 2 .. 41 (KS 3 | 5, both parities, 40 and 41 the first the split refuses), n_out = 64, 81, 289,
                 253 .. 285 (back waves, second modes), 1, 2, 3 rows, 1600 and 1601 rows (stride loop, overlapping last pair), 600 rows
  A_FUSED_*      n_phi = 46, 47 (KS = 6) and every reachable (NT, KS, EPT) of the one-role kernel
  A_WIDE         analysis_fused_wide_kernel: l = 17 .. 32, n_out = 320 (n_sec = 64), 323 .. 504 (384, 448, 512 threads), few modes at l = 32
  A_LARGE_*      phi_dft_folded_kernel + theta_quadrature_mfma_kernel: n_theta = 3 .. 104 with n_phi = 48 (so also n_theta <= 40: mt = 1,
                 kq = 1, an almost empty ring tile), n_out = 513 on small grids, every KS edge, NTC 1 | 2, NTQ 1 | 2 | 3, 255 .. 513 rows,
                 4100 rows (the phi stage's grid stride), 104 x 127 / l <= 32, 99 x 99 / l <= 24, s = -4 .. 4
  A_OLD          theta_quadrature_kernel<24 | 40 | 72 | 104> and its natural shapes (n_phi = 128, l = 33, 2100 rows)
  A_DENSE        n_theta = 105
  A_ONE_HOT, A_BAND   one shape per family each
Group B -- WaveformModes.transform with a small boost: the dense route hands the analysis gathered, sorted columns with the two pole
rings stored once (col_of_pixel); the split kernel gives the poles a closed form, the fused kernel the phase e^{-+i s phi_k}.  Every
data type of the container (s = 2, 1, 0, -1, -2, -2, 2, -2) on five grids, default route and SCRI_AMD_NO_SPLIT_ANALYSIS, against
oracle/waveform_grid_ref.py transform at the bar of tests/test_gpu_edge_cases.py _check, 1e-12 max(1, max|ref|).  On grids the fused
analysis does not take (41 x 41, 15 x 49) the call succeeds, matches, and the tags show the two-kernel analysis: no sorted columns.

Template instances (test_case_table_reaches_every_template_instance, no GPU: enumerated over every admissible shape).
  analysis_split_kernel<24 | 38 | 40, 3 | 5>: all six reachable, all in the table.
  phi_dft_folded_kernel<7 | 10 | 13 | 16, 1 | 2>, theta_quadrature_mfma_kernel<11 | 18 | 26, 1 | 2 | 3>, theta_quadrature_kernel<24 | 40 | 72 |
  104>: all reachable, all in the table.
  analysis_fused_kernel / analysis_fused_wide_kernel<NT, KS, EPT>: of the 2 x 18 instances the launcher can name, 15 are UNREACHABLE by
  its own arithmetic (EPT = ceil(n_theta nk / threads) with threads >= 256, nk = n_phi / 2 + 1 <= 4 KS):
    <24, 3, 3 | 4>, both kernels   n_theta nk <= 24 x 12 = 288 <= 2 x 256
    <24, 5, 3 | 4>, both           24 x 20 = 480 <= 2 x 256
    <24, 6, 4>, both               24 x 24 = 576 <= 3 x 256
    <40, 3, 3 | 4>, both           40 x 12 = 480 <= 2 x 256
    <40, 6, 2>, one-role only      l <= 16 means n_out <= 289, so 256 threads; KS = 6 with NT = 40 means n_theta >= 25 and nk >= 21: 525 items,
                                   EPT >= 3.  (The wide kernel reaches it with 384 or more threads.)
  They are compiled and never launched.  No admissible shape is left without an instance (EPT never exceeds F_EPT_MAX = 4).

MEASURED on an MI355X: the worst ratios of every family and their shapes stand next to analysis_cases.RULE.  No case needed a change of
a kernel; no family comes near the caps.
"""
import functools

import numpy as np
import pytest

from oracle import containers
from oracle import waveform_grid_ref as grid_ref
from tests.helpers import analysis_cases as an

gpu = pytest.mark.gpu

ROUTE_OPTIONS = {"NO_SPLIT": "SCRI_AMD_NO_SPLIT_ANALYSIS", "NO_LARGE": "SCRI_AMD_NO_LARGE_ANALYSIS", "NO_FUSED": "SCRI_AMD_NO_FUSED_ANALYSIS"}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _base(family):
    return family[: -len("_1hot")] if family.endswith("_1hot") else family


# ------------------------------------------------------------------------------------------------------------- the case table
def _pairs(pred):
    """every (ell_max, ell_min) with 0 <= ell_min <= ell_max <= 33 that satisfies pred(L, n_out)"""
    return [(L, lo) for L in range(1, 34) for lo in range(L + 1) if pred(L, an.n_out_of(L, lo))]


@functools.lru_cache(maxsize=None)
def _reachable_fused_and_split():
    fused, split, without = set(), set(), []
    shapes = sorted({(L > 16, L <= 16, an.n_out_of(L, lo)) for L, lo in _pairs(lambda L, n_out: L <= 32 and n_out <= 512)})
    for n_theta in range(2, 41):
        for n_phi in range(2, 48):
            for wide, small_l, n_out in shapes:
                L = 17 if wide else 16
                assert an.fused_takes(n_theta, n_phi, L, n_out)
                inst = an.fused_instance(n_theta, n_phi, L, n_out)
                if inst is None:
                    without.append((n_theta, n_phi, L, n_out))
                else:
                    fused.add(inst[:4])
                if small_l and an.split_takes(n_theta, n_phi, L, n_out, 2):
                    split.add(an.split_instance(n_theta, n_phi, L, n_out)[:2])
    return fused, split, without


def _reachable_large():
    # (one (ell_max, ell_min) per (NTC, NTQ): the grid enters the instance only through KS and KQ)
    one_each = lambda pairs: list({an.large_instance(9, 48, L, lo)[1::2]: (L, lo) for L, lo in pairs}.values())  # noqa: E731
    every = one_each(_pairs(lambda L, n_out: L <= 32))
    beyond = one_each(_pairs(lambda L, n_out: L <= 32 and n_out > 512))  # what the fused kernel refuses on a grid it would take
    out = set()
    for n_theta in range(2, 105):
        for n_phi in range(1, 128):
            assert an.large_takes(n_theta, n_phi, 1)
            small = n_theta <= 40 and 2 <= n_phi and n_phi // 2 + 1 <= 24
            out |= {an.large_instance(n_theta, n_phi, L, lo) for L, lo in (beyond if small else every)}
    return out


def _table(base):
    return [c for c in an.A_CASES if _base(an.family_of(c)) == base]


UNREACHABLE_FUSED = ({(w, 24, 3, e) for w in (False, True) for e in (3, 4)} | {(w, 24, 5, e) for w in (False, True) for e in (3, 4)}
                     | {(w, 24, 6, 4) for w in (False, True)} | {(w, 40, 3, e) for w in (False, True) for e in (3, 4)} | {(False, 40, 6, 2)})


@pytest.mark.parametrize("launcher", ["fused", "split", "large", "tq_old"])
def test_case_table_reaches_every_template_instance(launcher):
    """no GPU: the launchers' arithmetic (analysis_cases.*_instance) over every admissible shape against the table of group A"""
    n_out = lambda c: an.n_out_of(c.L, c.ell_min)  # noqa: E731
    if launcher in ("fused", "split"):
        fused, split, without = _reachable_fused_and_split()
        assert not without  # no shape the fused kernel takes is left without an instance
        every = {(w, nt, ks, e) for w in (False, True) for nt in (24, 40) for ks in (3, 5, 6) for e in (2, 3, 4)}
        assert every - fused == UNREACHABLE_FUSED and len(UNREACHABLE_FUSED) == 15
        assert split == {(nt, ks) for nt in (24, 38, 40) for ks in (3, 5)}
        if launcher == "fused":
            have = {an.fused_instance(c.n_theta, c.n_phi, c.L, n_out(c))[:4] for c in _table("fused") + _table("fused_wide")}
            assert have == fused
            wide = [an.fused_instance(c.n_theta, c.n_phi, c.L, n_out(c)) for c in _table("fused_wide")]
            assert {i[4] for i in wide} == {256, 384, 448, 512} and 64 in {i[5] for i in wide}  # every workgroup size, the largest n_sec
            assert {n_out(c) for c in _table("fused_wide")} >= {320, 323, 384, 391, 484, 504, 128, 189}
            assert {an.fused_instance(c.n_theta, c.n_phi, c.L, n_out(c))[5] for c in _table("fused")} >= {0, 29, 33}
            assert any(c.rows == 1 for c in _table("fused") if c.env is None)  # one row: refused by the split kernel
            assert any(c.rows >= 600 for c in _table("fused"))  # more rows than 2 x CUs (256 CUs) workgroups
        else:
            have = [an.split_instance(c.n_theta, c.n_phi, c.L, n_out(c)) for c in _table("split")]
            assert {i[:2] for i in have} == split
            assert {i[2] for i in have} == {1, 2, 3, 4, 5} and {i[3] for i in have} == {1, 2, 3, 4, 5}  # front waves, back waves
            assert {2, 3, 1600, 1601} <= {c.rows for c in _table("split")}
            # the first shapes it refuses
            assert not an.split_takes(9, 40, 8, 77, 5) and an.split_takes(9, 39, 8, 77, 5) and not an.split_takes(9, 9, 4, 21, 1)
            assert all(_base(an.family_of(c)) == "fused" for c in an.A_SMALL_PHI if c.n_phi >= 40)
    elif launcher == "large":
        reachable = _reachable_large()
        assert {i[:2] for i in reachable} == {(ks, ntc) for ks in (7, 10, 13, 16) for ntc in (1, 2)}
        assert {i[2:] for i in reachable} == {(kq, ntq) for kq in (11, 18, 26) for ntq in (1, 2, 3)}
        have = {an.large_instance(c.n_theta, c.n_phi, c.L, c.ell_min) for c in _table("large")}
        assert {i[:2] for i in have} == {i[:2] for i in reachable} and {i[2:] for i in have} == {i[2:] for i in reachable}
        # the edges of each rule
        assert [an.large_instance(5, nph, 4, 0)[0] for nph in (48, 55, 56, 57, 79, 80, 81, 103, 104, 105, 126, 127)] == [7, 7, 10, 10, 10, 13, 13, 13, 16, 16, 16, 16]
        assert [an.large_instance(nt, 48, 4, 0)[2] for nt in (3, 44, 45, 72, 73, 104)] == [11, 11, 18, 18, 26, 26]
        assert [an.large_instance(9, 48, L, lo)[1::2] for L, lo in ((16, 0), (16, 1), (17, 0), (17, 2), (32, 0), (32, 1), (31, 0))] == [
            (1, 2), (1, 1), (2, 2), (2, 1), (2, 3), (2, 2), (2, 2)]
        small = [c for c in _table("large") if c.n_theta <= 40]
        assert {c.n_theta for c in small} >= {3, 8, 9, 40} and any(n_out(c) == 513 for c in small)
        assert {255, 256, 257, 513, 4100} <= {c.rows for c in _table("large")}
        assert any(c.rows * -(-c.n_theta // 8) > 4096 for c in _table("large"))  # the phi stage's grid-stride loop
        assert set(range(-4, 5)) <= {c.spin for c in _table("large")}
        assert an.large_takes(6, 127, 32) and not an.large_takes(6, 128, 6) and not an.large_takes(9, 10, 33) and not an.large_takes(105, 6, 6)
    else:
        assert {an.tq_old_instance(c.n_theta) for c in _table("tq_old")} == {24, 40, 72, 104}
        assert any(c.rows > 2048 for c in _table("tq_old"))  # beyond the cap of 2048 row blocks
        assert [an.family_of(c) for c in an.A_OLD] == ["tq_old"] * len(an.A_OLD) and [an.family_of(c) for c in an.A_DENSE] == ["dense"]
    # the table as a whole
    assert len({an.case_id(c) for c in an.A_CASES}) == len(an.A_CASES)
    families = {an.family_of(c) for c in an.A_CASES}
    assert families == set(an.RULE), families ^ set(an.RULE)
    assert {_base(an.family_of(c)) for c in an.A_BAND} == set(an.TAGS)
    assert all(c.n_theta * c.n_phi * 16 * min(c.rows, 600) <= 12e6 for c in an.A_CASES if c.kind != "one_hot")  # about 10 MB of grid, row tests aside


# ------------------------------------------------------------------------------------------------------------- group A
def _set_route(route, env):
    for key, name in ROUTE_OPTIONS.items():
        route(name, "1" if key == env else None)


def _analysis_tags(ctx):
    return {k for k, v in ctx.get_timing(reset=True).items() if v[1]} & an.ANALYSIS_TAGS


@gpu
@pytest.mark.parametrize("c", an.A_CASES, ids=an.case_id)
def test_a_map2salm(ctx, route, c):
    from scri_amd import engine

    f, exact, ref = an.case_inputs(c)
    family = an.family_of(c)
    _set_route(route, c.env)
    call = lambda: engine.map2salm(f, c.spin, c.L, ell_min=c.ell_min, ctx=ctx)  # noqa: E731
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        got = call()
        tags = _analysis_tags(ctx)
    finally:
        ctx.enable_timing(False)
    assert tags == an.TAGS[_base(family)], f"{an.case_id(c)}: expected the {family} route, the context timed {sorted(tags)}"
    an.check(family, got, exact, ref, f"A {an.case_id(c)} {f.shape[0]} rows")
    assert _same_bits(got, call()), f"{an.case_id(c)}: a repeated call gives other bits"


# ------------------------------------------------------------------------------------------------------------- group B
def _series(name, n, seed):
    """a short smooth series of every mode l = |s| .. B_ELL_MAX of one data type, uniform axis"""
    s = containers.SpinWeights[getattr(containers, name)]
    lm = np.array([[ell, m] for ell in range(abs(s), an.B_ELL_MAX + 1) for m in range(-ell, ell + 1)])
    rng = np.random.default_rng(seed)
    a = rng.normal(size=lm.shape[0]) + 1j * rng.normal(size=lm.shape[0])
    t = np.linspace(0.0, 10.0, n)
    return t, abs(s), a[None, :] * np.exp(1j * lm[None, :, 1] * (0.05 * t + 1e-3 * t**2)[:, None])


def _pair(ctx, name, seed):
    import scri_amd

    t, ell_min, data = _series(name, an.B_STEPS, seed)
    w_o = containers.WM(t=t, data=data, ell_min=ell_min, ell_max=an.B_ELL_MAX, dataType=getattr(containers, name))
    w_g = scri_amd.WaveformModes(t=t, data=data, ell_min=ell_min, ell_max=an.B_ELL_MAX, dataType=getattr(scri_amd, name), frameType=scri_amd.Inertial,
                                 r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    return w_o, w_g


def _boosted(ctx, name, n_theta, n_phi):
    """(oracle result, a call of the library's transform): a small boost; psi0 .. psi3 get their companions up to psi4"""
    w_o, w_g = _pair(ctx, name, seed=n_theta * 64 + n_phi)
    kw = dict(boost_velocity=np.array(an.B_BOOST), n_theta=n_theta, n_phi=n_phi, ell_max=an.B_ELL_MAX)
    aux_o, aux_g = {}, {}
    if name in ("psi0", "psi1", "psi2", "psi3"):
        for n in range(int(name[-1]) + 1, 5):
            aux_o[f"psi{n}_modes"], aux_g[f"psi{n}_modes"] = _pair(ctx, f"psi{n}", seed=1000 + n)
    return grid_ref.transform(w_o, **kw, **aux_o), lambda: w_g.transform(**kw, **aux_g)


def _check_b(got, ref, what):
    """the _check of tests/test_gpu_edge_cases.py"""
    assert got.t.shape == ref.t.shape and np.abs(got.t - ref.t).max() < 1e-12, what
    assert got.data.shape == ref.data.shape and np.isfinite(got.data).all(), what
    err, scale = float(np.abs(got.data - ref.data).max()), max(1.0, float(np.abs(ref.data).max()))
    print(f"B {what}: max|got - oracle| = {err:.3e} = {err / scale:.3e} scale")
    assert err < 1e-12 * scale, what


@gpu
@pytest.mark.parametrize("name", an.B_TYPES)
@pytest.mark.parametrize("n_theta,n_phi", an.B_GRIDS, ids=lambda v: str(v))
def test_b_boosted_transform_gathered_grid(ctx, route, n_theta, n_phi, name):
    ref, run = _boosted(ctx, name, n_theta, n_phi)
    assert an.fused_takes(n_theta, n_phi, an.B_ELL_MAX, an.n_out_of(an.B_ELL_MAX, 0))
    for env in (None, "NO_SPLIT"):
        _set_route(route, env)
        ctx.enable_timing(True)
        try:
            ctx.get_timing(reset=True)
            got = run()
            tags = _analysis_tags(ctx)
        finally:
            ctx.enable_timing(False)
        assert tags == {"analysis_fused"}, (env, sorted(tags))
        _check_b(got, ref, f"{name} {n_theta}x{n_phi} {env or 'default'}")
        assert _same_bits(got.data, run().data), (name, env)


@gpu
@pytest.mark.parametrize("name", an.B_TYPES)
@pytest.mark.parametrize("n_theta,n_phi", an.B_NOT_FUSED, ids=lambda v: str(v))
def test_b_boosted_transform_where_the_fused_analysis_declines(ctx, route, n_theta, n_phi, name):
    """run_analysis refuses gathered columns on every route but the fused one: a boosted transform on such a grid must not sort them"""
    ref, run = _boosted(ctx, name, n_theta, n_phi)
    assert not an.fused_takes(n_theta, n_phi, an.B_ELL_MAX, an.n_out_of(an.B_ELL_MAX, 0)) and an.large_takes(n_theta, n_phi, an.B_ELL_MAX)
    _set_route(route, None)
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        got = run()
        tags = _analysis_tags(ctx)
    finally:
        ctx.enable_timing(False)
    assert tags == {"analysis_large"}, sorted(tags)
    _check_b(got, ref, f"{name} {n_theta}x{n_phi} default")
