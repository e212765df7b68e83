"""The plain dense products -- zgemm3m_mfma_kernel<false> (three products), zgemm3m_mfma_kernel<true> (four) and dgemm_mfma_kernel of
scri_amd/csrc/kernels_gemm.hip -- through bms_dense_product on operands this module owns, at every edge of their tiles, held to the
references and the two rules of tests/helpers/dense_product_cases.py (pinned without a GPU by tests/test_oracle_dense_product_exact.py).

Every call runs between guards: A between NaNs with NaN pitch gaps, B padded with finite garbage that must not reach a result, C
prefilled with sentinels.  After ctx.synchronize():
  * `integers`: every result has EQUAL BITS with the int64 reference; `rough`, `graded`: the derived per-element bound holds;
  * every result is finite (nothing outside the operands was read), every other double of C is still the sentinel;
  * A and B are unchanged; the same call into a fresh C gives equal bits.
Sweeps are one-at-a-time around a base shape ((70, 70, 9); real form (140, 140, 18)), each value with all three kinds, both pitches
and the three epilogues dealt round-robin: rows and columns across the staging, wave and fragment edges (16, 32, 64, 96 / 16, 32,
64, 128; real form 16, 64, 96, 128 / 16, 64, 128), K from one turn with nothing to prefetch to seven turns with every tail of
1 .. 7 k-steps behind which B holds garbage.  The tile map runs on `integers` at 2 x 2 and 3 x 3 super-tiles (q >> 6 reaches 1)
and on the st_rows_log2 = 6 branch of launch_zgemm3m (513 row tiles).  The refusals of the contract are tried once each; a refused
call launches nothing and leaves C alone.

Measured on an MI355X over every call of this module (recorded, not used as a bar): worst |got - exact| / bound
    three-product form  0.172  (70 x 70 x 1, graded)     four-product form  0.0881  (70 x 70 x 1, graded)     real form  0.167  (140 x 140 x 4, rough)
-- the figures of numpy's fp64 product and of the numpy emulation of the three-product scheme on the same operands (0.172, 0.0881, 0.167:
at K = 1 .. 4 the roundings of the epilogue dominate and the two agree to the bit) -- and equal bits on all 107 `integers` calls.
No kernel needed a change."""
import numpy as np
import pytest

from tests.helpers import dense_product_cases as dp

pytestmark = pytest.mark.gpu

WORST = {}  # form -> (worst got/bound, label): printed by the last test of the module


def _device(host):
    import torch

    return None if host is None else torch.from_numpy(np.array(host)).to(torch.device("cuda", 0))


def _addr(t, at):
    return None if t is None else t.data_ptr() + 8 * at


class _OnDevice:
    """the operands of one case in device memory; C is made afresh for every call"""

    def __init__(self, o):
        self.o = o
        self.a, self.b, self.off, self.scale = _device(o.a_buf), _device(o.b_buf), _device(o.off_buf), _device(o.scale_buf)

    def call(self, ctx, refused=False, **change):
        """one call into a fresh C, then the host-side wait; returns C's tensor.  change: arguments replaced (a function: of the
        argument).  refused: the call must come back with BMS_ERR_INVALID (the binding's ValueError)"""
        from scri_amd import _lib, engine

        o = self.o
        c = _device(o.c_buf)
        kw = dict(form=o.form, a_ptr=_addr(self.a, o.a_at), lda=o.lda, b_ptr=_addr(self.b, o.b_at), ldb=o.ldb, c_ptr=_addr(c, o.c_at), ldc=o.ldc,
                  M=o.M, N=o.N, K=o.K, col_off_ptr=_addr(self.off, o.off_at), col_scale_ptr=_addr(self.scale, o.scale_at))
        for k, v in change.items():
            kw[k] = v(kw[k]) if callable(v) else v
        if refused:
            with pytest.raises(ValueError) as err:
                engine.dense_product(ctx=ctx, **kw)
            assert f"status {_lib.BMS_ERR_INVALID}" in str(err.value), str(err.value)
        else:
            engine.dense_product(ctx=ctx, **kw)
        ctx.synchronize()
        return c


def _run(ctx, case, kind):
    o = dp.build(case.form, case.M, case.N, case.K, kind, case.pitch, case.epilogue, case.seed)
    d = _OnDevice(o)
    first = d.call(ctx).cpu().numpy()
    worst = dp.check(o, first)
    assert np.array_equal(d.a.cpu().numpy().view(np.uint64), o.a_buf.view(np.uint64)), "A was modified"
    assert np.array_equal(d.b.cpu().numpy().view(np.uint64), o.b_buf.view(np.uint64)), "B was modified"
    again = d.call(ctx).cpu().numpy()
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64)), "the same call into a fresh C gave other bits"
    if worst > WORST.get(o.form, (-1.0, ""))[0]:
        WORST[o.form] = (worst, o.label())
    return o


@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("case", dp.sweep_cases(dp.COMPLEX), ids=dp.case_id)
def test_three_product_form_at_every_edge(ctx, case, kind):
    _run(ctx, case, kind)


@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("case", dp.sweep_cases(dp.COMPLEX_4M), ids=dp.case_id)
def test_four_product_form(ctx, case, kind):
    _run(ctx, case, kind)


@pytest.mark.parametrize("kind", dp.KINDS)
@pytest.mark.parametrize("case", dp.sweep_cases(dp.REAL), ids=dp.case_id)
def test_real_form_at_every_edge(ctx, case, kind):
    _run(ctx, case, kind)


@pytest.mark.parametrize("case", dp.map_cases(), ids=dp.case_id)
def test_tile_map_over_several_super_tiles(ctx, case):
    """integers only: the reference costs nothing and every tile that a wrong block computed, or nobody did, differs in bits"""
    want = dp.MAP_CASES[(case.form, case.M, case.N, case.K)]
    t = dp.tiling(case.form, case.M, case.N)
    assert (t.st_rows_log2, t.super_rows, t.super_cols) == want and (t.super_rows > 1 and t.super_cols > 1)
    print(f"MAP {dp.FORM_NAMES[case.form]} {case.M} x {case.N} x {case.K}: {t.nbm} x {t.nbn} tiles, st_rows_log2 = {t.st_rows_log2}, "
          f"{t.super_rows} x {t.super_cols} = {t.n_super} super-tiles, grid {t.grid}")
    _run(ctx, case, "integers")


def _refusals(o):
    """(what, arguments replaced) for every refusal of the contract this form has"""
    per, _, panel, _ = dp.shape_of(o.form)
    out = [
        ("A null", dict(a_ptr=None)), ("B null", dict(b_ptr=None)), ("C null", dict(c_ptr=None)),
        ("form 3", dict(form=3)), ("form -1", dict(form=-1)),
        ("M < 0", dict(M=-1)), ("N < 0", dict(N=-1)), ("K = 0", dict(K=0)), ("K < 0", dict(K=-2)),
        ("lda below a row", dict(lda=per * o.K - 2)), ("ldc below a row", dict(ldc=per * o.N - 2)), ("ldb below the padded width", dict(ldb=per * o.n_pad - 2)),
        ("ldb of the unpadded width", dict(ldb=per * o.N + (per * o.N) % 2)),
        ("A off 16 bytes", dict(a_ptr=lambda p: p + 8)), ("B off 16 bytes", dict(b_ptr=lambda p: p + 8)),
        ("odd lda", dict(lda=o.lda + 1)), ("odd ldb", dict(ldb=o.ldb + 1)),
    ]
    if o.real:
        out += [("odd K", dict(K=o.K - 1, lda=o.lda)), ("C off 8 bytes", dict(c_ptr=lambda p: p + 4))]
    else:
        out += [("C off 16 bytes", dict(c_ptr=lambda p: p + 8)), ("odd ldc", dict(ldc=o.ldc + 1))]
    return out


@pytest.mark.parametrize("form", [dp.COMPLEX, dp.REAL, dp.COMPLEX_4M], ids=lambda f: dp.FORM_NAMES[f])
def test_refusals_leave_c_alone(ctx, form):
    """Each refusal of include/scri_amd.h once: BMS_ERR_INVALID (a ValueError of the binding) before anything is launched, C untouched;
    M = 0 or N = 0 is BMS_OK with nothing written; and the context still computes afterwards."""
    M, N, K = (140, 130, 18) if form == dp.REAL else (70, 70, 9)
    o = dp.build(form, M, N, K, "integers", "wide", "both", 5)
    assert o.n_pad > N  # (so that the unpadded width is a pitch too short)
    d = _OnDevice(o)
    for what, change in _refusals(o):
        c = d.call(ctx, refused=True, **change)
        assert np.array_equal(c.cpu().numpy().view(np.uint64), o.c_buf.view(np.uint64)), f"{what}: C was written by a refused call"
    for what, change in (("M = 0", dict(M=0)), ("N = 0", dict(N=0)), ("M = N = 0", dict(M=0, N=0))):
        c = d.call(ctx, **change)  # BMS_OK: no exception
        assert np.array_equal(c.cpu().numpy().view(np.uint64), o.c_buf.view(np.uint64)), f"{what}: C was written"
    dp.check(o, d.call(ctx).cpu().numpy())


def test_worst_ratio_per_form_is_reported():
    """(prints what the calls above measured: `pytest -s`; the figures of the docstring come from here)"""
    for form, (worst, label) in sorted(WORST.items()):
        print(f"WORST {dp.FORM_NAMES[form]} got/bound = {worst:.3g} | {label}")
