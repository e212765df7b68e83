"""The evaluating dense product (zgemm3m_eval_kernel + spline_straddle_eval_kernel) at the smallest shapes that reach every path of
its operand requests, its tile window and its row search, between guard regions (tests/test_gpu_guard_regions.py) and against the
NO_GEMM_EVAL route of the same context (back substitution on the grid) at the bar of that file, 1e-13 x scale:

* l <= 5: K = 33 k-steps, no multiple of the 8 of a turn -- the last turn asks for k-steps beyond K, which must read as zero;
* a 15 x 15 grid: 197 stored columns -- three full 64-column panels and a narrow one of 5;
* n = 331 rows (six tiles, the last of 11 rows: its second operand row group lies wholly beyond M), n = 70 (a tile of 64 and one
  of 6), n = 9 (a single ragged tile; its time step is ten times longer, so that output rows remain);
* a shard from the middle of a 700-step series whose buffer holds ONLY the planned rows.  The guards lie around the CALLER's rows: a
  read of the input past the shard's first or last row (the solve's run-in, the staging of the product's A operand) meets a NaN.
  The product itself reads A from the engine's own buffer of solved coefficients, so these tests see a descriptor that ends too
  EARLY (rows or k-steps read as zero: wrong values) or a wrong turn offset, not one that reaches a few rows too far -- that its
  bounds are exactly the rows and k-steps of the tile is established by reading the kernel, not here.  (That holds for the EVALUATING
  product only.  The plain products, zgemm3m_mfma_kernel and dgemm_mfma_kernel, are held to exactly that -- A between NaNs, garbage in
  B's padding, sentinels around C, a reference on operands the test owns -- by tests/test_gpu_dense_product_edges.py);
* the uniform, the jittered and the graded time axis (synthetic.time_axis) at a mild boost and at 40 times that boost (two samples in
  some intervals, none in others): the search's first guess accepted, one off, the nine steps, and tiles whose samples leave the
  window of output times staged in LDS.  ctx.eval_stats() = (tiles and boundary blocks launched, of those: the ones whose samples do
  not fit the window they stage, marches that went on from global memory) tells which of these ran, and the tests pin it: on the
  uniform and the jittered axis everything stays on the staged window at either boost; on the graded axis at 40 times the boost the
  late tiles of n = 331 and of the shard reject their window (the steps there are several times shorter than where the skew was
  earned); at n = 70 on the graded axis with 64-row steps a search cannot tell at the edge of its staged window (with 61-row steps,
  which have no boundary blocks, every search can) and the march goes on from global memory.  A change of synthetic.time_axis, of the window's margins or of these boosts that loses one of
  the exits fails the test instead of passing on the staged path alone.
The comparison here stays one between two routes of the library; where the evaluating product meets a reference -- the oracle's
from_modes restated in extended precision -- is tests/test_gpu_time_spline_edges.py (routes A3, A3', A3'')."""
import numpy as np
import pytest

from tests.test_gpu_guard_regions import GUARD, _check_guards, _guarded_input, _guarded_output

pytestmark = pytest.mark.gpu

ELL_MAX = 5
N_GRID = 15
DT = 0.1
BOOST = np.array([2e-3, -1e-3, 3e-3])
ROUTES = ("SCRI_AMD_GEMM_EVAL_STEP", "SCRI_AMD_TWO_SWEEPS", "SCRI_AMD_NO_GEMM_EVAL", "SCRI_AMD_NO_BSPLINE")


def _case(n, axis, boost_scale):
    from scri_amd import engine, synthetic

    t = synthetic.time_axis(n, DT if n >= 70 else 10 * DT, axis)  # (nine rows: a step longer than the supertranslation, or no output row is left)
    data = synthetic.chirp_modes(t, 2, ELL_MAX, 31)
    assert data.shape[1] + 1 == 33  # K: modes + the column of the constant, four turns of 8 and one k-step
    st = synthetic.real_supertranslation(0.1 * (np.arange(9) - 2.0 + 0.5j * np.arange(9)))
    tr = engine.make_transformation(st, [0.8, 0.2, -0.5, 0.1], list(boost_scale * BOOST), N_GRID, N_GRID, ELL_MAX)
    return t, data, tr


N_PANELS = 4  # 197 stored columns of the 15 x 15 grid: three panels of 64 and one of 5


def _blocks(rows, step):
    """row tiles of the evaluating product on `rows` rows, and with 64-row steps the boundaries between them (one block of the
    straddle kernel each); eval_stats()[0] counts both, once per column panel -- so the count also pins the four panels"""
    if step == 64:
        row_tiles = (rows + 63) // 64
        return 2 * row_tiles - 1
    return (rows - 3 + 60) // 61


def _check_paths(n, axis, boost_scale, step, off, cont):
    """which exits the run took (module docstring)"""
    if axis in ("uniform", "jitter"):
        assert off == 0 and cont == 0, (off, cont)  # every sample inside the window its tile staged; the search always answers
    elif n in (331, 700) and boost_scale == 40.0:
        assert off > 0, (off, cont)  # tiles whose samples do not fit the staged window: evaluated from global memory
    elif n == 70 and step == 64:
        assert off == 0 and cont > 0, (off, cont)  # the window was staged, the search could not tell: on from global memory
    else:
        assert off == 0, (off, cont)


def _reference(ctx, route, t, data, tr):
    """back substitution on the grid: no evaluating product"""
    from scri_amd import engine

    for k in ROUTES:
        route(k, None)
    route("SCRI_AMD_NO_GEMM_EVAL", "1")
    ctx.eval_stats(reset=True)
    t_ref, d_ref = engine.transform_modes(t, data, 2, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=ctx)
    assert ctx.eval_stats(reset=True)[0] == 0
    route("SCRI_AMD_NO_GEMM_EVAL", None)
    return t_ref, d_ref


@pytest.mark.parametrize("step", [64, 61])
@pytest.mark.parametrize("boost_scale", [1.0, 40.0])
@pytest.mark.parametrize("axis", ["uniform", "jitter", "sxs"])
@pytest.mark.parametrize("n", [331, 70, 9])
def test_small_dense_product_between_guards(ctx, route, n, axis, boost_scale, step):
    from scri_amd import engine

    t, data, tr = _case(n, axis, boost_scale)
    nm = data.shape[1]
    t_ref, d_ref = _reference(ctx, route, t, data, tr)
    assert d_ref.shape[0] > 0
    scale = max(1.0, np.abs(d_ref).max())
    if step != 64:
        route("SCRI_AMD_GEMM_EVAL_STEP", str(step))
    src, sp = _guarded_input(data)
    dst, dp = _guarded_output(n * nm)
    ctx.eval_stats(reset=True)
    t_out, n_new = engine.transform_modes(t, sp, 2, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=ctx, device=True, ld=nm, out_ptr=dp)
    ctx.synchronize()
    tiles, off, cont = ctx.eval_stats(reset=True)
    got = dst[GUARD : GUARD + n_new * nm].cpu().numpy().reshape(n_new, nm)
    assert n_new == d_ref.shape[0] and np.array_equal(t_out, t_ref)
    assert np.isfinite(got).all(), "a read outside the input rows"
    err = np.abs(got - d_ref).max()
    print(f"n={n} axis={axis} boost x{boost_scale:g} step={step}: {n_new} rows, max|err| = {err:.3e} (scale {scale:.3g}), "
          f"tiles {tiles}, off the window {off}, marches from global memory {cont}")
    assert err < 1e-13 * scale
    _check_guards(dst, n * nm)
    assert np.array_equal(src[GUARD : GUARD + n * nm].cpu().numpy().reshape(n, nm), data), "the input rows were modified"
    assert tiles == N_PANELS * _blocks(n, step), (tiles, off, cont)
    _check_paths(n, axis, boost_scale, step, off, cont)


@pytest.mark.parametrize("boost_scale", [1.0, 40.0])
@pytest.mark.parametrize("axis", ["uniform", "jitter", "sxs"])
def test_small_dense_product_on_a_shard_between_guards(ctx, route, axis, boost_scale):
    from scri_amd import engine

    n = 700
    t, data, tr = _case(n, axis, boost_scale)
    nm = data.shape[1]
    t_ref, d_ref = _reference(ctx, route, t, data, tr)
    scale = max(1.0, np.abs(d_ref).max())
    o0, o1 = 200, 350
    (r0, r1), (w0, w1) = engine.shard_plan(t, tr, o0, o1)
    assert 0 < r0 and r1 < n, "the shard must lie inside the series"
    src, sp = _guarded_input(data[r0:r1])
    dst, dp = _guarded_output((o1 - o0) * nm)
    ctx.eval_stats(reset=True)
    t_out, n_new, first = engine.transform_modes(t, sp, 2, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=ctx, device=True, ld=nm, out_ptr=dp,
                                                 shard=(r0, r1 - r0, o0, o1))
    ctx.synchronize()
    tiles, off, cont = ctx.eval_stats(reset=True)
    got = dst[GUARD : GUARD + n_new * nm].cpu().numpy().reshape(n_new, nm)
    assert n_new == min(o1, w1) - max(o0, w0) > 50 and first == max(o0, w0)
    assert np.isfinite(got).all(), "a read outside the shard's rows"
    err = np.abs(got - d_ref[first - w0 : first - w0 + n_new]).max()
    print(f"shard rows [{r0}, {r1}) axis={axis} boost x{boost_scale:g}: {n_new} rows, max|err| = {err:.3e} (scale {scale:.3g}), "
          f"tiles {tiles}, off the window {off}, marches from global memory {cont}")
    assert err < 1e-13 * scale
    _check_guards(dst, (o1 - o0) * nm)
    assert tiles == N_PANELS * _blocks(r1 - r0, 64), (tiles, off, cont)  # the product runs on the shard's rows
    _check_paths(n, axis, boost_scale, 64, off, cont)
