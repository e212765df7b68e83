"""GPU parity of the transformations' time spline -- the per-pixel not-a-knot spline along time, evaluated OFF its knots at each
pixel's own skewed time -- at every seam and on every route, against oracle/waveform_grid_ref.py from_modes (oracle/abd_ref.py in
group D) restated in extended precision (tests/helpers/time_spline_cases.py; tests/test_oracle_time_spline_exact.py pins that
reference and the case tables without a GPU).  The counterpart of tests/test_gpu_spline_edges.py, tests/test_gpu_synthesis_edges.py
and tests/test_gpu_analysis_edges.py for the stage between synthesis and analysis: kernels_bspline.hip (the table and factors
kernels, bspline_forward_modes_kernel, bspline_backward_modes_kernel, bspline_solve_modes_kernel<48, 32>, abd_mix_forward_kernel<5 | 6>,
bspline_backward_eval_kernel in its window and gather instances), the evaluation in the epilogue of zgemm3m_eval_kernel with
spline_straddle_eval_kernel, the one inside synthesis_eval_kernel, and the slope form of kernels_spline.hip.

The rule (tests/helpers/spline_cases.py): with E_got = max|got - exact|, E_ref = max|fp64 oracle - exact|, scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured,     and the bar below 1e-12 scale.
Always against the exact reference and the oracle's own distance from it, never against another route of the library.

Inputs: l = 2 .. 3 (12 modes, 13 columns with the constant), the rough signal of test_bspline_path_on_short_and_irregular_time_axes
(5 % noise per sample: a wrong row, a neighbour's column or a sample one row off is an O(0.05) error), axes with |t| of order 10.
Every call follows a call of the same shape on OTHER data (a row nobody writes shows as that data's), must be finite, and is
repeated (same bits).  The route of every call is pinned: by the calls of the launchers that ctx.get_timing() counts per kernel
class, by ctx.backward_stats() (kernel launches of bspline_backward_eval_kernel with the abscissa window | of its gather instance)
and by ctx.eval_stats() (tiles of the evaluating product).

Group A -- grid level (engine.transform_modes(grid=True): no analysis in the way), time_spline_cases.A_CASES:
  A1    no boost, NO_SMALL_DENSE, NO_SYNTHESIS_EVAL   bspline_forward_modes_kernel (tile 320, halo 32, ones column) + separable synthesis
                                                      + bspline_backward_eval_kernel (tile 96: the launcher's cost model at these shapes)
  A2    A1 with SYNTHESIS_EVAL                        bspline_solve_modes_kernel + synthesis_eval_kernel
  A3    boost, default                                bspline_solve_modes_kernel + zgemm3m_eval_kernel + spline_straddle_eval_kernel
  A3'   A3 with TWO_SWEEPS                            bspline_forward_modes_kernel + bspline_backward_modes_kernel
  A3''  A3 with GEMM_EVAL_STEP = 61                   as A3, 61-row steps
  A4    boost, NO_GEMM_EVAL                           zgemm3m + bspline_backward_eval_kernel
  A5    boost, NO_BSPLINE                             slope form (launch_spline_forward / launch_spline_backward_eval)
  A5'   boost, n = 4 .. 7                             slope form, chosen by length
  A6    psi3 with its psi4 companion, boost           elimination on the grid columns (with_ones = 0), launch_psi_mix
  A6b   the same without a boost, NO_SMALL_DENSE      elimination on the modes of both fields
  lengths  97 .. 101, 193, 194 (backward tile 96: open_top, has_top_extra, the k_min clamp, a tile with no interval of its own);
           47, 48, 49, 81, 384, 385, 433 (solve tile 48, run-in 32; 8 and 9 tiles: per_xcd 1 and 2); 320, 321, 352, 353, 641 (forward
           tile 320, halo 32); 8 .. 15 (groups of four knots in the marches, of three in the backward evaluation); 4 .. 7 (slope form)
  grids    7 x 7 (one block, 15 dead lanes), 9 x 9 (the second block has 47), 15 x 15 (four panels of the product)
  axes     uniform, jittered, alternating 0.2 / 0.01 (under a boost up to 194 rows: time_spline_cases._second_axis says why), and
           the family "graded under the guard" (GRADED: a geometric stretch of ratio 1.3 over 25 steps, or 1.15 over 47, that ends
           -- growing -- or begins -- shrinking -- at row 96, 48 or 320), held to the rule on the rows beside the seam
  supertranslation  a range of 0.5, 9 and 30 steps within a block of 64 columns (A1, A4, A6, A6b): the abscissa window, the ring's
           overflow (lanes more than RING = 8 rows apart), the gather instance; under A4 a series whose early tiles fit and whose
           late ones do not (one launch of either instance)
Group B -- a shard from the middle of n = 433 whose buffer holds only the planned rows, 96 k and 96 k + 1 of them, at mode level
  (exact reference followed by analysis_cases.exact_map2salm), routes A1, A3, A4.
Group C -- under A1, the pixel columns of a block's last live lane and of the next block's first lane, after a call on a series with
  one live mode column.
Group D -- AsymptoticBondiData at mode level, l <= 2 on 5 x 5, n = 97, 100, 321, 353, uniform and alternating axis: with a boost
  (abd_mix_forward_kernel<5>, sigma on the evaluating product; NO_ABD_SIGMA_EVAL: <6>) and without (fused; NO_FUSED_ABD_MIX).

MEASURED on an MI355X, every call of this module (F and G of tests/helpers/time_spline_cases.py are the next power of two above twice
the first two columns; second column only over calls with E_ref < 4 eps scale):
  family  worst E_got/E_ref                      worst E_got/(eps scale)                worst E_got/scale: E_got, E_ref, case
  A1      4.92  C n=194 column 79                 9.21  C n=194 column 80                 1.6e-14: 3.3e-14, 2.9e-14, A1-320-7-alternating-0.5
  A2      2.76  A2-15-7-uniform-0.5               6.79  A2-12-7-uniform-0.5               1.3e-14: 3.5e-14, 3.9e-14, A2-433-7-alternating-0.5
  A3      2.02  A3-12-7-uniform-0.5               5.90  A3-12-7-uniform-0.5               9.6e-15: 2.5e-14, 5.4e-14, A3-47-7-alternating-0.5
  A3'     2.02  A3'-12-7-uniform-0.5              5.90  A3'-12-7-uniform-0.5              9.8e-15: 2.2e-14, 2.2e-14, A3'-641-7-uniform-0.5
  A4      1.97  A4-15-7-uniform-0.5               5.70  A4-15-7-uniform-0.5               3.3e-14: 6.8e-14, 1.1e-13, A4-194-7-alternating-0.5
  A5      1.42  A5-9-9-alternating-0.5            2.61  A5-9-7-uniform-0.5                9.6e-15: 2.1e-14, 4.9e-14, A5-100-9-alternating-0.5
  A5'     1.87  A5'-4-7-jitter-0.5                4.20  A5'-7-7-uniform-0.5               9.3e-16: 2.0e-15, 1.2e-15, A5'-7-7-uniform-0.5
  A6      1.11  A6-9-7-uniform-0.5                3.73  A6-9-7-uniform-0.5                6.6e-15: 1.7e-14, 4.4e-14, A6-100-7-alternating-0.5
  A6b     2.25  A6b-100-7-uniform-0.5             8.53  A6b-100-9-uniform-30.0            1.0e-14: 2.2e-14, 3.0e-14, A6b-353-7-alternating-0.5
  graded  2.32  A1-390-320-1.15-47-True, seam     6.59  A1-390-320-1.15-47-True, beside   1.0e-14: 1.8e-14, 2.1e-14, A3'-390-320-1.3-25-False, beside
  modes   1.76  B A1-433-9-120-242                5.51  B A1-433-9-120-242                1.2e-15: 2.9e-15, 1.7e-15, B A1-433-9-120-242
  abd     2.20  D Dfused-97-uniform               5.36  D Dfused-100-uniform              1.2e-14: 3.6e-14, 8.1e-14, D D5-353-alternating
(case ids as the tests': route-n-grid-axis-supertranslation range in steps; graded: route-n-seam-ratio-steps-grows; A3'' under A3.)
Every family is inside the caps with no kernel change.  The graded family, on the rows beside its seams, stays within 7.4 eps scale
(6.6 next to the run-in of the 320-knot elimination tile on the stretch of ratio 1.15 over 47 steps; 4.9 .. 7.4 at the 96-knot
backward tile; 4.0 .. 6.3 at the 48-knot solve tile): the 32-knot halo has forgotten its start on every axis of these tables that the
guard lets through, so the guard (steps varying more than 1e3-fold within 48 samples) stays as it is.  Over ALL rows of a graded
case -- the steps of 1.4e-4 included, where the oracle itself is 500 .. 800 eps scale from the exact result -- E_got / E_ref is
0.24 .. 5.4 (A3-118-48-1.3-25-True: 5.5e-14 against 1.0e-14), which the test holds to the cap of F.
"""
import numpy as np
import pytest

from tests.helpers import time_spline_cases as ts
from tests.helpers.spline_cases import EPS, errors

pytestmark = pytest.mark.gpu

ALL_OPTIONS = ts.ROUTE_OPTIONS + ts.ABD_OPTIONS
WORST = {}  # family -> [worst E_got / E_ref, where, worst E_got / (eps scale) where E_ref < 4 eps scale, where, worst E_got / scale, (E_got, E_ref), where]


def _record(family, got, exact, ref, what):
    e_got, e_ref, scale = errors(got, exact, ref)
    w = WORST.setdefault(family, [0.0, "", 0.0, "", 0.0, (0.0, 0.0), ""])
    if e_ref > 0 and e_got / e_ref > w[0]:
        w[0], w[1] = e_got / e_ref, what
    if e_ref < 4 * EPS * scale and e_got / (EPS * scale) > w[2]:
        w[2], w[3] = e_got / (EPS * scale), what
    if e_got / scale > w[4]:
        w[4], w[5], w[6] = e_got / scale, (e_got, e_ref), what


def _check(family, got, exact, ref, what):
    _record(family, got, exact, ref, what)
    return ts.check(family, got, exact, ref, what)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture
def routed(ctx, route):
    """routed(options): exactly these route options for the rest of the test, launch counting on"""
    def set_(options):
        for name in ALL_OPTIONS:
            route(name, str(options[name]) if name in options else None)

    ctx.enable_timing(True)
    yield set_
    ctx.enable_timing(False)
    for name in ALL_OPTIONS:
        route(name, None)


def _counted(ctx, call):
    """(result, {kernel class: calls of its launchers} + the launches of the two backward-evaluation instances, eval_stats) of one call"""
    ctx.synchronize()
    ctx.get_timing(reset=True)
    ctx.eval_stats(reset=True)
    ctx.backward_stats(reset=True)
    assert ctx.backward_stats(reset=False) == (0, 0)
    out = call()
    ctx.synchronize()
    counts = {k: v[1] for k, v in ctx.get_timing(reset=True).items()}  # (calls of the launchers, not kernel launches)
    counts["backward_window"], counts["backward_gather"] = ctx.backward_stats(reset=True)
    return out, counts, ctx.eval_stats(reset=True)


def _transformation(b, ell_max_out=ts.ELL_MAX):
    from scri_amd import engine

    return engine.make_transformation(b["st"], b["rot"], b["v"], b["grid"], b["grid"], ell_max_out)


def _modes_call(ctx, b, data, aux, grid=True, shard=None, rows=slice(None)):
    """engine.transform_modes on the case's axis and transformation with the given data"""
    from scri_amd import engine

    w = b["w"]
    psi = b["name"] == "psi3"
    term = engine.BMS_TERM_PSI if psi else engine.BMS_TERM_H
    aux_in = [(np.ascontiguousarray(aux[rows]), ts.ELL_MIN, ts.ELL_MAX, -2, 1.0, 1)] if psi else ()
    return engine.transform_modes(b["t"], np.ascontiguousarray(data[rows]), ts.ELL_MIN, ts.ELL_MAX, w.spin_weight, w.conformal_weight, term, _transformation(b),
                                  aux=aux_in, ctx=ctx, grid=grid, shard=shard)


def _expected(b, cus, rows=None, g0=0):
    """what the route must show: (spline_forward, (launches of bspline_backward_eval_kernel with the abscissa window, of its gather
    instance) or the calls of another backward launcher, pointwise or None, tiles of the evaluating product)"""
    route, n = b["route"], b["n"]
    rows = n if rows is None else rows
    panels = (b["grid"] ** 2 + 63) // 64
    tile = ts.backward_tile(b["grid"] ** 2, rows, cus)
    assert tile == 96, (tile, cus)  # the launcher's cost model at this shape, on this device
    bwd = ts.launches_by_instance(ts.backward_launches(b["t"], b["tt"], *ts.spread_of(b), tile, g0, rows)[1])
    if route == "A1":
        return 1, bwd, None, 0
    if route == "A2":
        return 1, 0, None, 0
    if route in ("A3", "A3''"):
        return 1, 0, None, panels * ts.eval_blocks(rows, 61 if route == "A3''" else 64)
    if route == "A3'":
        return 1, 1, None, panels * ts.eval_blocks(rows)
    if route == "A4":
        return 1, bwd, None, 0
    if route in ("A5", "A5'"):
        return 1, 1, None, 0
    if route == "A6":
        return 1, bwd, 2, 0
    if route == "A6b":
        return 2, bwd, 2, 0
    raise KeyError(route)


def _pin_route(b, counts, stats, cus, what, **kw):
    fwd, bwd, pointwise, tiles = _expected(b, cus, **kw)
    by_instance = (counts["backward_window"], counts["backward_gather"])
    seen = (counts["spline_forward"], counts["spline_backward"], counts["pointwise"], stats[0])
    print(f"ROUTE {b['route']} forward={seen[0]} backward={seen[1]} window|gather={by_instance} pointwise={seen[2]} gemm_synthesis={counts['gemm_synthesis']} "
          f"eval_stats={stats} | {what}")
    if isinstance(bwd, tuple):  # bspline_backward_eval_kernel: one call of its launcher, and these launches of its two instances
        assert by_instance == bwd, f"{what}: launches (abscissa window, gather) = {by_instance}, expected {bwd}"
        bwd = 1
    else:
        assert by_instance == (0, 0), what
    assert seen[0] == fwd and seen[1] == bwd and stats[0] == tiles, f"{what}: another route ran -- launches {seen}, expected {(fwd, bwd, pointwise, tiles)}"
    if pointwise is not None:
        assert seen[2] == pointwise, f"{what}: {seen[2]} pointwise launches, expected {pointwise}"
    if b["route"] in ("A4", "A5", "A5'"):
        assert counts["gemm_synthesis"] == 1, what  # the plain dense product
    if b["route"] == "A6":
        assert counts["gemm_synthesis"] == 2, what  # the field and its companion


def _grid_case(ctx, routed, b, family, what, rows=None):
    routed(ts.ROUTES[b["route"]][0])
    cus = _cus()
    other = _modes_call(ctx, b, ts.other_data(b), None if b["aux"] is None else ts.other_data(b, "aux"))
    assert other[1].shape == b["exact"].shape, what
    (t_got, got), counts, stats = _counted(ctx, lambda: _modes_call(ctx, b, b["data"], b["aux"]))
    _pin_route(b, counts, stats, cus, what)
    assert t_got.shape == b["t_out"].shape and np.abs(t_got - b["t_out"]).max() <= 4 * EPS * max(1.0, np.abs(b["t_out"]).max()), what
    got = np.array(got)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result"
    for name, r in ([("", slice(None))] if rows is None else rows):
        _check(family, got[r], b["exact"][r], b["ref"][r], what + name)
    assert not _same_bits(got, other[1])
    assert _same_bits(got, _modes_call(ctx, b, b["data"], b["aux"])[1]), f"{what}: a repeated call gives other bits"
    return got


# ------------------------------------------------------------------------------------------------------------- group A
@pytest.mark.parametrize("case", ts.A_CASES, ids=ts.case_id)
def test_a_grid(ctx, routed, case):
    b = ts.build_case(case)
    _grid_case(ctx, routed, b, "A3" if case[0] == "A3''" else case[0], f"A {ts.case_id(case)} rows {b['exact'].shape[0]}")


def test_a_backward_classes_split_inside_the_series(ctx, routed):
    """A4: skew_rate_range |x - tt| crosses 10 dt inside the series -- the early tiles read the abscissa window, the late ones gather"""
    b = ts.build_case(ts.SPLIT_CASE)
    launches, f, tile = ts.expected_backward_launches(b, _cus())
    assert (launches, f) == (2, [True, True, True, False, False]) and ts.launches_by_instance(f) == (1, 1)
    _grid_case(ctx, routed, b, "A4", f"A split {ts.case_id(ts.SPLIT_CASE)}")


@pytest.mark.parametrize("case", ts.GRADED, ids=ts.case_id)
def test_a_graded_under_the_guard(ctx, routed, case):
    """the tiled recurrences on an axis the guard accepts: their run-in must have forgotten its start at the seam"""
    b = ts.build_graded(case)
    assert ts.regular_axis(b["t"])
    side, near = ts.graded_rows(case, b)
    assert side.size >= 40 and near.size >= 40
    got = _grid_case(ctx, routed, b, "graded", f"A graded {ts.case_id(case)}", rows=[(f" {side.size} rows beside the seam", side), (" rows at the seam", near)])
    e_got, e_ref, scale = errors(got, b["exact"], b["ref"])  # every row, the short steps included: recorded, and held to the cap of F alone
    print(f"GRADED all {got.shape[0]} rows: E_got={e_got:.3e} E_ref={e_ref:.3e} scale={scale:.3e} got/ref={e_got / e_ref:.3g} | {ts.case_id(case)}")
    assert e_got <= 32 * e_ref


# ------------------------------------------------------------------------------------------------------------- group B
@pytest.mark.parametrize("case", ts.B_CASES, ids=ts.case_id)
def test_b_shard_between_seams(ctx, routed, case):
    from scri_amd import engine

    route, n, g, o0, o1 = case
    b = ts.build_case((route, n, g, "uniform", 0.5))
    exact, ref = ts.exact_modes_of(b)
    tr = _transformation(b)
    (r0, r1), (w0, w1) = engine.shard_plan(b["t"], tr, o0, o1)
    assert 0 < r0 and r1 < n and (r1 - r0) == ts.needed_rows_of_case(case) and (r1 - r0) % 96 in (0, 1)
    assert (w0, w1) == ts.window_of(b) and w0 <= o0 and o1 <= w1
    routed(ts.ROUTES[route][0])
    shard = (r0, r1 - r0, o0, o1)
    what = f"B {ts.case_id(case)} rows [{r0}, {r1})"
    other = _modes_call(ctx, b, ts.other_data(b), None, grid=False, shard=shard, rows=slice(r0, r1))
    (t_got, got, first), counts, stats = _counted(ctx, lambda: _modes_call(ctx, b, b["data"], None, grid=False, shard=shard, rows=slice(r0, r1)))
    fwd, bwd, _, tiles = _expected(b, _cus(), rows=r1 - r0, g0=r0)
    by_instance = (counts["backward_window"], counts["backward_gather"])
    print(f"ROUTE {route} forward={counts['spline_forward']} backward={counts['spline_backward']} window|gather={by_instance} eval_stats={stats} | {what}")
    assert by_instance == (bwd if isinstance(bwd, tuple) else (0, 0)), what
    assert (counts["spline_forward"], counts["spline_backward"]) == (fwd, 1 if isinstance(bwd, tuple) else bwd), what
    assert (stats[0] > 0) == (tiles > 0), what
    assert first == o0 and got.shape[0] == o1 - o0 and other[1].shape == got.shape
    sl = slice(o0 - w0, o1 - w0)
    assert np.abs(t_got - b["t_out"][sl]).max() <= 4 * EPS * max(1.0, np.abs(b["t_out"]).max())
    got = np.array(got)
    _check("modes", got, exact[sl], ref[sl], what)
    assert _same_bits(got, _modes_call(ctx, b, b["data"], None, grid=False, shard=shard, rows=slice(r0, r1))[1]), f"{what}: a repeated call gives other bits"


# ------------------------------------------------------------------------------------------------------------- group C
@pytest.mark.parametrize("n", [100, 194])
def test_c_block_edge_columns(ctx, routed, n):
    """a dead lane of the last block carries p = n_cols - 1: it must not write.  One live mode column first, then the full series;
    columns 63 | 64 (last lane of block 0, first of block 1) and 80 (the last live lane, the dead lanes' alias) under the rule"""
    b = ts.build_case(("A1", n, 9, "uniform", 0.5))
    routed(ts.ROUTES["A1"][0])
    one = np.zeros_like(b["data"])
    one[:, 5] = b["data"][:, 5]
    first = _modes_call(ctx, b, one, None)[1]
    assert np.isfinite(first).all()
    got = np.array(_modes_call(ctx, b, b["data"], None)[1])
    for c in (62, 63, 64, 65, 79, 80):
        _check("A1", got[:, c : c + 1], b["exact"][:, c : c + 1], b["ref"][:, c : c + 1], f"C n={n} column {c}")
    _check("A1", got, b["exact"], b["ref"], f"C n={n} all columns")


# ------------------------------------------------------------------------------------------------------------- group D
def _abd_expected(route):
    """(calls of the spline_forward launchers, calls of launch_bspline_backward_eval, evaluating product ran?)"""
    if route == "D5":
        return 2, 5, True      # the solve of sigma's modes + abd_mix_forward_kernel<5>; five back substitutions
    if route == "D6":
        return 1, 6, False     # abd_mix_forward_kernel<6>
    if route == "Dfused":
        return 6, 6, False     # six eliminations on the modes, mixing in the phi stage
    return 1, 6, False         # Dgrid: separable synthesis, abd_mix_forward_kernel<6>


@pytest.mark.parametrize("case", ts.D_CASES, ids=ts.case_id)
def test_d_abd(ctx, routed, case):
    from scri_amd import engine

    route, n, ax = case
    b = ts.build_abd(*case)
    routed(ts.ABD_ROUTES[route][0])
    tr = engine.make_transformation(b["st"], b["rot"], b["v"], ts.ABD_GRID, ts.ABD_GRID, ts.ABD_ELL_MAX)
    what = f"D {ts.case_id(case)}"
    other = engine.transform_abd(b["u"], b["other"], ts.ABD_ELL_MAX, tr, ctx=ctx)
    (u_got, got), counts, stats = _counted(ctx, lambda: engine.transform_abd(b["u"], b["raw"], ts.ABD_ELL_MAX, tr, ctx=ctx))
    print(f"ROUTE {route} forward={counts['spline_forward']} backward={counts['spline_backward']} window|gather=({counts['backward_window']}, "
          f"{counts['backward_gather']}) pointwise={counts['pointwise']} gemm_synthesis={counts['gemm_synthesis']} eval_stats={stats} | {what}")
    fwd, bwd, evaluating = _abd_expected(route)
    assert (counts["spline_forward"], counts["spline_backward"], stats[0] > 0) == (fwd, bwd, evaluating), what
    assert counts["backward_window"] + counts["backward_gather"] >= bwd, what
    assert u_got.shape == b["u_out"].shape and np.abs(u_got - b["u_out"]).max() <= 4 * EPS * max(1.0, np.abs(b["u_out"]).max())
    got = np.array(got)
    assert other[1].shape == got.shape
    _check("abd", got, b["exact"], b["ref"], what)
    assert _same_bits(got, engine.transform_abd(b["u"], b["raw"], ts.ABD_ELL_MAX, tr, ctx=ctx)[1]), f"{what}: a repeated call gives other bits"


def test_zz_measured_table():
    """prints what the calls of this module measured (pytest -s): the figures next to RULE in the helper"""
    print("MEASURED family | worst E_got/E_ref | worst E_got/(eps scale) where E_ref < 4 eps scale | worst E_got/scale: E_got, E_ref")
    for family in sorted(WORST):
        w = WORST[family]
        print(f"MEASURED {family:12s} {w[0]:8.3g}  {w[1]}\nMEASURED {'':12s} {w[2]:8.3g}  {w[3]}\nMEASURED {'':12s} {w[4]:8.2e}: {w[5][0]:.2e}, {w[5][1]:.2e}  {w[6]}")
    for family, (F, G) in ts.RULE.items():
        assert F <= 32 and G <= 256, family
