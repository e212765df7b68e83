"""No GPU: pins the exact reference of tests/test_gpu_time_spline_edges.py (tests/helpers/time_spline_cases.py exact_from_modes and
build_abd -- oracle/waveform_grid_ref.py from_modes and oracle/abd_ref.py transform restated in extended precision) and holds its
case tables to the launchers' arithmetic, restated in the helper:

* under the identity transformation the exact reference is the exact synthesis of the input rows, to longdouble rounding;
* on data that is a cubic polynomial in time per mode, under a pure supertranslation, it is the closed form (the not-a-knot spline of
  a cubic is the cubic);
* its per-column evaluation is oracle/spline_exact.py evaluate column by column;
* it lies within the recorded distance of fp64 from_modes;
* every case reaches the tile, the instance and the route its group names, and its bar stays below 1e-12 x scale.

MEASURED here (x86-64, numpy longdouble = 80-bit): max|from_modes - exact| / (eps scale) over the tables is up to 160 without a boost
(n = 641 on the alternating axis), up to 240 under one (n = 194 on the alternating axis: the fp64 rounding of k (t - alpha), |t| eps,
times a slope of 0.05 per short step), and on the graded family up to 830 where the steps are 1.4e-4 but 2 .. 40 beside the seam."""
import numpy as np
import pytest

from oracle import containers, quat, wigner
from oracle import spline_exact as sx
from oracle import waveform_grid_ref as grid_ref
from tests.helpers import synthesis_cases as sy
from tests.helpers import time_spline_cases as ts
from tests.helpers.spline_cases import EPS, errors

LD_EPS = float(np.finfo(np.longdouble).eps)


@pytest.fixture(autouse=True)
def _robust_poles():
    """the exact reference is built with the oracle's well-conditioned pole angles, as the GPU tests that use it are"""
    old = quat.ROBUST_POLES
    quat.ROBUST_POLES = True
    yield
    quat.ROBUST_POLES = old


def _rotors(g):
    """the oracle's rotors of the g x g grid under the identity (its angles are np.linspace's, an ulp from pi j / (g - 1) here and there)"""
    return grid_ref.rotor_grid(np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3), g, g).reshape(-1, 4)


def test_identity_gives_the_exact_synthesis():
    n, g = 23, 7
    t = ts.axis("jitter", 100)[:n]
    data = ts.rough_signal(t, ts.N_MODES, 5)
    for name in ("h", "psi4", "sigma"):
        w = containers.WM(t=t, data=data, ell_min=2, ell_max=3, dataType=getattr(containers, name))
        t_out, exact, ref, alpha, k, gamma, tt = ts.exact_from_modes(w, n_theta=g, n_phi=g)
        assert np.array_equal(t_out, t) and gamma == 1.0 and tt == 0.0 and not alpha.any() and (k == 1.0).all()
        Y = wigner.swsh_grid(_rotors(g), w.spin_weight, 3)[:, 4:]
        want = sy.exact_product(data, Y)
        assert float(np.abs(exact - want).max()) <= 64 * LD_EPS * float(np.abs(want).max()), name


def test_cubic_in_time_under_a_supertranslation_is_the_closed_form():
    """f_lm(t) = a + b t + c t^2 + d t^3 per mode: the spline is the polynomial, so the result is the synthesis of the polynomial's
    values at t* = uprm + alpha_p (no boost: k = 1), minus the h term"""
    n, g = 40, 7
    t = ts.axis("jitter", 100)[:n] + 8.0
    rng = np.random.default_rng(9)
    coef = (rng.normal(size=(4, ts.N_MODES)) + 1j * rng.normal(size=(4, ts.N_MODES))) * np.array([1.0, 0.5, 0.2, 0.05])[:, None]
    tL = t.astype(np.longdouble)
    data = sum(coef[q][None, :] * t[:, None] ** q for q in range(4))  # fp64-rounded samples of the polynomial ...
    dataL = sum(coef[q].astype(np.clongdouble)[None, :] * tL[:, None] ** q for q in range(4))
    st = ts.supertranslation(0.07, 0.0)
    for name in ("psi4", "h"):
        w = containers.WM(t=t, data=data, ell_min=2, ell_max=3, dataType=getattr(containers, name))
        t_out, exact, ref, alpha, k, gamma, tt = ts.exact_from_modes(w, supertranslation=st, n_theta=g, n_phi=g)
        assert 30 < t_out.size < n and (k == 1.0).all() and gamma == 1.0 and np.ptp(alpha) > 0.03
        R = _rotors(g)
        Y = wigner.swsh_grid(R, -2, 4)
        aL = sy.exact_product(st[None, :], wigner.swsh_grid(R, 0, 2))[0].real
        tstar = t_out.astype(np.longdouble)[:, None] + aL[None, :]
        # sum_lm poly_lm(t*_p) Y_lm(p): power by power
        want = sum(sy.exact_product(coef[q][None, :], Y[:, 4:16])[0][None, :] * tstar**q for q in range(4))
        if name == "h":
            want = want - sy.exact_product((2 * ts._ld_ethbar(ts._ld_ethbar(st, 0), -1))[None, :], Y[:, :9])
        # ... so the spline interpolates the ROUNDED samples: their rounding, carried through the spline, is all that is left
        rounding = float(np.abs(data - dataL).max())
        err = float(np.abs(exact - want).max())
        print(f"{name}: max|exact - closed form| = {err:.3e}, rounding of the samples {rounding:.3e}, scale {float(np.abs(want).max()):.3e}")
        assert err <= 16 * rounding * np.sqrt(ts.N_MODES)
        assert err < 1e-3 * float(np.abs(ref - exact).max()) or err < 64 * EPS


def test_cubic_in_time_to_longdouble_rounding():
    """the same with samples that fp64 holds exactly (small integers on a dyadic axis): no rounding of the input is left, and the
    reference reproduces the polynomial to longdouble rounding"""
    n, g = 24, 7
    t = np.cumsum(np.where(np.arange(n) % 3 == 0, 0.25, 0.125)) - 1.0
    coef = np.array([[3, -2, 1, 2, 0, -1, 2, 1, -3, 1, 2, -1], [1, 2, -1, 0, 3, 1, -2, 1, 1, 0, -1, 2], [2, 0, 1, -1, 1, 2, 0, -2, 1, 1, 1, 0],
                     [1, -1, 0, 2, -1, 0, 1, 1, 0, -1, 2, 1]], dtype=float) * (1 + 1j)
    data = sum(coef[q][None, :] * t[:, None] ** q for q in range(4))
    assert np.array_equal(data, sum(coef[q].astype(np.clongdouble)[None, :] * t.astype(np.longdouble)[:, None] ** q for q in range(4)).astype(complex))
    st = ts.supertranslation(0.07, 0.0)
    w = containers.WM(t=t, data=data, ell_min=2, ell_max=3, dataType=containers.psi4)
    t_out, exact, ref, alpha, k, gamma, tt = ts.exact_from_modes(w, supertranslation=st, n_theta=g, n_phi=g)
    R = _rotors(g)
    aL = sy.exact_product(st[None, :], wigner.swsh_grid(R, 0, 2))[0].real
    tstar = t_out.astype(np.longdouble)[:, None] + aL[None, :]
    Y = wigner.swsh_grid(R, -2, 3)[:, 4:]
    want = sum(sy.exact_product(coef[q][None, :], Y)[0][None, :] * tstar**q for q in range(4))
    err = float(np.abs(exact - want).max())
    print(f"max|exact - closed form| = {err:.3e} = {err / LD_EPS / float(np.abs(want).max()):.1f} longdouble eps x scale")
    assert t_out.size > 15 and err <= 4096 * LD_EPS * float(np.abs(want).max())  # (the slope system's conditioning on a 2:1 axis)


def test_per_column_evaluation_is_spline_exact():
    t = ts.axis("alternating", 100)[:30]
    y = ts.rough_signal(t, 5, 3).astype(np.clongdouble)
    u = (t[3:-3, None] + np.linspace(-0.11, 0.13, 5)[None, :]).astype(np.longdouble)
    got = ts.evaluate_per_column(t, y, sx.slopes(t, y), u)
    for p in range(5):
        assert np.array_equal(got[:, p], sx.evaluate(t, y[:, p], u[:, p]))


def _all_built():
    for c in ts.A_CASES:
        yield ("A3" if c[0] == "A3''" else c[0]), ts.case_id(c), ts.build_case(c)  # (A3'' runs A3's kernels and counts under its family)
    for c in ts.GRADED:
        yield "graded", ts.case_id(c), ts.build_graded(c)
    yield ts.SPLIT_CASE[0], "split", ts.build_case(ts.SPLIT_CASE)


def test_distance_of_fp64_from_modes_and_every_bar():
    """the recorded distance of the oracle from the exact reference, and the rule's second condition: bar < 1e-12 x scale for every case"""
    worst = {}
    for family, name, b in _all_built():
        assert b["exact"].shape[0] >= 2, name
        e_ref, _, scale = errors(b["ref"], b["exact"], b["ref"])
        if family == "graded":  # held to the rule on the rows beside the seam (time_spline_cases.graded_rows says why)
            side, near = ts.graded_rows(next(c for c in ts.GRADED if ts.case_id(c) == name), b)
            assert side.size >= 40 and near.size >= 40, name
            for r in (side, near):
                e_r, _, scale_r = errors(b["ref"][r], b["exact"][r], b["ref"][r])
                assert ts.bar(family, e_r, scale_r) < ts.BAR_CAP * scale_r and e_r < 64 * EPS * scale_r, (name, e_r / (EPS * scale_r))
        else:
            assert ts.bar(family, e_ref, scale) < ts.BAR_CAP * scale, (name, e_ref / (EPS * scale))
        kind = "graded" if family == "graded" else ("boost-free" if not b["v"].any() else "boosted")
        worst[kind] = max(worst.get(kind, 0.0), e_ref / (EPS * scale))
    print({k: round(v, 1) for k, v in worst.items()})
    assert worst["boost-free"] < 200 and worst["boosted"] < 300 and worst["graded"] < 700
    for c in ts.D_CASES:
        b = ts.build_abd(*c)
        e_ref, _, scale = errors(b["ref"], b["exact"], b["ref"])
        assert b["exact"].shape[1] >= 2 and ts.bar("abd", e_ref, scale) < ts.BAR_CAP * scale, (c, e_ref / (EPS * scale))
        assert e_ref < 200 * EPS * scale
    for route, n, g, o0, o1 in ts.B_CASES:
        exact, ref = ts.exact_modes_of(ts.build_case((route, n, g, "uniform", 0.5)))
        e_ref, _, scale = errors(ref, exact, ref)
        assert ts.bar("modes", e_ref, scale) < ts.BAR_CAP * scale


def test_launcher_arithmetic_on_the_case_tables():
    # the backward tile is 96 at every shape of the tables, for any device with two CUs or more
    for cus in (2, 8, 64, 256, 304, 1024):
        for family, name, b in _all_built():
            g0, g1 = ts.launch_rows(b)
            assert (g0, g1) == (0, b["n"]), name  # one chunk on the whole series: the lengths below ARE the launches' rows
            assert ts.backward_tile(b["grid"] ** 2, g1 - g0, cus) == 96, (name, cus)
    assert ts.backward_tile(64 * 21, 100000, 256) != 96  # (the workload's size: the model does leave 96)
    # lengths: the seams of each kernel
    assert [n % 96 for n in ts.N_BACKWARD_96] == [1, 2, 3, 4, 5, 1, 2]
    assert [ts.solve_tiles(n)[:2] for n in ts.N_SOLVE_48] == [(1, 1), (1, 1), (2, 1), (2, 1), (8, 1), (9, 2), (10, 2)]
    assert ts.solve_tiles(81)[2] == 8 and ts.solve_tiles(385)[2] == 16 and 81 == ts.SOLVE_TILE + ts.SOLVE_RUN_IN + 1
    assert [ts.forward_tiles(n) for n in ts.N_FORWARD_320] == [1, 2, 2, 2, 3] and 352 == ts.SPLINE_TILE + ts.SPLINE_HALO
    have = lambda r: {c[1] for c in ts.A_CASES if c[0] == r}  # noqa: E731
    assert set(ts.N_BACKWARD_96) <= have("A1") & have("A4") and set(ts.N_FORWARD_320) <= have("A1") & have("A3'")
    assert set(ts.N_SOLVE_48) <= have("A2") & have("A3") and set(ts.N_GROUPS) <= have("A1") & have("A2") & have("A3") & have("A4")
    assert have("A5'") == set(ts.N_SLOPE) and all(n >= 8 for r in ts.ROUTES if r != "A5'" for n in have(r))
    assert {c[2] for c in ts.A_CASES} == set(ts.GRIDS) and {c[3] for c in ts.A_CASES} == set(ts.AXES)
    assert [(g * g, (g * g + 63) // 64, 64 * ((g * g + 63) // 64) - g * g) for g in ts.GRIDS] == [(49, 1, 15), (81, 2, 47), (225, 4, 31)]
    assert len({ts.case_id(c) for c in ts.A_CASES}) == len(ts.A_CASES)
    # supertranslation sizes: the abscissa window, the ring's overflow, the gather instance
    for c in ts.A_CASES:
        b = ts.build_case(c)
        launches, f, tile = ts.expected_backward_launches(b)
        ra, rb = ts.spread_of(b)
        dt = ts.base_step(c[1])
        full = [v for y, v in enumerate(f) if min(b["n"], (y + 1) * tile) - y * tile >= 2]
        if c[4] == 0.5 and not b["v"].any():
            assert all(full) and rb < dt, c                 # every lane within a sample of its neighbours
        if c[4] == 9.0 and not b["v"].any():
            assert all(full) and rb > ts.RING * dt, c       # the window is used and lanes stand more than RING rows apart
        if c[4] == 30.0:
            assert not any(f) and launches == 1, c          # the gather instance
        if c[4] == 9.0 and b["v"].any():
            assert not all(full) and ra * np.abs(b["t"] - b["tt"]).max() + rb > ts.RING * dt, c  # (the boost adds its rate: tiles at large |t| gather)
    b = ts.build_case(ts.SPLIT_CASE)
    assert ts.expected_backward_launches(b)[:2] == (2, [True, True, True, False, False])  # the early tiles fit, the late ones do not


def test_graded_family_passes_the_guard():
    for c in ts.GRADED:
        route, n, seam, ratio, steps, grow = c
        t = ts.graded_axis(n, seam, ratio, steps, grow)
        var = ts.window_variation(t)
        assert ts.regular_axis(t) and 700 < var < ts.GUARD_RATIO, (c, var)  # under the guard: the tiled recurrences run
        h = np.diff(t)
        lo, hi = (seam - steps, seam) if grow else (seam, seam + steps)
        assert np.allclose(h[lo + 1 : hi] / h[lo : hi - 1], ratio if grow else 1 / ratio) and t[seam] == 0.0
        assert np.allclose(h[:lo], h[0]) and np.allclose(h[hi:], h[-1]) and np.isclose(max(h[0], h[-1]), 0.1)
    assert {c[2] for c in ts.GRADED} == {48, 96, 320}
    assert abs(1.3**25 - 705.6) < 0.1 and abs(1.15**47 - 712.5) < 0.1
    # what the guard does refuse: two more steps of the steeper stretch.  Ratio 1.15 passes at ANY length (47 steps are all a window sees).
    assert not ts.regular_axis(ts.graded_axis(166, 96, 1.3, 27, True)) and ts.regular_axis(ts.graded_axis(166, 96, 1.15, 90, True))


def test_shard_cases_put_a_seam_at_either_end():
    """group B (checked again on the GPU against engine.shard_plan): with ROW_MARGIN rows of halo on either side of the knots its
    outputs read, the shard's buffer holds 96 k rows in one case and 96 k + 1 in the other"""
    for route, n, g, o0, o1 in ts.B_CASES:
        b = ts.build_case((route, n, g, "uniform", 0.5))
        sa, sb = ts.skews(b["alpha"], b["k"], b["gamma"], b["tt"])
        r0, r1 = ts.needed_rows(b["t"], sa, sb, b["tt"], o0, o1)
        assert 0 < r0 and r1 < n and (r1 - r0) % 96 in (0, 1), (route, o0, o1, r0, r1)
    assert {ts.needed_rows_of_case(c) % 96 for c in ts.B_CASES} == {0, 1}
