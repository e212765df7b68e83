"""The extended-precision reference of the series calculus (oracle/spline_exact.py) against three things it does not share code
with: a 50-digit mpmath spline built from the continuity conditions (no slope system), polynomial calculus (a cubic is its own
not-a-knot spline), and the scipy oracle the rest of the suite trusts.  No GPU.

MEASURED (x86-64, numpy longdouble = 80-bit), relative to max(1, max|f|):
  against mpmath, 12 knots, steps over two decades, orders -16 .. 3: worst 3.2e-18 (bar 1e-17);
  polynomial exactness, 30 knots: value 9.0e-20, antiderivatives 2.4e-18, derivatives 2.8e-18 (bar 1e-17);
  scipy's fp64 distance from the reference on the 1025-knot axes of tests/test_gpu_spline_edges.py (uniform / jittered):
      orders <= 0: 3.6e-15 / 4.8e-15     order 1: 1.3e-15 / 1.5e-15     order 2: 1.5e-13 / 1.9e-13     order 3: 7.4e-12 / 1.5e-11
  SCIPY_FLOOR below holds the bars: four times the largest distances found over uniform, jittered, graded, alternating and
  log-random axes of that length (1e-14, 4e-13, 2e-11, 5e-10); this is the fp64 floor the GPU parity tests measure against."""
import numpy as np
import pytest

from oracle import mode_calculations_ref as mc_ref
from oracle import modes_time_series_ref as mref
from oracle import spline_exact as sx
from tests.helpers import spline_cases as sc

ORDERS = list(range(-16, 4))
# scipy's distance from the extended reference, relative to max(1, max|f|), times four: orders <= 0, 1, 2, 3
SCIPY_FLOOR = {0: 4 * 1e-14, 1: 4 * 4e-13, 2: 4 * 2e-11, 3: 4 * 5e-10}


def _rel(a, b):
    b = np.asarray(b)
    return float(np.abs(np.asarray(a) - b).max() / max(1.0, float(np.abs(b).max())))


# ---------------------------------------------------------------------------------------------------- mpmath
def _mp_spline_levels(mp, x, y, k_max):
    """Per-interval polynomial coefficients (in t = u - x_j) of the not-a-knot spline through (x, y) and of its antiderivatives of
    order 1 .. k_max, each vanishing at x[0]: levels[r][j] is a coefficient list.  The spline comes from the 4 (n - 1) conditions
    on the coefficients themselves -- interpolation at both ends of every interval, f' and f'' continuous at the interior knots,
    f''' continuous at x_1 and x_{n-2} -- solved densely."""
    n = len(x)
    m = n - 1
    h = [x[j + 1] - x[j] for j in range(m)]
    A = mp.zeros(4 * m, 4 * m)
    b = mp.zeros(4 * m, 1)
    row = 0
    for j in range(m):
        A[row, 4 * j] = 1
        b[row] = y[j]
        row += 1
        for p in range(4):
            A[row, 4 * j + p] = h[j] ** p
        b[row] = y[j + 1]
        row += 1
    for j in range(m - 1):
        for p in range(1, 4):
            A[row, 4 * j + p] = p * h[j] ** (p - 1)
        A[row, 4 * (j + 1) + 1] = -1
        row += 1
        A[row, 4 * j + 2] = 2
        A[row, 4 * j + 3] = 6 * h[j]
        A[row, 4 * (j + 1) + 2] = -2
        row += 1
    for j in (0, m - 2):
        A[row, 4 * j + 3] = 1
        A[row, 4 * (j + 1) + 3] = -1
        row += 1
    assert row == 4 * m
    c = mp.lu_solve(A, b)
    levels = [[[c[4 * j + p] for p in range(4)] for j in range(m)]]
    for _ in range(k_max):
        prev, cur, start = levels[-1], [], mp.mpf(0)
        for j in range(m):
            poly = [start] + [prev[j][p] / (p + 1) for p in range(len(prev[j]))]
            cur.append(poly)
            start = mp.polyval(poly[::-1], h[j])
        levels.append(cur)
    return levels


def _mp_eval(mp, x, levels, u, order):
    n = len(x)
    j = 0
    while j < n - 2 and x[j + 1] <= u:
        j += 1
    t = u - x[j]
    if order <= 0:
        return mp.polyval(levels[-order][j][::-1], t)
    poly = levels[0][j]
    for _ in range(order):
        poly = [p * poly[p] for p in range(1, len(poly))] or [mp.mpf(0)]
    return mp.polyval(poly[::-1], t)


def test_agrees_with_a_50_digit_spline():
    from mpmath import mp

    mp.dps = 50
    rng = np.random.default_rng(5)
    # Steps over two decades, 0.16 .. 16, in a shuffled order.  Forming the cubic's upper coefficients from the slopes divides their
    # rounding (1e-19) by h^2, so the shortest step decides what an 80-bit evaluation can promise for order 3 (4e-17 with steps
    # from 0.06), and the Taylor shifts of the high antiderivatives lose digits over the longest (1e-17 with steps to 30 under a
    # signal of full frequency): this range and a signal slowed to 0.3 leave a factor three under the bar on both sides.
    x = sc.axis_from_steps(10.0 ** np.linspace(-0.8, 1.2, 11)[rng.permutation(11)])
    y = sc.signal(0.3 * x, 2, seed=5)
    mid = 0.5 * (x[1:] + x[:-1])
    u = np.concatenate([x, mid, [x[0] - 0.3 * (x[1] - x[0]), x[-1] + 0.3 * (x[-1] - x[-2])], np.nextafter(x[1:-1], -np.inf)])
    xm = [mp.mpf(float(v)) for v in x]
    worst = 0.0
    for col in range(2):
        for part in (np.real, np.imag):
            yc = part(y[:, col])
            levels = _mp_spline_levels(mp, xm, [mp.mpf(float(v)) for v in yc], 16)
            for order in ORDERS:
                got = sx.evaluate(x, yc, u, order)
                want = [_mp_eval(mp, xm, levels, mp.mpf(float(v)), order) for v in u]
                scale = max(1.0, max(abs(float(w)) for w in want))
                err = max(abs(float(mp.mpf(float(g)) + mp.mpf(float(g - np.longdouble(float(g)))) - w)) for g, w in zip(got, want))
                worst = max(worst, err / scale)
                assert err <= 1e-17 * scale, (col, order, err / scale)
    print(f"worst distance from the 50-digit spline: {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- polynomial calculus
def test_cubic_polynomial_calculus_is_exact():
    LD = np.longdouble
    # Knots on multiples of 1/4 and dyadic coefficients: the knot values are exact in the 64-bit significand, so what is measured is
    # the solver and the integration, not the divided differences of rounded data (half an ulp of y over h^2 is 1e-16 for order 2)
    rng = np.random.default_rng(3)
    x = sc.axis_from_steps(rng.choice([0.25, 0.5, 0.75, 1.0], 29))
    x0 = LD(x[0])
    a = [LD(0.75), LD(-0.5), LD(0.125), LD(-0.015625)]  # p(u) = sum a_p (u - x0)^p
    w = x.astype(LD) - x0
    y = sum(a[p] * w**p for p in range(4))
    rng = np.random.default_rng(4)
    u = np.concatenate([x, rng.uniform(x[0] - 0.2, x[-1] + 0.2, 200)])
    v = u.astype(LD) - x0

    def fact(k):
        f = LD(1)
        for q in range(2, k + 1):
            f *= q
        return f

    worst = {"value": 0.0, "anti": 0.0, "deriv": 0.0}
    for order in ORDERS:
        got = sx.evaluate(x, y, u, order)
        if order >= 0:
            want = sum(a[p] * (fact(p) / fact(p - order)) * v ** (p - order) for p in range(order, 4))
        else:
            k = -order
            want = sum(a[p] * (fact(p) / fact(p + k)) * v ** (p + k) for p in range(4))
        rel = _rel(got, want)
        worst["value" if order == 0 else ("anti" if order < 0 else "deriv")] = max(rel, worst["value" if order == 0 else ("anti" if order < 0 else "deriv")])
        assert rel <= 1e-17, (order, rel)
    print("polynomial exactness:", {k: f"{v:.1e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------- scipy
@pytest.mark.parametrize("axis", ["uniform", "jittered"])
def test_scipy_lies_within_its_fp64_floor_of_the_reference(axis):
    n = 1025
    t = sc.uniform_axis(n) if axis == "uniform" else sc.jittered_axis(n)
    y = sc.signal(t, 5)
    rng = np.random.default_rng(6)
    u = np.concatenate([t, 0.5 * (t[1:] + t[:-1]), rng.uniform(t[0] - 0.01, t[-1] + 0.01, 200)])
    worst = {}
    for order in ORDERS:
        rel = _rel(mref.interpolate(t, y, u, order), sx.evaluate(t, y, u, order))
        worst[max(order, 0)] = max(worst.get(max(order, 0), 0.0), rel)
        assert rel <= SCIPY_FLOOR[max(order, 0)], (axis, order, rel)
    print(f"scipy's distance from the reference, {axis}:", {k: f"{v:.1e}" for k, v in worst.items()})


# ---------------------------------------------------------------------------------------------------- angular velocity
def test_angular_velocity_agrees_with_the_fp64_oracle():
    ell_min, ell_max = 2, 8
    n_modes = (ell_max + 1) ** 2 - ell_min**2
    t = sc.jittered_axis(40, seed=8)
    data = sc.signal(t, n_modes, seed=8)
    ldt, ll, om = sx.ldt_ll_omega(t, data, ell_min, ell_max)
    ldt64 = mc_ref.LdtVector(data, mc_ref.data_dot(t, data), ell_min, ell_max)
    ll64 = mc_ref.LLMatrix(data, ell_min, ell_max)
    om64 = mc_ref.angular_velocity(t, data, ell_min, ell_max)
    # <LL>: an fp64 sum of 77 modes x 9 products, each a few eps of the sum of magnitudes; <Ldt> adds scipy's first derivative
    # (SCIPY_FLOOR[1]); omega multiplies both by the condition number of <LL>
    cond = float(np.linalg.cond(ll64).max())
    assert _rel(ll64, ll) <= 77 * 9 * 4 * sc.EPS
    assert _rel(ldt64, ldt) <= SCIPY_FLOOR[1] + 77 * 9 * 4 * sc.EPS
    assert _rel(om64, om) <= cond * (SCIPY_FLOOR[1] + 2 * 77 * 9 * 4 * sc.EPS)
    assert np.allclose(ll, np.swapaxes(ll, 1, 2), rtol=0, atol=0)  # symmetric by construction


def test_angular_velocity_of_a_rotation_about_z_is_along_z():
    # only m = +-2 modes: no ladder operator finds a partner, so the x and y components vanish term by term, whatever the spline's
    # derivative is; the z component is the rotation rate to the spline's truncation error
    ell_min, ell_max, rate = 2, 5, 0.37
    t = np.linspace(0.0, 6.0, 241)
    lm = [(l, m) for l in range(ell_min, ell_max + 1) for m in range(-l, l + 1)]
    rng = np.random.default_rng(9)
    data = np.zeros((t.size, len(lm)), dtype=complex)
    for i, (l, m) in enumerate(lm):
        if abs(m) == 2:
            data[:, i] = (rng.normal() + 1j * rng.normal()) * np.exp(-1j * m * rate * t)
    ldt, ll, om = sx.ldt_ll_omega(t, data, ell_min, ell_max)
    assert np.all(om[:, 0] == 0) and np.all(om[:, 1] == 0)
    assert np.all(ldt[:, :2] == 0) and np.all(ll[:, 0, 2] == 0) and np.all(ll[:, 1, 2] == 0)
    assert float(np.abs(om[:, 2] - rate).max()) < 1e-7  # (h^4 of the spline derivative: (0.025 * 0.74)^4 / 30 ~ 4e-9)
