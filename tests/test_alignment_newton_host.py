"""The refinement of the device route of scri_amd.alignment.align2d (a bounded, damped Newton iteration on (dt, dphi) fed by
correlation moments) driven by a numpy moments provider: host logic, no GPU.

The yardstick is never the code under test: the moments are the sums of the module's docstring written out on
scipy's CubicSpline(ta, A)(t + dt, nu), the cost is the direct sum of |A e^{i m dphi} - B|^2, and the optimum it is compared with is the
unchanged host route of align2d, on the six situations of tests/test_alignment.py."""
import numpy as np
import pytest
from scipy.interpolate import CubicSpline

from scri_amd.alignment import align2d

T1, T2 = -50.0, 50.0


class _Modes:
    def __init__(self, t, data, ell_min, ell_max):
        self.t, self.data, self.ell_min, self.ell_max = t, data, ell_min, ell_max

    def copy(self):
        return _Modes(self.t.copy(), self.data.copy(), self.ell_min, self.ell_max)


def _lm(ell_min, ell_max):
    return [(l, m) for l in range(ell_min, ell_max + 1) for m in range(-l, l + 1)]


def _chirp(t, ell_min, ell_max, seed=1):
    rng = np.random.default_rng(seed)
    LM = _lm(ell_min, ell_max)
    amp = rng.normal(size=len(LM)) + 1j * rng.normal(size=len(LM))
    phase = 0.07 * t + 2e-5 * t**2
    return np.stack([a * np.exp(-1j * m * phase) * (1 + 0.001 * t) for a, (l, m) in zip(amp, LM)], axis=1)


def _pair(dt, dphi, ell_min_a=2, ell_max_a=4):
    tb = np.linspace(-150.0, 150.0, 1501)
    ta = np.linspace(-160.0, 170.0, 1400)
    wb = _Modes(tb, _chirp(tb, 2, 4), 2, 4)
    m = np.array([m for _, m in _lm(2, 4)])
    full = _chirp(ta - dt, 2, 4) * np.exp(-1j * m * dphi)
    keep = [i for i, (l, _) in enumerate(_lm(2, 4)) if ell_min_a <= l <= ell_max_a]
    return _Modes(ta, full[:, keep], ell_min_a, ell_max_a), wb


def _residual_pair():
    wa, wb = _pair(1.0, 0.3)
    wb.data = wb.data.copy()
    wb.data[:, 2] += 0.5  # the (2, 0) mode: a residual no offset removes
    return wa, wb


# name -> (the two waveforms, include_modes, n_brute_force_dt of tests/test_alignment.py, the exact (dt, dphi, period of dphi) or None)
SITUATIONS = {
    "offset 3.217 / 1.234": (lambda: _pair(3.217, 1.234), None, 200, (3.217, 1.234, 2 * np.pi)),
    "offset -7.5 / 5.9": (lambda: _pair(-7.5, 5.9), None, 200, (-7.5, 5.9, 2 * np.pi)),
    "no offset": (lambda: _pair(0.0, 0.0), None, 200, (0.0, 0.0, 2 * np.pi)),
    "fewer modes in wa": (lambda: _pair(2.5, 0.7, 2, 3), None, 100, (2.5, 0.7, 2 * np.pi)),
    "m = +-2 only": (lambda: _pair(2.5, 0.7, 2, 3), [(2, 2), (2, -2), (3, 2)], 100, (2.5, 0.7, np.pi)),
    "irremovable (2, 0) residual": (_residual_pair, None, 100, None),
}


class _Problem:
    """The quantities of the module's docstring for one pair, from numpy and scipy alone"""

    def __init__(self, wa, wb, include_modes):
        ell_min, ell_max = max(wa.ell_min, wb.ell_min), min(wa.ell_max, wb.ell_max)
        LM = [lm for lm in _lm(ell_min, ell_max) if include_modes is None or lm in {tuple(x) for x in include_modes}]
        col = lambda w: [l * (l + 1) - w.ell_min**2 + m for l, m in LM]  # noqa: E731
        self.m_of = np.array([m for _, m in LM], dtype=float)
        self.ms = np.unique(self.m_of)
        self.ell_max = ell_max
        rows = (wb.t >= T1) & (wb.t <= T2)
        self.t = wb.t[rows]
        self.B = wb.data[rows][:, col(wb)]
        self.spline = CubicSpline(wa.t, wa.data[:, col(wa)])
        self.w = np.zeros_like(self.t)
        self.w[:-1] += 0.5 * np.diff(self.t)
        self.w[1:] += 0.5 * np.diff(self.t)
        self.N_b = self.w @ np.sum(np.abs(self.B) ** 2, axis=1)
        self.lower, self.upper = max(T1 - T2, wa.t[0] - T1), min(T2 - T1, wa.t[-1] - T2)
        self.calls = 0

    def moments(self, dts, order):
        self.calls += 1
        out = np.zeros((order + 1, len(dts), 1 + 2 * self.ms.size))
        for k, dt in enumerate(dts):
            A = [self.spline(self.t + dt, nu) for nu in range(order + 1)]
            N = [np.abs(A[0]) ** 2, 2 * (A[0].conj() * A[min(1, order)]).real, 2 * (np.abs(A[min(1, order)]) ** 2 + (A[0].conj() * A[min(2, order)]).real)]
            for o in range(order + 1):
                out[o, k, 0] = self.w @ np.sum(N[o], axis=1)
                cross = self.w @ (A[o] * self.B.conj())
                for s, m in enumerate(self.ms):
                    C = cross[self.m_of == m].sum()
                    out[o, k, 1 + 2 * s], out[o, k, 2 + 2 * s] = C.real, C.imag
        return out

    def cost(self, x):
        A = self.spline(self.t + x[0]) * np.exp(1j * self.m_of * x[1])
        return 0.5 * (self.w @ np.sum(np.abs(A - self.B) ** 2, axis=1)) / self.N_b

    def seed(self, n_dt):
        """the brute-force seed of align2d"""
        dts = np.linspace(self.lower, self.upper, n_dt)
        if not np.any(dts == 0.0):
            dts = np.sort(np.append(dts, 0.0))
        dphis = np.linspace(0.0, 2 * np.pi, 2 * self.ell_max + 1, endpoint=False)
        M = self.moments(dts, 0)[0]
        costs = M[:, :1] + self.N_b - 2 * ((M[:, 1::2] + 1j * M[:, 2::2]) @ np.exp(1j * np.outer(dphis, self.ms)).T).real
        i, j = np.unravel_index(np.argmin(costs), costs.shape)
        return dts[i], dphis[j]


@pytest.fixture(scope="module")
def host_optima():
    """the unchanged host route on every situation, once"""
    out = {}
    for name, (make, include, n_dt, _) in SITUATIONS.items():
        wa, wb = make()
        out[name] = align2d(wa, wb, T1, T2, n_brute_force_δt=n_dt, include_modes=include)[2]
    return out


@pytest.mark.parametrize("name", list(SITUATIONS))
def test_refinement_reaches_the_optimum_of_the_host_route(name, host_optima):
    from scri_amd.alignment import _refine

    make, include, n_dt, exact = SITUATIONS[name]
    wa, wb = make()
    P = _Problem(wa, wb, include)
    x0 = P.seed(n_dt)
    P.calls = 0
    x, f, grad, nfev, status, message = _refine(P.moments, P.ms, P.N_b, x0, P.lower, P.upper)
    cost_new, cost_host = P.cost(x), P.cost(host_optima[name].x)
    print(f"{name}: x = {x}, cost {cost_new:.3e} (host route {cost_host:.3e}), {nfev} evaluations, status {status}: {message}")
    assert status == 1 and nfev == P.calls <= 40
    assert P.lower <= x[0] <= P.upper
    assert cost_new <= cost_host * (1 + 1e-9) + 1e-13
    assert abs(f - cost_new) < 1e-12  # the moment form of the cost agrees with the direct sum up to its cancellation
    assert np.all(np.abs(grad) < 1e-9)
    if exact is not None:
        dt, dphi, period = exact
        assert abs(x[0] - dt) < 1e-5
        assert abs((x[1] - dphi + period / 2) % period - period / 2) < 1e-6


@pytest.mark.parametrize("bound", ["lower", "upper"])
def test_a_start_on_the_bound_stays_within_the_bounds(bound):
    from scri_amd.alignment import _refine

    wa, wb = _pair(3.217, 1.234)
    P = _Problem(wa, wb, None)
    seen = []

    def moments(dts, order):
        seen.extend(dts)
        return P.moments(dts, order)

    x, *_ = _refine(moments, P.ms, P.N_b, (getattr(P, bound), 1.0), P.lower, P.upper)
    assert seen and min(seen) >= P.lower and max(seen) <= P.upper  # no evaluation outside, where the spline would extrapolate
    assert P.lower <= x[0] <= P.upper
    # a seed beyond the bound is brought onto it first
    x, *_ = _refine(moments, P.ms, P.N_b, (P.upper + 5.0 if bound == "upper" else P.lower - 5.0, 1.0), P.lower, P.upper)
    assert min(seen) >= P.lower and max(seen) <= P.upper and P.lower <= x[0] <= P.upper


def test_a_window_that_allows_no_offset_moves_the_turn_alone():
    from scri_amd.alignment import _refine

    wa, wb = _pair(0.0, 0.7)
    P = _Problem(wa, wb, None)
    x, f, grad, nfev, status, _ = _refine(P.moments, P.ms, P.N_b, (0.0, 0.5), 0.0, 0.0)
    assert x[0] == 0.0 and status == 1
    assert abs(x[1] - 0.7) < 1e-6 and P.cost(x) < 1e-12
