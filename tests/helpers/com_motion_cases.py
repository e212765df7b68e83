"""Shared by tests/golden/make_golden_com_motion.py, tests/test_com_motion_host.py and tests/test_gpu_com_motion.py: seeded tracks, the
stand-in tables of a horizons / matter file, and the EXACT value (rationals) of what estimate_avg_com_motion computes -- scipy 1.15's
irregular composite Simpson rule over samples i_i .. i_f of the fp64 integrands com, fl(t com), fl(fl(t t) com), and the closed-form
minimiser from those moments and the fp64 t_i, t_f."""
from fractions import Fraction

import numpy as np

EPS = Fraction(1, 2**52)

A_MASS, A_CENTER = "AhA.dir/ChristodoulouMass.dat", "AhA.dir/CoordCenterInertial.dat"
B_MASS, B_CENTER = "AhB.dir/ChristodoulouMass.dat", "AhB.dir/CoordCenterInertial.dat"
NS1, NS2 = "InertialCenterOfMassNS1.dat", "InertialCenterOfMassNS2.dat"


def dyadic_axis(n, start, seed):
    """n times from `start` with steps that are small integer multiples of 2^-6"""
    rng = np.random.default_rng(seed)
    return float(start) + np.concatenate([[0.0], np.cumsum(rng.integers(1, 9, size=n - 1) / 64.0)])


def graded_axis(n, start, seed):
    """n times from `start` with generic steps growing about tenfold along the axis"""
    rng = np.random.default_rng(seed)
    steps = np.geomspace(0.05, 0.5, n - 1) * rng.uniform(0.8, 1.25, size=n - 1)
    return float(start) + np.concatenate([[0.0], np.cumsum(steps)])


def track(t, seed):
    """a drifting centre of mass with an orbital wobble, [n, 3]"""
    rng = np.random.default_rng(seed)
    s = t - t[0]
    x0, v0 = rng.normal(size=3) * 1e-2, rng.normal(size=3) * 1e-5
    phase = 0.3 * s + 1e-4 * s**2
    wobble = 1e-3 * np.stack([np.cos(phase), np.sin(phase), 0.1 * np.cos(phase + 0.4)], axis=1)
    return x0 + v0 * s[:, None] + wobble + 1e-6 * rng.normal(size=(t.size, 3))


def window(t, skip_beginning_fraction, skip_ending_fraction):
    """(t_i, t_f, i_i, i_f) by the rule of the issue: fp64 arithmetic, numpy's argmin"""
    t_i = t[0] + (t[-1] - t[0]) * skip_beginning_fraction
    t_f = t[-1] - (t[-1] - t[0]) * skip_ending_fraction
    return t_i, t_f, int(np.argmin(np.abs(t - t_i))), int(np.argmin(np.abs(t - t_f)))


def fractions_for_window(t, i_i, i_f):
    """skip fractions whose t_i, t_f fall next to samples i_i and i_f"""
    span = t[-1] - t[0]
    return (t[i_i] - t[0]) / span, (t[-1] - t[i_f]) / span


def _quotient(a, b):
    return a / b if b != 0 else Fraction(0)


def exact_moments(t, com, i_i, i_f):
    """C_k[component] for k = 0, 1, 2 as Fractions"""
    t = np.asarray(t, dtype=float)
    com = np.asarray(com, dtype=float)
    ys = [com[i_i : i_f + 1], (t[:, None] * com)[i_i : i_f + 1], (t[:, None] ** 2 * com)[i_i : i_f + 1]]
    T = [Fraction(float(x)) for x in t[i_i : i_f + 1]]
    N = len(T)
    weights = [Fraction(0)] * N
    if N == 2:
        weights[0] = weights[1] = (T[1] - T[0]) / 2
    else:
        for j in range(0, (N - 1) // 2 * 2, 2):
            h0, h1 = T[j + 1] - T[j], T[j + 2] - T[j + 1]
            hsum, r01 = h0 + h1, _quotient(h0, h1)
            weights[j] += hsum / 6 * (2 - _quotient(Fraction(1), r01))
            weights[j + 1] += hsum / 6 * (hsum * _quotient(hsum, h0 * h1))
            weights[j + 2] += hsum / 6 * (2 - r01)
        if N % 2 == 0:
            h0, h1 = T[-2] - T[-3], T[-1] - T[-2]
            weights[-1] += _quotient(2 * h1**2 + 3 * h0 * h1, 6 * (h1 + h0))
            weights[-2] += _quotient(h1**2 + 3 * h0 * h1, 6 * h0)
            weights[-3] -= _quotient(h1**3, 6 * h0 * (h0 + h1))
    return [[sum(w * Fraction(float(y)) for w, y in zip(weights, ys[k][:, c])) for c in range(3)] for k in range(3)]


def exact_fit(moments, t_i, t_f, fit_acceleration):
    """(x_i, v_i, a_i) as lists of three Fractions from the exact moments and the fp64 window ends"""
    a, b = Fraction(float(t_i)), Fraction(float(t_f))
    d = b - a
    x, v, g = [], [], []
    for c in range(3):
        C0, C1, C2 = moments[0][c], moments[1][c], moments[2][c]
        if fit_acceleration:
            x.append(3 * (C0 * (3 * b**4 + 12 * b**3 * a + 30 * b**2 * a**2 + 12 * b * a**3 + 3 * a**4)
                          - 12 * C1 * (b + a) * (b**2 + 3 * b * a + a**2) + C2 * (10 * b**2 + 40 * b * a + 10 * a**2)) / d**5)
            v.append(12 * (-3 * C0 * (b + a) * (b**2 + 3 * b * a + a**2) + C1 * (16 * b**2 + 28 * b * a + 16 * a**2) - 15 * C2 * (b + a)) / d**5)
            g.append(60 * (C0 * (b**2 + 4 * b * a + a**2) - 6 * C1 * (b + a) + 6 * C2) / d**5)
        else:
            x.append(2 * (C0 * (2 * b**3 - 2 * a**3) + C1 * (3 * a**2 - 3 * b**2)) / d**4)
            v.append(6 * (2 * C1 - C0 * (a + b)) / d**3)
            g.append(Fraction(0))
    return x, v, g


def distance(values, exact):
    """max over the components of |value - exact| as a Fraction"""
    return max(abs(Fraction(float(val)) - e) for val, e in zip(values, exact))


def bar(exact):
    """4 eps max_component |exact|: the final rounding of a correctly rounded result, with room for the hi + lo conversions"""
    return 4 * EPS * max(abs(e) for e in exact)


def table(t, columns):
    """a `[time, ...]` table as the files hold them"""
    return np.column_stack([t, columns])


def horizons_of_track(t, com):
    """horizon tables whose mass-weighted centre is `com` exactly: both holes on the track, unit masses"""
    one = np.ones_like(t)
    return {A_MASS: table(t, one), A_CENTER: table(t, com), B_MASS: table(t, one), B_CENTER: table(t, com)}


# fit cases of g31: name -> (t, skip_beginning_fraction, skip_ending_fraction); the track is track(t, seed = 100 + position)
def fit_cases():
    cases = {}
    for n in (2, 3, 4, 5):
        cases[f"whole_{n}_from_5000"] = (graded_axis(n, 5000.0, 10 + n), 0.0, 0.0)
        cases[f"whole_{n}_from_0"] = (graded_axis(n, 0.0, 20 + n), 0.0, 0.0)
    cases["graded_600_from_5000"] = (graded_axis(600, 5000.0, 31), 0.0, 0.0)
    cases["graded_599_from_5000"] = (graded_axis(599, 5000.0, 32), 0.0, 0.0)
    cases["default_fractions_500_from_0"] = (graded_axis(500, 0.0, 33), 0.01, 0.10)
    cases["default_fractions_501_from_5000"] = (graded_axis(501, 5000.0, 34), 0.01, 0.10)
    t = graded_axis(101, 5000.0, 35)
    t[41] = t[40]
    cases["repeated_time"] = (t, 0.0, 0.05)
    # a uniform dyadic axis and fractions that land halfway between two samples: t_i = 0.625, t_f = 15.125
    cases["argmin_tie"] = (np.arange(65) * 0.25, 5.0 / 128.0, 7.0 / 128.0)
    return cases


def fit_case_track(position, t):
    return track(t, 100 + position)


# ---- inputs of g31's com_motion and PN cases


def track_inputs():
    """tables and masses of the com_motion cases, by case name: (horizons or None, matter or None, m_A, m_B)"""
    rng = np.random.default_rng(7)
    n = 300
    t = graded_axis(n, 100.0, 41)
    xa, xb = track(t, 42) + [5.0, 0.0, 0.0], track(t, 43) - [4.0, 0.0, 0.0]
    ma, mb = 0.6 + 1e-6 * rng.normal(size=n), 0.4 + 1e-6 * rng.normal(size=n)
    horizons = {A_MASS: table(t, ma), A_CENTER: table(t, xa), B_MASS: table(t, mb),
                B_CENTER: table(t, xb)}
    long_t = np.concatenate([t, t[-1] + 0.5 * np.arange(1, 8)])
    long_horizons = {A_MASS: table(long_t, 0.6 + 1e-6 * rng.normal(size=n + 7)),
                     A_CENTER: table(long_t, track(long_t, 44))}
    return {
        "bbh": (horizons, None, None, None),
        "nsns": (None, {NS1: table(t, xa), NS2: table(t, xb)}, 1.35, 1.42),
        "bhns_longer_horizons": (long_horizons, {NS1: table(t, xb)}, None, 1.4),
        "bhns_given_mass": (horizons, {NS1: table(t, xb)}, 5.6, np.full(n, 1.4) + 1e-7 * rng.normal(size=n)),
    }


def error_inputs():
    t = np.arange(5.0)
    x = np.arange(15.0).reshape(5, 3)
    hz = {A_MASS: table(t, np.ones(5)), A_CENTER: table(t, x)}
    shifted = t + [0.0, 0.0, 0.25, 0.0, 0.5]
    return {
        "nsns_times_differ": (None, {NS1: table(t, x), NS2: table(shifted, x)}, 1.0, 1.0),
        "nsns_no_masses": (None, {NS1: table(t, x), NS2: table(t, x)}, None, 1.0),
        "bhns_horizons_shorter": ({k: v[:4] for k, v in hz.items()}, {NS1: table(t, x)}, None, 1.0),
        "bhns_times_differ": (hz, {NS1: table(shifted, x)}, None, 1.0),
        "bhns_no_star_mass": (hz, {NS1: table(t, x)}, None, None),
        "matter_without_stars": (hz, {"Other.dat": table(t, x)}, None, None),
    }


def pn_inputs():
    rng = np.random.default_rng(11)
    n = 64
    t = np.linspace(-300.0, -100.0, n)
    omega = np.stack([1e-3 * rng.normal(size=n), 1e-3 * rng.normal(size=n), 0.02 + 1e-4 * (t - t[0])], axis=1)
    modes = (rng.normal(size=(n, 21)) + 1j * rng.normal(size=(n, 21))) * 0.01
    modes[:, 3] = 0.05 * np.exp(-1j * (0.04 * (t - t[0]) + 5e-5 * (t - t[0]) ** 2 + 0.3))  # (2, 1): a phase that winds a few times
    return dict(pn_t=t, pn_omega=omega, pn_modes=modes, pn_m=np.float64(1.3), pn_nu=np.float64(0.21), pn_theta=rng.normal(size=8) * 1e-3)
