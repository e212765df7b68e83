"""The yardstick of the rotor interpolation: `scri_amd.quaternions.squad` (the project's statement of quaternion.squad) against the
same statement carried out in np.longdouble, on the inputs tests/test_gpu_squad.py gives to the GPU entry bms_squad.

The long-double statement below is the truth both modules measure against.  It reads the float64 rotors and times exactly and repeats
every step of the statement -- interval rule, step ratios of a non-uniform axis, the end rules in their order, the logarithm's zero
vector part below 1e-300, the mirrored last interval -- so its distance from the float64 statement is the float64 statement's rounding
error and nothing else.  Where long double is no wider than 64 significant bits short of 1e-18 (eps >= 1e-18) the module skips.

Inputs (cases()):  the rotor family R(t) = exp(phi z/2) exp(theta y/2) exp(psi z/2), phi = 0.3 t + 0.02 t^2,
theta = 0.4 + 0.1 sin 0.5 t, psi = -0.2 t, formed in long double, rounded to float64 and renormalised;  a uniform axis of step 0.1 and a
graded one, h_j = 0.1 * 10^-(1 + sin(2 pi j / 17)) (steps varying 100-fold);  n = 2, 3, 4, 5, 255, 256, 257, 1025;  the arguments are
every knot, every midpoint, one ulp either side of every knot, 0.3 of an end step beyond each end and 64 seeded random interior
points, once in ascending order and once shuffled.

MEASURED (this module, x86-64 long double), E_ref = max|float64 statement - truth| over all four components, in units of eps:
between 0.8 (n = 2, graded) and 2.9 (n >= 255, uniform) over the sixteen (axis, n) pairs; | |R| - 1 | (numpy.linalg.norm in float64)
between 1.0 and 4.0 eps.  The test asserts
E_ref <= 8 eps and norms within 4 eps of 1, so that the bar of the GPU test, which is a multiple of E_ref, cannot be widened by a
bad reference.

A rotor series whose sign flips half way (sign_flipped()) is NOT an accuracy input: the logarithm of a rotor next to -1 is ill
conditioned, and there the float64 statement itself is 5e3 .. 5e6 eps from this truth.  It is used for finiteness and norms only."""
import functools

import numpy as np
import pytest

from scri_amd import quaternions

LD = np.longdouble
EPS = float(np.finfo(float).eps)
SIZES = (2, 3, 4, 5, 255, 256, 257, 1025)
AXES = ("uniform", "graded")

pytestmark = pytest.mark.skipif(float(np.finfo(LD).eps) >= 1e-18, reason="np.longdouble is not wider than float64 by enough to serve as the truth")


# ------------------------------------------------------------------------------------------------ the statement in long double
def _mul(a, b):
    w1, x1, y1, z1 = np.moveaxis(a, -1, 0)
    w2, x2, y2, z2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=-1)


def _conj(a):
    return a * np.array([1, -1, -1, -1], dtype=LD)


def _norm(a):
    return np.sqrt((a * a).sum(axis=-1))


def _log(q):
    v = q[..., 1:]
    vn, qn = _norm(v), _norm(q)
    angle = np.arctan2(vn, q[..., 0])
    big = vn > 1e-300
    scale = np.where(big, angle / np.where(big, vn, LD(1)), LD(0))
    out = np.empty_like(q)
    out[..., 0] = np.log(np.where(qn > 0, qn, LD(1)))
    out[..., 1:] = v * scale[..., None]
    return out


def _exp(q):
    v = q[..., 1:]
    vn = _norm(v)
    e = np.exp(q[..., 0])
    big = vn > 1e-300
    s = np.where(big, np.sin(vn) / np.where(big, vn, LD(1)), LD(1))
    out = np.empty_like(q)
    out[..., 0] = e * np.cos(vn)
    out[..., 1:] = (e * s)[..., None] * v
    return out


def _slerp(q1, q2, tau):
    return _mul(q1, _exp(_log(_mul(_conj(q1), q2)) * tau[..., None]))


def squad_longdouble(R_in, t_in, t_out):
    """scri_amd.quaternions.squad, line for line, in np.longdouble (n >= 2, m >= 1); returns longdouble [m, 4]"""
    R, t_in, t_out = np.asarray(R_in, dtype=LD), np.asarray(t_in, dtype=LD), np.asarray(t_out, dtype=LD)
    assert R.dtype == LD and R.shape[0] >= 2 and t_out.size
    roll = lambda a, k: np.roll(a, k, axis=0)  # noqa: E731
    i = np.clip(t_in.searchsorted(t_out, side="right") - 1, 0, t_in.size - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        r_next = ((roll(t_in, -1) - t_in) / (t_in - roll(t_in, 1)))[:, None]
        r_after = ((roll(t_in, -1) - t_in) / (roll(t_in, -2) - roll(t_in, -1)))[:, None]
    step = _log(_mul(_conj(R), roll(R, -1)))
    back = _log(_mul(_conj(roll(R, 1)), R))
    ahead = _log(_mul(_conj(roll(R, -1)), roll(R, -2)))
    A = _mul(R, _exp((-step + back * r_next) * LD(0.25)))
    B = _mul(roll(R, -1), _exp((ahead * r_after - step) * LD(-0.25)))
    last_next = _mul(_mul(R[-1], _conj(R[-2])), R[-1])
    A[0] = R[0]
    A[-1] = R[-1]
    B[-2] = R[-1]
    B[-1] = last_next
    R_ip1 = roll(R, -1).copy()
    R_ip1[-1] = last_next
    t_ip1 = roll(t_in, -1).copy()
    t_ip1[-1] = t_in[-1] + (t_in[-1] - t_in[-2])
    tau = (t_out - t_in[i]) / (t_ip1 - t_in)[i]
    return _slerp(_slerp(R[i], R_ip1[i], tau), _slerp(A[i], B[i], tau), 2 * tau * (1 - tau))


# ------------------------------------------------------------------------------------------------ inputs
def axis(kind, n):
    j = np.arange(n - 1)
    h = np.full(n - 1, 0.1) if kind == "uniform" else 0.1 * 10.0 ** (-(1.0 + np.sin(2.0 * np.pi * j / 17.0)))
    return np.concatenate([[0.0], np.cumsum(h)])


def rotors(t):
    """the rotor family at the float64 times t: long-double products, rounded to float64, renormalised"""
    t = np.asarray(t, dtype=LD)
    phi, theta, psi = LD(0.3) * t + LD(0.02) * t * t, LD(0.4) + LD(0.1) * np.sin(LD(0.5) * t), LD(-0.2) * t
    zero = np.zeros_like(t)
    about_z = lambda a: np.stack([np.cos(a / 2), zero, zero, np.sin(a / 2)], axis=-1)  # noqa: E731
    about_y = np.stack([np.cos(theta / 2), zero, np.sin(theta / 2), zero], axis=-1)
    R = _mul(_mul(about_z(phi), about_y), about_z(psi)).astype(float)
    return R / np.linalg.norm(R, axis=1)[:, None]


def arguments(t, seed):
    """ascending: every knot, every midpoint, one ulp either side of every knot, 0.3 of an end step beyond each end, 64 random interior points"""
    rng = np.random.default_rng(seed)
    u = np.concatenate([t, 0.5 * (t[:-1] + t[1:]), np.nextafter(t, -np.inf), np.nextafter(t, np.inf),
                        [t[0] - 0.3 * (t[1] - t[0]), t[-1] + 0.3 * (t[-1] - t[-2])], rng.uniform(t[0], t[-1], 64)])
    return np.sort(u)


def sign_flipped(R):
    """the same rotations with the sign of the second half of the series flipped (finiteness and norms only: see the module docstring)"""
    R = R.copy()
    R[R.shape[0] // 2:] *= -1.0
    return R


@functools.lru_cache(maxsize=None)
def cases():
    """{(axis kind, n): dict(t, R, u ascending, perm, truth longdouble [m, 4] at u, ref float64 statement at u)}: computed once per
    process and shared by this module and tests/test_gpu_squad.py; the arrays are read-only"""
    out = {}
    for k, kind in enumerate(AXES):
        for n in SIZES:
            t = axis(kind, n)
            R = rotors(t)
            u = arguments(t, seed=100 * k + n)
            perm = np.random.default_rng(7000 + 100 * k + n).permutation(u.size)
            case = dict(t=t, R=R, u=u, perm=perm, truth=squad_longdouble(R, t, u), ref=quaternions.squad(R, t, u))
            for a in case.values():
                a.setflags(write=False)
            out[kind, n] = case
    return out


def error(got, truth):
    """max |got - truth| over arguments and components, as a float (the scale of a unit rotor's components is 1)"""
    return float(np.abs(np.asarray(got, dtype=LD) - truth).max())


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("kind", AXES)
@pytest.mark.parametrize("n", SIZES)
def test_float64_statement_is_within_8_eps_of_the_long_double_truth(kind, n):
    c = cases()[kind, n]
    assert c["u"].size == 3 * n + (n - 1) + 2 + 64 and np.all(np.diff(c["t"]) > 0)
    assert np.abs(np.linalg.norm(c["R"], axis=1) - 1).max() <= 2 * EPS
    e_ref = error(c["ref"], c["truth"])
    drift = float(np.abs(np.linalg.norm(c["ref"], axis=1) - 1).max())
    print(f"squad statement {kind} n={n}: E_ref = {e_ref / EPS:.2f} eps, | |R| - 1 | = {drift / EPS:.2f} eps over {c['u'].size} arguments")
    assert np.isfinite(c["ref"]).all()
    assert e_ref <= 8 * EPS
    assert drift <= 4 * EPS
    # the statement does not care about the order of its arguments
    p = c["perm"]
    assert np.array_equal(quaternions.squad(c["R"], c["t"], c["u"][p]), c["ref"][p])


def test_truth_interpolates_and_repeats_the_end_rules():
    """The long-double statement returns the knots' rotors at the knots (tau = 0 exactly), and at n = 2 it is the slerp of the two
    rotors (A_0 = R_0, B_0 = R_1: the two inner slerps coincide, and the outer one multiplies by |a|^(2 s), s <= 1/2, which is 1 to
    within the float64 rounding of the inputs' norms)."""
    for kind in AXES:
        c = cases()[kind, 5]
        at_knots = squad_longdouble(c["R"], c["t"], c["t"])
        assert float(np.abs(at_knots - c["R"].astype(LD)).max()) <= 4 * float(np.finfo(LD).eps)
    c = cases()["graded", 2]
    R, t = c["R"].astype(LD), c["t"].astype(LD)
    u = np.array([0.25, 0.5, 0.75], dtype=LD) * (t[1] - t[0]) + t[0]
    tau = (u - t[0]) / (t[1] - t[0])
    assert float(np.abs(squad_longdouble(R, t, u) - _slerp(R[:1], R[1:], tau)).max()) <= 2 * EPS


def test_sign_flipped_series_is_ill_conditioned_for_the_statement_itself():
    """why that series is not an accuracy input: the float64 statement is thousands of eps from the truth on it, and still finite and
    of unit norm to rounding"""
    c = cases()["uniform", 257]
    R = sign_flipped(c["R"])
    ref = quaternions.squad(R, c["t"], c["u"])
    e_ref = error(ref, squad_longdouble(R, c["t"], c["u"]))
    drift = float(np.abs(np.linalg.norm(ref, axis=1) - 1).max())
    print(f"sign-flipped series: E_ref = {e_ref / EPS:.3g} eps, | |R| - 1 | = {drift / EPS:.3g} eps")
    assert np.isfinite(ref).all() and e_ref > 100 * EPS
