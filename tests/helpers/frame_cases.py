"""Inputs, long-double truths, the tolerance rule and the case tables shared by tests/test_oracle_frame_exact.py (CPU: pins the
truths and bounds every E_ref) and tests/test_gpu_frame_edges.py (the kernels of kernels_frames.hip against them).

The rule is the project's (tests/helpers/spline_cases.py, tests/test_gpu_squad.py).  For one call with result `got`, the long-double
truth `exact` and a float64 reference `ref` that is host code and not the kernel:
    E_got = max|got - exact|,  E_ref = max|ref - exact|,  E_got <= max(F * E_ref, G * eps * scale),
scale = 1 for rotor and axis components and max(1, max|exact|) otherwise (1 / gap for the axis of a matrix with a small gap).  F and G
are set per family from the measured worst ratios (next power of two above twice the worst) under the caps F <= 32, G <= 256, which
are conditions and not measurements.

Long-double quaternion algebra is that of tests/test_squad_statement.py; spline slopes and antiderivatives are oracle/spline_exact.py."""
import functools
import math

import numpy as np

from oracle import spline_exact
from tests import test_squad_statement as st

LD = np.longdouble
EPS = float(np.finfo(float).eps)
F_CAP, G_CAP = 32.0, 256.0
MAX_SUBSTEPS = 1 << 20  # include/scri_amd.h, bms_frame_from_angular_velocity: "an interval is cut into at most 2^20 sub-steps"

# family -> (F, G): the next power of two above twice the worst ratio measured on an MI355X over every call of
# tests/test_gpu_frame_edges.py (its docstring has the figures).
#                        worst E_got / E_ref    worst E_got / (eps scale) where E_ref < 4 eps scale
RULE = {
    "frame": (2.0, 2.0),          # 0.84                   0.76
    "frame_exact": (1.0, 2.0),    # 0.35                   0.65
    "axis": (2.0, 2.0),           # 0.79                   0.55
    "axis_rayleigh": (2.0, 1.0),  # 0.98                   0.47
    "omega": (16.0, 32.0),        # 5.63                   9.73
    "minrot": (4.0, 8.0),         # 1.75                   3.09
    "adjust": (4.0, 4.0),         # 1.33                   1.62
}

mul, conj, norm, qlog, qexp = st._mul, st._conj, st._norm, st._log, st._exp


def error(got, truth):
    return float(np.abs(np.asarray(got, dtype=LD) - truth).max())


def check(family, got, exact, ref, what, scale=None):
    """Assert the rule for one call; prints the figures first (pytest -s shows them).  Returns (E_got, E_ref, scale)."""
    got = np.asarray(got)
    assert got.shape == np.asarray(exact).shape, (what, got.shape, np.asarray(exact).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result"
    F, G = RULE[family]
    assert F <= F_CAP and G <= G_CAP
    e_got, e_ref = error(got, exact), error(ref, exact)
    if scale is None:
        scale = max(1.0, float(np.abs(exact).max()))
    print(f"RULE {family} E_got={e_got / EPS:.3g} eps E_ref={e_ref / EPS:.3g} eps scale={scale:.3g} got/ref={e_got / max(e_ref, 1e-300):.3g} "
          f"got/(eps scale)={e_got / (EPS * scale):.3g} | {what}")
    bar = max(F * e_ref, G * EPS * scale)
    assert e_got <= bar, f"{what}: E_got = {e_got:.3e} > bar {bar:.3e} (E_ref = {e_ref:.3e}, scale = {scale:.3e})"
    return e_got, e_ref, scale


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


# ================================================================================================ A. interval rotors, prefix product
# n -> frame_scan_blocks(n): the scans work in blocks of 256, and one block walks the block totals in chunks of 256
FRAME_SIZES = {4: 1, 5: 1, 63: 1, 64: 1, 65: 1, 255: 1, 256: 1, 257: 2, 511: 2, 512: 2, 513: 3, 65535: 256, 65536: 256, 65537: 257,
               65793: 258, 131072: 512, 131073: 513}
GRADED_FRAME_SIZES = tuple(n for n in FRAME_SIZES if n <= 513) + (65537,)
TOLERANCES = (1e-12, 1.0, 1e-20, 0.0)  # at n = 257: amax = 0.00796, the clamp to 0.2, the clamp to 1e-3, the default (= 1e-12)
EXACT_SIZES = (5, 257, 65537)
R0 = np.array([0.5, -0.1, 0.7, 0.3]) / np.linalg.norm([0.5, -0.1, 0.7, 0.3])
freeze(R0)
# omega_k(s) = 3 (a0 + a1 s + a2 s^2 + a3 s^3), s = (t - t0) / T: three different cubics, |omega| about 3, so |omega| h about 0.3 at
# h = 0.1; the direction goes from (1, -0.4, 0.3) to (0.3, 0.5, 0.7), 1.26 radians apart
OMEGA_CUBICS = np.array([[1.0, -2.0, 0.5, 0.8], [-0.4, 1.5, 0.6, -1.2], [0.3, 0.9, -2.0, 1.5]])
freeze(OMEGA_CUBICS)
# the fixed direction of the exact case: c(t) a is exact in float64 for c a multiple of 2^-20 below 2^30, and |a| = 7/8 exactly
AXIS_DYADIC = np.array([2.0, -3.0, 6.0]) / 8.0


def amax_of(tolerance):
    """the clamp of engine_frames.hip / bms_integrate_angular_velocity, restated"""
    if not tolerance > 0:
        tolerance = 1e-12
    return min(0.2, max(1e-3, 2.0 * tolerance ** 0.2))


def time_axis(kind, n):
    return st.axis(kind, n)


def cubic_omega(t):
    """(omega float64 [n, 3], its analytic time derivative in long double [n, 3]) of the vector cubic at the times t"""
    tl = np.asarray(t, dtype=LD)
    T = tl[-1] - tl[0]
    s = (tl - tl[0]) / T
    a = OMEGA_CUBICS.astype(LD)
    val = 3 * (a[:, 0] + s[:, None] * (a[:, 1] + s[:, None] * (a[:, 2] + s[:, None] * a[:, 3])))
    der = 3 * (a[:, 1] + s[:, None] * (2 * a[:, 2] + s[:, None] * 3 * a[:, 3])) / T
    return val.astype(float), der


def substeps(t, om, tolerance):
    """(m int64 [n - 1], want float64 [n - 1]) by the kernel's own expression in float64: an integer decision, not a rounding"""
    t, om = np.asarray(t, dtype=float), np.asarray(om, dtype=float)
    h = t[1:] - t[:-1]
    nr = np.sqrt(om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1] + om[:, 2] * om[:, 2])
    ratio = np.maximum(nr[:-1], nr[1:]) * h / amax_of(tolerance)
    want = np.ceil(ratio)
    m = np.where(want >= float(MAX_SUBSTEPS), MAX_SUBSTEPS, np.where(want > 1.0, want, 1.0)).astype(np.int64)
    return m, ratio


def clear_of_integers(ratio):
    """distance of wmax h / amax from the nearest integer, the smallest over the intervals (the input condition: >= 1e-9)"""
    return float(np.abs(ratio - np.rint(ratio)).min())


def interval_rotors_longdouble(t, om, tolerance):
    """E[n - 1, 4]: the rule of interval_rotor_kernel restated in long double, all intervals side by side: m sub-steps, two Gauss
    points, one commutator, an exact exponential; cubic coefficients from the long-double knot slopes"""
    m, _ = substeps(t, om, tolerance)
    tl, y = np.asarray(t, dtype=LD), np.asarray(om, dtype=LD)
    s = spline_exact.slopes(t, om)
    h = (tl[1:] - tl[:-1])[:, None]
    y0, s0, s1 = y[:-1], s[:-1], s[1:]
    dd = (y[1:] - y0) / h
    tt = (s0 + s1 - 2 * dd) / h
    c3, c2 = tt / h, (dd - s0) / h - tt
    hs = h / m[:, None].astype(LD)
    root3 = np.sqrt(LD(3))
    g1, g2 = LD(0.5) - root3 / 6, LD(0.5) + root3 / 6
    k1, k2 = hs / 4, root3 / 24 * hs * hs
    E = np.zeros((t.shape[0] - 1, 4), dtype=LD)
    E[:, 0] = 1
    for q in range(int(m.max())):
        ta, tb = (q + g1) * hs, (q + g2) * hs
        wa = y0 + ta * (s0 + ta * (c2 + ta * c3))
        wb = y0 + tb * (s0 + tb * (c2 + tb * c3))
        v = np.zeros_like(E)
        v[:, 1:] = k1 * (wa + wb) + k2 * np.cross(wb, wa)
        E = np.where((q < m)[:, None], mul(qexp(v), E), E)
    return E


def prefix_frame_longdouble(E, R0):
    """R[n, 4]: R_0 = R0, R_j = normalised(E_{j-1} ... E_0 R0), the product by a doubling scan of depth log2 n in long double"""
    P = np.array(E, dtype=LD)
    off = 1
    while off < P.shape[0]:
        nxt = P.copy()
        nxt[off:] = mul(P[off:], P[:-off])  # the later factors on the left
        P, off = nxt, 2 * off
    R = mul(P, np.asarray(R0, dtype=LD)[None, :])
    R = R / norm(R)[:, None]
    return np.concatenate([np.asarray(R0, dtype=LD)[None, :], R], axis=0)


@functools.lru_cache(maxsize=None)
def frame_case(kind, n, tolerance=1e-12):
    """dict(t, om, m, ratio, truth longdouble [n, 4], ref = the host march): computed once per process, read-only"""
    from scri_amd import engine

    t = time_axis(kind, n)
    om, _ = cubic_omega(t)
    m, ratio = substeps(t, om, tolerance)
    truth = prefix_frame_longdouble(interval_rotors_longdouble(t, om, tolerance), R0)
    ref = engine.integrate_angular_velocity(t, om, R0=R0, tolerance=tolerance)
    case = dict(t=t, om=om, m=m, ratio=ratio, truth=truth, ref=ref)
    freeze(*case.values())
    return case


def scalar_cubic(t, C=3.0):
    """c(t_j) = C (1 - 0.8 s + 2.1 s^2 - 1.4 s^3) rounded to multiples of 2^-20 (for C = 3 at most 22 significant bits)"""
    t = np.asarray(t, dtype=float)
    s = (t - t[0]) / (t[-1] - t[0])
    return np.rint(C * (1.0 - 0.8 * s + 2.1 * s * s - 1.4 * s ** 3) * 2.0 ** 20) / 2.0 ** 20


def spline_integral_pairs(t, c, factor=LD(1)):
    """(hi, lo) [n] in long double with hi + lo = `factor` times the integral from t[0] to t[j] of the not-a-knot spline through (t, c): the exact
    integral of each interval's cubic, h (y0 + y1) / 2 + h^2 (s0 - s1) / 12, summed with the compensation of every addition kept
    (Neumaier), so that a running sum of 1e4 is not rounded to the 1e-15 that long double alone would leave it with"""
    tl, y = np.asarray(t, dtype=LD), np.asarray(c, dtype=LD)
    s = spline_exact.slopes(t, c)
    h = tl[1:] - tl[:-1]
    inc = factor * (h * (y[:-1] + y[1:]) / 2 + h * h * (s[:-1] - s[1:]) / 12)
    hi, lo = np.zeros(tl.shape[0], dtype=LD), np.zeros(tl.shape[0], dtype=LD)
    total, comp = LD(0), LD(0)
    for j, x in enumerate(inc):
        nxt = total + x
        comp += (total - nxt) + x if abs(total) >= abs(x) else (x - nxt) + total
        total = nxt
        hi[j + 1], lo[j + 1] = total, comp
    return hi, lo


def commuting_truth(t, c):
    """R[n, 4] = exp(a_hat theta_j / 2) R0, theta_j = |a| times the integral of the spline through c up to t_j, in long double: the
    closed form for omega = c(t) a with a fixed axis a, which owes nothing to the restated rule.  Half the angle, |a| / 2 = 7/16 times
    the integral, comes as a pair hi + lo and the two rotors are multiplied, so that an angle of 1e4 is never rounded to one long double."""
    unit = AXIS_DYADIC.astype(LD) / (LD(7) / 8)

    def rotor(half_angle):  # (cos, sin a_hat) directly: no rotation vector whose rounded length would be the angle
        return np.concatenate([np.cos(half_angle)[:, None], np.sin(half_angle)[:, None] * unit[None, :]], axis=1)

    hi, lo = spline_integral_pairs(t, c, factor=LD(7) / 16)
    R = mul(mul(rotor(hi), rotor(lo)), R0.astype(LD)[None, :])
    R = R / norm(R)[:, None]
    R[0] = R0
    return R


@functools.lru_cache(maxsize=None)
def commuting_case(n):
    """the exact case on the uniform axis: omega = c(t) a exactly in float64 (asserted), truth = the closed form"""
    from scri_amd import engine

    t = time_axis("uniform", n)
    c = scalar_cubic(t)
    om = c[:, None] * AXIS_DYADIC[None, :]
    assert np.array_equal(om.astype(LD), c.astype(LD)[:, None] * AXIS_DYADIC.astype(LD)[None, :])  # (no rounding in the product)
    m, ratio = substeps(t, om, 1e-12)
    case = dict(t=t, om=om, m=m, ratio=ratio, truth=commuting_truth(t, c), ref=engine.integrate_angular_velocity(t, om, R0=R0, tolerance=1e-12))
    freeze(*case.values())
    return case


@functools.lru_cache(maxsize=None)
def capped_case():
    """n = 4, the middle interval of length 1 with |omega| about 9200: wmax h / amax = 1.16e6 > 2^20, so the kernel runs it at
    MAX_SUBSTEPS while the host march takes 1.16e6 steps; the two end intervals (length 1e-3) take about 1100 steps"""
    from scri_amd import engine

    t = np.array([0.0, 1e-3, 1.0 + 1e-3, 1.0 + 2e-3])
    c = np.rint(10400.0 * (1.0 + 0.05 * t - 0.03 * t * t) * 2.0 ** 20) / 2.0 ** 20
    om = c[:, None] * AXIS_DYADIC[None, :]
    assert np.array_equal(om.astype(LD), c.astype(LD)[:, None] * AXIS_DYADIC.astype(LD)[None, :])
    m, ratio = substeps(t, om, 1e-12)
    case = dict(t=t, om=om, m=m, ratio=ratio, truth=commuting_truth(t, c), ref=engine.integrate_angular_velocity(t, om, R0=R0, tolerance=1e-12))
    freeze(*case.values())
    return case


# ================================================================================================ B. Jacobi and the sign scans
N_AXIS = 257
GAPS = (1e-3, 1e-6, 1e-9)
PLANES = ((0, 1), (0, 2), (1, 2))


def lower_symmetric(A):
    """the symmetric matrices whose lower triangle is A's (what numpy.linalg.eigh and the kernel read), in A's type"""
    A = np.asarray(A)
    L = np.tril(A)
    return L + np.swapaxes(np.tril(A, -1), -1, -2)


def eigen_longdouble(A, sweeps=16):
    """(eigenvalues [n, 3], eigenvectors [n, 3, 3] in columns) of the symmetric matrices whose lower triangle is A's, by cyclic Jacobi
    in long double carried to convergence (all matrices side by side; no ordering, no sign convention)"""
    a = lower_symmetric(np.asarray(A, dtype=float)).astype(LD)
    n = a.shape[0]
    V = np.zeros((n, 3, 3), dtype=LD)
    V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            if not (np.abs(a[:, 0, 1]) + np.abs(a[:, 0, 2]) + np.abs(a[:, 1, 2])).any():
                break
            for p, q in PLANES:
                r = 3 - p - q
                apq = a[:, p, q]
                live = apq != 0
                theta = np.where(live, (a[:, q, q] - a[:, p, p]) / (2 * np.where(live, apq, LD(1))), LD(0))
                tn = np.where(live, np.where(theta < 0, LD(-1), LD(1)) / (np.abs(theta) + np.sqrt(theta * theta + 1)), LD(0))
                c = 1 / np.sqrt(tn * tn + 1)
                s = tn * c
                app, aqq = a[:, p, p] - tn * apq, a[:, q, q] + tn * apq
                apr, aqr = c * a[:, p, r] - s * a[:, q, r], s * a[:, p, r] + c * a[:, q, r]
                a[:, p, p], a[:, q, q] = app, aqq
                a[:, p, q] = a[:, q, p] = 0
                a[:, p, r] = a[:, r, p] = apr
                a[:, q, r] = a[:, r, q] = aqr
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p], V[:, :, q] = c[:, None] * vp - s[:, None] * vq, s[:, None] * vp + c[:, None] * vq
    return np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], axis=1), V


def top_longdouble(A):
    """(lambda_top [n], unit eigenvector [n, 3], relative gap to the second eigenvalue [n]) in long double"""
    lam, V = eigen_longdouble(A)
    k = np.argmax(lam, axis=1)
    rows = np.arange(lam.shape[0])
    v = V[rows, :, k]
    v = v / np.sqrt((v * v).sum(axis=1))[:, None]
    srt = np.sort(lam, axis=1)
    top = srt[:, 2]
    with np.errstate(all="ignore"):
        gap = np.where(top != 0, (top - srt[:, 1]) / np.where(top != 0, np.abs(top), LD(1)), LD(0))
    return top, v, gap


def signed_like(v, truth):
    """v with the sign of each row fixed to the truth's"""
    v = np.asarray(v)
    flip = np.sum(v.astype(LD) * truth, axis=1) < 0
    return np.where(flip[:, None], -v, v)


def eigh_axis(A):
    """the float64 reference: numpy.linalg.eigh's eigenvector of the largest eigenvalue (it reads the lower triangle)"""
    return np.linalg.eigh(np.asarray(A, dtype=float))[1][:, :, 2]


def rayleigh_longdouble(A, v):
    a, v = lower_symmetric(np.asarray(A, dtype=float)).astype(LD), np.asarray(v).astype(LD)
    return np.einsum("ni,nij,nj->n", v, a, v) / (v * v).sum(axis=1)


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def _from_spectrum(rng, lam):
    Q = _rotations(rng, lam.shape[0])
    A = np.einsum("nik,nk,njk->nij", Q, lam, Q)
    return lower_symmetric(A)


def _seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) + 7919


@functools.lru_cache(maxsize=None)
def axis_family(name):
    """ll float64 [n, 3, 3] of one accuracy family (read-only).  Names: "generic"; "gap1e-3", "gap1e-6", "gap1e-9"; "plane01", "plane02",
    "plane12" (one non-zero off-diagonal element); "tiny" (one off-diagonal element 1e-20 times the diagonal); "diag0", "diag1",
    "diag2" (diagonal, the largest entry at that place); "zero"; "tie_diag", "tie_rotated" (the two top eigenvalues equal)"""
    n = N_AXIS
    rng = np.random.default_rng(_seed_of(name))
    size = rng.uniform(0.5, 8.0, n)
    if name == "generic" or name.startswith("gap"):
        g = rng.uniform(0.06, 0.6, n) if name == "generic" else np.full(n, float(name[3:]))
        lam = np.stack([rng.uniform(-0.5, 0.7, n), 1.0 - g, np.ones(n)], axis=1) * size[:, None]
        A = _from_spectrum(rng, lam)
    elif name.startswith("plane") or name == "tiny":
        d = np.array([1.0, 2.5, 4.0])[np.argsort(rng.uniform(size=(n, 3)), axis=1)] * size[:, None]
        A = np.zeros((n, 3, 3))
        A[:, 0, 0], A[:, 1, 1], A[:, 2, 2] = d.T
        if name == "tiny":
            plane = rng.integers(0, 3, n)
            e = 1e-20 * size * rng.choice([-1.0, 1.0], n)
        else:
            plane = np.full(n, PLANES.index((int(name[5]), int(name[6]))))
            e = rng.uniform(0.05, 0.5, n) * size * rng.choice([-1.0, 1.0], n)
        for i, (p, q) in enumerate(PLANES):
            A[:, q, p] = A[:, p, q] = np.where(plane == i, e, 0.0)
    elif name.startswith("diag"):
        k = int(name[4])
        A = np.zeros((n, 3, 3))
        for a in range(3):
            A[:, a, a] = size * (4.0 if a == k else 1.0 + ((a - k) % 3))
    elif name == "zero":
        A = np.zeros((n, 3, 3))
    elif name == "tie_diag":
        A = np.zeros((n, 3, 3))
        low = np.arange(n) % 3
        for a in range(3):
            A[:, a, a] = np.where(low == a, 1.0, 4.0) * size
    elif name == "tie_rotated":
        w = rng.normal(size=(n, 3))
        w /= np.linalg.norm(w, axis=1)[:, None]
        A = lower_symmetric(size[:, None, None] * (4.0 * np.eye(3)[None] - 3.0 * w[:, :, None] * w[:, None, :]))
    else:
        raise KeyError(name)
    return freeze(np.ascontiguousarray(A))


ACCURACY_FAMILIES = ("generic", "gap1e-3", "gap1e-6", "gap1e-9", "plane01", "plane02", "plane12", "tiny")


def nominal_gap(name):
    return float(name[3:]) if name.startswith("gap") else None


@functools.lru_cache(maxsize=None)
def axis_truth(name):
    """(lambda_top, v, gap) of axis_family(name) in long double, read-only"""
    return freeze(*top_longdouble(axis_family(name)))


# ---- the sign rule
def continuous_loop(dpa, rough, i_index):
    """the sign rule of scri/mode_calculations.py:316-363, restated: the anchor points along `rough`; going outwards a vector is
    flipped when it is further from its (fixed) neighbour than its own length; all normalised"""
    dpa = np.array(dpa, dtype=float)
    if np.dot(rough, dpa[i_index]) < 0.0:
        dpa[i_index] *= -1
    for i in range(i_index - 1, -1, -1):
        d = dpa[i] - dpa[i + 1]
        if d @ d > dpa[i] @ dpa[i]:
            dpa[i] *= -1
    for i in range(i_index + 1, dpa.shape[0]):
        d = dpa[i] - dpa[i - 1]
        if d @ d > dpa[i] @ dpa[i]:
            dpa[i] *= -1
    return dpa / np.linalg.norm(dpa, axis=1)[:, None]


def assert_neighbour_cosines_clear_of_half(raw):
    cos = np.sum(raw[1:] * raw[:-1], axis=1) / (np.linalg.norm(raw[1:], axis=1) * np.linalg.norm(raw[:-1], axis=1))
    assert np.abs(np.abs(cos) - 0.5).min() >= 0.1, np.abs(np.abs(cos) - 0.5).min()


class UnitVectorLoop:
    """continuous_loop for raw axes that are exactly +-e_k (asserted), where every sum of the rule is exact in float64 whatever its
    order: the comparisons are formed once for both signs of the neighbour, side by side, and a call walks the booleans outwards
    from its anchor.  The same result bit for bit (tests/test_oracle_frame_exact.py compares the two), at a cost that lets the
    longest series be walked from a dozen anchors."""

    def __init__(self, raw):
        raw = np.asarray(raw, dtype=float)
        ones = np.ones(raw.shape[0])
        assert np.array_equal(np.abs(raw).sum(axis=1), ones) and np.array_equal(np.abs(raw).max(axis=1), ones)

        def flips(v, u):  # is v flipped beside +u, beside -u
            vv = np.sum(v * v, axis=1)
            return (np.sum((v - u) ** 2, axis=1) > vv).tolist(), (np.sum((v + u) ** 2, axis=1) > vv).tolist()

        self.raw = raw
        self.fwd = flips(raw[1:], raw[:-1])  # entry i - 1: vector i beside its neighbour i - 1
        self.bwd = flips(raw[:-1], raw[1:])  # entry i: vector i beside its neighbour i + 1

    def __call__(self, rough, i_index):
        n = self.raw.shape[0]
        sign = [1.0] * n
        if float(np.dot(rough, self.raw[i_index])) < 0.0:
            sign[i_index] = -1.0
        (plus, minus), s = self.bwd, sign[i_index]
        for i in range(i_index - 1, -1, -1):
            sign[i] = s = -1.0 if (plus[i] if s > 0 else minus[i]) else 1.0
        (plus, minus), s = self.fwd, sign[i_index]
        for i in range(i_index + 1, n):
            sign[i] = s = -1.0 if (plus[i - 1] if s > 0 else minus[i - 1]) else 1.0
        out = np.asarray(sign)[:, None] * self.raw
        return out / np.linalg.norm(out, axis=1)[:, None]


def continuous_loop_on_unit_vectors(raw, rough, i_index):
    return UnitVectorLoop(raw)(rough, i_index)


@functools.lru_cache(maxsize=None)
def sign_loop(n, quiet=False):
    """the loop on the raw axes of sign_series(n, quiet), its comparisons formed once"""
    return UnitVectorLoop(sign_series(n, quiet)[1])


SIGN_SIZES = (1, 2, 3, 255, 256, 257, 513, 65536, 65537, 65793, 131073)


def sign_anchors(n):
    """0, 1, n - 2, n - 1 and whichever of 255, 256, 65535, 65536, n - 256, n - 257, n - 65536, n - 65537 lie in range: over
    SIGN_SIZES both scans (lengths n - anchor and anchor + 1) have length 1, 256, 257, 65536 and 65537 at least once"""
    wanted = (0, 1, n - 2, n - 1, 255, 256, 65535, 65536, n - 256, n - 257, n - 65536, n - 65537)
    return tuple(sorted({a for a in wanted if 0 <= a < n}))


@functools.lru_cache(maxsize=None)
def sign_series(n, quiet=False):
    """(ll [n, 3, 3] exactly diagonal, raw [n, 3] = e_k of the largest entry).  The place k jumps at random (three steps in ten draw
    a new place) and, wherever the series is long enough, on the last element of every block of 256 and on the first of the next.
    A jump is a CONSTANT map, which forgets whatever was scanned before it, so in such a series no block total ever matters to a
    later block.  quiet=True: one jump only, at step 100 -- every other map is the identity, and the sign fixed at the anchor (or
    at the jump) has to be carried through every block total and every chunk of totals to the far end of the series."""
    rng = np.random.default_rng(3300 + n)
    k = np.zeros(n, dtype=int)
    for i in range(1, n):
        if quiet:
            k[i] = 1 if i >= 100 else 0
        elif i % 256 in (0, 255):
            k[i] = (k[i - 1] + 1 + rng.integers(0, 2)) % 3
        else:
            k[i] = rng.integers(0, 3) if rng.uniform() < 0.3 else k[i - 1]
    ll = np.zeros((n, 3, 3))
    for a in range(3):
        ll[:, a, a] = np.where(k == a, 4.0, 1.0 + ((a - k) % 3))  # 4 at place k, 2 and 3 at the other two
    return freeze(ll, np.eye(3)[k])


@functools.lru_cache(maxsize=None)
def jumpy_series(n=513, seed=21):
    """the construction of test_sign_scan_on_a_jumpy_axis_series (tests/test_gpu_frame_chain.py): a principal axis that jumps by up
    to 49 degrees on a fifth of the steps, half of them turning over as well, eigenvalues 4, 2, 1"""
    rng = np.random.default_rng(seed)
    v = np.empty((n, 3))
    v[0] = [0.0, 0.0, 1.0]
    allowed = np.linspace(0.65, 1.0, 50)
    for i in range(1, n):
        c = rng.choice(allowed) * rng.choice([-1.0, 1.0]) if rng.uniform() < 0.2 else 1.0 - 1e-3 * rng.uniform()
        perp = np.cross(v[i - 1], rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        v[i] = c * v[i - 1] + math.sqrt(max(0.0, 1.0 - c * c)) * perp
        v[i] /= np.linalg.norm(v[i])
    a = np.cross(v, rng.normal(size=3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    b = np.cross(v, a)
    LL = 4.0 * v[:, :, None] * v[:, None, :] + 2.0 * a[:, :, None] * a[:, None, :] + 1.0 * b[:, :, None] * b[:, None, :]
    return freeze(0.5 * (LL + np.swapaxes(LL, 1, 2)))


# ================================================================================================ C. pointwise kernels
POINT_SIZES = (4, 5, 255, 256, 257, 1025)
ITERATIONS = (1, 2, 3)
Z = np.array([0, 0, 0, 1], dtype=LD)
RIGHT = np.array([0.8, -0.2, 0.3, 0.4]) / np.linalg.norm([0.8, -0.2, 0.3, 0.4])
freeze(RIGHT)
TRUNCATE_TOLERANCE = 1e-12
POW2 = 2.0 ** (-math.floor(math.log2(2 * TRUNCATE_TOLERANCE)))  # 2^39, as bms_frame_adjust forms it


def rotor_omega_longdouble(t, R):
    """omega [n, 3] = vector part of 2 Rdot R^-1, Rdot the long-double knot slopes"""
    R = np.asarray(R, dtype=LD)
    return 2 * mul(spline_exact.slopes(t, R), conj(R))[:, 1:]


def minimal_rotation_longdouble(t, R, iterations):
    """quaternions.minimal_rotation in long double: slopes and the antiderivative from oracle/spline_exact.py"""
    R = np.asarray(R, dtype=LD)
    for _ in range(iterations):
        hgd = mul(mul(spline_exact.slopes(t, R), Z[None, :]), conj(R))[:, 0]
        hg = spline_exact.evaluate(t, hgd, t, order=-1)
        zero = np.zeros_like(hg)
        R = mul(R, np.stack([np.cos(hg), zero, zero, np.sin(hg)], axis=1))
    return R


@functools.lru_cache(maxsize=None)
def rotor_case(kind, n):
    """dict(t, R, om_truth, om_ref, min_truth {iterations: .}, min_ref {iterations: .}); the references are the scipy statements of
    scri_amd.quaternions on the host"""
    from scri_amd import quaternions as Q

    t = time_axis(kind, n)
    R = st.rotors(t)
    case = dict(t=t, R=R, om_truth=rotor_omega_longdouble(t, R), om_ref=Q.angular_velocity(R, t),
                min_truth={it: freeze(minimal_rotation_longdouble(t, R, it)) for it in ITERATIONS},
                min_ref={it: freeze(Q.minimal_rotation(R, t, iterations=it)) for it in ITERATIONS})
    freeze(*case.values())
    return case


@functools.lru_cache(maxsize=None)
def adjust_frame(n):
    """rotors of the family with norms between 0.5 and 1.5: the normalisation of frame_adjust has something to do"""
    R = st.rotors(time_axis("uniform", n)) * (1.0 + 0.5 * np.sin(1.7 * np.arange(n)))[:, None]
    return freeze(R)


def adjust_longdouble(frame, right):
    """normalised(frame * right) in long double (right None: the frame alone)"""
    q = np.asarray(frame, dtype=LD)
    if right is not None:
        q = mul(q, np.asarray(right, dtype=LD)[None, :])
    return q / norm(q)[:, None]


def adjust_reference(frame, right):
    """the same on the host in float64 (scri_amd.quaternions.multiply, numpy's norm)"""
    from scri_amd import quaternions as Q

    q = np.array(frame, dtype=float) if right is None else Q.multiply(frame, np.asarray(right, dtype=float))
    return q / np.linalg.norm(q, axis=1)[:, None]
