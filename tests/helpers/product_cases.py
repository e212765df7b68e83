"""Yardstick of the products on Gauss-Legendre rows (tests/test_gpu_mode_product.py, pinned without a GPU by tests/test_mode_product_host.py):
the three sums of bms_mode_product in numpy's long double,
    A_m(theta_j) = sum_l a_lm lambda^sa_lm(theta_j),  B likewise;   G_M(theta_j) = sum_m1 A_m1 B_{M - m1};
    (a b)_{lM} = sum_j 2 pi w_j lambda^S_lM(theta_j) G_M(theta_j),   S = sa + sb,   n = floor((la + lb + lout) / 2) + 1 nodes,
with lambda^s_lm(theta) = sYlm(theta, 0) = (-1)^s sqrt((2 l + 1) / 4 pi) d^l_{m, -s}(theta) from oracle/wigner.wigner_d_chain (EXTENDED: long
double) and the nodes and weights from mpmath at 40 digits.  bar(x)_lm = (-1)^(s + m) conj(x_{l, -m}).

Beside each value stands its bar, derived the way tests/helpers/charge_cases.py derives its own: (K + 16) 2^-53 S.  S is the same triple sum
over magnitudes (|a| |lambda|, |b| |lambda|, |2 pi w lambda_out|), for the supermomenta with the epilogue's terms and weights included; K is
the length of the longest chain of additions behind one output: the l terms of A, the l terms of B, the m1 terms and the n nodes (the
epilogue adds three).  Sixteen roundings cover the tables, the complex products and the closing weights.  Derived, not measured.

Measured on the CPU (tests/test_mode_product_host.py prints them):
  * LAMBDA_ABS_ERROR: the largest absolute error of the long-double recurrence against a 40-digit evaluation of the literal sum for
    d^l_{m', m}: spins -2 .. 2, l <= 8, on the nodes of n = 1, 4, 7, 13, and l = 23, 24 on six of the 37 nodes (spins -2, 0), where the
    recurrence is longest: 4.5e-18 (numpy's long-double chain; the library's own lies within 7e-19).  The table test allows four times it
    beside one rounding of the value.
  * ORACLE_DISTANCE: the largest distance, in units of the bar, of the oracle's double-precision grid route
    (oracle.modes_time_series_ref.grid_multiply, oracle.bms_charges_ref.supermomentum / mass_aspect) from the yardstick on the inputs of the
    GPU tests: 4.75 for grid_multiply, 0.62 for the supermomenta and the mass aspect.  The GPU tests allow the bar plus four times the
    recorded distance where they compare with that route, which carries the roundings of its own grid."""
import functools

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
PI = LD("3.14159265358979323846264338327950288")
U = 2.0**-53
LAMBDA_ABS_ERROR = 4.5e-18
ORACLE_DISTANCE = {"grid_multiply": 4.75, "supermomenta": 0.62}
SUPERMOMENTA = ("bondi_sachs", "moreschi", "geroch", "geroch_winicour", "mass_aspect")
DEFINITIONS = {"bondi_sachs": "Bondi-Sachs", "moreschi": "Moreschi", "geroch": "Geroch", "geroch_winicour": "Geroch-Winicour"}


def index(l, m):
    return l * (l + 1) + m


def n_nodes(la, lb, lout):
    return (la + lb + lout) // 2 + 1


# ---- nodes, weights and tables
@functools.lru_cache(maxsize=None)
def nodes_mp(n, dps=40):
    """(x_j, w_j) of the n-point Gauss-Legendre rule as mpmath numbers, theta ascending (x descending)"""
    import mpmath as mp

    with mp.workdps(dps + 10):
        xs, ws = [], []
        slope = lambda z: n * (z * mp.legendre(n, z) - mp.legendre(n - 1, z)) / (z * z - 1)  # noqa: E731
        for i in range(n):
            x = mp.mpf(0) if 2 * i + 1 == n else mp.cos(mp.pi * (i + mp.mpf(3) / 4) / (n + mp.mpf(1) / 2))
            for _ in range(60 if 2 * i + 1 != n else 0):  # Newton from the Chebyshev guess: quadratic, so 60 steps are far beyond need
                step = mp.legendre(n, x) / slope(x)
                x -= step
                if abs(step) < mp.mpf(10) ** -(dps + 5):
                    break
            dp = slope(x)
            xs.append(+x), ws.append(2 / ((1 - x * x) * dp * dp))
        return tuple(xs), tuple(ws)


def _ld(v):
    import mpmath as mp

    return LD(mp.nstr(v, 30))


@functools.lru_cache(maxsize=None)
def nodes(n):
    """(cos theta_j, w_j) in long double"""
    x, w = nodes_mp(n)
    return np.array([_ld(v) for v in x], dtype=LD), np.array([_ld(v) for v in w], dtype=LD)


@functools.lru_cache(maxsize=None)
def lambda_table(spin, ell_max, n):
    """lambda^spin_lm(theta_j) in long double, [n, (ell_max + 1)^2], zero for l < |spin|"""
    from oracle import wigner

    assert wigner.EXTENDED
    x, _ = nodes(n)
    ra, rb = np.sqrt((1 + x) / 2), np.sqrt((1 - x) / 2)
    out = np.zeros((n, (ell_max + 1) ** 2), dtype=LD)
    for m in range(-ell_max, ell_max + 1):
        d = wigner.wigner_d_chain(m, -spin, ra, rb, ell_max)
        for l in range(max(abs(m), abs(spin)), ell_max + 1):
            out[:, index(l, m)] = (-1) ** (spin % 2) * np.sqrt(LD(2 * l + 1) / (4 * PI)) * d[:, l]
    out.setflags(write=False)
    return out


def lambda_mp(spin, l, m, x, dps=40):
    """lambda^spin_lm at cos(theta) = x (an mpmath number): the literal sum for d^l_{m, -spin}, independent of every recurrence"""
    import mpmath as mp

    with mp.workdps(dps + 10):
        if l < abs(spin) or abs(m) > l:
            return mp.mpf(0)
        ra, rb = mp.sqrt((1 + x) / 2), mp.sqrt((1 - x) / 2)
        a, b = m, -spin  # d^l_{a, b} = sqrt((l+b)!(l-b)!/((l+a)!(l-a)!)) sum_rho C(l+a, rho) C(l-a, l-rho-b) (-1)^rho ra^(2l+a-b-2rho) rb^(2rho-a+b)
        f = mp.factorial
        total = mp.mpf(0)
        for rho in range(max(0, a - b), min(l + a, l - b) + 1):
            total += mp.binomial(l + a, rho) * mp.binomial(l - a, l - rho - b) * (-1) ** rho * ra ** (2 * l + a - b - 2 * rho) * rb ** (2 * rho - a + b)
        d = mp.sqrt(f(l + b) * f(l - b) / (f(l + a) * f(l - a))) * total
        return (-1) ** (spin % 2) * mp.sqrt(mp.mpf(2 * l + 1) / (4 * mp.pi)) * d


# ---- inputs
def bar(x, spin):
    """bar(x)_lm = (-1)^(spin + m) conj(x_{l, -m}) of rows from l = 0"""
    ell_max = int(round(np.sqrt(x.shape[-1]))) - 1
    out = np.empty_like(x)
    for l in range(ell_max + 1):
        for m in range(-l, l + 1):
            out[..., index(l, m)] = (-1) ** ((spin + m) % 2) * np.conj(x[..., index(l, -m)])
    return out


def field(n_times, spin, ell_max, seed, garbage=0.0):
    """c16[n_times, (ell_max + 1)^2]: random modes that drift in time, zero (or `garbage`) below l = |spin|"""
    rng = np.random.default_rng(1000 * seed + 10 * ell_max + spin + 5)
    nm = (ell_max + 1) ** 2
    x = (rng.normal(size=(1, nm)) + 1j * rng.normal(size=(1, nm))) * (1 + 0.1 * np.arange(n_times)[:, None]) * np.exp(0.3j * np.arange(n_times)[:, None] * rng.normal(size=(1, nm)))
    x[:, : min(spin * spin, nm)] = garbage
    return x


def abd_fields(ell_max, n_times, seed, graded=False):
    """(t, psi2, sigma) of an AsymptoticBondiData: smooth chirps on a uniform or a graded time axis"""
    from tests.helpers import charge_cases as cc

    t, _, psi2, sigma, _ = cc.chirp_fields(ell_max, n_times, seed)
    if not graded:  # (chirp_fields is evaluated on its own axis; the fields are smooth functions of the index either way)
        t = np.linspace(2.0, 2.0 + 0.9 * n_times, n_times)
    else:
        t = 2.0 + 0.9 * n_times * (np.arange(n_times) / (n_times - 1.0)) ** 1.5
    return t, psi2, sigma


ELL_CASES = ((2, 2, 0), (2, 2, 2), (2, 2, 4), (3, 2, 2), (2, 3, 5), (4, 4, 1), (5, 3, 4), (8, 8, 8))  # (l_a, l_b, l_out)
SPIN_CASES = ((2, -2), (2, -1), (0, 1), (-2, -1), (2, 2), (-1, -3))
ABD_CASES = tuple((ell_max, graded) for ell_max in (2, 3, 8) for graded in (False, True))
ABD_STEPS = 65


def operands(la, lb, sa, sb, n_times=3, garbage=0.0):
    """the operands of one case of the GPU tests: rows of stored spins sa, sb"""
    return field(n_times, sa, la, 3 * la + lb, garbage), field(n_times, sb, lb, 7 * lb + la + 1, garbage)


def abd_case(ell_max, graded):
    return abd_fields(ell_max, ABD_STEPS, 40 + ell_max, graded)


# ---- the sums
def _clean(x, spin, ell_max):
    x = np.array(x[:, : (ell_max + 1) ** 2], dtype=CLD)
    x[:, : min(spin * spin, x.shape[1])] = 0
    return x


def _theta_sums(x, spin, ell_max, n):
    """(F [N, n, 2 l + 1], the same sum of magnitudes)"""
    lam = lambda_table(spin, ell_max, n)
    F = np.zeros((x.shape[0], n, 2 * ell_max + 1), dtype=CLD)
    SF = np.zeros((x.shape[0], n, 2 * ell_max + 1), dtype=LD)
    for m in range(-ell_max, ell_max + 1):
        cols = [index(l, m) for l in range(max(abs(m), abs(spin)), ell_max + 1)]
        if cols:
            F[:, :, m + ell_max] = x[:, cols] @ lam[:, cols].T.astype(CLD)
            SF[:, :, m + ell_max] = np.abs(x[:, cols]) @ np.abs(lam[:, cols]).T
    return F, SF


def sums(a, spin_a, la, conj_a, b, spin_b, lb, conj_b, lout, n=None):
    """(values CLD [N, (lout + 1)^2], S LD, K): the product, the sum of the terms' magnitudes and the longest chain"""
    sa, sb = (-spin_a if conj_a else spin_a), (-spin_b if conj_b else spin_b)
    S_out = sa + sb
    n = n_nodes(la, lb, lout) if n is None else n
    a = _clean(bar(a[:, : (la + 1) ** 2], spin_a) if conj_a else a, sa, la)
    b = _clean(bar(b[:, : (lb + 1) ** 2], spin_b) if conj_b else b, sb, lb)
    A, SA = _theta_sums(a, sa, la, n)
    B, SB = _theta_sums(b, sb, lb, n)
    _, w = nodes(n)
    lam = lambda_table(S_out, lout, n) * (2 * PI * w)[:, None]
    N = a.shape[0]
    out, S = np.zeros((N, (lout + 1) ** 2), dtype=CLD), np.zeros((N, (lout + 1) ** 2), dtype=LD)
    for M in range(-lout, lout + 1):
        G, SG = np.zeros((N, n), dtype=CLD), np.zeros((N, n), dtype=LD)
        for m1 in range(max(-la, M - lb), min(la, M + lb) + 1):
            G += A[:, :, m1 + la] * B[:, :, M - m1 + lb]
            SG += SA[:, :, m1 + la] * SB[:, :, M - m1 + lb]
        cols = [index(l, M) for l in range(max(abs(M), abs(S_out)), lout + 1)]
        if cols:
            out[:, cols] = G @ lam[:, cols].astype(CLD)
            S[:, cols] = SG @ np.abs(lam[:, cols])
    K = max(la - abs(sa) + 1, 0) + max(lb - abs(sb) + 1, 0) + min(2 * la + 1, 2 * lb + 1) + n
    return out, S, K


def yardstick(a, spin_a, la, conj_a, b, spin_b, lb, conj_b, lout, n=None):
    """(values, bars)"""
    v, S, K = sums(a, spin_a, la, conj_a, b, spin_b, lb, conj_b, lout, n)
    return v, (K + 16) * U * S


def _mirror(lout):
    return np.array([index(l, -m) for l in range(lout + 1) for m in range(-l, l + 1)])


def _sign(lout):
    return np.array([(-1) ** (m % 2) for l in range(lout + 1) for m in range(-l, l + 1)], dtype=LD)


def supermomenta_yardstick(psi2, sigma, sigma_dot, ell_max, lout, integrated=False):
    """{name: (values, bars)} of bms_supermomenta in long double: the product above with psi2 and the diagonal terms"""
    P, SP, K = sums(sigma, 2, ell_max, False, sigma_dot, 2, ell_max, True, lout)
    no = (lout + 1) ** 2
    f = np.array([np.sqrt(LD((l + 2) * (l + 1) * l * (l - 1))) / 2 if l >= 2 else LD(0) for l in range(lout + 1) for _ in range(2 * l + 1)], dtype=LD)
    sg = _clean(sigma, 2, ell_max)[:, :no]
    sb = bar(_clean(sigma, 2, ell_max), 2)[:, :no]
    p2 = np.array(psi2[:, :no], dtype=CLD)
    bs, S_bs = p2 + P, np.abs(p2) + SP
    e2, eb2 = f * sb, f * sg
    raw = {
        "bondi_sachs": (bs, S_bs),
        "moreschi": (bs + e2, S_bs + np.abs(e2)),
        "geroch": (bs + (e2 - eb2) / 2, S_bs + (np.abs(e2) + np.abs(eb2)) / 2),
        "geroch_winicour": (bs - eb2, S_bs + np.abs(eb2)),
    }
    mirror, sign = _mirror(lout), _sign(lout)
    out = {}
    for name, (v, S) in raw.items():
        if integrated:
            v, S = -sign * np.conj(v[:, mirror]) / (2 * np.sqrt(PI)), S[:, mirror] / (2 * np.sqrt(PI))
        out[name] = (v, (K + 3 + 16) * U * S)
    out["mass_aspect"] = (-(bs + sign * np.conj(bs[:, mirror])) / 2, (K + 3 + 16) * U * (S_bs + S_bs[:, mirror]) / 2)
    return out


def ratio(got, value, bar_):
    """the largest |got - value| / bar (an entry whose bar is zero must be exactly zero: inf otherwise)"""
    err = np.abs(np.asarray(got).astype(CLD) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar_ > 0, err / np.where(bar_ > 0, bar_, 1), np.where(err == 0, 0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- the independent exact product: the 3j (Gaunt) sum of tests/helpers/charge_cases.py:5-6 with sympy's wigner_3j at 40 digits
@functools.lru_cache(maxsize=None)
def _w3j(l1, l2, L, m1, m2, m3):
    from sympy.physics.wigner import wigner_3j

    return LD(str(wigner_3j(l1, l2, L, m1, m2, m3).evalf(40)))


def gaunt_product(a, sa, la, b, sb, lb, lout):
    """(values CLD [N, (lout + 1)^2], S) of the product of a (spin sa) and b (spin sb) by the 3j sum, long double"""
    S_out = sa + sb
    a, b = _clean(a, sa, la), _clean(b, sb, lb)
    out, S = np.zeros((a.shape[0], (lout + 1) ** 2), dtype=CLD), np.zeros((a.shape[0], (lout + 1) ** 2), dtype=LD)
    for L in range(abs(S_out), lout + 1):
        for M in range(-L, L + 1):
            for l1 in range(abs(sa), la + 1):
                for l2 in range(max(abs(sb), abs(L - l1)), min(lb, L + l1) + 1):
                    spin_part = _w3j(l1, l2, L, -sa, -sb, S_out)
                    if spin_part == 0:
                        continue
                    for m1 in range(max(-l1, M - l2), min(l1, M + l2) + 1):
                        m2 = M - m1
                        c = np.sqrt(LD((2 * l1 + 1) * (2 * l2 + 1) * (2 * L + 1)) / (4 * PI)) * _w3j(l1, l2, L, m1, m2, -M) * spin_part * (-1) ** ((M + S_out) % 2)
                        out[:, index(L, M)] += c * a[:, index(l1, m1)] * b[:, index(l2, m2)]
                        S[:, index(L, M)] += abs(c) * np.abs(a[:, index(l1, m1)]) * np.abs(b[:, index(l2, m2)])
    return out, S
