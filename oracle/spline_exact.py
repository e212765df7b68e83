"""ORACLE (test infrastructure only -- never imported by the product): the not-a-knot cubic spline, its derivatives and its
repeated antiderivatives, and the angular velocity built on its knot slopes, in extended precision (numpy longdouble, the x87
80-bit format: 64-bit significand, eps = 1.08e-19).  Independent of scipy: the rows of the slope system are written out below, the
solve is the Thomas algorithm, every integration is exact for the piecewise cubic.  What scipy's CubicSpline computes in fp64 lies
1e-16 .. 5e-10 from this (tests/test_oracle_spline_exact.py holds the measured distances); the GPU parity tests of the series
calculus measure both the kernels and scipy against it.

Row j of the slope system  a_j s_{j-1} + b_j s_j + c_j s_{j+1} = r_j  (scipy CubicSpline, bc_type="not-a-knot";
h_j = x_{j+1} - x_j, D_j = y_{j+1} - y_j):
    interior : a = h_j, b = 2 (h_{j-1} + h_j), c = h_{j-1}, r = 3 (h_j / h_{j-1}) D_{j-1} + 3 (h_{j-1} / h_j) D_j
    j = 0    : b = h_1, c = h_0 + h_1, r = ((3 h_0 + 2 h_1) h_1 / (d h_0)) D_0 + (h_0^2 / (d h_1)) D_1,  d = h_0 + h_1
    j = n-1  : a = h_{n-3} + h_{n-2}, b = h_{n-3},
               r = (h_{n-2}^2 / (d h_{n-3})) D_{n-3} + ((2 d + h_{n-2}) h_{n-3} / (d h_{n-2})) D_{n-2},  d = h_{n-3} + h_{n-2}
"""
import numpy as np

from .wigner import LM_range

LD = np.longdouble
CLD = np.clongdouble
assert np.finfo(LD).eps < 2e-19, "numpy longdouble is not an extended format on this machine"

MIN_ORDER, MAX_ORDER = -16, 3


def _extended(a):
    a = np.asarray(a)
    return a.astype(CLD if np.iscomplexobj(a) else LD)


def slopes(x, y):
    """Knot slopes s[n, ...] of the not-a-knot cubic spline through (x[n], y[n, ...]); axis 0 is the knot axis."""
    x = _extended(x)
    y = _extended(y)
    n = x.shape[0]
    if x.ndim != 1 or y.shape[0] != n:
        raise ValueError("x is one-dimensional and y carries one row per knot")
    if n < 4:
        raise ValueError("the not-a-knot spline of this module needs at least 4 knots")
    tail = y.shape[1:]
    y = y.reshape(n, -1)
    h = np.diff(x)
    if not np.all(h > 0):
        raise ValueError("knots must be strictly increasing")
    D = np.diff(y, axis=0)
    a = np.zeros(n, dtype=LD)
    b = np.zeros(n, dtype=LD)
    c = np.zeros(n, dtype=LD)
    r = np.zeros_like(y)
    d = h[0] + h[1]
    b[0], c[0] = h[1], d
    r[0] = ((3 * h[0] + 2 * h[1]) * h[1] / (d * h[0])) * D[0] + (h[0] * h[0] / (d * h[1])) * D[1]
    a[1:-1] = h[1:]
    b[1:-1] = 2 * (h[:-1] + h[1:])
    c[1:-1] = h[:-1]
    r[1:-1] = (3 * h[1:] / h[:-1])[:, None] * D[:-1] + (3 * h[:-1] / h[1:])[:, None] * D[1:]
    d = h[-2] + h[-1]
    a[-1], b[-1] = d, h[-2]
    r[-1] = (h[-1] * h[-1] / (d * h[-2])) * D[-2] + ((2 * d + h[-1]) * h[-2] / (d * h[-1])) * D[-1]
    # Thomas: forward elimination, back substitution
    cp = np.zeros(n, dtype=LD)
    m = 1 / b[0]
    cp[0] = c[0] * m
    r[0] *= m
    for j in range(1, n):
        m = 1 / (b[j] - a[j] * cp[j - 1])
        cp[j] = c[j] * m
        r[j] = (r[j] - a[j] * r[j - 1]) * m
    for j in range(n - 2, -1, -1):
        r[j] -= cp[j] * r[j + 1]
    return r.reshape((n,) + tail)


def interval_of(x, u):
    """Index of the last knot <= u, clamped to [0, n - 2]: the interval scipy's PPoly evaluates in (the end intervals extrapolate)."""
    x = _extended(x)
    return np.clip(np.searchsorted(x, _extended(u), side="right") - 1, 0, x.shape[0] - 2)


def _factorial(k):
    f = LD(1)
    for q in range(2, k + 1):
        f *= q
    return f


def evaluate(x, y, x_new, order=0):
    """d^order/dx^order of the spline through (x, y[n, ...]) at x_new[m] for order 0 .. 3; for order -k = -1 .. -16 the k-fold
    antiderivative, every level of which vanishes at x[0].  Returns [m, ...] in extended precision."""
    if not MIN_ORDER <= order <= MAX_ORDER:
        raise ValueError(f"order {order} outside [{MIN_ORDER}, {MAX_ORDER}]")
    x = _extended(x)
    y = _extended(y)
    u = _extended(x_new)
    n = x.shape[0]
    tail = y.shape[1:]
    s = slopes(x, y).reshape(n, -1)
    y = y.reshape(n, -1)
    h = np.diff(x)[:, None]
    # interval j: f(x_j + t) = c0 + c1 t + c2 t^2 + c3 t^3
    Dh = np.diff(y, axis=0) / h
    c0, c1 = y[:-1], s[:-1]
    c3 = (s[:-1] + s[1:] - 2 * Dh) / (h * h)
    c2 = (Dh - s[:-1]) / h - c3 * h
    coef = (c0, c1, c2, c3)
    j = interval_of(x, u)
    t = (u - x[j])[:, None]
    if order >= 0:
        # sum_{p >= order} p! / (p - order)! c_p t^(p - order), by Horner from the top
        out = np.zeros((u.shape[0], y.shape[1]), dtype=y.dtype)
        for p in range(3, order - 1, -1):
            out = out * t + (_factorial(p) / _factorial(p - order)) * coef[p][j]
        return out.reshape((u.shape[0],) + tail)
    k = -order

    def tail_poly(r, w, rows):
        # w^r sum_{p=0}^{3} c_p p! / (p + r)! w^p : the r-fold integral from x_j of the interval's own cubic
        acc = np.zeros_like(coef[0][rows])
        for p in range(3, -1, -1):
            acc = acc * w + (_factorial(p) / _factorial(p + r)) * coef[p][rows]
        return acc * w**r

    # knot values A_r(x_j) of the levels r = 1 .. k: A_r(x_{j+1}) - A_r(x_j) = sum_{q=1}^{r-1} A_{r-q}(x_j) h^q / q! + tail_poly(r, h)
    every = slice(None)
    A = [None] * (k + 1)
    for r in range(1, k + 1):
        inc = tail_poly(r, h, every)
        for q in range(1, r):
            inc = inc + A[r - q][:-1] * (h**q / _factorial(q))
        A[r] = np.concatenate([np.zeros((1, y.shape[1]), dtype=y.dtype), np.cumsum(inc, axis=0)], axis=0)
    out = tail_poly(k, t, j)
    for q in range(k):
        out = out + A[k - q][j] * (t**q / _factorial(q))
    return out.reshape((u.shape[0],) + tail)


def _ladder(l, m):
    return np.sqrt(np.maximum((l - m) * (l + m + 1), 0).astype(LD))  # (0 where m + 1 > l: such a term has no partner mode)


def ldt_ll_omega(t, data, ell_min, ell_max):
    """<Ldt>[n, 3], <LL>[n, 3, 3] and omega = -<LL>^-1 <Ldt> [n, 3] of modes data[n, n_modes] (l = ell_min .. ell_max): the ladder
    formulas of oracle/mode_calculations_ref.py (scri/mode_calculations.py:14-57, 209-313, 403-432) in extended precision, the time
    derivative being the knot slopes of the spline through the modes."""
    f = _extended(data).astype(CLD)
    n, n_modes = f.shape
    lm = LM_range(ell_min, ell_max)
    if lm.shape[0] != n_modes:
        raise ValueError("data does not carry the modes of that ell range")
    fd = slopes(t, f)
    l, m = lm[:, 0].astype(np.int64), lm[:, 1].astype(np.int64)

    def shifted(k):
        # conj(f[:, i + k]) where mode i + k belongs to the same l, else 0
        out = np.zeros_like(f)
        ok = np.nonzero((m + k <= l) & (m + k >= -l))[0]
        out[:, ok] = np.conjugate(f[:, ok + k])
        return out

    up1, up2, dn1, dn2, own = shifted(1), shifted(2), shifted(-1), shifted(-2), np.conjugate(f)
    mL = m.astype(LD)
    Lp = up1 * fd * _ladder(l, m)
    Lm = dn1 * fd * _ladder(l, -m)
    Lz = own * fd * mL
    ldt = np.stack([(0.5 * (Lp.imag + Lm.imag)).sum(axis=1), (-0.5 * (Lp.real - Lm.real)).sum(axis=1), Lz.imag.sum(axis=1)], axis=1)

    has_up, has_dn = (m + 1 <= l).astype(LD), (m - 1 >= -l).astype(LD)
    LpLp = up2 * f * (_ladder(l, m + 1) * _ladder(l, m))
    LpLm = own * f * (_ladder(l, m - 1) * _ladder(l, -m) * has_dn)
    LmLp = own * f * (_ladder(l, -(m + 1)) * _ladder(l, m) * has_up)
    LmLm = dn2 * f * (_ladder(l, -(m - 1)) * _ladder(l, -m))
    LpLz = up1 * f * (_ladder(l, m) * mL)
    LzLp = up1 * f * ((mL + 1) * _ladder(l, m))
    LmLz = dn1 * f * (_ladder(l, -m) * mL)
    LzLm = dn1 * f * ((mL - 1) * _ladder(l, -m))
    LzLz = own * f * (mL * mL)
    LxLx = 0.25 * (LpLp + LmLm + LmLp + LpLm)
    LxLy = -0.25j * (LpLp - LmLm + LmLp - LpLm)
    LxLz = 0.5 * (LpLz + LmLz)
    LyLx = -0.25j * (LpLp - LmLp + LpLm - LmLm)
    LyLy = -0.25 * (LpLp - LmLp - LpLm + LmLm)
    LyLz = -0.5j * (LpLz - LmLz)
    LzLx = 0.5 * (LzLp + LzLm)
    LzLy = -0.5j * (LzLp - LzLm)
    ll = np.zeros((n, 3, 3), dtype=LD)
    ll[:, 0, 0] = LxLx.real.sum(axis=1)
    ll[:, 1, 1] = LyLy.real.sum(axis=1)
    ll[:, 2, 2] = LzLz.real.sum(axis=1)
    ll[:, 0, 1] = ll[:, 1, 0] = ((LxLy + LyLx).real / 2).sum(axis=1)
    ll[:, 0, 2] = ll[:, 2, 0] = ((LxLz + LzLx).real / 2).sum(axis=1)
    ll[:, 1, 2] = ll[:, 2, 1] = ((LyLz + LzLy).real / 2).sum(axis=1)

    # omega = -<LL>^-1 <Ldt> by Cramer's rule
    def det3(M):
        return (M[:, 0, 0] * (M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1])
                - M[:, 0, 1] * (M[:, 1, 0] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 0])
                + M[:, 0, 2] * (M[:, 1, 0] * M[:, 2, 1] - M[:, 1, 1] * M[:, 2, 0]))

    det = det3(ll)
    omega = np.zeros((n, 3), dtype=LD)
    for col in range(3):
        M = ll.copy()
        M[:, :, col] = -ldt
        omega[:, col] = det3(M) / det
    return ldt, ll, omega
