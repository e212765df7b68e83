"""Yardstick of the Bondi-gauge violations (tests/test_gpu_bondi_constraints.py, pinned without a GPU by tests/test_constraint_yardstick_host.py):
the six relations of scri/asymptotic_bondi_data/constraints.py in numpy's long double, from the same rows bms_bondi_constraints takes,

    v0 = psi0' - eth psi1 - 3 sigma psi2      v3 = psi3 + eth bar(sigma')
    v1 = psi1' - eth psi2 - 2 sigma psi3      v4 = psi4 + bar(sigma'')
    v2 = psi2' - eth psi3 -   sigma psi4      v5 = Im[psi2 + eth^2 bar(sigma) + sigma bar(sigma')]

with the GHP eth (a row of spin s times f = sqrt((l - s)(l + s + 1) / 2), zero for l < |s| or l < |s + 1|, as DeviceModesTimeSeries.eth_GHP
has it), bar(x)_lm = (-1)^(s + m) conj(x_{l, -m}), Im(x) = -i (x - bar x) / 2, and the four products from product_cases.sums with the
kernel's spins.  The derivative rows are inputs: no spline enters a value or a bar.  The diagonal terms are taken as stored, columns below
the spin included; the products never read those.

Bars, derived the way product_cases derives its own (U = 2^-53; K, S_product from product_cases.sums; f the eth factor):
  * v0, v1, v2: (K + 16 + 4) U S, S = |psi'| + f |psi| + c S_product: the product's bar with its weight c = 3, 2, 1, and four roundings for
    the factor, its product with psi, the sum and the difference;
  * v5: (K + 16 + 6) U (S_x + S_x at the mirror column) / 2, S_x = |psi2| + f |bar sigma| + S_product: two factors more, and the mirror;
  * v3: 4 U (|psi3| + f |bar sigma'|): factor (two roundings), product, sum;   v4: 2 U (|psi4| + |bar sigma''|);
  * a norm: sqrt(sum_c bar_c^2) + ((l_max + 1)^2 + 3) U ||v||: the entries' bars through the triangle inequality, then one rounding per
    square, per addition of the sum, and the root.
Derived, not measured."""
import numpy as np

from tests.helpers import product_cases as pc

LD, CLD, U = pc.LD, pc.CLD, pc.U
SPINS = (2, 1, 0, -1, -2, 2)  # psi0 .. psi4, sigma
VIOLATION_SPINS = (2, 1, 0, -1, -2, 0)
ELL_CASES = tuple((ell_max, graded) for ell_max in (2, 3, 8) for graded in (False, True))
STEPS = 65
GARBAGE = 0.37 - 0.21j  # below each spin: of the size of the fields, so that a norm that reads it differently is seen


def eth_factor(ell_max, s):
    """f8 long double [(ell_max + 1)^2]: the GHP eth on a row of spin s"""
    return np.array([np.sqrt(LD((l - s) * (l + s + 1)) / 2) if l >= abs(s) and l >= abs(s + 1) else LD(0) for l in range(ell_max + 1) for _ in range(2 * l + 1)],
                    dtype=LD)


def mirror(ell_max):
    return np.array([pc.index(l, -m) for l in range(ell_max + 1) for m in range(-l, l + 1)])


def sides(fields, psi_dot, sigma_dot, sigma_ddot, ell_max):
    """[(lhs, rhs, bar)] of the six relations, long double: lhs - rhs is the violation, bar its entrywise bar"""
    L = ell_max
    x = [None if f is None else np.array(f, dtype=CLD) for f in fields]
    d = [None if f is None else np.array(f, dtype=CLD) for f in psi_dot]
    sigma = x[5]
    out = []
    for k in range(3):  # psi_k' = eth psi_{k+1} + (3 - k) sigma psi_{k+2}
        P, SP, K = pc.sums(fields[5], 2, L, False, fields[k + 2], -k, L, False, L)
        f, c = eth_factor(L, 1 - k), 3 - k
        out.append((d[k], f * x[k + 1] + c * P, (K + 16 + 4) * U * (np.abs(d[k]) + f * np.abs(x[k + 1]) + c * SP)))
    f = eth_factor(L, -2)
    b = pc.bar(np.array(sigma_dot, dtype=CLD), 2)
    out.append((x[3], -(f * b), 4 * U * (np.abs(x[3]) + f * np.abs(b))))
    b = pc.bar(np.array(sigma_ddot, dtype=CLD), 2)
    out.append((x[4], -b, 2 * U * (np.abs(x[4]) + np.abs(b))))
    P, SP, K = pc.sums(fields[5], 2, L, False, sigma_dot, 2, L, True, L)
    f2, mir, sign = eth_factor(L, -2) * eth_factor(L, -1), mirror(L), pc._sign(L)
    imag = lambda a: -0.5j * (a - sign * np.conj(a[:, mir]))  # noqa: E731
    e2 = f2 * pc.bar(sigma, 2)
    S_x = np.abs(x[2]) + np.abs(e2) + SP
    out.append((imag(x[2]), -imag(e2 + P), (K + 16 + 6) * U * (S_x + S_x[:, mir]) / 2))
    return out


def yardstick(fields, psi_dot, sigma_dot, sigma_ddot, ell_max):
    """([(value, bar)] of the six violations, (norms LD [N, 6], their bars))"""
    v = [(lhs - rhs, bar) for lhs, rhs, bar in sides(fields, psi_dot, sigma_dot, sigma_ddot, ell_max)]
    norms = np.stack([np.sqrt(np.sum(np.abs(value) ** 2, axis=1)) for value, _ in v], axis=1)
    bars = np.stack([np.sqrt(np.sum(bar**2, axis=1)) for _, bar in v], axis=1) + ((ell_max + 1) ** 2 + 3) * U * norms
    return v, (norms, bars)


def norm_ratio(got, value, bar_):
    err = np.abs(np.asarray(got).astype(LD) - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bar_ > 0, err / np.where(bar_ > 0, bar_, 1), np.where(err == 0, 0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- inputs
def fields_case(ell_max, graded=False, n_times=STEPS, garbage=GARBAGE):
    """(t, fields [6, n, (ell_max + 1)^2]): psi2 and sigma the smooth chirps of product_cases.abd_fields, psi0, psi1, psi3, psi4 from
    product_cases.field, `garbage` below each spin"""
    t, psi2, sigma = pc.abd_fields(ell_max, n_times, 40 + ell_max, graded)
    raw = np.empty((6, n_times, (ell_max + 1) ** 2), dtype=complex)
    raw[2], raw[5] = psi2, sigma
    for i in (0, 1, 3, 4):
        raw[i] = 0.05 * pc.field(n_times, SPINS[i], ell_max, 60 + i)
    for i, s in enumerate(SPINS):
        raw[i][:, : s * s] = garbage
    return t, raw


def host_derivatives(t, raw, garbage=GARBAGE):
    """(psi_dot [3], sigma_dot, sigma_ddot) of scipy's cubic spline through the fields, `garbage` below each spin"""
    from scipy.interpolate import CubicSpline

    d = lambda x, order: CubicSpline(t, x, axis=0).derivative(order)(t)  # noqa: E731
    rows = [d(raw[0], 1), d(raw[1], 1), d(raw[2], 1), d(raw[5], 1), d(raw[5], 2)]
    for x, s in zip(rows, (2, 1, 0, 2, 2)):
        x[:, : s * s] = garbage
    return rows[:3], rows[3], rows[4]
