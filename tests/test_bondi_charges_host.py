"""The yardstick of the one-pass Bondi charges (tests/helpers/charge_cases.py) pinned without a GPU: its closed forms against sympy's
exact 3j symbols, its long-double sums against a 50-digit evaluation of the product rule itself, the library's coefficient image
(bms_charge_coefficients, a host routine) against its coefficients, and the whole against the grid product of oracle/bms_charges_ref.py."""
import numpy as np
import pytest

from tests.helpers import charge_cases as cc

LD_EPS = float(np.finfo(cc.LD).eps)  # 2^-63


def _fields(ell_max, n, seed):
    """random fields with every mode a field of that spin has, and a sigma_dot of its own"""
    rng = np.random.default_rng(seed)

    def field(spin):
        a = rng.normal(size=(n, (ell_max + 1) ** 2)) + 1j * rng.normal(size=(n, (ell_max + 1) ** 2))
        a[:, : spin * spin] = 0
        return a

    return cc.axis(n, seed), field(1), field(0), field(2), field(2)


def _rows(ells):
    for l in ells:
        for m in range(-l, l + 1):
            for dl in (-1, 0, 1):
                for mu in (-1, 0, 1):
                    yield l, m, dl, mu


@pytest.mark.parametrize("ells", [range(2, 9), (23, 24)], ids=["l<=8", "l=23,24"])
def test_closed_forms_equal_sympy(ells):
    """every 3j symbol a coefficient is made of, and the coefficient: a few long-double roundings from the exact value"""
    worst = 0.0
    for l, m, dl, mu in _rows(ells):
        l2, M = l + dl, -mu
        m2 = M - m
        symbols = [(l, l2, 1, m, m2, -M), (l, l2, 1, -2, 2, 0), (l, l2, 1, -2, 1, 1)] + ([(l, l, 0, m, -m, 0), (l, l, 0, -2, 2, 0)] if dl == 0 and mu == 0 else [])
        for args in symbols:  # (outside the m ranges both sides are zero)
            exact = cc.LD(str(cc.w3j_sympy(*args).evalf(40)))
            err = abs(float(cc.w3j_closed(*args) - exact))
            worst = max(worst, err / LD_EPS)
            assert err <= 8 * LD_EPS * max(abs(float(exact)), 1e-3), args
        for name in cc.SETS:
            a, b = cc.coefficient(name, l, m, dl, mu, exact=False), cc.coefficient(name, l, m, dl, mu, exact=True)
            assert abs(float(a - b)) <= 16 * LD_EPS * max(abs(float(b)), 1e-3) and (a == 0) == (b == 0), (name, l, m, dl, mu)
    print(f"closed forms against sympy: at most {worst:.2f} x 2^-63")


def _mp_charges(t, psi1, psi2, sigma, sigma_dot, ell_max):
    """the four charges from the product rule itself, every symbol exact (sympy) and every operation with 50 digits (mpmath)"""
    import mpmath as mp
    import sympy

    mp.mp.dps = 50
    to_mp = lambda x: mp.mpf(str(sympy.N(x, 60)))  # noqa: E731
    c = lambda z: mp.mpc(float(z.real), float(z.imag))  # noqa: E731

    def product(a, b_of, s2, L, M, step):
        """(a b)_{LM} for a = sigma (spin 2) and b = bar(x) (s2 = -2) or eth bar(x) (s2 = -1), b_of(l2, m2) its mode"""
        S, total = 2 + s2, mp.mpc(0)
        for l1 in range(2, ell_max + 1):
            for m1 in range(-l1, l1 + 1):
                for l2 in range(max(2, l1 - L), min(ell_max, l1 + L) + 1):
                    m2 = M - m1
                    if abs(m2) > l2:
                        continue
                    w = cc.w3j_sympy(l1, l2, L, m1, m2, -M) * cc.w3j_sympy(l1, l2, L, -2, -s2, S)
                    if w == 0:
                        continue
                    norm = mp.sqrt(mp.mpf((2 * l1 + 1) * (2 * l2 + 1) * (2 * L + 1)) / (4 * mp.pi))
                    total += c(a[step, cc.index(l1, m1)]) * b_of(l2, m2) * norm * to_mp(w) * (-1) ** ((M + S) % 2)
        return total

    def vec(minus, zero, plus):
        return [(minus.real - plus.real) / mp.sqrt(6), (minus.imag + plus.imag) / mp.sqrt(6), zero.real / mp.sqrt(3)]

    out = {k: [] for k in cc.CHARGES}
    for step in range(len(t)):
        bar = lambda x: (lambda l2, m2: (-1) ** (m2 % 2) * mp.conj(c(x[step, cc.index(l2, -m2)])))  # noqa: E731
        eth_bar = lambda x: (lambda l2, m2: mp.sqrt(mp.mpf((l2 + 2) * (l2 - 1)) / 2) * bar(x)(l2, m2))  # noqa: E731
        r4 = mp.sqrt(4 * mp.pi)
        energy = {(L, M): c(psi2[step, cc.index(L, M)]) + product(sigma, bar(sigma_dot), -2, L, M, step) for L, M in ((0, 0), (1, -1), (1, 0), (1, 1))}
        common = {M: c(psi1[step, cc.index(1, M)]) + product(sigma, eth_bar(sigma), -1, 1, M, step) for M in (-1, 0, 1)}
        com = {M: -(common[M] + product(sigma, bar(sigma), -2, 1, M, step) / 2) for M in (-1, 0, 1)}
        u = mp.mpf(float(t[step]))
        out["four_momentum"].append([-energy[0, 0].real / r4] + [-x / r4 for x in vec(energy[1, -1], energy[1, 0], energy[1, 1])])
        out["angular"].append([x / r4 for x in vec(*(1j * common[M] for M in (-1, 0, 1)))])
        out["com"].append([x / r4 for x in vec(*(com[M] for M in (-1, 0, 1)))])
        out["boost"].append([x / r4 for x in vec(*(com[M] + u * energy[1, M] for M in (-1, 0, 1)))])
    return out


@pytest.mark.parametrize("ell_max", [2, 3, 4])
def test_yardstick_equals_a_50_digit_evaluation(ell_max):
    import mpmath as mp

    fields = _fields(ell_max, 3, 10 + ell_max)
    exact = _mp_charges(*fields, ell_max)
    for name, (value, S, n) in cc.sums(*fields, ell_max).items():
        for step in range(3):
            for k in range(value.shape[1]):
                err = abs(mp.mpf(str(value[step, k])) - exact[name][step][k])  # (numpy prints a long double with all its digits)
                assert err <= n[k] * 2.0**-63 * float(S[step, k]), (name, step, k, float(err))


@pytest.mark.parametrize("ell_max", [2, 3, 8, 24])
def test_library_coefficients_equal_the_yardsticks_within_one_rounding(ell_max):
    from scri_amd import engine

    got, ref = engine.charge_coefficients(ell_max), cc.image(ell_max)
    assert got.shape == ref.shape == (20, (ell_max + 1) ** 2)
    assert np.array_equal(got == 0, ref == 0)
    assert np.array_equal(got[19], ref[19].astype(float))
    # one rounding to double of a long-double value that is itself a few 2^-63 from the exact one
    err = np.abs(got.astype(cc.LD) - ref)
    assert np.all(err <= 0.501 * np.spacing(np.abs(got)))
    with pytest.raises(ValueError):
        engine.charge_coefficients(1)


def test_yardstick_against_the_grid_product():
    """oracle/bms_charges_ref.py with the given sigma_dot in the place of its spline derivative, l_max = 4: two double-precision
    evaluations of a product on a 17 x 17 grid stand between the two; 2e-13 of the scale is what tests/test_golden.py grants the oracle"""
    from oracle import bms_charges_ref as ref
    from oracle import wigner

    L = 4
    t, psi1, psi2, sigma, sigma_dot = _fields(L, 7, 1)
    y = cc.yardstick(t, psi1, psi2, sigma, sigma_dot, L)
    energy = ref.trunc(psi2, 1) + ref.multiply(sigma, 2, ref.bar(sigma_dot, 2), -2, 1)
    com_aspect = -(ref._psi1_sigma(psi1, sigma) + 0.5 * wigner.eth_GHP(ref.multiply(sigma, 2, ref.bar(sigma, 2), -2, 1), 0))
    oracle = {"four_momentum": ref.charge_vector_from_aspect(-ref.real(energy)), "angular": ref.angular_momentum(psi1, sigma), "com": ref.com_charge(psi1, sigma),
              "boost": ref.charge_vector_from_aspect(com_aspect + t[:, None] * wigner.eth_GHP(ref.real(energy), 0))[:, 1:]}
    for name, expect in oracle.items():
        distance, scale = float(np.abs(expect - y[name][0]).max()), float(np.abs(expect).max())
        print(f"{name}: {distance:.1e} from the grid product at scale {scale:.1f}")
        assert distance <= 2e-13 * scale
