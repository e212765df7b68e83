"""The products on Gauss-Legendre rows without a GPU: the library's nodes, weights and tables (bms_product_tables, a pure host routine)
against mpmath and the long-double recurrence; the yardstick of tests/helpers/product_cases.py against an independent exact product (the 3j
sum with sympy's wigner_3j); the node rule shown to be tight (one node fewer misses in the first digits); and the distance of the oracle's
double-precision grid route from the yardstick on the inputs of tests/test_gpu_mode_product.py, which that file allows for."""
import numpy as np
import pytest

from tests.helpers import product_cases as pc

U = pc.U
GAUNT_SPINS = ((2, -2), (2, -1), (0, 1), (-2, -1))


def _mpf(v):
    import mpmath as mp

    return mp.mpf(float(v))


def test_nodes_and_weights_within_one_rounding_of_mpmath():
    from scri_amd import engine

    for n in (1, 2, 3, 4, 7, 13, 25, 37, 43):
        x, w, _ = engine.product_tables(0, 0, n)
        xm, wm = pc.nodes_mp(n)
        assert np.all(np.diff(x) < 0) and np.array_equal(x, -x[::-1]) and np.array_equal(w, w[::-1]), n  # theta ascending, mirrored
        for j in range(n):
            assert abs(_mpf(x[j]) - xm[j]) <= 1.001 * U * abs(xm[j]), (n, j)
            assert abs(_mpf(w[j]) - wm[j]) <= 1.001 * U * abs(wm[j]), (n, j)


def test_tables_against_mpmath_and_the_long_double_chain():
    """one rounding of the value plus the recurrence's own absolute error (near a zero of lambda the relative bound means nothing); that
    error is measured here against the literal sum at 40 digits and four times the recorded largest value is allowed"""
    import mpmath as mp

    from scri_amd import engine

    measured = 0.0
    for spin in range(-2, 3):
        for n in (1, 4, 7, 13):
            _, _, table = engine.product_tables(spin, 8, n)
            chain = pc.lambda_table(spin, 8, n)
            xm, _ = pc.nodes_mp(n)
            for j in range(n):
                for l in range(9):
                    for m in range(-l, l + 1):
                        v = pc.lambda_mp(spin, l, m, xm[j])
                        c = pc.index(l, m)
                        with mp.workdps(50):
                            measured = max(measured, float(abs(mp.mpf(np.format_float_scientific(chain[j, c], precision=25)) - v)))
                        assert abs(_mpf(table[j, c]) - v) <= U * abs(v) + 4 * pc.LAMBDA_ABS_ERROR, (spin, n, j, l, m)
    for spin, n in ((-2, 37), (0, 37)):  # where the recurrence is longest: l = 23, 24 on the first, some inner and the last nodes
        _, _, table = engine.product_tables(spin, 24, n)
        chain = pc.lambda_table(spin, 24, n)
        xm, _ = pc.nodes_mp(n)
        for j in (0, 1, 9, 18, 35, 36):
            for l in (23, 24):
                for m in range(-l, l + 1):
                    v = pc.lambda_mp(spin, l, m, xm[j])
                    c = pc.index(l, m)
                    with mp.workdps(50):
                        measured = max(measured, float(abs(mp.mpf(np.format_float_scientific(chain[j, c], precision=25)) - v)))
                    assert abs(_mpf(table[j, c]) - v) <= U * abs(v) + 4 * pc.LAMBDA_ABS_ERROR, (spin, n, j, l, m)
    print(f"long-double recurrence against mpmath, spins -2 .. 2, l <= 8 and l = 23, 24: largest absolute error {measured:.2e} (recorded {pc.LAMBDA_ABS_ERROR:.2e})")
    assert measured <= 4 * pc.LAMBDA_ABS_ERROR
    for spin, ell_max, n in ((2, 16, 25), (-2, 24, 37), (0, 24, 37), (-3, 12, 19), (4, 9, 10), (1, 24, 12)):
        _, _, table = engine.product_tables(spin, ell_max, n)
        chain = pc.lambda_table(spin, ell_max, n)
        assert table.shape == chain.shape and np.all(table[:, : spin * spin] == 0)
        assert np.all(np.abs(table.astype(pc.LD) - chain) <= U * np.abs(chain) + 4 * pc.LAMBDA_ABS_ERROR), (spin, ell_max, n)


def _gaunt_cases():
    for sa, sb in GAUNT_SPINS:
        for la in range(abs(sa), 4):
            for lb in range(abs(sb), 4):
                a, b = pc.operands(la, lb, sa, sb, n_times=2)
                for lout in range(la + lb + 1):
                    yield sa, sb, la, lb, lout, a, b


def test_yardstick_against_the_exact_3j_product_and_the_rule_is_tight():
    """the yardstick's three sums give the 3j (Gaunt) product to a long-double rounding bound of the bar's form, for every l_out up to l_a + l_b;
    with one node fewer they miss it by more than 1e-3 of its scale wherever the product has modes at all (l_out >= |s_a + s_b|: below that both are exact zeros)"""
    tightest, worst = np.inf, 0.0
    for sa, sb, la, lb, lout, a, b in _gaunt_cases():
        exact, S_exact = pc.gaunt_product(a, sa, la, b, sb, lb, lout)
        value, S, K = pc.sums(a, sa, la, False, b, sb, lb, False, lout)
        bound = (K + 16) * 2.0**-64 * (S + S_exact)
        assert np.all(np.abs(value - exact) <= bound), (sa, sb, la, lb, lout)
        worst = max(worst, pc.ratio(value, exact, bound))
        n = pc.n_nodes(la, lb, lout)
        scale = float(np.abs(exact).max())
        if scale == 0.0 or n == 1:
            continue
        fewer, _, _ = pc.sums(a, sa, la, False, b, sb, lb, False, lout, n=n - 1)
        miss = float(np.abs(fewer - exact).max()) / scale
        tightest = min(tightest, miss)
        assert miss > 1e-3, (sa, sb, la, lb, lout, miss)
    print(f"yardstick against the 3j sum: at most {worst:.3f} of the long-double bound; with n - 1 nodes the smallest miss is {tightest:.3f} of the scale")


def test_bar_flag_is_the_bar_of_the_modes():
    a, b = pc.operands(3, 2, 2, 1, n_times=2)
    v1, _ = pc.yardstick(a, 2, 3, True, b, 1, 2, True, 4)
    v2, _ = pc.yardstick(pc.bar(a, 2), -2, 3, False, pc.bar(b, 1), -1, 2, False, 4)
    assert np.array_equal(v1, v2)


def test_distance_of_the_oracle_grid_route_from_the_yardstick():
    """measured, in units of the bar, on the inputs of the GPU tests; the recorded values (product_cases.ORACLE_DISTANCE) are what
    tests/test_gpu_mode_product.py adds four times over where it compares with the oracle's double-precision grid route"""
    from oracle import bms_charges_ref as cref
    from oracle import modes_time_series_ref as mref

    worst = 0.0
    for la, lb, lout in pc.ELL_CASES:
        for sa, sb in pc.SPIN_CASES:
            a, b = pc.operands(la, lb, sa, sb)
            value, bar = pc.yardstick(a, sa, la, False, b, sb, lb, False, lout)
            ref = mref.grid_multiply(a, sa, la, b, sb, lb, la + lb, lout)
            worst = max(worst, pc.ratio(ref, value, bar))
    print(f"oracle grid_multiply: at most {worst:.3f} bars from the yardstick (recorded {pc.ORACLE_DISTANCE['grid_multiply']})")
    assert worst <= pc.ORACLE_DISTANCE["grid_multiply"]
    worst = 0.0
    for ell_max, graded in pc.ABD_CASES:
        t, psi2, sigma = pc.abd_case(ell_max, graded)
        sigma_dot = mref.interpolate(t, sigma, t, 1)
        for integrated in (False, True):
            y = pc.supermomenta_yardstick(psi2, sigma, sigma_dot, ell_max, ell_max, integrated)
            for name, definition in pc.DEFINITIONS.items():
                worst = max(worst, pc.ratio(cref.supermomentum(t, psi2, sigma, definition, integrated=integrated), *y[name]))
        for lout in sorted({ell_max, max(ell_max - 1, 1)}):
            y = pc.supermomenta_yardstick(psi2, sigma, sigma_dot, ell_max, lout)
            worst = max(worst, pc.ratio(cref.mass_aspect(t, psi2, sigma, lout), *y["mass_aspect"]))
    print(f"oracle supermomentum / mass_aspect: at most {worst:.3f} bars from the yardstick (recorded {pc.ORACLE_DISTANCE['supermomenta']})")
    assert worst <= pc.ORACLE_DISTANCE["supermomenta"]


def test_table_export_refuses_bad_arguments():
    from scri_amd import engine

    for spin, ell_max, n in ((5, 4, 3), (0, -1, 3), (0, 4, 0)):
        with pytest.raises(ValueError, match="bms_product_tables"):
            engine.product_tables(spin, ell_max, n)
    assert engine.product_nodes(16, 16, 16) == 25 and engine.product_nodes(2, 3, 5) == 6
