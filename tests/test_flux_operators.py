"""The reference's flux building blocks as scri_amd.flux mirrors them (scri/flux.py:11-179, 213-300, 345-391), without a GPU: the
generators against the reference's own triplets (tests/golden/g32_ref_flux_operators.npz, made by make_golden_flux_operators.py), their
caching, the checks of matrix_expectation_value, and the coefficient tables the fused kernel reads (bms_flux_coefficients, a host
routine) against the same combination of the generators' triplets in extended precision."""
import functools
import json
import os

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANGES = ((2, 2), (2, 3), (3, 5), (2, 8))
OPERATORS = ("p_z", "p_plus", "p_minus", "j_z", "j_plus", "j_minus")
SPINS = (-1, -2, -3)
# A value of the reference is a product of a few correctly rounded square roots of exact rationals, each factor within 2^-53 of exact
# and each product adding 2^-53; the package's value is the exact one rounded once.  Eight roundings bound the difference.
VALUE_BOUND = 8 * 2.0**-53


@pytest.fixture(scope="module")
def g32():
    return np.load(os.path.join(G, "g32_ref_flux_operators.npz"), allow_pickle=False)


def reference_triplets(g, lmin, lmax):
    """{(operator name, s or None): (rows, columns, values)} of fixture (a)"""
    tag = f"{lmin}_{lmax}"
    counts, index = g[f"a_{tag}_counts"], g[f"a_{tag}_index"]
    edges = np.concatenate([[0], np.cumsum(counts)])
    out, p_total = {}, int(edges[3])
    for k, name in enumerate(OPERATORS):
        rows, columns = index[0, edges[k]:edges[k + 1]], index[1, edges[k]:edges[k + 1]]
        if k < 3:
            for i, s in enumerate(SPINS):
                out[(name, s)] = (rows, columns, g[f"a_{tag}_p_values"][i, edges[k]:edges[k + 1]])
        else:
            out[(name, None)] = (rows, columns, g[f"a_{tag}_j_values"][edges[k] - p_total:edges[k + 1] - p_total])
    return out


@pytest.mark.parametrize("lmin,lmax", RANGES)
def test_generators_equal_the_reference(g32, lmin, lmax):
    from scri_amd import flux

    worst = 0.0
    for (name, s), (rows, columns, values) in reference_triplets(g32, lmin, lmax).items():
        got = getattr(flux, name)(lmin, lmax) if s is None else getattr(flux, name)(lmin, lmax, s=s)
        assert np.array_equal(got[0], rows) and np.array_equal(got[1], columns), (name, s)
        assert got[0].dtype == np.dtype(int) and got[2].dtype == values.dtype and got[2].shape == values.shape, (name, s)
        err = np.abs(got[2] - values)
        assert np.all(err <= VALUE_BOUND * np.abs(values)), (name, s, (err / np.maximum(np.abs(values), 1e-300)).max() / 2.0**-53)
        nz = values != 0
        if nz.any():
            worst = max(worst, (err[nz] / np.abs(values[nz])).max())
    print(f"l = {lmin}..{lmax}: largest relative difference {worst / 2.0**-53:.2f} x 2^-53 (bound 8)")


def test_repeated_calls_return_the_cached_object():
    from scri_amd import flux

    for gen, kw in ((flux.p_z, dict(s=-3)), (flux.p_plus, dict(s=-1)), (flux.p_minus, {}), (flux.j_z, {}), (flux.j_plus, {}), (flux.j_minus, {})):
        assert gen(2, 4, **kw) is gen(2, 4, **kw)
    assert flux.p_plusminus(2, 3, 1) is flux.p_plusminus(2, 3, 1) and flux.j_plusminus(2, 3, -1) is flux.j_plusminus(2, 3, -1)
    assert flux.p_z.__name__ == "p_z" and "cos(theta)" in flux.p_z.__doc__
    with pytest.raises(ValueError, match="sign must be either 1 or -1"):
        flux.p_plusminus(2, 3, 0)
    with pytest.raises(ValueError, match="sign must be either 1 or -1"):
        flux.j_plusminus(2, 3, 2)

    @flux.swsh_indices_to_matrix_indices
    def identity(ell_min, ell_max):
        for ell in range(ell_min, ell_max + 1):
            for m in range(-ell, ell + 1):
                yield ell, m, ell, m, 1.0

    rows, columns, values = identity(1, 2)
    assert np.array_equal(rows, np.arange(8)) and np.array_equal(columns, np.arange(8)) and np.array_equal(values, np.ones(8))
    assert identity(1, 2) is identity(1, 2)


def test_the_names_are_exported():
    import scri_amd
    from scri_amd.flux import (swsh_indices_to_matrix_indices, p_z, p_plusminus, p_plus, p_minus, j_z, j_plusminus, j_plus, j_minus,  # noqa: F401
                               sparse_expectation_value, matrix_expectation_value)

    for name in ("swsh_indices_to_matrix_indices", "p_z", "p_plusminus", "p_plus", "p_minus", "j_z", "j_plusminus", "j_plus", "j_minus",
                 "sparse_expectation_value", "matrix_expectation_value"):
        assert getattr(scri_amd, name) is getattr(scri_amd.flux, name)


def _waveform(t, lmin, lmax, data_type, seed=1):
    import scri_amd
    from scri_amd import synthetic

    return scri_amd.WaveformModes(t=t, data=synthetic.chirp_modes(t, lmin, lmax, seed), ell_min=lmin, ell_max=lmax, dataType=data_type,
                                  frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True)


def test_matrix_expectation_value_refuses_with_the_reference_texts(g32):
    """every refusal comes before anything is computed: no device is needed"""
    import scri_amd
    from scri_amd import flux

    texts = json.loads(str(g32["c_errors_json"]))
    ta, tb = g32["c_ta"], g32["c_tb"]
    a, M = _waveform(ta, 2, 4, scri_amd.h), functools.partial(flux.p_plus, s=-2)
    cases = {"lm": (_waveform(ta, 3, 5, scri_amd.h), {}), "times": (_waveform(tb, 2, 4, scri_amd.h), {}), "both": (_waveform(tb, 3, 5, scri_amd.h), {}),
             "spin": (_waveform(ta, 2, 4, scri_amd.psi3), dict(allow_LM_differ=True)), "empty": (_waveform(ta, 5, 6, scri_amd.h), dict(allow_LM_differ=True))}
    assert set(cases) == set(texts)
    for name, (b, kw) in cases.items():
        kind, text = texts[name]
        assert kind == "ValueError"
        with pytest.raises(ValueError) as e:
            flux.matrix_expectation_value(a, M, b, **kw)
        assert str(e.value) == text, name
    # (with different times only the times are refused, with different l ranges the l ranges first)
    with pytest.raises(ValueError, match="Time samples must match"):
        flux.matrix_expectation_value(a, M, _waveform(tb, 3, 5, scri_amd.h), allow_LM_differ=True)


@pytest.mark.parametrize("lmin,lmax", RANGES + ((2, 16),))
def test_kernel_tables_are_the_generators_combined(lmin, lmax):
    """bms_flux_coefficients against P = chi(-2), B1 = (1/8)[eb' chi(-3) eb - e' chi(-1) e + 6 chi(-2)] - (1/4) e' (eth chi),
    B2 = (1/8)[...] + (1/4) (ethbar chi) e built from the package's triplets in long double (e, eb: the ladder factors of eth and ethbar at
    s = -2, scri/waveform_modes.py:478-572; signs as scri/flux.py:704-707, 740-741).  The table is the exact value rounded once; the
    yardstick combines five doubles that carry one rounding each: 8 x 2^-53 of the sum of the terms' magnitudes bounds the difference."""
    from scri_amd import engine, flux
    from scri_amd.mode_algebra import LM_range

    LD = np.longdouble
    n = engine.LM_total_size(lmin, lmax)
    image = engine.flux_coefficients(lmin, lmax)
    assert image.shape == (30, n)
    LM = LM_range(lmin, lmax)
    ell, m = LM[:, 0], LM[:, 1]
    e = np.sqrt(((ell + 2) * (ell - 1)).astype(LD))
    eb = -np.sqrt(((ell - 2) * (ell + 3)).astype(LD))
    assert np.array_equal(image[29], ell)
    assert np.array_equal(image[27], np.sqrt(((ell - m) * (ell + m + 1)).astype(LD)).astype(float))
    assert np.array_equal(image[28], np.sqrt(((ell + m) * (ell - m + 1)).astype(LD)).astype(float))
    expect, scale = np.zeros((27, n), dtype=LD), np.zeros((27, n), dtype=LD)
    gens = {+1: flux.p_plus, -1: flux.p_minus, 0: flux.p_z}
    for mu in (-1, 0, 1):
        rows, cols, _ = gens[mu](lmin, lmax, s=-2)
        k = 3 * (ell[rows] - ell[cols] + 1) + (mu + 1)
        chi = {s: gens[mu](lmin, lmax, s=s)[2].astype(LD) for s in SPINS}
        up, down = flux._eth_chi_elements(lmin, lmax, mu)[2].astype(LD), flux._ethbar_chi_elements(lmin, lmax, mu)[2].astype(LD)
        assert np.array_equal(flux._eth_chi_elements(lmin, lmax, mu)[0], rows) and np.array_equal(flux._ethbar_chi_elements(lmin, lmax, mu)[1], cols)
        terms = (eb[rows] * chi[-3] * eb[cols] / 8, -e[rows] * chi[-1] * e[cols] / 8, 6 * chi[-2] / 8)
        bracket, size = sum(terms), sum(abs(x) for x in terms)
        expect[3 * k + 0, cols], scale[3 * k + 0, cols] = chi[-2], abs(chi[-2])
        expect[3 * k + 1, cols], scale[3 * k + 1, cols] = bracket - e[rows] * up / 4, size + abs(e[rows] * up / 4)
        expect[3 * k + 2, cols], scale[3 * k + 2, cols] = bracket + down * e[cols] / 4, size + abs(down * e[cols] / 4)
    err = np.abs(image[:27].astype(LD) - expect)
    assert np.all(err <= VALUE_BOUND * scale), float((err / np.maximum(scale, LD(1e-300))).max() / 2.0**-53)
    assert np.all(image[:27][scale == 0] == 0)


@pytest.mark.parametrize("lmin,lmax", RANGES)
def test_yardstick_equals_the_reference_fluxes(g32, lmin, lmax):
    """fixture (b): the long-double yardstick of the GPU tests (tests/helpers/flux_cases.py) against the reference's own numbers, which
    sum the same terms in double in another order: twice the yardstick's bar.  hdot derived: from oracle.flux_ref.data_dot."""
    from oracle import flux_ref
    from tests.helpers import flux_cases as fc

    tag = f"{lmin}_{lmax}"
    t, (h, given), fluxes = g32[f"b_{tag}_t"], g32[f"b_{tag}_modes"], g32[f"b_{tag}_fluxes"]
    for k, hdot in enumerate((flux_ref.data_dot(t, h), given)):
        y = fc.yardstick(t, h, hdot, lmin, lmax)
        for name, cols in (("energy", 0), ("momentum", slice(1, 4)), ("angular", slice(4, 7)), ("boost", slice(7, 10))):
            value, bar = y[name]
            r = fc.ratio(fluxes[k][:, cols], value, 2 * bar)
            print(f"l = {lmin}..{lmax} {'derived' if k == 0 else 'given'} {name}: {r:.3f} of the bar")
            assert r <= 1.0, (name, k, r)


def _kernel_sums_in_numpy(image, t, h, hdot, lmin, lmax):
    """what kernels_flux.hip states, column by column in double: the neighbour (l + dl, m + mu) of column (l, m) with the three
    coefficients of image rows 3 k + set -- a check of the tables' layout and signs that needs no device"""
    n = h.shape[1]
    P, B, J = np.zeros((3, len(t)), dtype=complex), np.zeros((3, len(t)), dtype=complex), np.zeros((3, len(t)), dtype=complex)
    for c in range(n):
        l = int(image[29, c])
        m = c + lmin * lmin - l * (l + 1)
        for dl in (-1, 0, 1):
            lp = l + dl
            if lp < lmin or lp > lmax:
                continue
            for mu in (-1, 0, 1):
                if abs(m + mu) > lp:
                    continue
                r, k = c + (0 if dl == 0 else (2 * l + 2 if dl > 0 else -2 * l)) + mu, 3 * (dl + 1) + (mu + 1)
                P[mu + 1] += image[3 * k, c] * np.conj(hdot[:, r]) * hdot[:, c]
                B[mu + 1] += image[3 * k + 1, c] * np.conj(hdot[:, r]) * h[:, c] + image[3 * k + 2, c] * np.conj(h[:, r]) * hdot[:, c]
                if dl == 0:
                    J[mu + 1] += 1j * (m if mu == 0 else image[27 if mu == 1 else 28, c]) * np.conj(hdot[:, r]) * h[:, c]
    xyz = lambda v: np.stack([0.5 * (v[2].real + v[0].real), 0.5 * (v[2].imag - v[0].imag), v[1].real], axis=1)  # noqa: E731
    T = B - 0.5 * t[None, :] * P
    return (np.abs(hdot) ** 2).sum(axis=1) / (16 * np.pi), xyz(P) / (16 * np.pi), xyz(J) / (-16 * np.pi), xyz(T) / (-32 * np.pi)


@pytest.mark.parametrize("lmin,lmax", RANGES)
def test_kernel_tables_give_the_fluxes(lmin, lmax):
    from scri_amd import engine
    from tests.helpers import flux_cases as fc

    t, h, hdot = fc.chirp_pair(lmin, lmax, 5, 11 + lmax)
    got = _kernel_sums_in_numpy(engine.flux_coefficients(lmin, lmax), t, h, hdot, lmin, lmax)
    y = fc.yardstick(t, h, hdot, lmin, lmax)
    for name, g in zip(fc.FLUXES, got):
        r = fc.ratio(g, *y[name])
        assert r <= 1.0, (name, r)
