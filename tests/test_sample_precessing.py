"""`pn_leading_order_amplitude`, the argument checks of `fake_precessing_waveform` and the fixture of the GPU tests (g30,
tests/golden/make_golden_sample_precessing.py: the reference's own functions on the stand-ins).  No GPU needed."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.golden.make_golden_sample_precessing import AMPLITUDE_ELL_MAX, AMPLITUDE_MASS_RATIOS, AMPLITUDE_X, CASES, ERROR_CASES

G30 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g30_ref_fake_precessing.npz")
EPS = np.finfo(float).eps
SHAPES = {"A": (841, 21), "B": (257, 12), "C": (1281, 5)}


@pytest.fixture(scope="module")
def g30():
    return np.load(G30)


def test_amplitudes_match_the_reference(g30):
    """every (l, m), l <= 8, at three x and three mass ratios (one of them inverted inside): 8 eps relative -- a coefficient is a
    product of a few correctly rounded factors; where the reference is exactly zero (equal masses, m = 0) so is the package"""
    from scri_amd.sample_waveforms import pn_leading_order_amplitude

    assert list(g30["amplitude_x"]) == list(AMPLITUDE_X) and list(g30["amplitude_mass_ratios"]) == list(AMPLITUDE_MASS_RATIOS)
    worst, zeros = 0.0, 0
    for i, q in enumerate(AMPLITUDE_MASS_RATIOS):
        for j, x in enumerate(AMPLITUDE_X):
            k = 0
            for ell in range(2, AMPLITUDE_ELL_MAX + 1):
                for m in range(-ell, ell + 1):
                    got, ref = pn_leading_order_amplitude(ell, m, x, mass_ratio=q), g30["amplitude"][i, j, k]
                    k += 1
                    if ref == 0:
                        zeros += 1
                        assert got == 0, (q, x, ell, m, got)
                    else:
                        worst = max(worst, abs(got - ref) / abs(ref))
    print(f"amplitudes: largest relative difference {worst / EPS:.2f} eps, {zeros} exact zeros")
    assert worst <= 8 * EPS and zeros > 0
    # an array of x broadcasts as in the reference
    x = np.array(AMPLITUDE_X)
    np.testing.assert_array_equal(pn_leading_order_amplitude(3, -2, x, mass_ratio=2.0),
                                  [pn_leading_order_amplitude(3, -2, v, mass_ratio=2.0) for v in x])


def test_amplitude_tables_of_the_kernel_come_from_the_same_code():
    from scri_amd.sample_waveforms import _pn_amplitude_tables, pn_leading_order_amplitude

    coef, power = _pn_amplitude_tables(5, 2.0)
    assert coef.shape == power.shape == (32,) and np.all(2 * power == np.round(2 * power)) and power.min() == 1.0
    k = 0
    for ell in range(2, 6):
        for m in range(-ell, ell + 1):
            ref = pn_leading_order_amplitude(ell, m, 0.3, mass_ratio=2.0)
            assert abs(coef[k] * 0.3 ** power[k] - ref) <= 4 * EPS * abs(ref), (ell, m)
            k += 1


def test_too_early_a_merger_is_refused_in_the_reference_s_words(g30):
    from scri_amd.sample_waveforms import fake_precessing_waveform

    errors = json.loads(str(g30["errors_json"]))
    assert set(errors) == set(ERROR_CASES)
    for name, kw in ERROR_CASES.items():
        kind, message = errors[name]
        assert kind == "ValueError"
        with pytest.raises(ValueError) as e:
            fake_precessing_waveform(**kw)
        assert str(e.value) == message, name


def test_fixture_keys_and_shapes(g30):
    assert set(CASES) == set(SHAPES)
    for name, (n, n_modes) in SHAPES.items():
        for frame in ("inertial", "corotating"):
            assert g30[f"{name}_{frame}_data"].shape == (n, n_modes) and g30[f"{name}_{frame}_data"].dtype == complex
            assert g30[f"{name}_{frame}_frame"].shape == (n, 4) and g30[f"{name}_{frame}_t"].shape == (n,)
        kw = CASES[name]
        np.testing.assert_array_equal(g30[f"{name}_corotating_t"], np.arange(kw.get("t_0", -20.0), kw["t_1"] + 0.99 * kw["dt"], kw["dt"]))
    assert g30["amplitude"].shape == (3, 3, 77)
    assert g30["A_energy_flux"].shape == (841,) and g30["A_momentum_flux"].shape == (841, 3) and g30["A_angular_momentum_flux"].shape == (841, 3)
    # case B: equal masses leave 8 of the 12 columns exactly zero in the reference's own output
    assert int(np.sum(np.all(g30["B_corotating_data"] == 0, axis=0))) == 8


def test_library_exports_the_entries():
    import scri_amd
    from scri_amd import _lib

    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "bms_precessing_waveform") and hasattr(lib, "bms_radius_terms")
    assert ctypes.sizeof(_lib.bms_precessing_params) == 6 * 8 + 2 * 4 + 2 * 8
    assert scri_amd.sample_waveforms.fake_precessing_waveform and scri_amd.sample_waveforms.fake_finite_radius_waveforms
