"""The retardation of raw finite-radius series without a GPU: the numpy yardstick of tests/helpers/finite_radius_ref.py against the
reference's own read_finite_radius_waveform (g33, tests/golden/make_golden_finite_radius.py), the keep rule the kernel scans against
monotonic_indices, the selection rules and errors of finite_radius_data, and the names."""
import os

import numpy as np
import pytest

from tests.golden.make_golden_finite_radius import CH_MASS, COORD_RADIUS, DATA_TYPES, INITIAL_ADM_ENERGY, ROW_STEP, inputs
from tests.helpers import finite_radius_ref as ref

G33 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g33_ref_finite_radius.npz")
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def g33():
    return np.load(G33)


@pytest.mark.parametrize("data_type", DATA_TYPES)
def test_yardstick_matches_the_reference(g33, data_type):
    t, areal, lapse, data = inputs(data_type)
    y = ref.retard(t, areal, lapse, data, COORD_RADIUS, INITIAL_ADM_ENERGY, CH_MASS, data_type)
    assert np.array_equal(y["idx"], np.arange(t.size))
    np.testing.assert_array_equal(y["t_cumsum"], g33[f"{data_type}_t"])  # numpy's own running sum: the reference's arithmetic to the bit
    np.testing.assert_array_equal(y["radii"], g33[f"{data_type}_radii"])
    np.testing.assert_array_equal(y["data"][::ROW_STEP], g33[f"{data_type}_data"])
    # exactly rounded prefix sums differ from the sequential sum by at most its standard bound, n 2^-53 times the largest partial sum
    bound = t.size * 2.0**-53 * np.abs(y["t_cum"]).max() / CH_MASS
    assert np.abs(y["t"] - y["t_cumsum"]).max() <= bound
    assert str(g33[f"{data_type}_history"][0]).startswith("# extrapolation.read_finite_radius_waveform(")


@pytest.mark.parametrize("step", [0.0, 1e-3, 0.2])
def test_keep_rule_gives_monotonic_indices(step):
    from scri_amd.extrapolation import monotonic_indices

    rng = np.random.default_rng(3301)
    for _ in range(300):
        t = ref.restarting_axis(rng, int(rng.integers(1, 60)), step)
        for min_step in (0.0, 1e-3, 0.2):
            np.testing.assert_array_equal(ref.keep_rule(t, min_step), monotonic_indices(t, min_step))
    T = np.array([0.0, 1.0, 2.0, 1.5, 2.5, 3.0, 3.0005, 4.0, 3.9, 3.95, 5.0, 6.0])
    g29 = np.load(os.path.join(os.path.dirname(G33), "g29_ref_extrapolation.npz"))
    np.testing.assert_array_equal(ref.keep_rule(T), g29["mono_default"])  # the reference's own loop, where it terminates
    np.testing.assert_array_equal(ref.keep_rule(T, 0.2), g29["mono_step"])


def test_names_are_exported():
    import scri_amd
    from scri_amd import _lib, engine, extrapolation, sample_waveforms

    for name in ("finite_radius_waveform", "finite_radius_data", "monotonic_indices"):
        assert name in extrapolation.__all__ and callable(getattr(extrapolation, name))
    assert callable(sample_waveforms.fake_finite_radius_data)
    assert callable(engine.finite_radius_retard) and callable(engine.retard_tile)
    for name in ("bms_finite_radius_retard", "bms_retard_tile"):
        assert name in _lib.SIGNATURES
    assert engine.retard_tile() >= 64
    assert scri_amd.extrapolation is extrapolation


class _Recorder:
    """finite_radius_waveform replaced by a recorder: the selection runs without a GPU"""

    def __init__(self, monkeypatch):
        from scri_amd import extrapolation

        self.calls = []
        monkeypatch.setattr(extrapolation, "finite_radius_waveform", self)

    def __call__(self, **kw):
        self.calls.append(kw)
        return f"W{kw['tag']}", f"R{kw['tag']}"


def test_selection_rules_of_finite_radius_data(monkeypatch):
    from scri_amd.extrapolation import finite_radius_data

    rec = _Recorder(monkeypatch)
    groups = {"R0100.dir": dict(tag=0), "R0247.dir": dict(tag=1), "VersionHist.ver": dict(tag=9), "R0600.dir": dict(tag=2)}
    Ws, Radii, radii = finite_radius_data(groups, 1.5)
    assert (Ws, Radii, radii) == (["W0", "W1", "W2"], ["R0", "R1", "R2"], ["0100", "0247", "0600"])
    assert all(c["ChMass"] == 1.5 and c["ctx"] is None for c in rec.calls)
    Ws, _, radii = finite_radius_data(groups, 1.5, CoordRadii=[2, 0])  # positions, in the order given
    assert (Ws, radii) == (["W2", "W0"], ["0600", "0100"])
    Ws, _, radii = finite_radius_data(groups, 1.5, CoordRadii=["0247", "R06"])  # regular expressions, in the order of the groups
    assert (Ws, radii) == (["W1", "W2"], ["0247", "0600"])
    Ws, _, radii = finite_radius_data(groups, 1.5, CoordRadii=[r"R0[16]"])
    assert (Ws, radii) == (["W0", "W2"], ["0100", "0600"])


def test_errors_of_finite_radius_data(monkeypatch):
    from scri_amd.extrapolation import finite_radius_data

    _Recorder(monkeypatch)
    groups = {"R0100.dir": dict(tag=0), "R0247.dir": dict(tag=1)}
    with pytest.raises(ValueError, match=r"ChMass=0\.0 is not a valid input value\."):
        finite_radius_data(groups)
    with pytest.raises(ValueError, match="No waveform groups matched the requested CoordRadii"):
        finite_radius_data(groups, 1.0, CoordRadii=["0999"])
    with pytest.raises(ValueError, match="Mismatch between requested radii and matched waveform groups"):
        finite_radius_data({"R0100.dir": dict(tag=0), "Rxyz": dict(tag=1)}, 1.0, CoordRadii=["R"])
    with pytest.raises(ValueError, match="Could not convert CoordRadii entries to float"):
        finite_radius_data({"R01a0.dir": dict(tag=0)}, 1.0)
    with pytest.raises(ValueError, match="Could not parse radius from waveform name"):
        finite_radius_data({"S0100": dict(tag=0)}, 1.0, CoordRadii=[0])


def test_errors_of_finite_radius_waveform_before_the_gpu():
    import scri_amd
    from scri_amd.extrapolation import finite_radius_waveform

    t = np.arange(4.0)
    data = np.zeros((4, 21), dtype=complex)
    with pytest.raises(ValueError, match=r"ChMass=0\.0 is not a valid input value\."):
        finite_radius_waveform(t, data, t + 100, t * 0 + 1, 99.0, 1.0, 0.0, scri_amd.h)
    with pytest.raises(ValueError, match=f'DataType "{scri_amd.sigma}" is unknown.'):
        finite_radius_waveform(t, data, t + 100, t * 0 + 1, 99.0, 1.0, 1.0, scri_amd.sigma)
    with pytest.raises(ValueError, match="do not hold the modes"):
        finite_radius_waveform(t, data[:, :20], t + 100, t * 0 + 1, 99.0, 1.0, 1.0, scri_amd.h)
