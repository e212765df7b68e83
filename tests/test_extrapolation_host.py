"""scri_amd.extrapolation without a GPU: argument checks and error texts, intersection / monotonic_indices, the copies of the
negative orders (history, metadata), the two refusals, the graft of `scri.extrapolation._Extrapolate`, and the C export
`bms_extrapolate`.  The fixture g29 comes from the reference's own scri/extrapolation.py (tests/golden/make_golden_extrapolation.py)."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from tests.golden.make_golden_extrapolation import fit_inputs

G29 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g29_ref_extrapolation.npz")


@pytest.fixture(scope="module")
def g29():
    return np.load(G29)


def _wm(t, data, ell_min=2, ell_max=8, dataType=None, history=None):
    import scri_amd

    return scri_amd.WaveformModes(t=t, data=data, ell_min=ell_min, ell_max=ell_max, frameType=scri_amd.Corotating,
                                  dataType=scri_amd.h if dataType is None else dataType, r_is_scaled_out=True, m_is_scaled_out=True,
                                  history=history or [])


def test_module_exports():
    import scri_amd
    from scri_amd import extrapolation

    assert scri_amd._Extrapolate is extrapolation._Extrapolate
    assert scri_amd.extrapolate_waveforms is extrapolation.extrapolate_waveforms
    from scri_amd import mode_operators

    assert extrapolation.intersection is mode_operators.time_intersection  # one restatement, not two


def test_intersection_and_monotonic_indices_match_g29(g29):
    from scri_amd.extrapolation import intersection, monotonic_indices

    t1, t2 = g29["isect_t1"], g29["isect_t2"]
    np.testing.assert_array_equal(intersection(t1, t2), g29["isect_plain"])
    np.testing.assert_array_equal(intersection(t1, t2, 0.2), g29["isect_step"])
    np.testing.assert_array_equal(intersection(t1, t2, min_time=2.0, max_time=7.5), g29["isect_bounds"])
    np.testing.assert_array_equal(intersection([-3e300, 3e300], t1, 0.005, -3e300, 3e300), g29["isect_limits"])
    np.testing.assert_array_equal(np.asarray(monotonic_indices(g29["mono_T"])), g29["mono_default"])
    np.testing.assert_array_equal(np.asarray(monotonic_indices(g29["mono_T"], MinTimeStep=0.2)), g29["mono_step"])


def test_monotonic_indices_where_the_first_kept_time_gives_way():
    """A time within MinTimeStep of the first kept one: the reference's loop does not end there (it compares index 0 with
    index -1 again and again); here the earlier time is dropped as it would be anywhere else."""
    from scri_amd.extrapolation import monotonic_indices

    np.testing.assert_array_equal(monotonic_indices([0.0, 0.0005, 1.0, 2.0]), [1, 2, 3])
    np.testing.assert_array_equal(monotonic_indices([0.0, 1.0, 2.0, 0.5, 3.0], MinTimeStep=0.1), [0, 3, 4])
    np.testing.assert_array_equal(monotonic_indices([]), np.zeros(0, dtype=int))


def test_argument_errors_match_g29(g29, capsys):
    """Same exception and message as the reference -- except where the reference's own message formatting fails (KeyError 'i_W',
    scri/extrapolation.py:1336-1351): there the intended ValueError("scri_VectorSizeMismatch") is raised."""
    from scri_amd.extrapolation import _Extrapolate

    ref = json.loads(str(g29["errors_json"]))
    t, radii, data, _ = fit_inputs("poly")
    n = 50
    base = lambda k=4: [_wm(t[:n], data[i, :n]) for i in range(k)]
    rad = lambda k=4: [radii[i, :n] for i in range(k)]
    cases = {
        "min_order_beyond_radii": lambda: _Extrapolate(base(), rad(), [-5, 2]),
        "max_order_beyond_radii": lambda: _Extrapolate(base(), rad(), [4]),
        "radii_count": lambda: _Extrapolate(base(), rad(3), [2]),
        "n_times": lambda: _Extrapolate(base(3) + [_wm(t[: n - 1], data[0, : n - 1])], rad(), [2]),
        "n_modes": lambda: _Extrapolate(base(3) + [_wm(t[:n], data[0, :n, :45], 2, 6)], rad(), [2]),
        "radius_length": lambda: _Extrapolate(base(), rad(3) + [radii[3, : n - 1]], [2]),
    }
    assert set(cases) == set(ref)
    for name, call in cases.items():
        kind, message = ref[name]
        if kind == "KeyError":
            kind, message = "ValueError", "scri_VectorSizeMismatch"
        with pytest.raises(ValueError) as info:
            call()
        assert type(info.value).__name__ == kind and str(info.value) == message, name
        assert "ERROR" in capsys.readouterr().out
    with pytest.raises(ValueError, match="scri_VectorSizeMismatch"):  # Radii[0] too short for a fit (an IndexError in the reference)
        _Extrapolate(base(), [radii[0, : n - 1]] + rad()[1:], [2])
    # ... while copies alone never read Radii[0], in the reference either
    copies = _Extrapolate(base(), [radii[0, : n - 1]] + rad()[1:], [-1, -4])
    np.testing.assert_array_equal(copies[1].data, data[0, :n])


def test_negative_orders_are_copies_with_history_and_metadata(g29):
    import scri_amd
    from scri_amd.extrapolation import _Extrapolate

    rng = np.random.default_rng(4)
    t = np.linspace(0.0, 1.0, 30)
    Ws = [_wm(t, rng.normal(size=(30, 21)) + 1j * rng.normal(size=(30, 21)), 2, 4, scri_amd.psi4, history=[f"# radius {i}"])
          for i in range(5)]
    out = _Extrapolate(Ws, [np.full(30, 100.0 * (i + 1)) for i in range(5)], [-1, -3, -5])
    for N, W in zip((-1, -3, -5), out):
        src = Ws[5 + N]
        assert W is not src and W.data is not src.data
        np.testing.assert_array_equal(W.data, src.data)
        np.testing.assert_array_equal(W.t, src.t)
        assert W.history[: len(src.history)] == src.history and W.history[-1] == f"### Extrapolating with N={N}\n"
        assert (W.ell_min, W.ell_max, W.dataType, W.frameType) == (2, 4, scri_amd.psi4, scri_amd.Corotating)
    assert list(g29["poly_N-1_history_tail"]) == ["### Extrapolating with N=-1\n"]


def test_refusals_of_the_two_branches_that_fail_in_the_reference():
    import scri_amd
    from scri_amd.extrapolation import _Extrapolate

    t = np.linspace(0.0, 1.0, 30)
    Ws = [_wm(t, np.ones((30, 21), dtype=complex), 2, 4, scri_amd.psi0) for _ in range(4)]
    radii = [np.full(30, 100.0 * (i + 1)) for i in range(4)]
    with pytest.raises(NotImplementedError, match="Omegas.*1450"):
        _Extrapolate(Ws, radii, [2], Omegas=np.ones(30))
    with pytest.raises(NotImplementedError, match="NoiseFloor.*UnboundLocalError"):
        _Extrapolate(Ws, radii, [-1, 2], NoiseFloor=1e-8)
    # the branches are only refused where the reference would reach them: negative orders alone never fit anything
    assert len(_Extrapolate(Ws, radii, [-1], Omegas=np.ones(30), NoiseFloor=1e-8)) == 1
    # NoiseFloor on other data types is inert in the reference too; an empty Omegas list means "no Omegas" (the driver passes [])
    hs = [_wm(t, np.ones((30, 21), dtype=complex), 2, 4) for _ in range(4)]
    with pytest.raises(ValueError, match="scri_IndexOutOfBounds"):  # (checked before anything runs)
        _Extrapolate(hs, radii, [-9], Omegas=[], NoiseFloor=1e-8)


def _stub_scri_with_extrapolation():
    from tests.test_patch_scri import make_stub_scri

    scri = make_stub_scri()
    ext = types.ModuleType("scri.extrapolation")

    def _Extrapolate(FiniteRadiusWaveforms, Radii, ExtrapolationOrders, Omegas=None, NoiseFloor=None):
        raise RuntimeError("the reference's CPU fit was called")

    ext._Extrapolate = _Extrapolate
    scri.extrapolation = ext
    return scri


def test_graft_of_extrapolate_install_and_uninstall():
    import scri_amd
    from scri_amd import adapters

    scri = _stub_scri_with_extrapolation()
    ref = scri.extrapolation._Extrapolate
    patched = scri_amd.patch_scri(scri)
    assert "extrapolation._Extrapolate" in patched
    assert scri.extrapolation._Extrapolate is not ref and scri.extrapolation._Extrapolate_reference is ref
    scri_amd.patch_scri(scri)  # idempotent
    assert scri.extrapolation._Extrapolate_reference is ref
    # the patched function takes scri's waveforms and returns scri's waveforms (negative orders: no GPU needed)
    t = np.linspace(0.0, 1.0, 20)
    Ws = [scri.WaveformModes(t, np.full((20, 21), i + 1.0, dtype=complex), 2, 4, history=[f"# r{i}"]) for i in range(3)]
    out = scri.extrapolation._Extrapolate(Ws, [np.full(20, 10.0 * (i + 1)) for i in range(3)], [-1, -2])
    assert all(isinstance(w, scri.WaveformModes) for w in out)
    np.testing.assert_array_equal(out[0].data, Ws[2].data)
    np.testing.assert_array_equal(out[1].data, Ws[1].data)
    assert out[0].history == ["# r2", "### Extrapolating with N=-1\n"]
    adapters.uninstall(scri)
    assert scri.extrapolation._Extrapolate is ref and not hasattr(scri.extrapolation, "_Extrapolate_reference")
    # a scri without the submodule (tests/test_patch_scri.py's stub) is patched as before
    from tests.test_patch_scri import make_stub_scri

    plain = make_stub_scri()
    assert "extrapolation._Extrapolate" not in scri_amd.patch_scri(plain)
    adapters.uninstall(plain)


def test_export_present_and_a_call_without_context_fails_with_a_status():
    from scri_amd import _lib

    lib = _lib.load()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bms_extrapolate")
    orders = (ctypes.c_int * 1)(2)
    counts = (ctypes.c_int64 * 1)()
    rc = lib.bms_extrapolate(None, 4, None, None, _lib.BMS_HOST, 10, 21, None, 1, orders, None, 0, counts)
    assert rc == _lib.BMS_ERR_INVALID
