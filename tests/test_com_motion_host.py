"""scri_amd.SpEC.com_motion and scri_amd.pn.boosted_comcharge, the parts that need no GPU: the dotted paths, what `com_motion` reads
from a mapping or a path in each of the reference's three branches (the arrays it hands to the engine, against the reference's own
result in g31 through the numpy expression), the reference's error texts, and the host arithmetic of the PN model.  The kernels are
tested in tests/test_gpu_com_motion.py."""
import importlib
import json
import os
import sys
import types

import numpy as np
import pytest

from tests.helpers import com_motion_cases as cases
from tests.helpers.com_motion_cases import error_inputs, pn_inputs, track_inputs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_ref_com_motion.npz")


@pytest.fixture(scope="module")
def g31():
    return np.load(GOLDEN)


@pytest.fixture
def captured(monkeypatch):
    """com_motion with the engine call replaced by the numpy expression of bms_com_motion's contract; the arguments are recorded"""
    from scri_amd import engine

    calls = []

    def com_track(t, x_a, x_b, m_a, m_b, matter=False, ctx=None):
        calls.append(dict(t=t, x_a=x_a, x_b=x_b, m_a=m_a, m_b=m_b, matter=matter))
        m = m_a + m_b
        com = ((m_a[:, np.newaxis] * x_a) + (m_b[:, np.newaxis] * x_b)) / m[:, np.newaxis]
        return (t / m, com / m[:, np.newaxis]) if matter else (np.array(t), com)

    monkeypatch.setattr(engine, "com_track", com_track)
    return calls


def test_dotted_paths_resolve():
    import scri_amd

    module = importlib.import_module("scri_amd.SpEC.com_motion")
    assert module is importlib.import_module("scri_amd.com_motion")
    for name in ("com_motion", "estimate_avg_com_motion", "remove_avg_com_motion"):
        assert getattr(scri_amd.SpEC, name) is getattr(module, name)
    from scri_amd.SpEC.com_motion import com_motion, estimate_avg_com_motion  # noqa: F401  (the import line of the reference's docstring)

    pn = importlib.import_module("scri_amd.pn.boosted_comcharge")
    assert scri_amd.pn.boosted_comcharge is pn and callable(pn.PN_charges) and callable(pn.analytical_CoM_func)


@pytest.mark.parametrize("name", ["bbh", "nsns", "bhns_longer_horizons", "bhns_given_mass"])
def test_branches_read_what_the_reference_reads(name, g31, captured):
    from scri_amd.SpEC.com_motion import com_motion

    hz, mt, m_A, m_B = track_inputs()[name]
    before = {k: v.copy() for d in (hz, mt) if d is not None for k, v in d.items()}
    t, com = com_motion(hz, mt, m_A, m_B)
    assert np.array_equal(t, g31[f"track_{name}_t"]) and np.array_equal(com, g31[f"track_{name}_com"])
    (call,) = captured
    assert call["matter"] == (mt is not None)
    for d in (hz, mt):  # the caller's tables are left alone (the reference divides its own copy of t in place)
        for k, v in (d or {}).items():
            assert np.array_equal(v, before[k])


def test_bhns_cuts_the_longer_horizon_table(captured):
    from scri_amd.SpEC.com_motion import com_motion

    hz, mt, m_A, m_B = track_inputs()["bhns_longer_horizons"]
    n = mt[cases.NS1].shape[0]
    assert hz[cases.A_MASS].shape[0] == n + 7
    t, com = com_motion(hz, mt, m_A, m_B)
    (call,) = captured
    assert call["t"].shape == (n,) and call["x_a"].shape == (n, 3) and call["m_a"].shape == (n,) and call["m_b"].shape == (1,)
    assert t.shape == (n,) and com.shape == (n, 3)
    # a given m_A of length one is not cut
    captured.clear()
    com_motion(hz, mt, 5.0, m_B)
    assert captured[0]["m_a"].shape == (1,) and captured[0]["x_a"].shape == (n, 3)


def test_error_texts_are_the_references(g31, captured):
    from scri_amd.SpEC.com_motion import com_motion

    expected = json.loads(str(g31["errors_json"]))
    inputs = error_inputs()
    assert set(expected) == set(inputs) and all(v is not None for v in expected.values())
    for name, (hz, mt, m_A, m_B) in inputs.items():
        kind, text = expected[name]
        with pytest.raises(Exception) as info:
            com_motion(hz, mt, m_A, m_B)
        assert type(info.value).__name__ == kind and str(info.value) == text, name
    assert not captured  # every one is raised before anything is computed


def test_paths_go_through_h5py(monkeypatch, captured, g31):
    from scri_amd.SpEC.com_motion import com_motion, estimate_avg_com_motion

    monkeypatch.setitem(sys.modules, "h5py", None)  # (import h5py now raises ImportError)
    with pytest.raises(ImportError, match="h5py"):
        com_motion("Horizons.h5")
    with pytest.raises(ImportError, match="h5py"):
        estimate_avg_com_motion(os.path.join("some", "where", "Horizons.h5"))
    # with an importable h5py a path is opened read-only and used as the mapping it is
    hz, mt, m_A, m_B = track_inputs()["bhns_longer_horizons"]
    files, opened = {"Horizons.h5": hz, "Matter.h5": mt}, []

    class File:
        def __init__(self, name, mode):
            opened.append((name, mode))
            self.tables = files[name]

        def __enter__(self):
            return self.tables

        def __exit__(self, *exc):
            opened.append((None, "closed"))
            return False

    standin = types.ModuleType("h5py")
    standin.File = File
    monkeypatch.setitem(sys.modules, "h5py", standin)
    t, com = com_motion("Horizons.h5", "Matter.h5", m_A, m_B)
    assert np.array_equal(com, g31["track_bhns_longer_horizons_com"])
    assert sorted(o for o in opened if o[0]) == [("Horizons.h5", "r"), ("Matter.h5", "r")] and opened.count((None, "closed")) == 2


def test_plot_is_refused_and_a_pair_is_accepted(monkeypatch, capsys):
    from scri_amd import engine
    from scri_amd.SpEC.com_motion import estimate_avg_com_motion

    with pytest.raises(NotImplementedError, match="plot"):
        estimate_avg_com_motion({}, plot=True)
    seen = []

    def com_fit(t, com, fb, fe, acc, ctx=None):
        seen.append((t, com, fb, fe, acc))
        return dict(x_i=np.array([1.0, 2.0, 3.0]), v_i=np.array([0.1, 0.2, 0.3]), a_i=np.array([0.0, 0.5, 0.25]), t_i=np.float64(1.5),
                    t_f=np.float64(9.0), i_i=1, i_f=8, moments=np.zeros((3, 3)))

    monkeypatch.setattr(engine, "com_fit", com_fit)
    t, com = np.arange(10.0), np.zeros((10, 3))
    out = estimate_avg_com_motion((t, com), skip_beginning_fraction=0.2)
    assert len(out) == 4 and seen[0][0] is t and seen[0][1] is com and seen[0][2:] == (0.2, 0.10, False)
    assert capsys.readouterr().out == "Optimal x_i: [1.0, 2.0, 3.0]\nOptimal v_i: [0.1, 0.2, 0.3]\nt_i, t_f: 1.5, 9.0\n"
    out = estimate_avg_com_motion((t, com), fit_acceleration=True)
    assert len(out) == 5 and np.array_equal(out[2], [0.0, 0.5, 0.25]) and out[3:] == (1.5, 9.0)
    assert capsys.readouterr().out.splitlines()[2] == "Optimal a_i: [0.0, 0.5, 0.25]"


def test_remove_takes_the_masses_from_the_metadata(monkeypatch):
    from scri_amd import com_motion as module

    seen = {}

    def estimate(horizons, **kw):
        seen.update(kw, horizons=horizons)
        return np.array([1e-3, 0.0, 0.0]), np.array([0.0, 1e-5, 0.0]), 0.0, 1.0

    monkeypatch.setattr(module, "estimate_avg_com_motion", estimate)

    class W:
        metadata = types.SimpleNamespace(reference_mass1=1.35, reference_mass2=1.45)
        version_hist = [["abc", "first"]]
        extrapolate_coord_radii = [100.0, 200.0]

    class Out:
        pass

    def transform(**kw):
        o = Out()
        o.kw = kw
        return o

    w = W()
    w.transform = transform
    out = module.remove_avg_com_motion(w, {"h": 1}, matter={"m": 2}, psi4_modes="companion")
    assert seen["m_A"] == 1.35 and seen["m_B"] == 1.45 and seen["matter"] == {"m": 2} and seen["horizons"] == {"h": 1}
    assert set(out.kw) == {"space_translation", "boost_velocity", "psi4_modes"} and out.kw["psi4_modes"] == "companion"
    assert np.array_equal(out.space_translation, [1e-3, 0.0, 0.0]) and np.array_equal(out.boost_velocity, [0.0, 1e-5, 0.0])
    assert out.version_hist == [["abc", "first"]] and out.extrapolate_coord_radii == [100.0, 200.0]
    # given masses win; without matter the metadata is not consulted
    module.remove_avg_com_motion(w, {}, matter={}, m_A=2.0)
    assert seen["m_A"] == 2.0 and seen["m_B"] == 1.45
    module.remove_avg_com_motion(w, {})
    assert seen["m_A"] is None and seen["m_B"] is None and seen["matter"] is None


def _ulp_distance(a, b, scale):
    return np.abs(a - b).max() / np.spacing(scale)


def test_pn_charges_on_the_stand_in_abd(g31):
    """the four callables on g31's stand-in abd (its angular velocity is given): to 8 ulp of each result"""
    from scri_amd.pn.boosted_comcharge import PN_charges

    assert all(np.array_equal(v, g31[k]) for k, v in pn_inputs().items())
    h = types.SimpleNamespace(angular_velocity=lambda: g31["pn_omega"], data=g31["pn_modes"], index=lambda ell, m: ell * (ell + 1) - 4 + m)
    abd = types.SimpleNamespace(h=h)
    functions = PN_charges(float(g31["pn_m"]), float(g31["pn_nu"]))
    assert [f.__name__ for f in functions] == ["energy_pn", "angular_momentum_pn", "G_mag_pn", "orbital_phase"]
    for f, ref in zip(functions, g31["pn_charges"]):
        got = f(abd)
        assert got.shape == ref.shape and np.all(np.abs(got - ref) <= 8 * np.spacing(np.abs(ref))), f.__name__
    assert np.ptp(g31["pn_charges"][3]) > 2 * np.pi  # (the phase winds: the unwrapping matters)


def test_analytical_com_func_against_the_reference(g31):
    """a handful of fp64 operations per entry: to 4 ulp of its largest term"""
    from scri_amd.pn.boosted_comcharge import analytical_CoM_func

    θ, t = g31["pn_theta"], g31["pn_t"]
    E, J, Gm, ψ = g31["pn_charges"]
    G = analytical_CoM_func(θ, t, E, J, Gm, ψ)
    ref = g31["pn_G"]
    assert G.shape == ref.shape == (t.size, 3)
    largest = np.maximum.reduce([np.abs(θ[6] * Gm / E), np.abs(θ[7] * Gm / E), np.abs(θ[:3]).max() * np.abs(J / E), np.abs(t) * np.abs(θ[:3]).max(),
                                 np.full(t.size, np.abs(θ[3:6]).max())])
    assert np.all(np.abs(G - ref) <= 4 * np.spacing(largest)[:, None])
    assert np.abs(ref).max() > 0
