"""Generator of g31_ref_com_motion.npz: the reference's own `com_motion`, `estimate_avg_com_motion` (scri/SpEC/com_motion.py) and
`PN_charges`, `analytical_CoM_func` (scri/pn/boosted_comcharge.py), both files loaded unmodified by path, run on the inputs of
tests/helpers/com_motion_cases.py.  Run from the repository root where the reference is available:

    python tests/golden/make_golden_com_motion.py

`h5py` is a stand-in here (and only here): its `File` is a context manager over a dict of tables registered under a file name, so that
the reference's three branches and its error paths run.  scipy's `simpson` is wrapped to record which samples the reference hands it
(i_i, i_f).  Stored: inputs, the reference's outputs, type and text of its exceptions.
  fit_<case>_*        t, com, the two fractions; x_i, v_i, t_i, t_f without and x_i, v_i, a_i with acceleration; i_i, i_f
  track_<case>_*      tables of the stand-in files, masses; the reference's t and CoM (BBH, NSNS, BHNS with a longer horizon table, BHNS
                      with a given m_A)
  errors_json         {case: [exception type, text]}
  pn_*                omega[64, 3] and modes[64, 21] of a stand-in abd, m, nu; the four callables' values; theta and analytical_CoM_func
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests.helpers import com_motion_cases as cases  # noqa: E402

FILES = {}


class _File:
    def __init__(self, name, mode="r"):
        self.tables = FILES[name]

    def __enter__(self):
        return self.tables

    def __exit__(self, *exc):
        return False


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def main():
    import reference_standins as standins
    import scipy.integrate

    sys.modules["h5py"] = types.ModuleType("h5py")
    sys.modules["h5py"].File = _File
    seen = []
    simpson = scipy.integrate.simpson

    def recording_simpson(y, x=None, **kw):
        seen.append(((x.__array_interface__["data"][0] - x.base.__array_interface__["data"][0]) // x.strides[0], x.shape[0]))
        return simpson(y, x, **kw)

    scipy.integrate.simpson = recording_simpson
    ref = _load(os.path.join(standins.REFERENCE, "scri", "SpEC", "com_motion.py"), "_ref_com_motion")
    pn = _load(os.path.join(standins.REFERENCE, "scri", "pn", "boosted_comcharge.py"), "_ref_boosted_comcharge")
    out = {}
    for position, (name, (t, fb, fe)) in enumerate(cases.fit_cases().items()):
        com = cases.fit_case_track(position, t)
        FILES["h"] = cases.horizons_of_track(t, com)
        assert np.array_equal(ref.com_motion("h")[1], com)
        out[f"fit_{name}_t"], out[f"fit_{name}_com"], out[f"fit_{name}_fractions"] = t, com, np.array([fb, fe])
        with contextlib.redirect_stdout(io.StringIO()):
            del seen[:]
            x, v, t_i, t_f = ref.estimate_avg_com_motion("h", skip_beginning_fraction=fb, skip_ending_fraction=fe)
            x2, v2, a2, t_i2, t_f2 = ref.estimate_avg_com_motion("h", skip_beginning_fraction=fb, skip_ending_fraction=fe, fit_acceleration=True)
        assert len(set(seen)) == 1 and (t_i, t_f) == (t_i2, t_f2)
        out[f"fit_{name}_linear"] = np.array([x, v])
        out[f"fit_{name}_accelerated"] = np.array([x2, v2, a2])
        out[f"fit_{name}_window"] = np.array([t_i, t_f])
        out[f"fit_{name}_indices"] = np.array([seen[0][0], seen[0][0] + seen[0][1] - 1])
    for name in cases.track_inputs():
        hz, mt, m_A, m_B = cases.track_inputs()[name]  # (fresh tables: the reference divides its view of the times in place)
        FILES["h"], FILES["m"] = hz, mt
        t, com = ref.com_motion("h" if hz is not None else None, "m" if mt is not None else None, m_A, m_B)
        out[f"track_{name}_t"], out[f"track_{name}_com"] = np.array(t), np.array(com)
    errors = {}
    for name, (hz, mt, m_A, m_B) in cases.error_inputs().items():
        FILES["h"], FILES["m"] = hz, mt
        try:
            ref.com_motion("h" if hz is not None else None, "m", m_A, m_B)
            errors[name] = None
        except Exception as e:  # noqa: BLE001  (recorded as it is)
            errors[name] = [type(e).__name__, str(e)]
    out["errors_json"] = np.array(json.dumps(errors))
    p = cases.pn_inputs()
    h = types.SimpleNamespace(angular_velocity=lambda: p["pn_omega"], data=p["pn_modes"], index=lambda ell, m: ell * (ell + 1) - 4 + m)
    abd = types.SimpleNamespace(h=h)
    values = [f(abd) for f in pn.PN_charges(float(p["pn_m"]), float(p["pn_nu"]))]
    out.update(p)
    out["pn_charges"] = np.array(values)
    out["pn_G"] = pn.analytical_CoM_func(p["pn_theta"], p["pn_t"], *values)
    np.savez_compressed(os.path.join(HERE, "g31_ref_com_motion.npz"),
                        source="scri/SpEC/com_motion.py, scri/pn/boosted_comcharge.py (the reference's files; h5py a stand-in over dicts)", **out)


if __name__ == "__main__":
    main()
    print("wrote g31")
