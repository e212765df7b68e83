"""Generator of g30_ref_fake_precessing.npz: the reference's own `fake_precessing_waveform` and `pn_leading_order_amplitude`
(scri/sample_waveforms.py:383-593, unmodified) and its fluxes (scri/flux.py, unmodified) run on the stand-ins of
reference_standins.py (numba, quaternion with quaternion.calculus, spherical_functions ...).  Run from the repository root where the
reference is available:

    python tests/golden/make_golden_sample_precessing.py

Cases (the keyword arguments are in CASES below, so that the tests call the package with the same ones):
  A  t_1=400, dt=0.5, ell_max=4, other defaults: 841 steps x 21 modes (no block of 64 or 256 divides 841)
  B  t_0=-20, t_1=236, dt=1, ell_max=3, equal masses, no precession: 257 steps x 12 modes, 8 of them exactly zero
  C  t_1=300, dt=0.25, ell_max=2, mass ratio 0.5 (inverted inside), every optional parameter given: 1281 steps x 5 modes
each with inertial=True and inertial=False: data, frame and t.
  D  pn_leading_order_amplitude for every (l, m), l <= 8, at x = 0.05, 0.2, 0.4 and mass ratios 1, 2, 0.25: c16[3][3][77]
  E  type and message of the exception of two calls whose merger comes too early
  F  energy, momentum and angular-momentum flux of case A's inertial waveform
Arrays and message strings only.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = {
    "A": dict(t_1=400.0, dt=0.5, ell_max=4),
    "B": dict(t_0=-20.0, t_1=236.0, dt=1.0, ell_max=3, mass_ratio=1.0, precession_opening_angle=0.0),
    "C": dict(t_1=300.0, dt=0.25, ell_max=2, mass_ratio=0.5, precession_opening_angle=0.4, precession_opening_angle_dot=1e-3,
              precession_relative_rate=0.25, precession_nutation_angle=0.07),
}
AMPLITUDE_X = (0.05, 0.2, 0.4)
AMPLITUDE_MASS_RATIOS = (1.0, 2.0, 0.25)
AMPLITUDE_ELL_MAX = 8
ERROR_CASES = {
    "merger_before_start": dict(t_0=0.0, t_1=110.0, dt=1.0),
    "too_few_steps": dict(t_0=90.0, t_1=100.0, dt=1.0),
}


def main():
    sys.path.insert(0, HERE)
    import reference_standins as standins

    scri = standins.install()
    import quaternion
    import scri.flux as flux
    from scri.sample_waveforms import fake_precessing_waveform, pn_leading_order_amplitude

    out = {}
    for name, kw in CASES.items():
        for inertial in (True, False):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                w = fake_precessing_waveform(inertial=inertial, **kw)
            tag = f"{name}_{'inertial' if inertial else 'corotating'}"
            out[f"{tag}_data"] = np.asarray(w.data)
            out[f"{tag}_frame"] = quaternion.as_float_array(w.frame)
            out[f"{tag}_t"] = np.asarray(w.t)
            if name == "A" and inertial:
                out["A_energy_flux"] = np.asarray(flux.energy_flux(w))
                out["A_momentum_flux"] = np.asarray(flux.momentum_flux(w))
                out["A_angular_momentum_flux"] = np.asarray(flux.angular_momentum_flux(w))
    amp = np.zeros((len(AMPLITUDE_MASS_RATIOS), len(AMPLITUDE_X), (AMPLITUDE_ELL_MAX + 1) ** 2 - 4), dtype=complex)
    for i, q in enumerate(AMPLITUDE_MASS_RATIOS):
        for j, x in enumerate(AMPLITUDE_X):
            k = 0
            for ell in range(2, AMPLITUDE_ELL_MAX + 1):
                for m in range(-ell, ell + 1):
                    amp[i, j, k] = pn_leading_order_amplitude(ell, m, x, mass_ratio=q)
                    k += 1
    out["amplitude"] = amp
    out["amplitude_x"] = np.array(AMPLITUDE_X)
    out["amplitude_mass_ratios"] = np.array(AMPLITUDE_MASS_RATIOS)
    errors = {}
    for name, kw in ERROR_CASES.items():
        try:
            fake_precessing_waveform(**kw)
            errors[name] = None
        except Exception as e:  # noqa: BLE001  (recorded as it is)
            errors[name] = [type(e).__name__, str(e)]
    out["errors_json"] = np.array(json.dumps(errors))
    np.savez_compressed(os.path.join(HERE, "g30_ref_fake_precessing.npz"),
                        source="scri/sample_waveforms.py:383-593, scri/flux.py (the reference's files, stand-ins underneath)", **out)


if __name__ == "__main__":
    main()
    print("wrote g30")
