"""Generator of g33_ref_finite_radius.npz: the reference's own `read_finite_radius_waveform` (scri/extrapolation.py:343-417, unmodified)
run on the stand-ins of reference_standins.py, with its file reader `read_finite_radius_waveform_nrar` replaced by a function that
returns the arrays of `inputs` below.  Run from the repository root where the reference is available:

    python tests/golden/make_golden_finite_radius.py

The inputs come from a fixed seed (plain numpy), so the tests regenerate them instead of storing them: 300 strictly increasing steps
(the reference's reader thins a restarting axis by another rule before its indices are applied, so it is no yardstick there), 77 modes
(l = 2..8), areal radius and lapse varying by 1e-3, one case per data type.  Every ROW_STEP-th row of the modes is kept (the size limit
of a committed file); the times and radii are kept whole.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA_TYPES = ("h", "hdot", "psi4", "psi3", "psi2", "psi1", "psi0")
ROW_STEP = 10
CH_MASS = 0.9873
COORD_RADIUS = 247.0
INITIAL_ADM_ENERGY = 0.9921


def inputs(data_type):
    """(t f8[300], areal radius, lapse, data c16[300][77]) of one case"""
    rng = np.random.default_rng(3300 + DATA_TYPES.index(data_type))
    n, n_m = 300, 77
    t = np.cumsum(rng.uniform(0.05, 0.6, n)) + 11.0
    areal = (COORD_RADIUS + 1.3) * (1.0 + 1e-3 * np.sin(0.01 * t + 0.4))
    lapse = 0.99 * (1.0 + 1e-3 * np.cos(0.013 * t))
    data = (rng.normal(size=(n, n_m)) + 1j * rng.normal(size=(n, n_m))) * np.exp(-0.002 * t)[:, None]
    return t, areal, lapse, data


def main():
    sys.path.insert(0, HERE)
    import reference_standins as standins

    scri = standins.install()
    import scri.extrapolation as ref

    out = {"row_step": ROW_STEP, "ch_mass": CH_MASS, "coord_radius": COORD_RADIUS, "initial_adm_energy": INITIAL_ADM_ENERGY}
    for name in DATA_TYPES:
        t, areal, lapse, data = inputs(name)

        def reader(filename, WaveformName, t=t, areal=areal, lapse=lapse, data=data, name=name):
            T = t.copy()
            Indices = ref.monotonic_indices(T)
            W = scri.WaveformModes(t=t.copy(), data=data.copy(), ell_min=2, ell_max=8, frameType=scri.Inertial, dataType=getattr(scri, name),
                                   r_is_scaled_out=True, m_is_scaled_out=False)
            return W, T[Indices], Indices, areal[Indices], lapse[Indices], COORD_RADIUS, INITIAL_ADM_ENERGY

        ref.read_finite_radius_waveform_nrar = reader
        W, Radii = ref.read_finite_radius_waveform("in_memory.h5", None, "R0247.dir", CH_MASS)
        assert W.n_times == t.size and W.m_is_scaled_out
        out[f"{name}_t"] = np.asarray(W.t)
        out[f"{name}_radii"] = np.asarray(Radii)
        out[f"{name}_data"] = np.asarray(W.data)[::ROW_STEP]
        out[f"{name}_history"] = np.array(W.history)
    np.savez_compressed(os.path.join(HERE, "g33_ref_finite_radius.npz"),
                        source="scri/extrapolation.py:343-417 (the reference's file, stand-ins underneath, arrays for its file reader)", **out)


if __name__ == "__main__":
    main()
    print("wrote g33")
