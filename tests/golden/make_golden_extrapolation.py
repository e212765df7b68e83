"""Generator of g29_ref_extrapolation.npz: the reference's own extrapolation code (scri/extrapolation.py, unmodified -- `_Extrapolate`,
`set_common_time`, `intersection`, `monotonic_indices`) run on the stand-ins of reference_standins.py (numba, quaternion,
spherical_functions ...; tqdm is real).  Run from the repository root where the reference is available:

    python tests/golden/make_golden_extrapolation.py

The inputs are built by `fit_inputs` / `common_time_inputs` below from fixed seeds (plain numpy), so the tests regenerate them
instead of storing them:
  fit_inputs:  12 radii r_i(t) = R_i (1 + 0.01 sin(0.003 t + i)), R_i from 100 to 1000, 2000 steps, l = 2..8 (77 modes).
               "poly": y_i = sum_{k<=3} c_k(t) / r_i^k, so the limit c_0 is known exactly; "noisy": the same plus 1e-3 noise.
               Orders [-1, 2, 3, 4, 5]; every 40th output row is kept (the size limit of a committed file).
  common_time_inputs: four waveforms (l = 2..3) on shifted, non-uniform time axes with their radii, through set_common_time.
Also kept: intersection / monotonic_indices on fixed axes, and the exception type and message of each malformed call of
_Extrapolate.
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORDERS = [-1, 2, 3, 4, 5]
ROW_STEP = 40


def fit_inputs(kind):
    """(t, radii f8[12][2000], data c16[12][2000][77], exact limit c16[2000][77]); kind "poly" or "noisy" """
    rng = np.random.default_rng(2029)
    n_r, n_t, n_m = 12, 2000, 77
    t = np.linspace(0.0, 2000.0, n_t)
    R = np.geomspace(100.0, 1000.0, n_r)
    radii = R[:, None] * (1.0 + 0.01 * np.sin(0.003 * t[None, :] + np.arange(n_r)[:, None]))
    omega = rng.uniform(0.01, 0.2, n_m)
    phase = np.exp(1j * omega[None, :] * t[:, None])
    c = [(rng.normal(size=n_m) + 1j * rng.normal(size=n_m)) * s * phase * (1 + 0.3 * np.cos(0.001 * k * t))[:, None]
         for k, s in enumerate((1.0, 50.0, 1.0e3, 1.0e4))]
    data = sum(c[k][None, :, :] / radii[:, :, None] ** k for k in range(4))
    if kind == "noisy":
        data = data + 1e-3 * (np.random.default_rng(2030).normal(size=data.shape) + 1j * np.random.default_rng(2031).normal(size=data.shape))
    return t, radii, data, c[0]


def common_time_inputs():
    rng = np.random.default_rng(2032)
    out = []
    for i in range(4):
        n = 200 + 7 * i
        t = np.sort(rng.uniform(0.0, 100.0, n)) + 2.0 * i - 3.0
        t[0], t[-1] = -3.0 + 2.0 * i, 97.0 + 2.0 * i
        r = 100.0 * (i + 1) + 0.5 * np.sin(0.05 * t)
        data = (rng.normal(size=12) + 1j * rng.normal(size=12))[None, :] * np.exp(1j * 0.1 * (i + 1) * t)[:, None]
        out.append((t, r, data))
    return out


def main():
    sys.path.insert(0, HERE)
    import reference_standins as standins

    scri = standins.install()
    from scri.extrapolation import _Extrapolate, intersection, monotonic_indices, set_common_time

    def wm(t, data, ell_min=2, ell_max=8):
        return scri.WaveformModes(t=t, data=data, ell_min=ell_min, ell_max=ell_max, frameType=scri.Corotating, dataType=scri.h,
                                  r_is_scaled_out=True, m_is_scaled_out=True)

    out = {"orders": np.array(ORDERS), "row_step": ROW_STEP}
    for kind in ("poly", "noisy"):
        t, radii, data, _ = fit_inputs(kind)
        Ws = [wm(t, data[i]) for i in range(len(radii))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = _Extrapolate(Ws, list(radii), ORDERS)
        for N, W in zip(ORDERS, res):
            out[f"{kind}_N{N}"] = np.asarray(W.data)[::ROW_STEP]
            out[f"{kind}_N{N}_history_tail"] = np.array([h for h in W.history if h.startswith("### Extrapolating")])
    # set_common_time
    items = common_time_inputs()
    Ws = [wm(t, d, 2, 3) for t, _, d in items]
    Radii = [r for _, r, _ in items]
    set_common_time(Ws, Radii, 0.005, -3e300, 3e300)
    out["common_t"] = Ws[0].t
    out["common_radii"] = np.array(Radii)
    out["common_data"] = np.array([np.asarray(W.data) for W in Ws])
    # intersection / monotonic_indices
    t1 = np.linspace(0.0, 9.0, 40) + 0.03 * np.sin(np.arange(40))
    t2 = np.linspace(0.7, 11.0, 31) + 0.05 * np.cos(np.arange(31))
    out.update(isect_t1=t1, isect_t2=t2, isect_plain=intersection(t1, t2), isect_step=intersection(t1, t2, 0.2),
               isect_bounds=intersection(t1, t2, min_time=2.0, max_time=7.5),
               isect_limits=intersection([-3e300, 3e300], t1, 0.005, -3e300, 3e300))
    T = np.array([0.0, 1.0, 2.0, 1.5, 2.5, 3.0, 3.0005, 4.0, 3.9, 3.95, 5.0, 6.0])
    out["mono_T"] = T
    out["mono_default"] = np.asarray(monotonic_indices(T))
    out["mono_step"] = np.asarray(monotonic_indices(T, MinTimeStep=0.2))
    # errors of malformed calls
    t, radii, data, _ = fit_inputs("poly")
    n = 50
    base = lambda k=4: [wm(t[:n], data[i, :n]) for i in range(k)]
    rad = lambda k=4: [radii[i, :n] for i in range(k)]
    short = wm(t[: n - 1], data[0, : n - 1])
    fewer_modes = wm(t[:n], data[0, :n, :45], 2, 6)
    cases = {
        "min_order_beyond_radii": lambda: _Extrapolate(base(), rad(), [-5, 2]),
        "max_order_beyond_radii": lambda: _Extrapolate(base(), rad(), [4]),
        "radii_count": lambda: _Extrapolate(base(), rad(3), [2]),
        "n_times": lambda: _Extrapolate(base(3) + [short], rad(), [2]),
        "n_modes": lambda: _Extrapolate(base(3) + [fewer_modes], rad(), [2]),
        "radius_length": lambda: _Extrapolate(base(), rad(3) + [radii[3, : n - 1]], [2]),
    }
    errors = {}
    for name, call in cases.items():
        try:
            call()
            errors[name] = None
        except Exception as e:  # noqa: BLE001  (recorded as it is)
            errors[name] = [type(e).__name__, str(e)]
    out["errors_json"] = np.array(json.dumps(errors))
    np.savez_compressed(os.path.join(HERE, "g29_ref_extrapolation.npz"),
                        source="scri/extrapolation.py:27-125, 539-554, 1270-1474 (the reference's file, stand-ins underneath)", **out)


if __name__ == "__main__":
    main()
    print("wrote g29")
