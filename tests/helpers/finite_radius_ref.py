"""The yardstick of the retardation of raw finite-radius series (scri/extrapolation.py:27-45 and :356-402 restated in numpy), shared by
tests/test_finite_radius_host.py and tests/test_gpu_finite_radius.py.  The one change: the running sum of the cumulative trapezoid is
replaced by EXACTLY rounded prefix sums (math.fsum over each prefix), so that the yardstick carries no summation error of its own;
numpy's own cumsum -- the reference's arithmetic to the bit -- is kept as a second output."""
import math

import numpy as np

# (UnitScaleFactor as a function of ChMass, RadiusRatioExp) by the name of the data type (scri/extrapolation.py:364-386)
SCALING = {
    "h": (lambda M: 1.0 / M, 1),
    "hdot": (lambda M: 1.0, 1),
    "psi4": (lambda M: M, 1),
    "psi3": (lambda M: 1.0, 2),
    "psi2": (lambda M: 1.0 / M, 3),
    "psi1": (lambda M: 1.0 / M**2, 4),
    "psi0": (lambda M: 1.0 / M**3, 5),
}
DATA_TYPES = tuple(SCALING)


def restarting_axis(rng, n, step):
    """n times with restarts (back into the axis, back before its start), ties and steps of `step`"""
    t = np.cumsum(rng.choice([step, step, 0.05, 0.3, 1.0], n)) + rng.uniform(-5.0, 5.0)
    for _ in range(rng.integers(0, 4) if n > 1 else 0):
        k = int(rng.integers(1, n))
        t[k:] -= rng.choice([0.0, 1e-3, 0.4, 2.5, 1e3])
    for _ in range(rng.integers(0, 3) if n > 1 else 0):
        k = int(rng.integers(1, n))
        t[k] = t[k - 1]
    return t


def keep_rule(T, MinTimeStep=1.0e-3):
    """indices k with fl(T[k] + MinTimeStep) < min_{j > k} T[j]: the statement the kernel scans"""
    T = np.asarray(T, dtype=float)
    later = np.full(T.size, np.inf)
    if T.size > 1:
        later[:-1] = np.minimum.accumulate(T[::-1])[::-1][1:]
    return np.flatnonzero(T + MinTimeStep < later)


def retard(t, areal_radius, average_lapse, data, coord_radius, initial_adm_energy, ch_mass, data_type, frame=None, MinTimeStep=1.0e-3, exact=True):
    """dict(idx, t, t_cumsum, t_cum, r_star, radii, data, factor, frame): t from exactly rounded prefix sums, t_cumsum from np.cumsum;
    t_cum (the integral plus T[0]) and r_star unscaled, for the bars.  exact=False (long axes: the exact sums cost n^2) leaves numpy's
    cumsum in both"""
    idx = keep_rule(t, MinTimeStep)
    T = np.asarray(t, dtype=float)[idx]
    Radii = np.asarray(areal_radius, dtype=float)[idx]
    lapse = np.asarray(average_lapse, dtype=float)[idx]
    g = lapse / np.sqrt(((-2.0 * initial_adm_energy) / Radii) + 1.0)
    terms = np.diff(T) * (g[1:] + g[:-1]) / 2.0  # (scipy.integrate.cumulative_trapezoid: d * (y[1:] + y[:-1]) / 2.0, then cumsum)
    exact = np.array([math.fsum(terms[: j + 1]) for j in range(terms.size)]) if exact else np.cumsum(terms)
    r_star = Radii + (2.0 * initial_adm_energy) * np.log((Radii / (2.0 * initial_adm_energy)) - 1.0)
    out = {}
    for name, sums in (("t", exact), ("t_cumsum", np.cumsum(terms))):
        Tc = T.copy()
        Tc[1:] = sums + T[0]
        if name == "t":
            out["t_cum"] = Tc.copy()
        Tc -= r_star
        out[name] = Tc / ch_mass
    unit, p = SCALING[data_type][0](ch_mass), SCALING[data_type][1]
    factor = (Radii / coord_radius) ** float(p) * unit
    out.update(idx=idx, r_star=r_star, radii=Radii / ch_mass, factor=factor, exponent=p, data=np.asarray(data)[idx] * factor[:, None],
               frame=None if frame is None else np.asarray(frame)[idx])
    return out
