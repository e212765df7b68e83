"""scri/asymptotic_bondi_data/map_to_superrest_frame.py:108-224 restated statement by statement on numpy, scipy.interpolate.CubicSpline and
the oracle's spinsfast (oracle.spinsfast_ref): the yardstick of bms_supermomentum_on_cut and bms_alpha_perturbation.  The splines are per
pixel and through the WHOLE series, as the reference takes them; `window` restricts them to rows [lo, hi) for the window identity."""
import numpy as np
from scipy.interpolate import CubicSpline

from oracle.spinsfast_ref import map2salm, salm2map

REACH = 64


def LM_index(ell, m, ell_min=0):
    return ell * (ell + 1) - ell_min**2 + m


def charge_vector_from_aspect(charge):
    """bms_charges.py:50-67"""
    charge = np.asarray(charge)
    four_vector = np.empty(charge.shape[:-1] + (4,), dtype=float)
    four_vector[..., 0] = charge[..., 0].real
    four_vector[..., 1] = (charge[..., 1] - charge[..., 3]).real / np.sqrt(6)
    four_vector[..., 2] = (charge[..., 1] + charge[..., 3]).imag / np.sqrt(6)
    four_vector[..., 3] = charge[..., 2].real / np.sqrt(3)
    return four_vector / np.sqrt(4 * np.pi)


def ell_factors(ell_max, f):
    return np.concatenate([np.full(2 * ell + 1, f(ell)) for ell in range(ell_max + 1)])


def D(h, ell_max):
    """:76-92"""
    return np.asarray(h) * ell_factors(ell_max, lambda l: 0.0 if l < 2 else (l + 2) * (l + 1) * l * (l - 1) / 4.0)


def D_inverse(h, ell_max):
    """:95-105"""
    return np.asarray(h) * ell_factors(ell_max, lambda l: 0.0 if l < 2 else 4.0 / ((l + 2) * (l + 1) * l * (l - 1)))


def rest_mass_and_conformal_factor(PsiM, ell_max):
    """:108-152"""
    PsiM = np.asarray(PsiM)
    n = 2 * ell_max + 1
    P = -charge_vector_from_aspect(PsiM[..., :4])
    grids = []
    for L, M in [(0, 0), (1, -1), (1, 0), (1, +1)]:
        modes = np.zeros((ell_max + 1) ** 2, dtype=complex)
        modes[LM_index(L, M)] = 1
        grids.append(salm2map(modes, 0, ell_max, n, n))
    r_vector = 4 * np.pi * charge_vector_from_aspect(np.array(grids).transpose()).transpose()
    if PsiM.ndim > 1:
        M_Grid = np.sqrt(P[:, 0] ** 2 - (P[:, 1] ** 2 + P[:, 2] ** 2 + P[:, 3] ** 2))
        K_Grid = M_Grid[:, None, None] / (
            np.tensordot(P[:, 0], r_vector[0], axes=0)
            - (np.tensordot(P[:, 1], r_vector[1], axes=0) + np.tensordot(P[:, 2], r_vector[2], axes=0) + np.tensordot(P[:, 3], r_vector[3], axes=0))
        )
    else:
        M_Grid = np.sqrt(P[0] ** 2 - (P[1] ** 2 + P[2] ** 2 + P[3] ** 2))
        K_Grid = M_Grid / (P[0] * r_vector[0] - (P[1] * r_vector[1] + P[2] * r_vector[2] + P[3] * r_vector[3]))
    return M_Grid, K_Grid


def rows_near(t, times, reach=REACH):
    """the window rule of the engine entry (scri_amd.map_to_superrest_frame._rows_near)"""
    times = np.asarray(times, dtype=float)
    lo = int(np.searchsorted(t, times.min(), side="right")) - 1 - reach
    hi = int(np.searchsorted(t, times.max(), side="left")) + 1 + reach
    return max(lo, 0), min(hi, len(t))


def supermomentum_on_cut(t, PsiM, alpha, ell_max, window=None):
    """:155-197.  Returns (modes, PsiM at alpha, K at alpha, D alpha on the grid), the last three [2 ell_max + 1, 2 ell_max + 1]."""
    t, PsiM, alpha = np.asarray(t, dtype=float), np.asarray(PsiM), np.asarray(alpha, dtype=float)
    if window is not None:
        t, PsiM = t[window[0] : window[1]], PsiM[window[0] : window[1]]
    n = 2 * ell_max + 1
    M_Grid, K_Grid = rest_mass_and_conformal_factor(PsiM, ell_max)
    PsiM_Grid = salm2map(PsiM, 0, ell_max, n, n).real  # (PsiM.grid(): every row)
    PsiM_Grid_interp, K_Grid_interp = np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            PsiM_Grid_interp[i, j] = CubicSpline(t, PsiM_Grid[:, i, j])(alpha[i, j])
            K_Grid_interp[i, j] = CubicSpline(t, K_Grid[:, i, j])(alpha[i, j])
    alpha_modes = map2salm(alpha.astype(complex), 0, ell_max)
    D_alpha_Grid = salm2map(D(alpha_modes, ell_max), 0, ell_max, n, n)
    modes = map2salm((PsiM_Grid_interp - D_alpha_Grid) / K_Grid_interp**3, 0, ell_max)
    return modes, PsiM_Grid_interp, K_Grid_interp, D_alpha_Grid


def alpha_perturbation(PsiM, M_Grid, K_Grid, ell_max):
    """:200-224; M_Grid / K_Grid None: those of PsiM itself (:108-152 on the one row)"""
    n = 2 * ell_max + 1
    if M_Grid is None or K_Grid is None:
        M_own, K_own = rest_mass_and_conformal_factor(PsiM, ell_max)
        M_Grid = M_own if M_Grid is None else M_Grid
        K_Grid = K_own if K_Grid is None else K_Grid
    PsiM_Grid = salm2map(np.asarray(PsiM), 0, ell_max, n, n)
    PsiM_plus_M_K3 = map2salm(PsiM_Grid + M_Grid * K_Grid**3, 0, ell_max)
    return salm2map(D_inverse(PsiM_plus_M_K3, ell_max), 0, ell_max, n, n).real


# ------------------------------------------------------------------------------------------------ cases
def smooth_series(t, ell_max, seed, mass=1.0, size=0.02):
    """Psi_M rows with a monopole of -sqrt(4 pi) mass and small smooth higher modes, decaying with l: M^2 > 0 and K > 0 on every row
    (asserted), so that no case is ever left out"""
    rng = np.random.default_rng(seed)
    t = np.asarray(t, dtype=float)
    nm = (ell_max + 1) ** 2
    ells = np.concatenate([np.full(2 * l + 1, l) for l in range(ell_max + 1)])
    amp = size / (1.0 + ells) ** 2
    span = max(t[-1] - t[0], 1.0)
    s = (t - t[0]) / span
    data = np.zeros((t.size, nm), dtype=complex)
    for k in range(1, 4):
        c = (rng.standard_normal(nm) + 1j * rng.standard_normal(nm)) * amp
        data += c[None, :] * np.sin(k * (1.3 * s[:, None] + rng.uniform(0, 2 * np.pi, nm)[None, :]))
    data[:, 0] += -np.sqrt(4 * np.pi) * mass * (1.0 + 0.01 * s)
    P = -charge_vector_from_aspect(data[:, :4])
    assert np.all(P[:, 0] ** 2 - (P[:, 1:] ** 2).sum(axis=1) > 0.5), "the case needs a timelike four-momentum on every row"
    return data


def smooth_alpha(ell_max, seed, centre, half_range):
    """a smooth real function on the grid with values in [centre - half_range, centre + half_range]"""
    rng = np.random.default_rng(seed)
    n = 2 * ell_max + 1
    low = min(ell_max, 3)
    modes = np.zeros((ell_max + 1) ** 2, dtype=complex)
    for l in range(low + 1):
        for m in range(0, l + 1):
            c = rng.standard_normal() + (1j * rng.standard_normal() if m else 0)
            modes[LM_index(l, m)] = c
            modes[LM_index(l, -m)] = (-1) ** m * np.conj(c)
    g = salm2map(modes, 0, ell_max, n, n).real
    g = g - 0.5 * (g.max() + g.min())
    return centre + half_range * g / max(np.abs(g).max(), 1e-300)
