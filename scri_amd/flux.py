"""Fluxes of energy, momentum, angular momentum and boost carried by a waveform h (scri/flux.py:182-798; Ruiz et al. 0707.4654
eqs. (2.8), (2.11), (2.24); Flanagan & Nichols 1510.03386 eq. (C.1) for the boost flux).

The reference writes every term as an expectation value <a|M|b> = sum conj(a_jn) M_jnlm b_lm with sparse matrices of Clebsch-Gordan
coefficients.  Every one of those operators is multiplication by an l = 1 function -- chi = cos(theta), sin(theta) e^{+-i phi}, or
eth chi / ethbar chi -- so <a|chi|b> is the integral of conj(a) b against that function, i.e. a combination of the l = 1 modes of
the product conj(a) b: ONE `bms_grid_multiply` with output_ell_max = 1 per pair (a, b) (synthesis of both factors on a grid that
resolves the product, pointwise product, analysis), no matrix-element tables; the angular-momentum operators act along the mode axis
(`bms_mode_map`) and leave an l = 0 mode to take.  Same numbers as the sparse sums to rounding (tests/test_golden.py, vectors made
by the reference's own flux.py).

That is the route of host-resident waveforms (the host_* functions).  A waveform resident on the GPU goes through ONE launch of
bms_poincare_fluxes instead (kernels_flux.hip: the banded sums themselves, read from h and hdot where they are), and the reference's
building blocks behind the fluxes -- the generators p_z ... j_minus, sparse_expectation_value, matrix_expectation_value -- are mirrored
at the end of this file."""
import functools
import math

import numpy as np

from . import engine
from . import h as htype, hdot as hdottype
from .mode_algebra import LM_range

SQRT_8PI_3 = math.sqrt(8.0 * math.pi / 3.0)
SQRT_4PI_3 = math.sqrt(4.0 * math.pi / 3.0)


class _Field:
    """modes from l = 0 of a function of spin weight s at every time step (host array)"""

    def __init__(self, data, s, ell_min, ell_max, ctx):
        full = np.zeros((data.shape[0], (ell_max + 1) ** 2), dtype=complex)
        full[:, ell_min**2:] = data
        self.data, self.s, self.ell_max, self.ctx = full, s, ell_max, ctx

    def bar(self):
        """modes of the conjugate function: (-1)^(s+m) conj(f_l,-m), spin -s (one launch of bms_mode_map)"""
        LM = LM_range(0, self.ell_max)
        ell, m = LM[:, 0], LM[:, 1]
        partner = (ell * (ell + 1) - m).astype(np.int32)
        sign = np.where((self.s + m) % 2 == 0, 1.0, -1.0).astype(complex)
        out = _Field.__new__(_Field)
        out.data = engine.mode_map(self.data, partner, sign, True, ctx=self.ctx)
        out.s, out.ell_max, out.ctx = -self.s, self.ell_max, self.ctx
        return out

    def laddered(self, step):
        """eth (step = +1) or ethbar (-1), Newman-Penrose convention (scri/waveform_modes.py:478-572)"""
        LM = LM_range(0, self.ell_max)
        ell = LM[:, 0].astype(float)
        s = self.s
        f = np.where(ell >= abs(s), np.sqrt(np.maximum((ell - s * step) * (ell + s * step + 1.0), 0.0)), 0.0) * step
        out = _Field.__new__(_Field)
        out.data = engine.mode_map(self.data, np.arange(ell.size, dtype=np.int32), f.astype(complex), ctx=self.ctx)
        out.s, out.ell_max, out.ctx = s + step, self.ell_max, self.ctx
        return out


def _ell1_of_product(a, b):
    """modes (0,0), (1,-1), (1,0), (1,1) of conj(a) b, a function of spin b.s - a.s, at every time step"""
    abar = a.bar()
    L = max(a.ell_max, b.ell_max)
    return engine.grid_multiply(abar.data, abar.s, a.ell_max, b.data, b.s, b.ell_max, 2 * L, 1, ctx=a.ctx)


def _chi(a, b):
    """<a|chi|b> for chi = sin(theta) e^{+i phi}, sin(theta) e^{-i phi}, cos(theta) (the reference's p_plus, p_minus, p_z,
    scri/flux.py:213-301): integral of P Y_1m = (-1)^m P_1,-m with P = conj(a) b (spin 0)"""
    P = _ell1_of_product(a, b)
    return SQRT_8PI_3 * P[:, 1], -SQRT_8PI_3 * P[:, 3], SQRT_4PI_3 * P[:, 2]


def _eth_chi(a, b):
    """<a|eth chi|b>, a of spin s + 1, b of spin s (scri/flux.py:471-560): eth Y_1m = sqrt2 1Y_1m, and the integral of
    Q 1Y_1m = (-1)^(1+m) Q_1,-m with Q = conj(a) b (spin -1)"""
    Q = _ell1_of_product(a, b)
    r2 = math.sqrt(2.0)
    # chi_+ = -sqrt(8pi/3) Y_11, chi_- = +sqrt(8pi/3) Y_1-1, chi_z = sqrt(4pi/3) Y_10
    plus = -SQRT_8PI_3 * r2 * (+1.0) * Q[:, 1]   # m = +1: (-1)^(1+1) Q_{1,-1}
    minus = SQRT_8PI_3 * r2 * (+1.0) * Q[:, 3]   # m = -1: (-1)^(1-1) Q_{1,+1}
    z = SQRT_4PI_3 * r2 * (-1.0) * Q[:, 2]       # m = 0: (-1)^1 Q_{1,0}
    return plus, minus, z


def _ethbar_chi(a, b):
    """<a|ethbar chi|b>, a of spin s, b of spin s + 1: ethbar Y_1m = -sqrt2 -1Y_1m, and the integral of
    R -1Y_1m = (-1)^(1+m) R_1,-m with R = conj(a) b (spin +1).  (The reference's matrix element of this name, scri/flux.py:487-600,
    leaves the minus sign of ethbar Y out and subtracts the term instead: the same sum.)"""
    R = _ell1_of_product(a, b)
    r2 = -math.sqrt(2.0)
    plus = -SQRT_8PI_3 * r2 * (+1.0) * R[:, 1]
    minus = SQRT_8PI_3 * r2 * (+1.0) * R[:, 3]
    z = SQRT_4PI_3 * r2 * (-1.0) * R[:, 2]
    return plus, minus, z


def _xyz(plus, minus, z):
    """(plus, minus, z) components -> (x, y, z) as the reference does (scri/flux.py:337-341)"""
    return np.stack([0.5 * (plus.real + minus.real), 0.5 * (plus.imag - minus.imag), z.real], axis=1)


def _check(h, what):
    from .waveform_modes import WaveformModes

    if not isinstance(h, WaveformModes):
        raise ValueError(f"{what} can only be calculated from a `WaveformModes` object; this object is of type `{type(h)}`.")


def _hdot_data(h):
    if h.dataType == hdottype:
        return h.data
    if h.dataType == htype:
        return h.data_dot
    raise ValueError(f"Input argument is expected to have data of type `h` or `hdot`; this waveform data has type `{h.data_type_string}`")


def _h_and_hdot(h, hdot, what):
    from .waveform_modes import WaveformModes

    _check(h, what)
    if (hdot is not None) and (not isinstance(hdot, WaveformModes)):
        raise ValueError(f"{what} can only be calculated from a `WaveformModes` object; `hdot` is of type `{type(hdot)}`.")
    if h.dataType != htype:
        raise ValueError(f"Input argument `h` is expected to have data of type `h`; this `h` waveform data has type `{h.data_type_string}`")
    if hdot is None:
        return h.data, h.data_dot
    if hdot.dataType != hdottype:
        raise ValueError(f"Input argument `hdot` is expected to have data of type `hdot`; this `hdot` waveform data has type `{h.data_type_string}`")
    return h.data, hdot.data


def host_energy_flux(h):
    """Energy flux, eq. (2.8) of Ruiz et al.: sum_lm |hdot_lm|^2 / 16 pi"""
    _check(h, "Energy flux")
    hdot = _hdot_data(h)
    return np.einsum("ij, ij -> i", hdot.conjugate(), hdot).real / (16.0 * np.pi)


def host_momentum_flux(h):
    """Momentum flux, eq. (2.11) of Ruiz et al.: the integral of |hdot|^2 n / 16 pi"""
    _check(h, "Momentum flux")
    f = _Field(_hdot_data(h), -2, h.ell_min, h.ell_max, h._ctx)
    return _xyz(*_chi(f, f)) / (16.0 * np.pi)


def host_angular_momentum_flux(h, hdot=None):
    """Angular-momentum flux, eq. (2.24) of Ruiz et al.: -<hdot| J |h> / 16 pi with <j,n|J_z|l,m> = i m,
    <l,m+-1|J_+-|l,m> = i sqrt((l -+ m)(l +- m + 1))"""
    hd, hdd = _h_and_hdot(h, hdot, "Angular momentum flux")
    LM = LM_range(h.ell_min, h.ell_max)
    ell, m = LM[:, 0], LM[:, 1]
    own = np.arange(ell.size, dtype=np.int32)
    # (J h) column by column: J_z keeps the column; J_+ fills (l, m) from (l, m - 1), J_- from (l, m + 1)
    jz = engine.mode_map(hd, own, 1j * m.astype(complex), ctx=h._ctx)
    up_src = np.where(m - 1 >= -ell, own - 1, -1).astype(np.int32)
    up = engine.mode_map(hd, up_src, 1j * np.sqrt(np.maximum((ell - (m - 1)) * (ell + (m - 1) + 1.0), 0.0)).astype(complex), ctx=h._ctx)
    dn_src = np.where(m + 1 <= ell, own + 1, -1).astype(np.int32)
    dn = engine.mode_map(hd, dn_src, 1j * np.sqrt(np.maximum((ell + (m + 1)) * (ell - (m + 1) + 1.0), 0.0)).astype(complex), ctx=h._ctx)
    dot = lambda x: np.einsum("ij, ij -> i", hdd.conjugate(), x)  # noqa: E731
    return _xyz(dot(up), dot(dn), dot(jz)) / (-16.0 * np.pi)


def host_boost_flux(h, hdot=None):
    """Boost flux, eq. (C.1) of Flanagan & Nichols in the Newman-Penrose form of scri/flux.py:444-748:
    (-1/32 pi) { (1/8) [<ebN|chi|ebh> - <eN|chi|eh> + 6 <N|chi|h> + <ebh|chi|ebN> - <eh|chi|eN> + 6 <h|chi|N>]
                 - (u/2) <N|chi|N> - (1/4) [<eN|e chi|h> + <h|eb chi|eN>] },   N = hdot, e = eth, eb = ethbar"""
    hd, hdd = _h_and_hdot(h, hdot, "Boost fluxes")
    H = _Field(hd, -2, h.ell_min, h.ell_max, h._ctx)
    N = _Field(hdd, -2, h.ell_min, h.ell_max, h._ctx)
    eH, ebH, eN, ebN = H.laddered(+1), H.laddered(-1), N.laddered(+1), N.laddered(-1)
    terms = [np.zeros(h.n_times, dtype=complex) for _ in range(3)]

    def add(factor, values):
        for k in range(3):
            terms[k] = terms[k] + factor * values[k]

    add(1 / 8, _chi(ebN, ebH))
    add(-1 / 8, _chi(eN, eH))
    add(6 / 8, _chi(N, H))
    add(1 / 8, _chi(ebH, ebN))
    add(-1 / 8, _chi(eH, eN))
    add(6 / 8, _chi(H, N))
    nn = _chi(N, N)
    add(-0.5, tuple(h.t * v for v in nn))
    add(-1 / 4, _eth_chi(eN, H))
    add(-1 / 4, _ethbar_chi(H, eN))
    return _xyz(*terms) / (-32.0 * np.pi)


def host_poincare_fluxes(h, hdot=None):
    """(energy, momentum, angular-momentum, boost) flux with one time derivative for all four (scri/flux.py:750-798)"""
    from .waveform_modes import WaveformModes

    _check(h, "Poincare fluxes")
    if (hdot is not None) and (not isinstance(hdot, WaveformModes)):
        raise ValueError(f"Poincare fluxes can only be calculated from a `WaveformModes` object; `hdot` is of type `{type(hdot)}`.")
    if h.dataType != htype:
        raise ValueError(f"Input argument `h` is expected to have data of type `h`; this `h` waveform data has type `{h.data_type_string}`")
    if hdot is None:
        hdot = h.copy()
        hdot.dataType = hdottype
        hdot.data = h.data_dot
    elif hdot.dataType != hdottype:
        raise ValueError(f"Input argument `hdot` is expected to have data of type `hdot`; this `hdot` waveform data has type `{h.data_type_string}`")
    return host_energy_flux(hdot), host_momentum_flux(hdot), host_angular_momentum_flux(h, hdot), host_boost_flux(h, hdot)


# ---------------------------------------------------------------------------------------------------- device-resident waveforms
# A waveform moved to the GPU with to_device() goes through ONE launch of bms_poincare_fluxes (kernels_flux.hip): the banded sums of
# scri/flux.py with the ladder factors folded into three real coefficient sets, read once from h and hdot where they are.  Its weights
# (and a given hdot's) stay in HBM; only the N x 10 doubles of the result cross the link.  Host-resident waveforms, and device-resident
# ones that start below l = 2, keep the route above and its values bit for bit.


def _resident(w):
    return w.is_device_resident and w.ell_min >= 2 and w.ell_max >= w.ell_min and len(w._data_shape()) == 2 and w.n_times >= 1


def _device_modes(w, like):
    """the device tensor of w's weights for a fused call with the device-resident waveform `like` (a host-resident hdot is staged beside
    it and stays host resident); None if the two do not describe the same modes and times"""
    if (w.ell_min, w.ell_max, w.n_times) != (like.ell_min, like.ell_max, like.n_times) or len(w._data_shape()) != 2:
        return None
    if w.is_device_resident:
        return w._dev
    from . import device_series

    return device_series.to_device(like._ctx, np.ascontiguousarray(w._host, dtype=complex))


def _derivative_on_device(w):
    return engine.spline_derivative(w.t, w._dev, w.t, 1, ctx=w._ctx)


def _fused(t, h_dev, hdot_dev, w, want):
    out = engine.poincare_fluxes(t, h_dev, hdot_dev, w.ell_min, w.ell_max, want=want, ctx=w._ctx)
    return out.cpu().numpy() if isinstance(want, str) else tuple(o.cpu().numpy() for o in out)


def _device_hdot_only(h, what):
    """energy / momentum flux: the device tensor of hdot for a device-resident `h` of type h or hdot (the checks and texts of the host
    route, none of which reads the data)"""
    _check(h, what)
    if h.dataType == hdottype:
        return h._dev
    if h.dataType == htype:
        return _derivative_on_device(h)
    raise ValueError(f"Input argument is expected to have data of type `h` or `hdot`; this waveform data has type `{h.data_type_string}`")


def _device_pair(h, hdot, what):
    """(h, hdot) as device tensors for a device-resident h, after the host route's checks; None if a given hdot does not fit h"""
    from .waveform_modes import WaveformModes

    _check(h, what)
    if (hdot is not None) and (not isinstance(hdot, WaveformModes)):
        raise ValueError(f"{what} can only be calculated from a `WaveformModes` object; `hdot` is of type `{type(hdot)}`.")
    if h.dataType != htype:
        raise ValueError(f"Input argument `h` is expected to have data of type `h`; this `h` waveform data has type `{h.data_type_string}`")
    if hdot is None:
        return h._dev, _derivative_on_device(h)
    if hdot.dataType != hdottype:
        raise ValueError(f"Input argument `hdot` is expected to have data of type `hdot`; this `hdot` waveform data has type `{h.data_type_string}`")
    n = _device_modes(hdot, h)
    return None if n is None else (h._dev, n)


def _is_waveform(h):
    from .waveform_modes import WaveformModes

    return isinstance(h, WaveformModes)


def energy_flux(h):
    """Energy flux, eq. (2.8) of Ruiz et al.: sum_lm |hdot_lm|^2 / 16 pi"""
    if _is_waveform(h) and _resident(h):
        return _fused(None, None, _device_hdot_only(h, "Energy flux"), h, "energy")
    return host_energy_flux(h)


def momentum_flux(h):
    """Momentum flux, eq. (2.11) of Ruiz et al.: the integral of |hdot|^2 n / 16 pi"""
    if _is_waveform(h) and _resident(h):
        return _fused(None, None, _device_hdot_only(h, "Momentum flux"), h, "momentum")
    return host_momentum_flux(h)


def angular_momentum_flux(h, hdot=None):
    """Angular-momentum flux, eq. (2.24) of Ruiz et al.: -<hdot| J |h> / 16 pi"""
    if _is_waveform(h) and _resident(h):
        pair = _device_pair(h, hdot, "Angular momentum flux")
        if pair is not None:
            return _fused(None, pair[0], pair[1], h, "angular")
    return host_angular_momentum_flux(h, hdot)


def boost_flux(h, hdot=None):
    """Boost flux, eq. (C.1) of Flanagan & Nichols in the Newman-Penrose form of scri/flux.py:444-748 (host_boost_flux spells it out)"""
    if _is_waveform(h) and _resident(h):
        pair = _device_pair(h, hdot, "Boost fluxes")
        if pair is not None:
            return _fused(h.t, pair[0], pair[1], h, "boost")
    return host_boost_flux(h, hdot)


def poincare_fluxes(h, hdot=None):
    """(energy, momentum, angular-momentum, boost) flux with one time derivative for all four (scri/flux.py:750-798); of a
    device-resident waveform: one derivative and one launch"""
    if _is_waveform(h) and _resident(h):
        pair = _device_pair(h, hdot, "Poincare fluxes")
        if pair is not None:
            return _fused(h.t, pair[0], pair[1], h, engine.FLUX_NAMES)
    return host_poincare_fluxes(h, hdot)


# ---------------------------------------------------------------------------------------------------- the reference's building blocks
# swsh_indices_to_matrix_indices, the generators p_z ... j_minus, sparse_expectation_value and matrix_expectation_value
# (scri/flux.py:11-179, 213-300, 345-391) with the reference's signatures.  The matrix elements are closed forms -- coupling with j = 1 --
# evaluated in extended precision and rounded once; the sums run on the GPU (bms_expectation_values).
_LD = np.longdouble


def _cg_one(ell, m, mu, J):
    """<ell, m; 1, mu | J, m + mu> (Condon-Shortley) in extended precision; zero outside the triangle and the m ranges"""
    M = m + mu
    if ell < 0 or J < 0 or abs(J - ell) > 1 or abs(m) > ell or abs(M) > J or abs(mu) > 1:
        return _LD(0)
    L, Md = _LD(ell), _LD(M)
    if J == ell + 1:
        if mu == 1:
            return np.sqrt((L + Md) * (L + Md + 1) / ((2 * L + 1) * (2 * L + 2)))
        if mu == 0:
            return np.sqrt((L - Md + 1) * (L + Md + 1) / ((2 * L + 1) * (L + 1)))
        return np.sqrt((L - Md) * (L - Md + 1) / ((2 * L + 1) * (2 * L + 2)))
    if J == ell:
        if ell == 0:
            return _LD(0)
        if mu == 1:
            return -np.sqrt((L + Md) * (L - Md + 1) / (2 * L * (L + 1)))
        if mu == 0:
            return Md / np.sqrt(L * (L + 1))
        return np.sqrt((L - Md) * (L + Md + 1) / (2 * L * (L + 1)))
    if mu == 1:
        return np.sqrt((L - Md) * (L - Md + 1) / (2 * L * (2 * L + 1)))
    if mu == 0:
        return -np.sqrt((L - Md) * (L + Md) / (L * (2 * L + 1)))
    return np.sqrt((L + Md + 1) * (L + Md) / (2 * L * (2 * L + 1)))


def _chi_element(s, ellp, ell, m, mu):
    """<s, ellp, m + mu| chi_mu |s, ell, m> in extended precision: chi_0 = cos(theta), chi_+-1 = sin(theta) e^{+-i phi}"""
    ratio = (2 * _LD(ell) + 1) / (2 * _LD(ellp) + 1)
    spin = _cg_one(ell, -s, 0, ellp)
    if mu == 0:
        return np.sqrt(ratio) * _cg_one(ell, m, 0, ellp) * spin
    return -mu * np.sqrt(2 * ratio) * _cg_one(ell, m, mu, ellp) * spin


def _ladder_chi_element(raise_, ellp, ell, m, mu):
    """the elements of eth chi between spins -1 and -2 (raise_) and of ethbar chi between spins -2 and -1, as the generators inside the
    reference's boost_flux give them (scri/flux.py:480-598)"""
    ratio = (2 * _LD(ell) + 1) / (2 * _LD(ellp) + 1)
    spin = _cg_one(ell, 2, -1, ellp) if raise_ else _cg_one(ell, 1, 1, ellp)
    if mu == 0:
        return np.sqrt(2 * ratio) * _cg_one(ell, m, 0, ellp) * spin
    return -mu * 2 * np.sqrt(ratio) * _cg_one(ell, m, mu, ellp) * spin


def _banded(ell_min, ell_max, mu, element):
    """(ellp, m + mu, ell, m, element) over the band ellp = ell - 1 .. ell + 1, in the reference's order: ell, then ellp, then m"""
    for ell in range(ell_min, ell_max + 1):
        for ellp in range(max(ell_min, ell - 1), min(ell_max, ell + 1) + 1):
            for m in range(-ell, ell + 1):
                if abs(m + mu) <= ellp:
                    yield ellp, m + mu, ell, m, float(element(ellp, ell, m))


def swsh_indices_to_matrix_indices(matrix_iterator):
    """Decorator: a generator f(ell_min, ell_max, ...) of (ellp, mp, ell, m, value) becomes a cached function of the same arguments that
    returns (rows, columns, values), the indices of (ellp, mp) and (ell, m) in a mode array that starts at ell_min
    (scri/flux.py:11-37); what sparse_expectation_value takes."""
    from .mode_algebra import LM_index

    @functools.lru_cache()
    def indexed(ell_min, ell_max, *args, **kwargs):
        rows, columns, values = [], [], []
        for ellp, mp, ell, m, value in matrix_iterator(ell_min, ell_max, *args, **kwargs):
            rows.append(LM_index(ellp, mp, ell_min))
            columns.append(LM_index(ell, m, ell_min))
            values.append(value)
        return np.array(rows, dtype=int), np.array(columns, dtype=int), np.array(values)

    functools.update_wrapper(indexed, matrix_iterator)
    return indexed


@swsh_indices_to_matrix_indices
def p_z(ell_min, ell_max, s=-2):
    """Matrix elements <s, j, n| cos(theta) |s, l, m> (nonzero for n = m only), for matrix_expectation_value (scri/flux.py:213-246)"""
    return _banded(ell_min, ell_max, 0, lambda ellp, ell, m: _chi_element(s, ellp, ell, m, 0))


@swsh_indices_to_matrix_indices
def p_plusminus(ell_min, ell_max, sign, s=-2):
    """Matrix elements of p+ = sin(theta) e^{+i phi} (sign = +1) or p- = sin(theta) e^{-i phi} (sign = -1), nonzero for n = m + sign
    (scri/flux.py:249-294)"""
    if (sign != 1) and (sign != -1):
        raise ValueError("sign must be either 1 or -1 in j_plusminus")
    return _banded(ell_min, ell_max, sign, lambda ellp, ell, m: _chi_element(s, ellp, ell, m, sign))


p_plus = functools.partial(p_plusminus, sign=+1)
p_minus = functools.partial(p_plusminus, sign=-1)
p_plus.__doc__ = p_plusminus.__doc__
p_minus.__doc__ = p_plusminus.__doc__


@swsh_indices_to_matrix_indices
def j_z(ell_min, ell_max):
    """Matrix elements <j, n| j_z |l, m> = i m (diagonal), the convention of Ruiz et al. (scri/flux.py:345-358)"""
    for ell in range(ell_min, ell_max + 1):
        for m in range(-ell, ell + 1):
            yield ell, m, ell, m, 1.0j * m


@swsh_indices_to_matrix_indices
def j_plusminus(ell_min, ell_max, sign):
    """Matrix elements <l, m + sign| j+- |l, m> = i sqrt((l -+ m)(l +- m + 1)) (scri/flux.py:361-385)"""
    if (sign != 1) and (sign != -1):
        raise ValueError("sign must be either 1 or -1 in j_plusminus")
    for ell in range(ell_min, ell_max + 1):
        for m in range(-ell, ell + 1):
            if abs(m + sign) <= ell:
                yield ell, m + sign, ell, m, 1.0j * float(np.sqrt(_LD((ell - sign * m) * (ell + sign * m + 1))))


j_plus = functools.partial(j_plusminus, sign=+1)
j_minus = functools.partial(j_plusminus, sign=-1)
j_plus.__doc__ = j_plusminus.__doc__
j_minus.__doc__ = j_plusminus.__doc__


# the generators inside the reference's boost_flux (not public there): <eth N| eth chi |h> and <h| ethbar chi |eth N> for s = -2
@swsh_indices_to_matrix_indices
def _eth_chi_elements(ell_min, ell_max, mu):
    return _banded(ell_min, ell_max, mu, lambda ellp, ell, m: _ladder_chi_element(True, ellp, ell, m, mu))


@swsh_indices_to_matrix_indices
def _ethbar_chi_elements(ell_min, ell_max, mu):
    return _banded(ell_min, ell_max, mu, lambda ellp, ell, m: _ladder_chi_element(False, ellp, ell, m, mu))


def _modes_of(x):
    """the mode weights of a waveform where they live (a device tensor or the host array), or the array / tensor itself"""
    if _is_waveform(x):
        return x._dev if x.is_device_resident else x.data
    return x


def sparse_expectation_value(abar, rows, columns, values, b):
    """sum_e abar[t, rows[e]] b[t, columns[e]] values[e] for every time step (scri/flux.py:41-78): abar is <a| with the complex
    conjugation already applied.  abar and b: host arrays [N, n] (a host array back), device tensors (a device tensor back), or
    waveforms, whose weights are read where they live and stay there."""
    a, bb = _modes_of(abar), _modes_of(b)
    ctx = next((x._ctx for x in (abar, b) if _is_waveform(x) and x._ctx is not None), None)
    return engine.expectation_values(a, rows, columns, values, bb, conj_a=False, ctx=ctx)


def matrix_expectation_value(a, M, b, allow_LM_differ=False, allow_times_differ=False):
    """The matrix expectation value <a|M|b>(u) = sum conj(a_jn(u)) M_jnlm b_lm(u) of two waveforms of one spin weight
    (scri/flux.py:81-179).  M(ell_min, ell_max) returns (rows, columns, values), as the generators above do.  allow_LM_differ: use the
    common ell range; allow_times_differ: interpolate both to the intersection of their times.  Returns (times, values), host arrays;
    device-resident waveforms are read, clipped and interpolated in HBM and stay resident."""
    from .mode_operators import time_intersection

    if a.spin_weight != b.spin_weight:
        raise ValueError("Spin weights must match in matrix_expectation_value")
    LM_clip = slice(a.ell_min, a.ell_max + 1)
    if (a.ell_min != b.ell_min) or (a.ell_max != b.ell_max):
        if not allow_LM_differ:
            raise ValueError("ell_min and ell_max must match in matrix_expectation_value (use allow_LM_differ=True to override)")
        LM_clip = slice(max(a.ell_min, b.ell_min), min(a.ell_max, b.ell_max) + 1)
        if LM_clip.start >= LM_clip.stop:
            raise ValueError("Intersection of (ell,m) modes is empty.  Assuming this is not desired.")
    t_clip = None
    if not np.array_equal(a.t, b.t):
        if not allow_times_differ:
            raise ValueError("Time samples must match in matrix_expectation_value (use allow_times_differ=True to override)")
        t_clip = time_intersection(a.t, b.t)
    times = a.t
    A, B = a[:, LM_clip], b[:, LM_clip]
    if t_clip is not None:
        times = t_clip
        A, B = A.interpolate(t_clip), B.interpolate(t_clip)
    rows, columns, values = M(LM_clip.start, LM_clip.stop - 1)
    ctx = A._ctx if A._ctx is not None else B._ctx
    if A.is_device_resident != B.is_device_resident:  # (one pair of rows lives in one memory: the host-resident side is staged beside the other)
        from . import device_series

        stage = lambda w: w._dev if w.is_device_resident else device_series.to_device(ctx if ctx is not None else engine._ctx(None), w.data)  # noqa: E731
        out = engine.expectation_values(stage(A), rows, columns, values, stage(B), conj_a=True, ctx=ctx)
    else:
        out = engine.expectation_values(_modes_of(A), rows, columns, values, _modes_of(B), conj_a=True, ctx=ctx)
    return times, (out.cpu().numpy() if hasattr(out, "cpu") else out)
