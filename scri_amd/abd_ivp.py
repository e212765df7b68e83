"""Bondi-gauge initial-value construction and constraint checks of AsymptoticBondiData
(scri/asymptotic_bondi_data/from_initial_values.py:2-154, constraints.py:9-278):

    psi0' = eth psi1 + 3 sigma psi2      psi1' = eth psi2 + 2 sigma psi3      psi2' = eth psi3 + sigma psi4
    psi3 = -eth d_u sigma-bar            psi4 = -d_u^2 sigma-bar              Im psi2 = -Im(eth^2 sigma-bar + sigma d_u sigma-bar)

Products of fields run on the GPU (bms_grid_multiply on a grid that is exact for the sum of the band limits, truncated to
ell_max as the reference's multiplication_truncator=max does), time derivatives and integrals through
bms_spline_derivative; the mode-space operators are diagonal maps applied with numpy.
"""
import math

import numpy as np

from . import engine
from .mode_algebra import LM_index


# ------------------------------------------------------------------------------------------------- helpers on [n, (L+1)^2] arrays
def _lfac(L, f):
    return np.concatenate([np.full(2 * l + 1, f(l)) for l in range(L + 1)])


def _eth(a, s, L):
    """GHP eth: x sqrt((l-s)(l+s+1)/2), spin s -> s+1"""
    return a * _lfac(L, lambda l: math.sqrt((l - s) * (l + s + 1) / 2.0) if l >= abs(s) and l >= abs(s + 1) else 0.0)


def _bar(a, s, L):
    out = np.empty_like(a)
    for l in range(L + 1):
        for m in range(-l, l + 1):
            out[..., LM_index(l, m, 0)] = (-1.0) ** (s + m) * np.conj(a[..., LM_index(l, -m, 0)])
    return out


def _real(a, L):
    return 0.5 * (a + _bar(a, 0, L))


def _imag(a, L):
    return -0.5j * (a - _bar(a, 0, L))


def _mul(a, sa, b, sb, L, ctx):
    """product of two fields, truncated to ell_max (rows broadcast: [1, nm] x [n, nm] is allowed)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    n = max(a.shape[0], b.shape[0])
    a = np.ascontiguousarray(np.broadcast_to(a, (n, a.shape[1])))
    b = np.ascontiguousarray(np.broadcast_to(b, (n, b.shape[1])))
    return engine.grid_multiply(a, sa, L, b, sb, L, 2 * L, L, ctx=ctx)


def _zero_below_spin(a, s):
    a = np.array(a, dtype=complex)
    a[..., : s * s] = 0
    return a


def _as_row(x, nm):
    x = np.asarray(x) + 0j
    if x.ndim == 0:
        return np.full((1, nm), complex(x)) if x != 0 else np.zeros((1, nm), dtype=complex)
    if x.ndim == 1:
        return x[np.newaxis, :].astype(complex)
    return x.astype(complex)


def _resident_from_shear(cls, time, L, sigma0, psi2, psi1, psi0, ctx):
    """from_initial_values for a shear series in HBM: sigma0 a device tensor [n_times, (L + 1)^2] or a DeviceModesTimeSeries of spin 2.
    The statements of the host route, stage by stage (bms_bianchi_rhs) with the time integrals between the stages
    (bms_spline_derivative of order -1), written into the [6, N, nm] tensor of a device-resident object.  Only one-row arrays cross PCIe:
    the three constant rows go up, one row of the Moreschi supermomentum comes down for the imaginary part of psi2 at time[0]."""
    from . import _lib, device_series
    from .device_series import DeviceModesTimeSeries

    torch = device_series._torch()
    nm = (L + 1) ** 2
    if isinstance(sigma0, DeviceModesTimeSeries):
        if sigma0.spin_weight != 2:
            raise ValueError(f"Input `sigma0` must have spin weight 2; it has {sigma0.spin_weight}")
        ctx = ctx if ctx is not None else sigma0._ctx
        sigma0 = sigma0._from_ell_0()
    ctx = ctx if ctx is not None else _lib.default_context()
    u = np.array(time, dtype=float)
    n = u.size if u.ndim == 1 else 0
    abd = cls(u, L, multiplication_truncator=max, ctx=ctx, _raw=device_series.empty(ctx, (6, n, nm)), device=True)
    if tuple(sigma0.shape) != (n, nm):
        raise ValueError(f"Input `sigma0` must have shape {(n, nm)}; it has {tuple(sigma0.shape)}")
    if sigma0.dtype != torch.complex128:
        raise ValueError(f"Input `sigma0` must be a complex128 device array; it is {sigma0.dtype}")
    engine._on_device_of(ctx, sigma0)
    psi2 = _zero_below_spin(_as_row(psi2, nm), 0)
    psi1 = _zero_below_spin(_as_row(psi1, nm), 1)
    psi0 = _zero_below_spin(_as_row(psi0, nm), 2)
    raw = abd._raw_dev  # psi0 .. psi4, sigma
    sig = raw[5]
    sig.copy_(sigma0)
    sig[:, :4].zero_()
    d = lambda x, k: engine.spline_derivative(u, x, u, k, ctx=ctx)  # noqa: E731
    # field = the integral of rhs from time[0] plus a constant row, written where the field lives
    settle = lambda field, rhs, row: torch.add(d(rhs, -1), device_series.to_device(ctx, row), out=raw[field])  # noqa: E731
    if L >= 2 and engine.product_launch_shape(L, L, L) is not None:
        sdot = d(sig, 1)
        rhs = device_series.empty(ctx, (n, nm))
        engine.bianchi_rhs(2, sig, sdot, d(sig, 2), L, ctx=ctx, out=(rhs, raw[3], raw[4]))
        # psi2 + eth^2 sigma-bar + sigma sigma-bar-dot at time[0] with psi2 = 0: what fixes Im psi2 there
        zero = torch.zeros((1, nm), dtype=torch.complex128, device=sig.device)
        at_0 = device_series.to_host(engine.supermomenta(zero, sig[:1], sdot[:1], L, want="moreschi", ctx=ctx))
        settle(2, rhs, _real(psi2, L) - 1j * _imag(at_0, L))
        engine.bianchi_rhs(1, sig, raw[2], raw[3], L, ctx=ctx, out=rhs)
        settle(1, rhs, psi1)
        engine.bianchi_rhs(0, sig, raw[1], raw[2], L, ctx=ctx, out=rhs)
        settle(0, rhs, psi0)
        return abd
    # no shear below ell = 2, or a time step beyond the kernel's LDS: the same statements from the series operators
    series = lambda i, s: DeviceModesTimeSeries(raw[i], u, s, 0, L, ctx=ctx, multiplication_truncator=max)  # noqa: E731
    S = series(5, 2)
    sb = S.bar
    sbdot = sb.dot
    raw[4].copy_((-sb.ddot).buf)
    raw[3].copy_((-sbdot.eth_GHP).buf)
    sb_0, sbdot_0, sig_0 = sb.rows(0, 1), sbdot.rows(0, 1), S.rows(0, 1)
    adjust = _real(psi2, L) - 1j * _imag(_eth(_eth(sb_0, -2, L), -1, L) + _mul(sig_0, 2, sbdot_0, -2, L, ctx), L)
    settle(2, (series(3, -1).eth_GHP + S * series(4, -2)).buf, adjust)
    settle(1, (series(2, 0).eth_GHP + 2 * (S * series(3, -1))).buf, psi1)
    settle(0, (series(1, 1).eth_GHP + 3 * (S * series(2, 0))).buf, psi0)
    return abd


def from_initial_values(cls, time, ell_max=8, sigma0=0.0, sigmadot0=0.0, sigmaddot0=0.0, psi2=0.0, psi1=0.0, psi0=0.0, ctx=None, device=None):
    """Bondi data from the shear and initial values of psi2, psi1, psi0.

    sigma0 of dimension 0 or 1: sigma = sigma0 + u sigmadot0 + u^2 sigmaddot0 / 2 and everything is integrated exactly as
    polynomials in u (values given at u = 0).  sigma0 of dimension 2 ([n_times, modes]): sigma as a function of time; the
    rest is integrated with cubic splines from the values at time[0].

    A shear series may live in HBM: sigma0 a device tensor [n_times, (ell_max + 1)^2] (complex128, unit column stride) or a
    DeviceModesTimeSeries of spin 2.  The result is then device-resident and nothing of the series' size crosses PCIe
    (_resident_from_shear).  device=True takes that route for a numpy series too, uploaded once, and is `.to_device()` of the result
    for the polynomial branch; device=False brings a resident result home; None leaves the result where sigma0 is."""
    from .device_series import DeviceModesTimeSeries

    L = int(ell_max)
    resident = engine._is_device_array(sigma0) or isinstance(sigma0, DeviceModesTimeSeries)
    if resident or (device and np.ndim(sigma0) == 2):
        if not resident:
            from . import _lib, device_series

            ctx = ctx if ctx is not None else _lib.default_context()
            sigma0 = device_series.to_device(ctx, sigma0)
        abd = _resident_from_shear(cls, time, L, sigma0, psi2, psi1, psi0, ctx)
        return abd.to_host() if device is not None and not device else abd
    if device:
        return from_initial_values(cls, time, L, sigma0, sigmadot0, sigmaddot0, psi2, psi1, psi0, ctx=ctx).to_device(ctx)
    nm = (L + 1) ** 2
    abd = cls(time, L, multiplication_truncator=max, ctx=ctx)
    u = abd.time
    psi2 = _zero_below_spin(_as_row(psi2, nm), 0)
    psi1 = _zero_below_spin(_as_row(psi1, nm), 1)
    psi0 = _zero_below_spin(_as_row(psi0, nm), 2)
    eth = lambda x, s: _eth(x, s, L)  # noqa: E731
    mul = lambda a, sa, b, sb: _mul(a, sa, b, sb, L, ctx)  # noqa: E731
    if np.ndim(sigma0) in (0, 1):
        s0 = _zero_below_spin(_as_row(sigma0, nm), 2)
        s1 = _zero_below_spin(_as_row(sigmadot0, nm), 2)
        s2 = _zero_below_spin(_as_row(np.asarray(sigmaddot0) / 2, nm), 2)
        poly = lambda *c: sum(cn * u[:, None] ** n for n, cn in enumerate(c))  # noqa: E731
        abd._raw_data[5] = poly(s0, s1, s2)
        p4_0 = -2 * _bar(s2, 2, L)  # psi4 = -d_u^2 sigma-bar
        abd._raw_data[4] = poly(p4_0)
        p3_0 = -eth(_bar(s1, 2, L), -2)  # psi3 = -eth d_u sigma-bar
        p3_1 = -2 * eth(_bar(s2, 2, L), -2)
        abd._raw_data[3] = poly(p3_0, p3_1)
        # psi2 = int (eth psi3 + sigma psi4) du; its imaginary part is fixed by the mass-aspect condition
        p2_0 = _real(psi2, L) - 1j * _imag(eth(eth(_bar(s0, 2, L), -2), -1) + mul(s0, 2, _bar(s1, 2, L), -2), L)
        p2_1 = mul(s0, 2, p4_0, -2) + eth(p3_0, -1)
        p2_2 = (mul(s1, 2, p4_0, -2) + eth(p3_1, -1)) / 2
        p2_3 = (1 / 3) * mul(s2, 2, p4_0, -2)
        abd._raw_data[2] = poly(p2_0, p2_1, p2_2, p2_3)
        # psi1 = int (eth psi2 + 2 sigma psi3) du
        p1_0 = psi1
        p1_1 = 2 * mul(s0, 2, p3_0, -1) + eth(p2_0, 0)
        p1_2 = mul(s0, 2, p3_1, -1) + mul(s1, 2, p3_0, -1) + eth(p2_1, 0) / 2
        p1_3 = (2 * mul(s1, 2, p3_1, -1) + 2 * mul(s2, 2, p3_0, -1) + eth(p2_2, 0)) / 3
        p1_4 = (2 * mul(s2, 2, p3_1, -1) + eth(p2_3, 0)) / 4
        abd._raw_data[1] = poly(p1_0, p1_1, p1_2, p1_3, p1_4)
        # psi0 = int (eth psi1 + 3 sigma psi2) du
        p0_0 = psi0
        p0_1 = 3 * mul(s0, 2, p2_0, 0) + eth(p1_0, 1)
        p0_2 = (3 * mul(s0, 2, p2_1, 0) + 3 * mul(s1, 2, p2_0, 0) + eth(p1_1, 1)) / 2
        p0_3 = mul(s0, 2, p2_2, 0) + mul(s1, 2, p2_1, 0) + mul(s2, 2, p2_0, 0) + eth(p1_2, 1) / 3
        p0_4 = (3 * mul(s0, 2, p2_3, 0) + 3 * mul(s1, 2, p2_2, 0) + 3 * mul(s2, 2, p2_1, 0) + eth(p1_3, 1)) / 4
        p0_5 = (3 * mul(s1, 2, p2_3, 0) + 3 * mul(s2, 2, p2_2, 0) + eth(p1_4, 1)) / 5
        p0_6 = mul(s2, 2, p2_3, 0) / 2
        abd._raw_data[0] = poly(p0_0, p0_1, p0_2, p0_3, p0_4, p0_5, p0_6)
    elif np.ndim(sigma0) == 2:
        sig = _zero_below_spin(sigma0, 2)
        if sig.shape != (u.size, nm):
            raise ValueError(f"Input `sigma0` must have shape {(u.size, nm)}; it has {sig.shape}")
        d = lambda x, k: engine.spline_derivative(u, x, u, k, ctx=ctx)  # noqa: E731
        abd._raw_data[5] = sig
        sb = _bar(sig, 2, L)
        p4 = -d(sb, 2)
        sbdot = d(sb, 1)
        p3 = -eth(sbdot, -2)
        adjust = _real(psi2, L) - 1j * _imag(eth(eth(sb[:1], -2), -1) + mul(sig[:1], 2, sbdot[:1], -2), L)
        p2 = d(eth(p3, -1) + mul(sig, 2, p4, -2), -1) + adjust
        p1 = d(eth(p2, 0) + 2 * mul(sig, 2, p3, -1), -1) + psi1
        p0 = d(eth(p1, 1) + 3 * mul(sig, 2, p2, 0), -1) + psi0
        abd._raw_data[4], abd._raw_data[3], abd._raw_data[2], abd._raw_data[1], abd._raw_data[0] = p4, p3, p2, p1, p0
    else:
        raise ValueError(f"Input `sigma0` must have 1 or 2 dimensions; it has {np.ndim(sigma0)}")
    return abd


# ------------------------------------------------------------------------------------------------- constraints (constraints.py)
def _sides(lhs, rhs, lhs_value, rhs_value):
    if lhs and rhs:
        return (lhs_value(), rhs_value())
    if lhs:
        return lhs_value()
    if rhs:
        return rhs_value()


def bianchi_0(self, lhs=True, rhs=True):
    """psi0' = eth psi1 + 3 sigma psi2"""
    return _sides(lhs, rhs, lambda: self.psi0.dot, lambda: self.psi1.eth_GHP + 3 * (self.sigma * self.psi2))


def bianchi_1(self, lhs=True, rhs=True):
    """psi1' = eth psi2 + 2 sigma psi3"""
    return _sides(lhs, rhs, lambda: self.psi1.dot, lambda: self.psi2.eth_GHP + 2 * (self.sigma * self.psi3))


def bianchi_2(self, lhs=True, rhs=True):
    """psi2' = eth psi3 + sigma psi4"""
    return _sides(lhs, rhs, lambda: self.psi2.dot, lambda: self.psi3.eth_GHP + self.sigma * self.psi4)


def constraint_3(self, lhs=True, rhs=True):
    """psi3 = -eth d_u sigma-bar"""
    return _sides(lhs, rhs, lambda: self.psi3, lambda: -self.sigma.bar.dot.eth_GHP)


def constraint_4(self, lhs=True, rhs=True):
    """psi4 = -d_u^2 sigma-bar"""
    return _sides(lhs, rhs, lambda: self.psi4, lambda: -self.sigma.bar.ddot)


def constraint_mass_aspect(self, lhs=True, rhs=True):
    """Im psi2 = -Im(eth^2 sigma-bar + sigma d_u sigma-bar)"""
    return _sides(lhs, rhs, lambda: self.psi2.imag, lambda: -(self.sigma.bar.eth_GHP.eth_GHP + self.sigma * self.sigma.bar.dot).imag)


def bondi_constraints(self, lhs=True, rhs=True):
    """The six Bondi-gauge relations as (lhs, rhs) pairs (constraints.py:9-39)"""
    return (
        self.bianchi_0(lhs, rhs), self.bianchi_1(lhs, rhs), self.bianchi_2(lhs, rhs), self.constraint_3(lhs, rhs),
        self.constraint_4(lhs, rhs), self.constraint_mass_aspect(lhs, rhs),
    )


def _one_launch(self):
    """whether the violations of this object come from bms_bondi_constraints: fields in HBM, a shear to read, products that end at the
    fields' band (the `max` truncator) and a time step that fits the kernel's LDS"""
    if not getattr(self, "is_device_resident", False) or self.ell_max < 2:
        return False
    if int(self._truncator((self.ell_max, self.ell_max))) != self.ell_max:
        return False
    return engine.product_launch_shape(self.ell_max, self.ell_max, self.ell_max) is not None


_VIOLATION_SPINS = (2, 1, 0, -1, -2, 0)
# bondi_violations takes the one launch up to here: measured at 1e5 steps, 24 ms against 55 ms through the grid products at ell_max = 16 (three
# workgroups per compute unit by LDS), but 142 ms against 117 ms at ell_max = 24 (one).  The norms gain at both ("Constraints")
_VIOLATIONS_ONE_LAUNCH_ELL_MAX = 16


def bondi_gauge_check(self, violations=True, norms=True):
    """(violations, norms): lhs - rhs of the six relations as a list of six series and their L2 norms over the sphere as a list of six
    arrays [n_times]; either is None if not asked for.  A device-resident object with ell_max >= 2, the `max` truncator and a time step
    that fits takes five spline derivatives in HBM and ONE launch (bms_bondi_constraints): the series stay resident and only the
    norms come to the host; bondi_violation_norms of such an object is this call, and bondi_violations up to ell_max = 16.  Every other object goes
    through the series operators and norm(), as it always did."""
    if not violations and not norms:
        return None, None
    if not _one_launch(self):
        v = bondi_violations(self)
        return (v if violations else None), ([x.norm() for x in v] if norms else None)
    from .device_series import DeviceModesTimeSeries

    raw, t, ctx = self._raw_dev, self.t, self._ctx  # psi0 .. psi4, sigma
    d = lambda x, order: engine.spline_derivative(t, x, t, order, ctx=ctx)  # noqa: E731
    # (bar commutes with the derivative: the kernel bars sigma_dot and sigma_ddot as it reads them)
    out, nrm = engine.bondi_constraints(raw, [d(raw[0], 1), d(raw[1], 1), d(raw[2], 1)], d(raw[5], 1), d(raw[5], 2), self.ell_max,
                                        want=range(6) if violations else (), norms=norms, ctx=ctx)
    series = [DeviceModesTimeSeries(o, t, s, 0, self.ell_max, ctx=ctx, multiplication_truncator=self._truncator) for o, s in zip(out, _VIOLATION_SPINS)]
    return (series if violations else None), ([np.ascontiguousarray(nrm[:, k]) for k in range(6)] if norms else None)


def bondi_violations(self):
    """lhs - rhs of the six relations (constraints.py:42-66); of a device-resident object in one launch where bondi_gauge_check has one
    and it was measured to be the quicker route (ell_max <= 16)"""
    if self.ell_max <= _VIOLATIONS_ONE_LAUNCH_ELL_MAX and _one_launch(self):
        return bondi_gauge_check(self, norms=False)[0]
    return [lhs - rhs for (lhs, rhs) in self.bondi_constraints(True, True)]


def bondi_violation_norms(self):
    """L2 norm over the sphere of each violation, at every time (constraints.py:69-94)"""
    if _one_launch(self):
        return bondi_gauge_check(self, violations=False)[1]
    return [v.norm() for v in self.bondi_violations]


METHODS = (bianchi_0, bianchi_1, bianchi_2, constraint_3, constraint_4, constraint_mass_aspect, bondi_constraints, bondi_gauge_check)
