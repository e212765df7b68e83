"""Sample waveforms with known behaviour (scri/sample_waveforms.py): the objects the reference's own tests are built on --
constant and single-mode data, random data, the single mode proportional to time with its analytically supertranslated counterpart
(the known answer of tests/test_waveform_grid.py), and the precessing binary `fake_precessing_waveform` (:383-593) with the
finite-radius family the reference builds on it (:596-755).  The first group are host-side generators; what is done WITH them runs on
the GPU.  The precessing waveform is generated on the GPU itself, per time step (bms_precessing_waveform), and may stay there.  Of
`create_fake_finite_radius_strain_h5file` the in-memory core is here, `fake_finite_radius_waveforms`, and what it writes, as arrays in
memory, `fake_finite_radius_data`; the HDF5 file is not written."""
import math
import warnings
from fractions import Fraction

import numpy as np

from . import DataType, Inertial, Corotating, SpinWeights, h
from .mode_algebra import LM_index, LM_range, LM_total_size, vector_as_ell_1_modes


def wigner_3j(j1, j2, j3, m1, m2, m3):
    """Wigner 3-j symbol for integer arguments by Racah's formula, the sum in exact rational arithmetic (sf.Wigner3j)"""
    j1, j2, j3, m1, m2, m3 = (int(x) for x in (j1, j2, j3, m1, m2, m3))
    if m1 + m2 + m3 != 0 or abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3 or j3 > j1 + j2 or j3 < abs(j1 - j2):
        return 0.0
    f = math.factorial
    delta = Fraction(f(j1 + j2 - j3) * f(j1 - j2 + j3) * f(-j1 + j2 + j3), f(j1 + j2 + j3 + 1))
    norm = delta * f(j1 + m1) * f(j1 - m1) * f(j2 + m2) * f(j2 - m2) * f(j3 + m3) * f(j3 - m3)
    total = Fraction(0)
    for k in range(max(0, j2 - j3 - m1, j1 - j3 + m2), min(j1 + j2 - j3, j1 - m1, j2 + m2) + 1):
        total += Fraction((-1) ** k, f(k) * f(j1 + j2 - j3 - k) * f(j1 - m1 - k) * f(j2 + m2 - k) * f(j3 - j2 + m1 + k) * f(j3 - j1 - m2 + k))
    return float((-1) ** (j1 - j2 - m3) * total) * math.sqrt(norm)


def _unused(kwargs):
    if kwargs:
        import pprint

        warnings.warn(f"\nUnused kwargs passed to this function:\n{pprint.pformat(kwargs, width=1)}")


def modes_constructor(constructor_statement, data_functor, **kwargs):
    """WaveformModes filled by `data_functor(t, LM)`; t (default 1101 samples on [-10, 100]), frame, frameType (Inertial), dataType
    (h), r_is_scaled_out / m_is_scaled_out (True), ell_min (|s| of the data type), ell_max (8) as keywords"""
    from .waveform_modes import WaveformModes

    t = np.array(kwargs.pop("t", np.linspace(-10.0, 100.0, num=1101)), dtype=float)
    frame = kwargs.pop("frame", None)
    frameType = int(kwargs.pop("frameType", Inertial))
    dataType = int(kwargs.pop("dataType", h))
    r_out, m_out = bool(kwargs.pop("r_is_scaled_out", True)), bool(kwargs.pop("m_is_scaled_out", True))
    ell_min = int(kwargs.pop("ell_min", abs(SpinWeights[dataType])))
    ell_max = int(kwargs.pop("ell_max", 8))
    ctx = kwargs.pop("ctx", None)
    _unused(kwargs)
    data = data_functor(t, LM_range(ell_min, ell_max))
    return WaveformModes(t=t, frame=frame, data=data, history=["# Called from constant_waveform"], frameType=frameType, dataType=dataType,
                         r_is_scaled_out=r_out, m_is_scaled_out=m_out, constructor_statement=constructor_statement, ell_min=ell_min,
                         ell_max=ell_max, ctx=ctx)


def constant_waveform(**kwargs):
    """every mode constant in time: (l, m) -> m - i m"""
    _unused({k: v for k, v in kwargs.items() if k not in ("t", "ell_min", "ell_max", "ctx")})
    keep = {k: v for k, v in kwargs.items() if k in ("t", "ell_min", "ell_max", "ctx")}
    return modes_constructor(f"constant_waveform(**{kwargs})", lambda t, LM: np.repeat((LM[:, 1] - 1j * LM[:, 1])[None, :].astype(complex), t.shape[0], axis=0), **keep)


def single_mode(ell, m, **kwargs):
    """1 in the (ell, m) slot and 0 elsewhere"""
    def functor(t, LM):
        data = np.zeros((t.shape[0], LM.shape[0]), dtype=complex)
        data[:, LM_index(ell, m, int(LM[:, 0].min()))] = 1.0
        return data

    keep = {k: kwargs.pop(k) for k in ("t", "ell_min", "ell_max", "ctx") if k in kwargs}
    _unused(kwargs)
    return modes_constructor(f"single_mode({ell}, {m}, **{kwargs})", functor, **keep)


def _random_setup(kwargs):
    begin, end, n_times = float(kwargs.pop("begin", -10.0)), float(kwargs.pop("end", 100.0)), int(kwargs.pop("n_times", 1101))
    rng = np.random.default_rng(kwargs.pop("seed", None))
    if kwargs.pop("uniform_time", False):
        t = np.linspace(begin, end, num=n_times)
    else:
        t = np.sort(rng.uniform(begin, end, size=n_times))
    rotating = kwargs.pop("rotating", True)
    frame = None
    if rotating:
        frame = rng.normal(size=(n_times, 4))
        frame /= np.linalg.norm(frame, axis=1)[:, None]
    return rng, t, frame, (Corotating if rotating else Inertial)


def random_waveform(**kwargs):
    """random data at each time step on (by default) random times, in a randomly oriented corotating frame (uniform_time, begin,
    end, n_times, rotating, seed as keywords)"""
    rng, t, frame, frameType = _random_setup(kwargs)
    return modes_constructor(f"random_waveform(**{kwargs})", lambda t_, LM: rng.normal(size=(t_.shape[0], LM.shape[0])) + 1j * rng.normal(size=(t_.shape[0], LM.shape[0])),
                             t=t, frame=frame, frameType=frameType, **kwargs)


def random_waveform_proportional_to_time(**kwargs):
    """every mode a random complex constant times the time"""
    rng, t, frame, frameType = _random_setup(kwargs)
    return modes_constructor(f"random_waveform_proportional_to_time(**{kwargs})",
                             lambda t_, LM: np.outer(t_, rng.normal(size=LM.shape[0]) + 1j * rng.normal(size=LM.shape[0])), t=t, frame=frame,
                             frameType=frameType, **kwargs)


def _single_mode_series(kwargs, values_of_t):
    from .waveform_modes import WaveformModes

    s = kwargs.pop("s", -2)
    ell = kwargs.pop("ell", abs(s))
    m = kwargs.pop("m", -ell)
    ell_min, ell_max = kwargs.pop("ell_min", abs(s)), kwargs.pop("ell_max", 8)
    data_type = kwargs.pop("data_type", DataType[SpinWeights.index(s)])
    t_0, t_1, dt = kwargs.pop("t_0", -20.0), kwargs.pop("t_1", 20.0), kwargs.pop("dt", 1.0 / 10.0)
    t = np.arange(t_0, t_1 + dt, dt)
    data = np.zeros((t.size, LM_total_size(ell_min, ell_max)), dtype=complex)
    data[:, LM_index(ell, m, ell_min)] = values_of_t(t)
    make = lambda d, ctx=None: WaveformModes(t=t, data=d, ell_min=ell_min, ell_max=ell_max, frameType=Inertial, dataType=data_type,  # noqa: E731
                                             r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    return s, ell, m, ell_min, ell_max, t, data, make


def single_mode_constant_rotation(**kwargs):
    """one nonzero mode exp(i omega t) (omega may be complex: damping); s, ell, m, ell_min, ell_max, data_type, t_0, t_1, dt, omega"""
    omega = complex(kwargs.pop("omega", 0.5))
    ctx = kwargs.pop("ctx", None)
    *_, data, make = _single_mode_series(kwargs, lambda t: np.exp(1j * omega * t))
    _unused(kwargs)
    return make(data, ctx)


def single_mode_proportional_to_time(**kwargs):
    """one nonzero mode beta t"""
    beta = kwargs.pop("beta", 1.0)
    ctx = kwargs.pop("ctx", None)
    *_, data, make = _single_mode_series(kwargs, lambda t: beta * t)
    _unused(kwargs)
    return make(data, ctx)


def single_mode_proportional_to_time_supertranslated(**kwargs):
    """single_mode_proportional_to_time after an analytically applied supertranslation (`supertranslation` modes, or
    `space_translation`, default none): a mode beta t sY_lm seen at u - alpha picks up -beta alpha sY_lm, whose modes are the
    Gaunt coefficients of alpha_l''m'' against (l, m) -- sqrt((2l''+1)(2l+1)(2l'+1)/4pi) times two 3-j symbols and a sign."""
    beta = kwargs.pop("beta", 1.0)
    ctx = kwargs.pop("ctx", None)
    supertranslation = np.array(kwargs.pop("supertranslation", np.array([], dtype=complex)), dtype=complex)
    if "space_translation" in kwargs:
        if supertranslation.size < 4:
            supertranslation = np.concatenate([supertranslation, np.zeros(4 - supertranslation.size, dtype=complex)])
        supertranslation[1:4] = -vector_as_ell_1_modes(kwargs.pop("space_translation"))
    s, ell, m, ell_min, ell_max, t, data, make = _single_mode_series(kwargs, lambda t_: beta * t_)
    _unused(kwargs)
    lst = int(math.sqrt(supertranslation.size) - 1) if supertranslation.size else -1
    if supertranslation.size and lst * (lst + 2) + 1 != supertranslation.size:
        raise ValueError(f"Bad number of elements in supertranslation: {supertranslation.size}")
    for i, (ellpp, mpp) in enumerate(LM_range(0, lst) if lst >= 0 else []):
        if supertranslation[i] == 0.0:
            continue
        mp = m + mpp
        for ellp in range(ell_min, min(ell_max, ell + ellpp) + 1):
            if ellp < abs(mp):
                continue
            term = (beta * supertranslation[i] * math.sqrt(((2 * ellpp + 1) * (2 * ell + 1) * (2 * ellp + 1)) / (4 * math.pi))
                    * wigner_3j(ellpp, ell, ellp, 0, -s, s) * wigner_3j(ellpp, ell, ellp, mpp, m, -mp))
            data[:, LM_index(ellp, mp, ell_min)] += -term if (s + mp) % 2 == 1 else term
    return make(data, ctx)


def pn_leading_order_amplitude(ell, m, x, mass_ratio=1.0):
    """Leading-order amplitude of r h / M in PN theory, Eqs. (330) of Blanchet's Living Review (2014), of the mode (ell, m) at
    x = (orbital angular velocity)^(2/3)  (scri/sample_waveforms.py:536-593)"""
    if m < 0:
        return (-1) ** ell * np.conjugate(pn_leading_order_amplitude(ell, -m, x, mass_ratio=mass_ratio))
    coefficient, power = _pn_amplitude_coefficient(ell, m, mass_ratio)
    return coefficient * x**power * x


def _pn_amplitude_coefficient(ell, m, mass_ratio):
    """(c, p) with pn_leading_order_amplitude(ell, m, x) = c x^p x for m >= 0: the reference's expression, factor by factor, without x"""
    f = lambda k: float(math.factorial(k))  # noqa: E731
    f2 = lambda k: float(math.prod(range(k, 0, -2)))  # noqa: E731  (double factorial of an odd k >= 1)
    if mass_ratio < 1.0:
        mass_ratio = 1.0 / mass_ratio
    nu = mass_ratio / (1 + mass_ratio) ** 2
    X1 = mass_ratio / (mass_ratio + 1)
    X2 = 1 / (mass_ratio + 1)
    sigma = lambda k: X2 ** (k - 1) + (-1) ** k * X1 ** (k - 1)  # noqa: E731
    if (ell + m) % 2 == 0:
        amplitude = (
            ((-1) ** ((ell - m + 2) // 2) / (2 ** (ell + 1) * f((ell + m) // 2) * f((ell - m) // 2) * f2(2 * ell - 1)))
            * np.sqrt((5 * (ell + 1) * (ell + 2) * f(ell + m) * f(ell - m)) / (ell * (ell - 1) * (2 * ell + 1)))
            * sigma(ell)
            * (1j * m) ** ell
        )
        power = ell / 2 - 1
    else:
        amplitude = (
            ((-1) ** ((ell - m - 1) // 2) / (2 ** (ell - 1) * f((ell + m - 1) // 2) * f((ell - m - 1) // 2) * f2(2 * ell + 1)))
            * np.sqrt((5 * (ell + 2) * (2 * ell + 1) * f(ell + m) * f(ell - m)) / (ell * (ell - 1) * (ell + 1)))
            * sigma(ell + 1)
            * 1j
            * (1j * m) ** ell
        )
        power = (ell - 1) / 2
    return 8 * np.sqrt(np.pi / 5) * nu * amplitude, power


def _pn_amplitude_tables(ell_max, mass_ratio):
    """what the mode kernel takes: amplitude of column k = coef[k] x^power[k], l = 2 .. ell_max"""
    coef, power = [], []
    for ell in range(2, ell_max + 1):
        for m in range(-ell, ell + 1):
            c, p = _pn_amplitude_coefficient(ell, abs(m), mass_ratio)
            coef.append((-1) ** ell * np.conjugate(c) if m < 0 else c)
            power.append(p + 1)
    return np.array(coef, dtype=complex), np.array(power, dtype=float)


def fake_precessing_waveform(t_0=-20.0, t_1=20_000.0, dt=0.1, ell_max=8, mass_ratio=2.0, precession_opening_angle=np.pi / 6.0,
                             precession_opening_angle_dot=None, precession_relative_rate=0.1, precession_nutation_angle=None, inertial=True,
                             device=False, ctx=None):
    """Strain waveform with realistic precession effects (scri/sample_waveforms.py:383-533): the lowest-order PN phasing up to a
    constant merger frequency, leading-order mode amplitudes modulated antisymmetrically in m, a smooth transition to an exponential
    ringdown, in a frame whose orbital rotation precesses about a cone of growing opening angle and nutates on it, settling after the
    merger; `inertial` transforms it back to the inertial frame.  The merger is 100 time units before t_1.

    t_0, t_1, dt: the time axis np.arange(t_0, t_1 + 0.99 dt, dt).  mass_ratio: for the phasing and the amplitudes (a ratio below 1 is
    inverted).  precession_opening_angle [pi/6], precession_opening_angle_dot [2 opening angle / (end of the ringdown transition - t_0)],
    precession_relative_rate [0.1], precession_nutation_angle [opening angle / 10].
    Every step is computed on the GPU.  device=True leaves the mode weights there (`is_device_resident`); the values are the same."""
    from . import _lib, device_series, engine, quaternions
    from .waveform_modes import WaveformModes

    statement = (f"fake_precessing_waveform(t_0={t_0}, t_1={t_1}, dt={dt}, ell_max={ell_max}, mass_ratio={mass_ratio}, "
                 f"precession_opening_angle={precession_opening_angle}, precession_opening_angle_dot={precession_opening_angle_dot}, "
                 f"precession_relative_rate={precession_relative_rate}, precession_nutation_angle={precession_nutation_angle}, "
                 f"inertial={inertial}, device={device})")
    if mass_ratio < 1.0:
        mass_ratio = 1.0 / mass_ratio
    ell_min = 2
    t = np.arange(t_0, t_1 + 0.99 * dt, dt)
    t_merger = t_1 - 100.0
    i_merger = np.argmin(abs(t - t_merger))
    if i_merger < 20:
        raise ValueError(f"Insufficient space between initial time (t={t_merger}) and merger (t={t_0}).")
    ctx = ctx if ctx is not None else _lib.default_context()
    coef, power = _pn_amplitude_tables(ell_max, mass_ratio)
    out = device_series.empty(ctx, (t.size, LM_total_size(ell_min, ell_max))) if device else None
    data, frame = engine.precessing_waveform(t, ell_max, t_merger, mass_ratio, precession_opening_angle, precession_opening_angle_dot,
                                             precession_relative_rate, precession_nutation_angle, coef, power, inertial=inertial, out=out, ctx=ctx)
    W = WaveformModes(t=t, frame=frame, data=np.empty((0, LM_total_size(ell_min, ell_max)), dtype=complex) if device else data, ell_min=ell_min,
                      ell_max=ell_max, history=["# Called from fake_precessing_waveform"], frameType=Corotating, dataType=h,
                      r_is_scaled_out=True, m_is_scaled_out=True, constructor_statement=statement, ctx=ctx)
    if device:
        W._host, W._dev = None, data
    if inertial:  # the bookkeeping of to_inertial_frame (scri/rotations.py:106-111, :313-321); the rotation itself ran on the GPU
        W.frame = quaternions.multiply(W.frame, quaternions.conjugate(W.frame))
        W.frameType = Inertial
        W._append_history(f"{W}.to_inertial_frame()")
    return W


def fake_finite_radius_waveforms(n_subleading=3, amp=1.0, t_0=0.0, t_1=3000.0, dt=0.1, r_min=100.0, r_max=600.0, n_radii=24, ell_max=8,
                                 avg_areal_radius_diff=1.0, mass_ratio=1.0, precession_opening_angle=0.0, device=False, ctx=None, **kwargs):
    """The finite-radius strain waveforms of `create_fake_finite_radius_strain_h5file` (scri/sample_waveforms.py:596-755) in memory:
    (Ws, Radii, h0) with h0 = fake_precessing_waveform(t_0, t_1, dt, ell_max, mass_ratio, precession_opening_angle, **kwargs) and, at the
    areal radii R_i = coordinate radius + avg_areal_radius_diff, coordinate radii equally spaced in 1 / r from r_min to r_max,

        Ws[i].data = h0.data + sum_{n = 1 .. n_subleading} amp R_i^-n exp(i n 50 pi t / N) |h0.data|      (N time steps),

    Radii[i] the constant series R_i; what `_Extrapolate(Ws, Radii, orders)` takes.  The terms are added on the GPU; device=True
    leaves h0 and every Ws[i] there.  Two differences from the reference are deliberate: the file, the warp to
    coordinate time, the zero padding and the 1e-14 drift belong to the file writer and are absent; and every radius carries ITS OWN
    terms on the one h0, as the reference's docstring says -- its loop adds them into h0 in place (and its call drops mass_ratio)."""
    from . import _lib, device_series, engine
    from .waveform_modes import WaveformModes

    ctx = ctx if ctx is not None else _lib.default_context()
    h0 = fake_precessing_waveform(t_0=t_0, t_1=t_1, dt=dt, ell_max=ell_max, mass_ratio=mass_ratio, precession_opening_angle=precession_opening_angle,
                                  device=True, ctx=ctx, **kwargs)
    coord_radii = (1 / np.linspace(1 / r_min, 1 / r_max, n_radii)).astype(int)
    Ws, Radii = [], []
    for coord_radius in coord_radii:
        R = float(coord_radius + avg_areal_radius_diff)
        data = engine.radius_terms(h0.t, h0._dev, n_subleading, amp, R, device_series.empty(ctx, h0._dev.shape), ctx=ctx)
        W = WaveformModes(t=h0.t, frame=h0.frame, data=np.empty((0, h0.n_modes), dtype=complex), ell_min=h0.ell_min, ell_max=h0.ell_max,
                          history=list(h0.history) + [f"# finite-radius terms: n_subleading={n_subleading}, amp={amp}, R={R}"], frameType=h0.frameType,
                          dataType=h0.dataType, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
        W._host, W._dev = None, data
        Ws.append(W if device else W.to_host())
        Radii.append(np.full(h0.n_times, R))
    ctx.synchronize()
    return Ws, Radii, (h0 if device else h0.to_host())


def fake_finite_radius_data(n_subleading=3, amp=1.0, t_0=0.0, t_1=3000.0, dt=0.1, r_min=100.0, r_max=600.0, n_radii=24, ell_max=8,
                            initial_adm_energy=0.99, avg_lapse=0.99, avg_areal_radius_diff=1.0, mass_ratio=1.0, precession_opening_angle=0.0,
                            device=False, ctx=None, **kwargs):
    """What `create_fake_finite_radius_strain_h5file` writes (scri/sample_waveforms.py:704-745), in memory: an ordered mapping from the
    group names "R0100.dir" ... to the keyword arguments of extrapolation.finite_radius_waveform, so that
    `extrapolation.finite_radius_data(fake_finite_radius_data(...), 1.0)` is the reference's file followed by its reader.

    Every group is on all_times = linspace(0, t_1 + r_max, N + int(r_max / dt)) with constant coordinate radius, areal radius (larger by
    avg_areal_radius_diff) and lapse; its modes are those of fake_finite_radius_waveforms at that radius, moved to the simulation time
    (t + r*) sqrt(1 - 2E/R) / lapse, r* = R + 2E log(R / 2E - 1), splined onto all_times (engine.cubic_spline), zero outside the warped
    range, plus the drift (1 + i) 1e-14 t.  The two deliberate differences of fake_finite_radius_waveforms hold here as well.
    device=True leaves the modes of every group on the device."""
    from . import _lib, device_series, engine

    ctx = ctx if ctx is not None else _lib.default_context()
    Ws, Radii, h0 = fake_finite_radius_waveforms(n_subleading=n_subleading, amp=amp, t_0=t_0, t_1=t_1, dt=dt, r_min=r_min, r_max=r_max,
                                                 n_radii=n_radii, ell_max=ell_max, avg_areal_radius_diff=avg_areal_radius_diff,
                                                 mass_ratio=mass_ratio, precession_opening_angle=precession_opening_angle, device=True, ctx=ctx,
                                                 **kwargs)
    coord_radii = (1 / np.linspace(1 / r_min, 1 / r_max, n_radii)).astype(int)
    n_times = int(h0.t.shape[0] + r_max / dt)
    all_times = np.linspace(0, t_1 + r_max, n_times)
    torch = device_series._torch()
    dev = device_series.attach(ctx)
    drift = torch.from_numpy(((1 + 1j) * 1e-14 * all_times).reshape(-1, 1)).to(dev)
    groups = {}
    for coord_radius, W, R_series in zip(coord_radii, Ws, Radii):
        R = float(R_series[0])
        tortoise_coord = R + 2 * initial_adm_energy * np.log(R / (2 * initial_adm_energy) - 1)
        simulation_time = (h0.t + tortoise_coord) * np.sqrt(1 - 2 * initial_adm_energy / R) / avg_lapse
        data = engine.cubic_spline(simulation_time, W._dev, all_times, ctx=ctx)
        outside = torch.from_numpy((all_times < simulation_time[0]) | (all_times > simulation_time[-1])).to(dev)
        data[outside] = 0.0
        data += drift
        groups[f"R{coord_radius:04}.dir"] = dict(
            t=all_times.copy(), data=data if device else data.cpu().numpy(), ArealRadius=np.full(n_times, R),
            AverageLapse=np.full(n_times, float(avg_lapse)), CoordRadius=float(coord_radius), InitialAdmEnergy=float(initial_adm_energy),
            dataType=h, ell_min=h0.ell_min, ell_max=h0.ell_max)
    ctx.synchronize()
    return groups
