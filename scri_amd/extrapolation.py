"""Extrapolation of finite-radius waveforms to null infinity: the in-memory core of scri/extrapolation.py.

    monotonic_indices   scri/extrapolation.py:27-45
    intersection        scri/extrapolation.py:47-125 (mode_operators.time_intersection)
    finite_radius_waveform  scri/extrapolation.py:343-417 from :356 on (read_finite_radius_waveform behind its file reader): the raw series
                        of one radius retarded to tortoise time and scaled on the GPU (bms_finite_radius_retard)
    finite_radius_data  scri/extrapolation.py:419-537 (read_finite_radius_data) on groups held in memory
    set_common_time     scri/extrapolation.py:539-554, the radii and the waveforms through the GPU cubic spline
    _Extrapolate        scri/extrapolation.py:1270-1474, the per-time-step fit in 1/r on the GPU (bms_extrapolate)
    extrapolate_waveforms   the steps of the file driver `extrapolate` (:744-853) between reading and writing the files

Same names, arguments, history lines and errors as the reference, with two deliberate refusals: fits in
M Omega r (`Omegas`) and the exclusion of insignificant radii for psi0 / psi1 (`NoiseFloor`), two branches that fail in the
reference, raise NotImplementedError.  The file readers and writers are out of scope.
"""
import warnings

import numpy as np

from . import Inertial, Corotating, h, hdot, psi0, psi1, psi2, psi3, psi4
from . import engine
from .mode_operators import time_intersection as intersection
from .waveform_modes import WaveformModes

__all__ = ["monotonic_indices", "intersection", "finite_radius_waveform", "finite_radius_data", "set_common_time", "_Extrapolate",
           "extrapolate_waveforms"]


def monotonic_indices(T, MinTimeStep=1.0e-3):
    """Indices of a strictly increasing subsequence of the times T: walking forward, a time that does not exceed the last kept
    one by more than MinTimeStep is kept, and every kept time it does not exceed by more than MinTimeStep is dropped -- the
    earlier pass of a restarted segment gives way to the later one.  Where the reference's loop would not end (a time within
    MinTimeStep of the first kept one), the first one is dropped as well."""
    kept = []
    for k in range(len(T)):
        while kept and T[kept[-1]] + MinTimeStep >= T[k]:
            kept.pop()
        kept.append(k)
    return np.array(kept, dtype=int)


def _mass_scaling(dataType, ChMass):
    """(UnitScaleFactor, RadiusRatioExp) of scri/extrapolation.py:364-386"""
    table = {h: (1.0 / ChMass, 1), hdot: (1.0, 1), psi4: (ChMass, 1), psi3: (1.0, 2), psi2: (1.0 / ChMass, 3), psi1: (1.0 / ChMass**2, 4),
             psi0: (1.0 / ChMass**3, 5)}
    if dataType not in table:
        raise ValueError(f'DataType "{dataType}" is unknown.')
    return table[dataType]


def finite_radius_waveform(t, data, ArealRadius, AverageLapse, CoordRadius, InitialAdmEnergy, ChMass, dataType, ell_min=2, ell_max=None,
                           frame=None, MinTimeStep=1.0e-3, ctx=None):
    """One finite-radius waveform as a simulation writes it -> (W, Radii) on the retarded time axis, with the mass scaled out: what
    scri's read_finite_radius_waveform does after it has read its file (scri/extrapolation.py:356-417), on the GPU
    (bms_finite_radius_retard).

    t, ArealRadius, AverageLapse: the raw series, one value per written step (coordinate times, with the repeated stretches of
    restarts).  data [len(t), n_modes]: the modes in code units, a numpy array or a device tensor, which is read where it is; W is then
    device resident.  frame: None or [len(t), 4].  The raw arrays are taken rather than a WaveformModes because a waveform on a
    restarting time axis is not a valid one.

    The steps monotonic_indices(t, MinTimeStep) names are kept; their times become the cumulative trapezoid of
    AverageLapse / sqrt(1 - 2 InitialAdmEnergy / ArealRadius) minus the tortoise coordinate, over ChMass; Radii = ArealRadius / ChMass;
    every row of modes is multiplied by (ArealRadius / CoordRadius)^p UnitScaleFactor, p and the factor by dataType.
    A kept radius that is not finite or not beyond 2 InitialAdmEnergy raises ValueError (the reference: a NaN time axis and a warning)."""
    if ChMass == 0.0:
        raise ValueError("ChMass=0.0 is not a valid input value.")
    unit, p = _mass_scaling(dataType, ChMass)
    n_cols = int(data.shape[1])
    if ell_max is None:
        ell_max = int(round(np.sqrt(n_cols + ell_min**2))) - 1
    if n_cols != engine.LM_total_size(ell_min, ell_max):
        raise ValueError(f"data of {n_cols} columns do not hold the modes of ell = {ell_min} .. {ell_max}")
    if ctx is None:
        from . import _lib

        ctx = _lib.default_context()
    resident = hasattr(data, "data_ptr")
    if resident:
        from . import device_series

        dev = device_series.attach(ctx)
        if frame is not None and not hasattr(frame, "data_ptr"):
            frame = device_series._torch().from_numpy(np.ascontiguousarray(frame, dtype=float)).to(dev)
    T, Radii, rows, frame_out = engine.finite_radius_retard(t, ArealRadius, AverageLapse, data, CoordRadius, InitialAdmEnergy, ChMass, unit, p,
                                                            frame=frame, min_time_step=MinTimeStep, ctx=ctx)
    if frame_out is None:
        frame_out = np.empty((0, 4))
    elif resident:
        frame_out = frame_out.cpu().numpy()
    history = f"# extrapolation.read_finite_radius_waveform({CoordRadius}, {InitialAdmEnergy}, {dataType}, {ChMass})"
    W = WaveformModes(t=T.copy(), frame=frame_out, data=np.empty((0, n_cols), dtype=complex) if resident else rows, ell_min=ell_min, ell_max=ell_max,
                      frameType=Inertial, dataType=dataType, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    W.history = [history]  # (the one line, as the reference assigns it: :415)
    if resident:
        W._host, W._dev = None, rows
    return W, Radii.copy()


def finite_radius_data(groups, ChMass=0.0, CoordRadii=[], ctx=None):
    """(Ws, Radii, CoordRadii) of the groups of a finite-radius file held in memory: the selection rules and errors of scri's
    read_finite_radius_data (scri/extrapolation.py:419-537) around finite_radius_waveform.  groups: an ordered mapping from names such as
    "R0247.dir" to the keyword arguments of finite_radius_waveform (without ChMass and ctx).  CoordRadii: empty for every group, integers
    for positions, or strings searched in the names as regular expressions.  The file, its validation and the progress messages are
    out of scope."""
    import numbers
    import re

    if ChMass == 0.0:
        raise ValueError("ChMass=0.0 is not a valid input value.")
    radius_of = re.compile(r"""R(?P<r>.*?)\.dir""")

    def radius_string(name):
        m = radius_of.search(str(name))
        if not m:
            raise ValueError(f"Could not parse radius from waveform name {name!r}")
        return m.group("r")

    names = [name for name in groups if name != "VersionHist.ver"]
    all_names = list(names)
    if not CoordRadii:
        CoordRadii = [m.group("r") for name in names for m in [radius_of.search(name)] if m]
    elif isinstance(CoordRadii[0], numbers.Integral):
        names = [names[i] for i in CoordRadii]
        CoordRadii = [radius_string(name) for name in names]
    else:
        names = [name for name in names for radius in CoordRadii for m in [re.compile(radius).search(name)] if m]
        try:
            CoordRadii = [radius_string(name) for name in names]
        except Exception:
            pass
    if not names:
        raise ValueError("No waveform groups matched the requested CoordRadii. "
                         f"Requested CoordRadii={CoordRadii}; available groups={all_names}.")
    if len(names) != len(CoordRadii):
        raise ValueError("Mismatch between requested radii and matched waveform groups. "
                         f"Requested CoordRadii={CoordRadii}; matched groups={names}.")
    try:
        [float(r) for r in CoordRadii]
    except Exception as e:
        raise ValueError(f"Could not convert CoordRadii entries to float: CoordRadii={CoordRadii}") from e
    Ws, Radii = [], []
    for name in names:
        W, R = finite_radius_waveform(ChMass=ChMass, ctx=ctx, **groups[name])
        Ws.append(W)
        Radii.append(R)
    return Ws, Radii, CoordRadii


def _resident(W):
    return getattr(W, "is_device_resident", False)


def _host_data(W):
    """the modes of W on the host for a fit whose inputs are not all device resident (the fit reads one kind of memory): a copy, which
    leaves a device-resident W where it is"""
    return W._dev.cpu().numpy() if _resident(W) else W.data


def set_common_time(Ws, Radii, MinTimeStep=0.005, EarliestTime=-3e300, LatestTime=3e300):
    """Replace Ws[k] and Radii[k] (k < len(Radii)), in the two lists, by their values on one time axis: the intersection of
    every waveform's axis with [EarliestTime, LatestTime], steps of at least MinTimeStep.

    The radii go through the not-a-knot cubic spline -- the interpolant scipy's InterpolatedUnivariateSpline(k=3) builds in
    the reference -- and the waveforms through WaveformModes.interpolate, both on the GPU.  The waveforms passed in are not
    changed; the interpolated copy of a device-resident one is device resident."""
    T = intersection([EarliestTime, LatestTime], Ws[0].t, MinTimeStep, EarliestTime, LatestTime)
    for W in Ws[1 : len(Radii)]:
        T = intersection(T, W.t)
    for k in range(len(Radii)):
        r = np.asarray(Radii[k], dtype=float).astype(np.complex128)
        Radii[k] = engine.cubic_spline(Ws[k].t, r, T, ctx=Ws[k]._ctx).real
        Ws[k] = Ws[k].interpolate(T)  # (a device-resident waveform is read where it is, and so is the result)


def _check_arguments(Ws, Radii, orders, Omegas):
    """The argument checks of scri/extrapolation.py:1290-1355 (same order, same exceptions); returns the sizes."""
    n_w = len(Ws)
    n_t, n_m = Ws[0].n_times, Ws[0].n_modes
    lo, hi = min(orders), max(orders)

    def refuse(kind, text):
        print("ERROR: " + text + "\n")
        raise ValueError(kind)

    if abs(lo) > n_w:
        refuse("scri_IndexOutOfBounds", f"order {lo} asks for a finite-radius waveform beyond the {n_w} given")
    if hi > 0 and hi >= n_w:
        refuse("scri_IndexOutOfBounds", f"a fit of order {hi} needs {hi + 1} finite-radius waveforms, {n_w} given")
    if len(Radii) != n_w:
        refuse("scri_VectorSizeMismatch", f"{n_w} waveforms but {len(Radii)} radius series")
    if Omegas is not None and len(Omegas) != 0 and len(Omegas) != n_t:
        refuse("scri_VectorSizeMismatch", f"{len(Omegas)} values of Omega for {n_t} time steps")
    for k in range(1, n_w):
        if Ws[k].n_times != n_t:
            refuse("scri_VectorSizeMismatch", f"waveform {k} has {Ws[k].n_times} time steps, waveform 0 has {n_t}")
        if Ws[k].n_modes != n_m:
            refuse("scri_VectorSizeMismatch", f"waveform {k} has {Ws[k].n_modes} modes, waveform 0 has {n_m}")
        if len(Radii[k]) != n_t:
            refuse("scri_VectorSizeMismatch", f"radius series {k} has {len(Radii[k])} values for {n_t} time steps")
    return n_w, n_t, n_m


def _Extrapolate(FiniteRadiusWaveforms, Radii, ExtrapolationOrders, Omegas=None, NoiseFloor=None):
    """Extrapolate the waveforms at finite radii (all on one time axis, `Radii[i][t]` the radius of waveform i at step t) to
    infinity: for each N >= 0 of ExtrapolationOrders the constant term of the polynomial of degree N in 1/r fitted to each mode
    at each time step; N < 0 takes a copy of FiniteRadiusWaveforms[N].  Returns one WaveformModes per order, with the metadata of
    the outermost (last) waveform.  The fit runs on the GPU; when every input is device resident the results are too.  The
    inputs are not moved.

    A step whose fit of order N is rank deficient (numpy's rcond = n_radii eps), or whose radii are not finite, is NaN in that
    output and counted in a RankWarning -- the reference's polyfit warns and returns a minimum-norm answer."""
    Ws, orders = FiniteRadiusWaveforms, list(ExtrapolationOrders)
    n_w, n_t, n_m = _check_arguments(Ws, Radii, orders, Omegas)
    last = Ws[-1]
    results = [None] * len(orders)
    for slot, N in enumerate(orders):
        if N < 0:  # a copy of one radius, as given
            results[slot] = WaveformModes(Ws[N])
            results[slot].history.append(f"### Extrapolating with N={N}\n")
    fits = [(slot, int(N)) for slot, N in enumerate(orders) if N >= 0]
    if not fits:
        return results
    if Omegas is not None and len(Omegas) != 0:
        raise NotImplementedError(
            "_Extrapolate with Omegas: the reference's fit in M Omega r indexes its data as data[:, i_m, i_t] (scri/extrapolation.py:1450, "
            "time and mode swapped), so it fails once i_t >= n_modes, and its driver calls a method Python scri does not have (:798)")
    if NoiseFloor and last.dataType in (psi0, psi1):
        raise NotImplementedError(
            "_Extrapolate with NoiseFloor on psi0 / psi1 data: the reference reads `Re` before it is assigned on this branch "
            "(scri/extrapolation.py:1411) and raises UnboundLocalError, so there is no behaviour to reproduce")
    if len(Radii[0]) < n_t:  # (the reference never checks Radii[0]; its fit then fails with IndexError)
        print(f"ERROR: radius series 0 has {len(Radii[0])} values for {n_t} time steps\n")
        raise ValueError("scri_VectorSizeMismatch")

    ctx = last._ctx
    fit_orders = [N for _, N in fits]
    radii = np.stack([np.asarray(r, dtype=float)[:n_t] for r in Radii]).reshape(n_w, n_t)
    resident = n_t > 0 and all(_resident(W) for W in Ws)
    if resident:
        from . import device_series

        dev = device_series.attach(ctx)
        sources = [W._dev.contiguous() for W in Ws]
        r_dev = device_series._torch().from_numpy(radii).to(dev)
        fitted = device_series.empty(ctx, (len(fits), n_t, n_m))
        _, deficient = engine.extrapolate([x.data_ptr() for x in sources], (r_dev.data_ptr(), n_t, n_m), fit_orders, ctx=ctx,
                                          device=True, out=fitted.data_ptr())
    else:
        fitted, deficient = engine.extrapolate([_host_data(W) for W in Ws], radii, fit_orders, ctx=ctx)
    for k, (slot, N) in enumerate(fits):
        W = WaveformModes(t=last.t, frame=last.frame, data=np.empty((0, n_m), dtype=complex) if resident else fitted[k], ell_min=last.ell_min,
                          ell_max=last.ell_max, frameType=last.frameType, dataType=last.dataType, r_is_scaled_out=last.r_is_scaled_out,
                          m_is_scaled_out=last.m_is_scaled_out, history=list(last.history) + [f"### Extrapolating with N={N}\n"], ctx=ctx)
        if resident:
            W._host, W._dev = None, fitted[k]
        if deficient[k]:
            warnings.warn(f"The fit with N={N} is rank deficient at {int(deficient[k])} of {n_t} time steps; those rows are NaN",
                          np.exceptions.RankWarning, stacklevel=2)
        results[slot] = W
    return results


def extrapolate_waveforms(Ws, Radii, ExtrapolationOrders=[-1, 2, 3, 4, 5, 6], OutputFrame=Inertial, MinTimeStep=0.005,
                          EarliestTime=-3e300, LatestTime=3e300):
    """What scri's file driver `extrapolate` does between reading and writing its files (scri/extrapolation.py:728-853), on
    WaveformModes in memory.  Returns one WaveformModes per order:

      1. all waveforms and radii onto one time axis (set_common_time);
      2. the outermost waveform -- the one with the largest mean radius; the driver sorts by the nominal radii of its file --
         must be in the inertial frame; it goes into its corotating frame, aligned on (0.1, 0.8) of the inspiral;
      3. every other waveform is rotated into that frame;
      4. the fit (_Extrapolate);
      5. each result goes back to the inertial frame and, with OutputFrame = Corotating, into its own corotating frame.

    The waveforms and lists passed in are not changed.  With every input device resident, the results are too."""
    lo, hi = min(ExtrapolationOrders), max(ExtrapolationOrders)
    if hi >= 0 and hi >= len(Ws):
        raise ValueError("Not enough data sets ({}) for max extrapolation order (N={}).".format(len(Ws), hi))
    if lo < -len(Ws):
        raise ValueError("Not enough data sets ({}) for min extrapolation order (N={}).".format(len(Ws), lo))
    by_radius = np.argsort([np.mean(np.asarray(r, dtype=float)) for r in Radii], kind="stable")
    common, radii = list(Ws), list(Radii)
    set_common_time(common, radii, MinTimeStep, EarliestTime, LatestTime)
    frame_source = common[by_radius[-1]]
    if frame_source.frameType != Inertial:
        raise ValueError("Extrapolation assumes that the input data are in the inertial frame")
    frame_source.to_corotating_frame(z_alignment_region=(0.1, 0.8))
    for k in by_radius[:-1]:
        common[k].rotate_decomposition_basis(frame_source.frame)
        common[k].frameType = Corotating
    results = _Extrapolate(common, radii, ExtrapolationOrders, [], None)
    for W in results:
        if OutputFrame in (Inertial, Corotating):
            W.to_inertial_frame()
            if OutputFrame == Corotating:
                W.to_corotating_frame()
    return results
