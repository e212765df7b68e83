"""Centre-of-mass correction of SpEC waveforms from the horizon (and star) trajectories: `scri.SpEC.com_motion`
(scri/SpEC/com_motion.py) on the GPU.

    com_motion               the mass-weighted centre of the two trajectories              bms_com_motion  (kernels_com.hip)
    estimate_avg_com_motion  position and velocity (and acceleration) that bring that track
                             closest to the origin: window, Simpson moments, closed form   bms_com_fit
    remove_avg_com_motion    `w_m.transform(space_translation=x_0, boost_velocity=v_0)` with the result

Where the reference takes paths of `Horizons.h5` / `Matter.h5`, these take anything indexable by the same dataset names: a dict of
arrays, an open `h5py.File`, or a path (opened with `h5py` where it is importable).  Tables given as torch tensors on the context's
device stay there: the track is built and fitted in HBM and only the fit comes back.  Files are neither written nor plotted
(DESIGN section 7); the companions `psi{n}_modes` the reference reads from sibling files are passed in.

The fit is the correctly rounded value of the reference's rule on the same fp64 inputs (double-double sums and closed form), which the
reference's own fp64 evaluation approaches to 1e-15 .. 1e-7 depending on the time axis.
"""
import contextlib
import os

import numpy as np

from . import engine

_HORIZON_A_MASS = "AhA.dir/ChristodoulouMass.dat"
_HORIZON_A_CENTER = "AhA.dir/CoordCenterInertial.dat"
_HORIZON_B_MASS = "AhB.dir/ChristodoulouMass.dat"
_HORIZON_B_CENTER = "AhB.dir/CoordCenterInertial.dat"
_STAR_1 = "InertialCenterOfMassNS1.dat"
_STAR_2 = "InertialCenterOfMassNS2.dat"


def _opened(source):
    """context manager over the mapping behind `source`: a path is opened with h5py, anything else is the mapping itself"""
    if isinstance(source, (str, bytes, os.PathLike)):
        try:
            import h5py
        except ImportError as e:
            raise ImportError("com_motion needs h5py to open a file; with arrays at hand pass a mapping of the dataset names") from e
        return h5py.File(source, "r")
    return contextlib.nullcontext(source)


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "data_ptr") else np.asarray(x)


def _mass_array(m):
    """np.atleast_1d for numbers, numpy arrays and tensors"""
    if hasattr(m, "data_ptr"):
        return m.reshape(-1) if m.dim() == 0 else m
    return np.atleast_1d(m)


def _differ(a, b):
    return bool((a != b).any())


def com_motion(horizons, matter=None, m_A=None, m_B=None, ctx=None):
    """Centre-of-mass motion (t, CoM[n, 3]) from the horizon and/or matter tables (scri/SpEC/com_motion.py:19-120).

    horizons, matter: mappings of the reference's dataset names to `[time, ...]` tables (dict, h5py.File) or paths of the files.
    matter=None: two black holes, both in `horizons`.  Otherwise a neutron-star binary (both stars in `matter`, masses m_A, m_B
    required) or a black hole and a star (`m_B` required; a horizon table longer than the star's is cut to it).  With matter, t and CoM
    are divided by the total mass.  As there, no further input checking is done."""
    if matter is None:
        with _opened(horizons) as hz:
            t = hz[_HORIZON_A_MASS][:, 0]
            m_A = hz[_HORIZON_A_MASS][:, 1]
            x_A = hz[_HORIZON_A_CENTER][:, 1:]
            m_B = hz[_HORIZON_B_MASS][:, 1]
            x_B = hz[_HORIZON_B_CENTER][:, 1:]
        return engine.com_track(t, x_A, x_B, m_A, m_B, matter=False, ctx=ctx)
    with _opened(matter) as mt:
        if _STAR_1 in mt and _STAR_2 in mt:
            x_A = mt[_STAR_1][:, 1:]
            t = mt[_STAR_1][:, 0]
            x_B = mt[_STAR_2][:, 1:]
            t_check = mt[_STAR_2][:, 0]
            if _differ(t, t_check):
                raise ValueError(f"Two NSs do not have the same time: diff = {_host(t) - _host(t_check)}")
            if m_A is None or m_B is None:
                raise ValueError(f"Cannot figure out masses of NSs: {m_A}, {m_B}")
            m_A = _mass_array(m_A)
            m_B = _mass_array(m_B)
        elif _STAR_1 in mt:
            with _opened(horizons) as hz:
                t = hz[_HORIZON_A_MASS][:, 0]
                x_A = hz[_HORIZON_A_CENTER][:, 1:]
                m_A = hz[_HORIZON_A_MASS][:, 1] if m_A is None else _mass_array(m_A)
            x_B = mt[_STAR_1][:, 1:]
            t_check = mt[_STAR_1][:, 0]
            n_hole, n_star = len(t), len(t_check)
            if n_hole < n_star:
                raise ValueError(f"BH and NS time arrays have different lengths: {n_hole} vs {n_star}")
            if n_hole > n_star:
                # the horizon table may run on after the star's has ended: only the steps both have are used (and must agree, below);
                # a mass given per horizon step is cut with them, a single value is not
                per_step_mass = m_A.shape[0] == n_hole
                t, x_A = t[:n_star], x_A[:n_star]
                if per_step_mass:
                    m_A = m_A[:n_star]
            if _differ(t, t_check):
                raise ValueError(
                    "BH and NS do not have the same time: "
                    f"tsize={len(t)}, tchecksize={len(t_check)}, max diff = {max(abs(_host(t) - _host(t_check)))}"
                )
            if m_B is None:
                raise ValueError(f"Cannot figure out mass of NS: {m_B}")
            m_B = _mass_array(m_B)
        else:
            raise Exception(f"Cannot find expected keys in file.  Found {mt.keys()}")
    return engine.com_track(t, x_A, x_B, m_A, m_B, matter=True, ctx=ctx)


def estimate_avg_com_motion(horizons="Horizons.h5", skip_beginning_fraction=0.01, skip_ending_fraction=0.10, plot=False,
                            fit_acceleration=False, matter=None, m_A=None, m_B=None, ctx=None):
    """Optimal translation and boost from the horizon tables (scri/SpEC/com_motion.py:123-303): the initial position x_i and velocity
    v_i (and, with fit_acceleration, the acceleration a_i) for which the centre of mass is closest to the origin in the sense of the
    squared distance integrated over [t_i, t_f], the span of the data less the two skipped fractions.

    Returns (x_i, v_i, t_i, t_f) or (x_i, v_i, a_i, t_i, t_f).  `horizons` may also be a ready pair (t, com) as `com_motion` returns
    it.  plot=True is not provided."""
    if plot:
        raise NotImplementedError("plotting is not part of this package (DESIGN section 7): plot the returned values with the tools at hand")
    if isinstance(horizons, tuple) and len(horizons) == 2:
        t, com = horizons
    else:
        t, com = com_motion(horizons, matter, m_A, m_B, ctx=ctx)
    fit = engine.com_fit(t, com, skip_beginning_fraction, skip_ending_fraction, fit_acceleration, ctx=ctx)
    x_i, v_i, a_i, t_i, t_f = fit["x_i"], fit["v_i"], fit["a_i"], fit["t_i"], fit["t_f"]
    print("Optimal x_i: [{}, {}, {}]".format(*x_i))
    print("Optimal v_i: [{}, {}, {}]".format(*v_i))
    if fit_acceleration:
        print("Optimal a_i: [{}, {}, {}]".format(*a_i))
    print(f"t_i, t_f: {t_i}, {t_f}")
    if fit_acceleration:
        return x_i, v_i, a_i, t_i, t_f
    return x_i, v_i, t_i, t_f


def remove_avg_com_motion(w_m, horizons, matter=None, skip_beginning_fraction=0.01, skip_ending_fraction=0.10, m_A=None, m_B=None,
                          ctx=None, **psi_companions):
    """The waveform in the centre-of-mass frame (scri/SpEC/com_motion.py:306-534, its in-memory part): estimate_avg_com_motion, then
    `w_m.transform(space_translation=x_0, boost_velocity=v_0, **psi_companions)`.  A Weyl scalar below psi4 needs the ones above it
    (`psi4_modes=...`, `psi3_modes=...`), which the reference reads from sibling files.  With `matter` and no masses given, the masses are
    `w_m.metadata.reference_mass1`, `reference_mass2` where the waveform carries them.  A device-resident waveform stays on the device."""
    version_hist = getattr(w_m, "version_hist", None)
    extrapolate_coord_radii = getattr(w_m, "extrapolate_coord_radii", None)
    if matter is not None:
        metadata = getattr(w_m, "metadata", None)
        if m_A is None:
            m_A = getattr(metadata, "reference_mass1", None)
        if m_B is None:
            m_B = getattr(metadata, "reference_mass2", None)
    x_0, v_0, t_0, t_f = estimate_avg_com_motion(horizons, skip_beginning_fraction=skip_beginning_fraction,
                                                 skip_ending_fraction=skip_ending_fraction, matter=matter, m_A=m_A, m_B=m_B, ctx=ctx)
    w_m = w_m.transform(space_translation=x_0, boost_velocity=v_0, **psi_companions)
    w_m.boost_velocity = v_0
    w_m.space_translation = x_0
    if version_hist is not None:
        w_m.version_hist = version_hist
    if extrapolate_coord_radii is not None:
        w_m.extrapolate_coord_radii = extrapolate_coord_radii
    return w_m
