"""Frame-construction quantities that feed the rotation path (scri/mode_calculations.py:46-57 LdtVector,
:298-313 LLMatrix, :403-432 angular_velocity), SURVEY 8(f) rank 3.  One GPU pass (bms_angular_velocity): the cubic-spline
time derivative of the modes, the <Ldt> and <LL> sums over modes per time step, and the 3 x 3 solve.

corotating_frame (:435-491) integrates that angular velocity on the device (bms_corotating_frame: the rotors of the sampling
intervals are independent, the frame is their prefix product).

LLDominantEigenvector (:316-399) is bms_coprecessing_frame without the frame: a Jacobi eigensolve per time step and the sign
choice that makes the axis continuous as a scan of sign maps.

The modes of a device-resident waveform are read where they are: only per-step quantities (vectors, 3 x 3 matrices, rotors) come
to the host.  That holds for the two-waveform forms LVector and LLComparisonMatrix too (:60-180): with a device-resident waveform on
either side they are one bms_pair_brackets launch over both rows; two host-resident waveforms keep the composition of ladder operators.
"""
import numpy as np

from . import engine, quaternions


def _modes(W):
    """the modes as the engine takes them: the device tensor of a resident waveform, else the host array"""
    return W._dev if getattr(W, "is_device_resident", False) else W.data


def _context(W):
    from . import _lib

    ctx = getattr(W, "_ctx", None)
    return ctx if ctx is not None else _lib.default_context()


def _parts(W):
    return engine.angular_velocity(W.t, _modes(W), W.ell_min, W.ell_max, ctx=getattr(W, "_ctx", None), parts=True)


def LdtVector(W):
    r"""<Ldt>^a = \sum \bar f^{l,m'} <l,m'|L_a|l,m> (df/dt)^{l,m}, in the mode frame; [n_times, 3]"""
    return _parts(W)[0]


def LLMatrix(W):
    r"""<LL>^{ab} = Re \sum \bar f^{l,m'} <l,m'|L_a L_b|l,m> f^{l,m}; [n_times, 3, 3]"""
    n = W.n_times
    if 0 < n < 4:
        # the kernel also forms <Ldt>, whose spline needs four samples; <LL> needs none: pad the series with copies of its last row
        if getattr(W, "is_device_resident", False):
            from . import device_series

            data = device_series._torch().cat([W._dev, W._dev[-1:].expand(4 - n, -1)], dim=0).contiguous()
        else:
            data = np.concatenate([W.data, np.repeat(W.data[-1:], 4 - n, axis=0)], axis=0)
        return engine.angular_velocity(np.arange(4.0), data, W.ell_min, W.ell_max, ctx=getattr(W, "_ctx", None), parts=True)[1][:n]
    return _parts(W)[1]


def angular_velocity(W, include_frame_velocity=False):
    """Angular velocity of the waveform (arXiv:1302.2919 Sec. II): solve <Ldt> = -<LL> . omega at every time step."""
    omega = _parts(W)[2]
    if include_frame_velocity and len(W.frame) == W.n_times:
        # + 2 Rdot R^-1 of the frame, its derivative from a cubic spline (scri/mode_calculations.py:426-430)
        omega = omega + engine.rotor_angular_velocity(W.t, W.frame, ctx=getattr(W, "_ctx", None))
    return omega


def _dominant_axis(W, rows, rough, i_index):
    """continuous principal axis of <LL> on the time steps rows = (i1, i2), anchored at step i1 + i_index on the side of `rough`"""
    i1, i2 = rows
    modes = _modes(W)[i1:i2]
    return engine.coprecessing_frame(W.t[i1:i2], modes, W.ell_min, W.ell_max, rough=rough, rough_index=i_index, want_axis=True,
                                     ctx=getattr(W, "_ctx", None))[1]


def LLDominantEigenvector(W, RoughDirection=np.array([0.0, 0.0, 1.0]), RoughDirectionIndex=0):
    """Principal axis of the <LL> matrix at every time step, made continuous in time (mode frame)."""
    n = W.n_times
    if n == 0:
        return np.zeros((0, 3))
    i_index = int(RoughDirectionIndex)
    if i_index < 0:
        i_index += n
    return _dominant_axis(W, (0, n), np.asarray(RoughDirection, dtype=float), i_index)


def _qsqrt(q):
    """square root of a unit quaternion"""
    p = np.array(q, dtype=float)
    p[0] += 1.0
    return p / np.linalg.norm(p)


def _corotating_frame_on_device(W, R0, tolerance, z_alignment_region, want_omega):
    """The frame as a device array [n_times, 4] (not yet normalised), the constant rotor that z_alignment_region asks to multiply it by
    on the right (or None), and the angular velocity on the host (or None)."""
    from . import device_series

    ctx = _context(W)
    frame_dev = device_series.empty_real(ctx, (W.n_times, 4))
    R0 = np.asarray(getattr(R0, "components", R0), dtype=float)
    _, omega = engine.corotating_frame(W.t, _modes(W), W.ell_min, W.ell_max, frame_dev, R0=R0, tolerance=tolerance,
                                       want_omega=want_omega or z_alignment_region is not None, ctx=ctx)
    correction = None
    if z_alignment_region is not None:
        initial_time = W.t[0]
        n4 = W.n_times // 4  # WaveformBase.max_norm_time: skips the first quarter (scri/waveform_base.py:553-575)
        norm = engine.row_norm(None, ctx=ctx, device_tensor=W._dev[n4:]) if getattr(W, "is_device_resident", False) else engine.row_norm(W.data[n4:], ctx=ctx)
        inspiral_time = W.t[n4 + int(np.argmax(norm))] - initial_time
        t1 = initial_time + z_alignment_region[0] * inspiral_time
        t2 = initial_time + z_alignment_region[1] * inspiral_time
        i1 = int(np.argmin(np.abs(W.t - t1)))
        i2 = int(np.argmin(np.abs(W.t - t2)))
        if i2 <= i1:
            raise ValueError(f"z_alignment_region={z_alignment_region} selects no time steps")
        R = frame_dev[i1:i2].cpu().numpy()
        i1m = max(0, i1 - 10)
        rough = omega[i1m + 10]
        Vhat = _dominant_axis(W, (i1, i2), rough, 0)
        V = np.concatenate([np.zeros((Vhat.shape[0], 1)), Vhat], axis=1)
        Vhat_corot = quaternions.multiply(quaternions.multiply(quaternions.conjugate(R), V), R)[:, 1:]
        mean = np.concatenate([[0.0], np.mean(Vhat_corot, axis=0)])
        mean /= np.linalg.norm(mean)
        correction = quaternions.conjugate(_qsqrt(quaternions.multiply(np.array([0.0, 0.0, 0.0, -1.0]), mean)))  # sqrt(-z V)^-1
    return frame_dev, correction, (omega if want_omega else None)


def corotating_frame(W, R0=(1.0, 0.0, 0.0, 0.0), tolerance=1e-12, z_alignment_region=None, return_omega=False):
    """Rotor taking the current mode frame into the corotating frame: the integral of the waveform's angular velocity
    starting from R0 (scri/mode_calculations.py:435-491).  z_alignment_region = (f1, f2): additionally align the dominant
    eigenvector of <LL>, averaged over that fraction of the inspiral, with the z axis."""
    frame_dev, correction, omega = _corotating_frame_on_device(W, R0, tolerance, z_alignment_region, return_omega)
    engine.frame_adjust(frame_dev, right=correction, ctx=_context(W))
    frame = frame_dev.cpu().numpy()
    return (frame, omega) if return_omega else frame


# ---- two-waveform versions (scri/mode_calculations.py:55-260): <f| L_a |g> and <f| L_a L_b |g>
def _ladder_applied(W, which):
    """L_+ g, L_- g or L_z g along the mode axis (one bms_mode_map launch): (L_+ g)_{l,m} = sqrt((l - m + 1)(l + m)) g_{l,m-1}, ..."""
    LM = np.asarray(W.LM)
    ell, m = LM[:, 0], LM[:, 1]
    own = np.arange(ell.size, dtype=np.int32)
    if which == "z":
        src, coef = own, m.astype(float)
    elif which == "+":
        src = np.where(m - 1 >= -ell, own - 1, -1).astype(np.int32)
        coef = np.sqrt(np.maximum((ell - (m - 1)) * (ell + (m - 1) + 1.0), 0.0))
    else:
        src = np.where(m + 1 <= ell, own + 1, -1).astype(np.int32)
        coef = np.sqrt(np.maximum((ell + (m + 1)) * (ell - (m + 1) + 1.0), 0.0))
    out = W.copy()
    out.data = engine.mode_map(W.data, src, coef.astype(complex), ctx=getattr(W, "_ctx", None))
    return out


def _braket(W1, W2):
    return np.einsum("ij, ij -> i", np.conjugate(W1.data), W2.data)


def _is_resident(W):
    return getattr(W, "is_device_resident", False) and len(W._data_shape()) == 2


def _either_resident(W1, W2):
    return _is_resident(W1) or _is_resident(W2)


def pair_brackets(W1, W2, want, ell_min=None, ell_max=None):
    """The brackets `want` (engine.PAIR_NAMES) of two waveforms of which at least one is device resident, on l = ell_min .. ell_max
    (default: the range of W1, which W2 then shares), in one bms_pair_brackets launch: device tensors.  The range is read where it lies in
    either row; a host-resident partner is uploaded for the call and stays host resident; nobody's `data` is read."""
    from . import device_series

    resident = [W for W in (W1, W2) if _is_resident(W)]
    if len(resident) == 2 and W1._ctx is not W2._ctx:
        raise ValueError("the two device-resident waveforms live on different contexts")
    ctx = resident[0]._ctx
    if ell_min is None:
        if (W1.ell_min, W1.ell_max) != (W2.ell_min, W2.ell_max):
            raise ValueError(f"the waveforms hold different modes: l = {W1.ell_min} .. {W1.ell_max} and {W2.ell_min} .. {W2.ell_max}")
        ell_min, ell_max = W1.ell_min, W1.ell_max
    if W1.n_times != W2.n_times:
        raise ValueError(f"the waveforms hold {W1.n_times} and {W2.n_times} time steps")
    a, b = (W._dev if _is_resident(W) else device_series.to_device(ctx, np.ascontiguousarray(W.data, dtype=complex)) for W in (W1, W2))
    return engine.pair_brackets(a, b, ell_min, ell_max, W1.ell_min, W2.ell_min, want=want, ctx=ctx)


def _plus_minus_z(W1, W2, which):
    """the brackets "L" [n, 3] or "LL" [n, 9] in the (+, -, z) basis on the host: one launch with a device-resident waveform, else the
    composition of ladder operators on host data"""
    if _either_resident(W1, W2):
        return pair_brackets(W1, W2, which).cpu().numpy()
    if which == "L":
        return np.stack([_braket(W1, _ladder_applied(W2, w)) for w in "+-z"], axis=1)
    T = {}
    for b in "+-z":
        right = _ladder_applied(W2, b)
        for a in "+-z":
            T[a + b] = _braket(W1, _ladder_applied(right, a))
    return np.stack([T[k] for k in ("++", "+-", "-+", "--", "+z", "z+", "-z", "z-", "zz")], axis=1)


def LVector(W1, W2):
    r"""<L>^a = \sum \bar f^{l,m'} <l,m'|L_a|l,m> g^{l,m} for two waveforms with the same modes; complex [n_times, 3], mode frame.
    Device-resident waveforms are read in HBM (bms_pair_brackets) and stay resident."""
    Lp, Lm, Lz = _plus_minus_z(W1, W2, "L").T
    return np.stack([0.5 * (Lp + Lm), -0.5j * (Lp - Lm), Lz], axis=1)


def LLComparisonMatrix(W1, W2):
    r"""<LL>^{ab} = \sum \bar f^{l,m'} <l,m'|L_a L_b|l,m> g^{l,m}; complex [n_times, 3, 3].  Device-resident waveforms are read in HBM
    (bms_pair_brackets) and stay resident.

    As in the reference (scri/mode_calculations.py:187), the <L_y L_z> term is added to the (y, y) element and the (y, z) element
    stays zero -- a slip of an index there, kept so that the numbers are the reference's."""
    T = dict(zip(("++", "+-", "-+", "--", "+z", "z+", "-z", "z-", "zz"), _plus_minus_z(W1, W2, "LL").T))
    LL = np.empty((W1.n_times, 3, 3), dtype=complex)
    LL[:, 0, 0] = (T["++"] + T["+-"] + T["-+"] + T["--"]) / 4
    LL[:, 0, 1] = -1j * (T["++"] - T["+-"] + T["-+"] - T["--"]) / 4
    LL[:, 0, 2] = (T["+z"] + T["-z"]) / 2
    LL[:, 1, 0] = -1j * (T["++"] + T["+-"] - T["-+"] - T["--"]) / 4
    LL[:, 1, 1] = -(T["++"] - T["+-"] - T["-+"] + T["--"]) / 4 - 1j * (T["+z"] - T["-z"]) / 2
    LL[:, 1, 2] = 0.0
    LL[:, 2, 0] = (T["z+"] + T["z-"]) / 2
    LL[:, 2, 1] = -1j * (T["z+"] - T["z-"]) / 2
    LL[:, 2, 2] = T["zz"]
    return LL


def inner_product(t, abar, b, axis=None, apply_conjugate=False, ctx=None):
    """Time-domain complex inner product <a, b> of two arrays of samples (scri/mode_calculations.py:493-533): the definite integral
    over `t` of abar * b (of conj(abar) * b with apply_conjugate), through the not-a-knot cubic spline of the integrand -- the GPU
    spline antiderivative (bms_spline_derivative, order -1).  The time axis is `axis` (default: the first axis whose length is
    len(t), as quaternion.calculus.spline_definite_integral infers it)."""
    t = np.asarray(t, dtype=float)
    integrand = (np.conjugate(abar) if apply_conjugate else np.asarray(abar)) * np.asarray(b)
    if axis is None:
        matches = [i for i, n in enumerate(integrand.shape) if n == t.shape[0]]
        if not matches:
            raise ValueError(f"no axis of the integrand (shape {integrand.shape}) has the length of t ({t.shape[0]})")
        axis = matches[0]
    moved = np.moveaxis(np.asarray(integrand, dtype=complex), axis, 0)
    flat = np.ascontiguousarray(moved.reshape(moved.shape[0], -1))
    total = engine.spline_derivative(t, flat, t[-1:], order=-1, ctx=ctx)[0]
    out = total.reshape(moved.shape[1:])
    return out if np.iscomplexobj(integrand) else out.real
