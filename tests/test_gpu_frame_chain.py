"""The frame chain on the device (scri_amd/csrc/kernels_frames.hip, engine_frames.hip): corotating and coprecessing frames built
from modes that stay in HBM -- frame integration as a prefix product of interval rotors, the dominant axis by Jacobi and a scan of
sign maps, the minimal rotation from spline slopes and a spline antiderivative -- against the oracle, the retained host routine,
numpy/scipy restatements in this file, and the host-resident path (bit for bit).  Every measured figure is printed before its
assertion.  No test masks a time step except where the existing tests of the same quantity do (the spline ends)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import mode_calculations_ref as mc
from oracle import quat, rotations_ref
from tests.helpers.frame_cases import assert_neighbour_cosines_clear_of_half as _assert_neighbour_cosines_clear_of_half
from tests.helpers.frame_cases import continuous_loop as _continuous_loop

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps


def _about(axis, angle):
    axis = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    return np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis[None, :]], axis=-1)


def _precessing_rotors(t, spin=0.15):
    """cone precession of the body axis (tilt growing from 0.3, carried around z) plus a spin about the body's own axis"""
    span = t[-1] - t[0]
    return quat.qmul(quat.qmul(_about([0, 0, 1], 0.02 * t), _about([0, 1, 0], 0.3 + 0.2 * (t - t[0]) / span)), _about([0, 0, 1], spin * t))


def _wm(t, data, ell_min, ell_max, ctx):
    import scri_amd

    return scri_amd.WaveformModes(t=t, data=data, ell_min=ell_min, ell_max=ell_max, dataType=scri_amd.h, frameType=scri_amd.Inertial,
                                  r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)


def _precessing_chirp(n, seed=4):
    """l = 2..8: a chirp that is simple in a precessing frame -- (2, +-2) dominant, every other mode small and generic -- seen from the
    inertial frame.  Built with the oracle's rotation on the CPU: nothing of the code under test enters the input."""
    t = np.linspace(0.0, 200.0, n)
    LM = np.array([[l, m] for l in range(2, 9) for m in range(-l, l + 1)])
    rng = np.random.default_rng(seed)
    amp = 0.01 * (rng.normal(size=LM.shape[0]) + 1j * rng.normal(size=LM.shape[0]))
    for i, (l, m) in enumerate(LM):
        amp[i] += {(2, 2): 1.0, (2, -2): 1.0, (3, 3): 0.2j, (3, -3): 0.2j, (4, 4): 0.05, (4, -4): 0.05}.get((l, m), 0.0)
    phase = 0.3 * t + 0.002 * t**2
    data = amp[None, :] * (1.0 + 0.004 * t)[:, None] * np.exp(-1j * LM[None, :, 1] * phase[:, None])
    R = _precessing_rotors(t, spin=0.0)
    # rotate_physical_system(R) = rotate_decomposition_basis(R^-1)
    return t, rotations_ref.rotate_by_series(data, quat.as_spinor_array(quat.qconj(R)), 2, 8)


# ---------------------------------------------------------------------------------------------------------------- 1. residency
def _small_precessing_waveform(ctx, n=4000):
    t = np.linspace(0.0, 200.0, n)
    LM = np.array([[l, m] for l in range(2, 5) for m in range(-l, l + 1)])
    amp = np.zeros(LM.shape[0], dtype=complex)
    for i, (l, m) in enumerate(LM):
        amp[i] = {(2, 2): 1.0, (2, -2): 1.0, (3, 3): 0.1j, (3, -3): 0.1j, (4, 4): 0.03, (4, -4): 0.03, (2, 0): 0.05}.get((l, m), 0.0)
    data = amp[None, :] * np.exp(-1j * LM[None, :, 1] * (0.2 * t + 0.0005 * t**2)[:, None])
    w = _wm(t, data, 2, 4, ctx)
    w.rotate_physical_system(_precessing_rotors(t))
    w.frame = np.zeros((0, 4))  # the inertial frame we start from
    return w


def test_frames_leave_a_resident_waveform_resident_and_equal_the_host_path(ctx):
    base = _small_precessing_waveform(ctx)
    n = base.n_times
    cases = [
        ("corotating", lambda w: w.to_corotating_frame()),
        ("corotating, z aligned, omega", lambda w: w.to_corotating_frame(z_alignment_region=(0.1, 0.8), return_omega=True)),
        ("corotating, truncated log", lambda w: w.to_corotating_frame(truncate_log_frame=True)),
        ("coprecessing", lambda w: w.to_coprecessing_frame()),
        ("coprecessing, transition", lambda w: w.to_coprecessing_frame(transition_times=(120.0, 160.0))),
    ]
    for name, call in cases:
        host, dev = base.copy(), base.copy().to_device()
        out_h, out_d = call(host), call(dev)
        assert dev.is_device_resident and dev._host is None, name
        assert not host.is_device_resident
        assert np.array_equal(dev.frame, host.frame) and dev.frame.shape == (n, 4), name
        assert dev.frameType == host.frameType and len(dev.history) == len(host.history)
        if isinstance(out_h, tuple):
            for a, b in zip(out_h[1:], out_d[1:]):
                assert np.array_equal(a, b), name
        assert dev.is_device_resident  # (nothing above read .data)
        assert np.array_equal(dev.copy().data, host.data), name
    host, dev = base.copy(), base.copy().to_device()
    for kw in (dict(), dict(RoughDirection=np.array([0.0, 0.0, -1.0]), RoughDirectionIndex=n // 3)):
        a, b = host.LLDominantEigenvector(**kw), dev.LLDominantEigenvector(**kw)
        assert dev.is_device_resident and dev._host is None
        assert np.array_equal(a, b)
    assert np.array_equal(host.LLMatrix(), dev.LLMatrix()) and np.array_equal(host.angular_velocity(), dev.angular_velocity())
    assert dev.is_device_resident and dev._host is None


def test_frame_branches_do_what_they_say(ctx):
    """transition_times: before the transition the frame is the coprecessing frame, after it the frame stands still;
    truncate_log_frame: the assertions of the existing test (test_gpu_mode_calculations.py:182-185) on a resident waveform"""
    from scri_amd import quaternions as Q

    base = _small_precessing_waveform(ctx)
    t = base.t
    plain = base.copy().to_device().to_coprecessing_frame()
    faded = base.copy().to_device().to_coprecessing_frame(transition_times=(120.0, 160.0))
    i0, i1 = int(np.argmin(np.abs(t - 120.0))), int(np.argmin(np.abs(t - 160.0)))
    assert np.array_equal(faded.frame[:i0], plain.frame[:i0])
    om = Q.angular_velocity(faded.frame, t)
    print("frame angular velocity after the transition:", np.abs(om[i1 + 5 : -5]).max())
    assert np.abs(om[i1 + 5 : -5]).max() < 1e-8 and np.abs(Q.angular_velocity(plain.frame, t)[i1 + 5 : -5]).max() > 1e-3
    w, log_frame = base.copy().to_device().to_corotating_frame(truncate_log_frame=True)
    assert w.is_device_resident and log_frame.shape == (w.n_times, 4)
    power_of_2 = 2 ** int(-np.floor(np.log2(2e-12)))
    assert np.array_equal(log_frame * power_of_2, np.round(log_frame * power_of_2))
    assert np.abs(w.frame - Q.exp(log_frame)).max() < 4 * EPS


def test_extrapolation_with_resident_inputs_never_materialises_host_data(ctx):
    import scri_amd
    from scri_amd import extrapolate_waveforms

    rng = np.random.default_rng(12)
    items = []
    for i in range(4):
        t = np.linspace(-10.0 + 0.5 * i, 400.0 + 0.3 * i, 1500 + 13 * i)
        phase = 0.02 * t + 0.00004 * t**2
        data = np.zeros((t.size, 21), dtype=complex)
        data[:, 4 + 2] = 0.1 * np.exp(1j * phase)
        data[:, 4 + 4] = np.exp(-2j * phase) * (1 + 10.0 / (100.0 * (i + 1)))
        data[:, 4 + 0] = np.exp(2j * phase) * (1 + 10.0 / (100.0 * (i + 1)))
        data += 1e-3 * (rng.normal(size=data.shape) + 1j * rng.normal(size=data.shape))
        items.append((scri_amd.WaveformModes(t=t, data=data, ell_min=2, ell_max=4, frameType=scri_amd.Inertial, dataType=scri_amd.h,
                                             r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx), 100.0 * (i + 1) * (1.0 + 0.001 * np.sin(0.01 * t))))
    Ws, Radii = [w for w, _ in items], [r for _, r in items]
    resident = [w.copy().to_device() for w in Ws]
    for frame in (scri_amd.Inertial, scri_amd.Corotating):
        dev = extrapolate_waveforms(resident, Radii, [-1, 2], OutputFrame=frame)
        for w in resident + dev:
            assert w.is_device_resident and w._host is None
        host = extrapolate_waveforms(Ws, Radii, [-1, 2], OutputFrame=frame)
        for D, H in zip(dev, host):
            assert np.array_equal(D.frame, H.frame)
            assert np.array_equal(D.copy().data, H.data)
            assert D.is_device_resident


# ------------------------------------------------------------------------------------------- 2. frame integration vs the oracle
def _smooth_omega(t):
    return np.stack([0.30 * np.sin(0.11 * t) + 0.05, 0.20 * np.cos(0.07 * t + 0.4), 0.25 + 0.10 * np.sin(0.05 * t) + 0.002 * t], axis=1)


@pytest.mark.parametrize("axis", ["uniform", "jittered"])
def test_frame_integration_against_the_oracle(ctx, axis):
    """Bar 1e-10: the reference's own tolerance for the corotating frame (scri tests/test_mode_calculations.py:113-128)."""
    from scri_amd import engine

    n = 20001
    t = np.linspace(0.0, 100.0, n)
    if axis == "jittered":
        t = t + np.random.default_rng(3).uniform(-0.3, 0.3, n) * (t[1] - t[0])
    om = _smooth_omega(t)
    R0 = np.array([0.5, -0.1, 0.7, 0.3])
    R0 /= np.linalg.norm(R0)
    R = engine.frame_from_angular_velocity(t, om, R0=R0, tolerance=1e-12, ctx=ctx)
    ref = mc.integrate_angular_velocity(t, om, R0, rtol=1e-13, atol=1e-13)
    err, drift = np.abs(R - ref).max(), np.abs(np.linalg.norm(R, axis=1) - 1).max()
    print(f"scan vs DOP853 ({axis}, N = {n}): {err:.3e}; | |R| - 1 |: {drift:.3e}")
    assert err < 1e-10
    assert drift <= 4 * EPS  # one normalisation per step: four quotients by a correctly rounded norm, each within eps
    assert np.array_equal(R[0], R0)
    # a device array in, a device array out, the same numbers
    import torch

    R_dev = engine.frame_from_angular_velocity(t, torch.from_numpy(om).to(f"cuda:{ctx.device}"), R0=R0, tolerance=1e-12, ctx=ctx)
    assert R_dev.is_cuda and np.array_equal(R_dev.cpu().numpy(), R)


# ---------------------------------------------------------------------------------------------------------- 3. scan vs march
@pytest.mark.parametrize("n", [100001, 1000001])
def test_prefix_product_against_the_sequential_march(ctx, n):
    """Same sub-step rule, same Magnus step; only the order of the multiplications and the renormalisation differ.  Bar 8 N eps: the
    rounding error of an N-fold product of unit quaternions grows at worst linearly in N."""
    from scri_amd import engine

    t = np.linspace(0.0, 0.005 * (n - 1), n)
    om = _smooth_omega(t)
    R0 = np.array([1.0, 2.0, 3.0, 4.0]) / math.sqrt(30.0)
    R = engine.frame_from_angular_velocity(t, om, R0=R0, tolerance=1e-12, ctx=ctx)
    march = engine.integrate_angular_velocity(t, om, R0=R0, tolerance=1e-12)
    err = np.abs(R - march).max()
    print(f"scan vs march, N = {n}: {err:.3e} (bar {8 * n * EPS:.3e}); | |R| - 1 |: {np.abs(np.linalg.norm(R, axis=1) - 1).max():.3e}")
    assert err <= 8 * n * EPS
    again = engine.frame_from_angular_velocity(t, om, R0=R0, tolerance=1e-12, ctx=ctx)
    assert np.array_equal(again, R)  # no atomics, a fixed order: the same bits every run


# ------------------------------------------------------------------------------------------------------------ 4. dominant axis
def _reference_axis(t, data, ell_min, ell_max, rough, i_index):
    LL = mc.LLMatrix(data, ell_min, ell_max)
    vals, vecs = np.linalg.eigh(LL)
    raw = vecs[:, :, 2]
    gap = (vals[:, 2] - vals[:, 1]) / vals[:, 2]
    return _continuous_loop(raw, rough, i_index), raw, gap, vals[:, 2], np.abs(LL).max()


def test_dominant_axis_of_a_precessing_chirp(ctx):
    n = 5000
    t, data = _precessing_chirp(n)
    w = _wm(t, data, 2, 8, ctx).to_device()
    for i_index in (0, n // 8, n - 1):
        for side in (1.0, -1.0):
            rough = side * np.array([0.1, 0.2, 1.0])
            ref, raw, gap, lam, ll_max = _reference_axis(t, data, 2, 8, rough, i_index)
            # the input conditions, on the reference's own numbers
            assert gap.min() >= 0.05, gap.min()
            _assert_neighbour_cosines_clear_of_half(raw)
            got = w.LLDominantEigenvector(RoughDirection=rough, RoughDirectionIndex=i_index)
            assert w.is_device_resident
            dots = np.sum(got * ref, axis=1)
            assert np.array_equal(np.sign(dots), np.ones(n)), (i_index, side, int(np.sum(dots <= 0)))
            # Davis-Kahan with the existing <LL> bar delta = 1e-13 max|LL| (test_gpu_mode_calculations.py:25)
            bar = 2 * 1e-13 * ll_max / (gap * lam) + 64 * EPS
            err = np.linalg.norm(got - ref, axis=1)
            print(f"axis, anchor {i_index}, side {side:+.0f}: max err {err.max():.3e}, min bar {bar.min():.3e}, min gap {gap.min():.3f}")
            assert np.all(err <= bar)
            assert math.copysign(1.0, float(np.dot(rough, got[i_index]))) == 1.0


def test_dominant_axis_of_the_exactly_diagonal_waveforms(ctx):
    """the reference's constant and linear waveforms (scri tests/test_mode_calculations.py:14-71): <LL> is exactly diagonal"""
    n = 300
    t = np.linspace(1.0, 100.0, n)
    LM = np.array([[l, m] for l in range(0, 9) for m in range(-l, l + 1)])
    base = (LM[:, 1] - 1j * LM[:, 1]).astype(complex)
    for data in (np.repeat(base[None, :], n, axis=0), base[None, :] * t[:, None]):
        ref, raw, gap, lam, ll_max = _reference_axis(t, data, 0, 8, np.array([0.0, 0.0, 1.0]), 0)
        assert gap.min() >= 0.05
        _assert_neighbour_cosines_clear_of_half(raw)
        got = _wm(t, data.copy(), 0, 8, ctx).to_device().LLDominantEigenvector()
        assert np.array_equal(np.sign(np.sum(got * ref, axis=1)), np.ones(n))
        assert np.all(np.linalg.norm(got - ref, axis=1) <= 2 * 1e-13 * ll_max / (gap * lam) + 64 * EPS)


def test_sign_scan_on_a_jumpy_axis_series(ctx):
    """bms_dominant_axis on matrices whose principal axis jumps about, with random raw signs: the scan of sign maps gives the loop's
    signs exactly.  A fifth of the steps jump by up to 49 degrees, half of them turning over as well; every neighbour cosine is at least 0.1 away from
    +-1/2 (asserted)."""
    from scri_amd import engine

    rng = np.random.default_rng(21)
    n = 70001
    v = np.empty((n, 3))
    v[0] = [0.0, 0.0, 1.0]
    # |cos| of a jump.  (Below 1/2 the rule keeps whichever sign the eigensolver happened to return, so its outcome is a property of
    # the solver, not of the matrices: such jumps cannot be compared between two solvers and are left out.)
    allowed = np.linspace(0.65, 1.0, 50)
    for i in range(1, n):
        c = rng.choice(allowed) * rng.choice([-1.0, 1.0]) if rng.uniform() < 0.2 else 1.0 - 1e-3 * rng.uniform()
        perp = np.cross(v[i - 1], rng.normal(size=3))
        perp /= np.linalg.norm(perp)
        v[i] = c * v[i - 1] + math.sqrt(max(0.0, 1.0 - c * c)) * perp
        v[i] /= np.linalg.norm(v[i])
    a = np.cross(v, rng.normal(size=3))
    a /= np.linalg.norm(a, axis=1)[:, None]
    b = np.cross(v, a)
    LL = 4.0 * v[:, :, None] * v[:, None, :] + 2.0 * a[:, :, None] * a[:, None, :] + 1.0 * b[:, :, None] * b[:, None, :]
    LL = 0.5 * (LL + np.swapaxes(LL, 1, 2))
    vals, vecs = np.linalg.eigh(LL)
    raw = vecs[:, :, 2]
    assert ((vals[:, 2] - vals[:, 1]) / vals[:, 2]).min() >= 0.05
    _assert_neighbour_cosines_clear_of_half(raw)
    import torch

    for i_index in (0, n // 8, n - 1):
        rough = np.array([0.3, -0.2, -1.0])
        ref = _continuous_loop(raw, rough, i_index)
        got = engine.dominant_axis(LL, rough=rough, rough_index=i_index, ctx=ctx)
        assert np.array_equal(np.sign(np.sum(got * ref, axis=1)), np.ones(n)), i_index
        err = np.linalg.norm(got - ref, axis=1).max()
        print(f"jumpy axis, anchor {i_index}: max err {err:.3e}")
        assert err <= 2 * 1e-13 * 4.0 / (0.5 * 4.0) + 64 * EPS
        got_dev = engine.dominant_axis(torch.from_numpy(LL).to(f"cuda:{ctx.device}"), rough=rough, rough_index=i_index, ctx=ctx)
        assert np.array_equal(got_dev.cpu().numpy(), got)


def test_sign_scan_with_constant_maps_in_mid_series(ctx):
    """Where |cos| < 1/2 between neighbours the rule flips the vector whatever its neighbour's sign: a CONSTANT map, the case that
    makes the scan a composition of maps and not a product of signs.  Exactly diagonal matrices whose largest entry moves between
    the three places have a known raw eigenvector (Jacobi leaves a diagonal matrix alone: +e_k), neighbour cosines of exactly 0 or
    1, and so runs of identity maps broken by constant ones all along the series (every vector behind the first jump away from
    the anchor ends up flipped, whichever way the anchor points).  Reference: the loop on that raw axis."""
    from scri_amd import engine

    rng = np.random.default_rng(33)
    n = 50001
    k = np.zeros(n, dtype=int)
    for i in range(1, n):
        k[i] = rng.integers(0, 3) if rng.uniform() < 0.3 else k[i - 1]
    assert 5000 < np.count_nonzero(np.diff(k)) < n - 5000
    LL = np.zeros((n, 3, 3))
    for a in range(3):
        LL[:, a, a] = np.where(k == a, 4.0, 1.0 + ((a - k) % 3))  # 4 at place k, 2 and 3 at the other two
    raw = np.eye(3)[k]
    _assert_neighbour_cosines_clear_of_half(raw)
    assert (LL[np.arange(n), k, k] == 4.0).all() and (np.sort(np.diagonal(LL, axis1=1, axis2=2), axis=1)[:, 1] == 3.0).all()  # gap 0.25
    for i_index in (0, n // 8, n - 1):
        for rough in (np.array([1.0, 1.0, 1.0]), np.array([-1.0, -1.0, -1.0])):
            ref = _continuous_loop(raw, rough, i_index)
            got = engine.dominant_axis(LL, rough=rough, rough_index=i_index, ctx=ctx)
            assert np.array_equal(got, ref), (i_index, rough[0], int(np.sum(np.any(got != ref, axis=1))))


# ------------------------------------------------------------------------------- 5. minimal rotation, rotor angular velocity
def _scipy_minimal_rotation(R, t, iterations):
    from scipy.interpolate import CubicSpline

    z = np.array([0.0, 0.0, 0.0, 1.0])
    for _ in range(iterations):
        Rdot = CubicSpline(t, R).derivative()(t)
        hgd = quat.qmul(quat.qmul(Rdot, z), quat.qconj(R))[:, 0]
        hg = CubicSpline(t, hgd).antiderivative()(t)
        R = quat.qmul(R, np.stack([np.cos(hg), 0 * hg, 0 * hg, np.sin(hg)], axis=1))
    return R


@pytest.mark.parametrize("n", [3000, 100000])
def test_minimal_rotation_and_rotor_angular_velocity_against_scipy(ctx, n):
    """Bars: the project's spline parity bars for O(1) smooth data, tests/test_gpu_mode_calculations.py:57-58 -- 1e-9 for a quantity
    that is a spline derivative (the rotor angular velocity), 1e-11 for one that is a spline integral (the minimally rotated frame)."""
    from scipy.interpolate import CubicSpline

    from scri_amd import engine
    from scri_amd import quaternions as Q

    t = np.linspace(0.0, 200.0, n)
    R = _precessing_rotors(t)
    om = engine.rotor_angular_velocity(t, R, ctx=ctx)
    om_ref = 2.0 * quat.qmul(CubicSpline(t, R).derivative()(t), quat.qconj(R))[:, 1:]
    print(f"rotor angular velocity, N = {n}: {np.abs(om - om_ref).max():.3e}")
    assert np.abs(om - om_ref).max() <= 1e-9
    Rm = engine.minimal_rotation(t, R, iterations=3, ctx=ctx)
    ref = _scipy_minimal_rotation(R, t, 3)
    bar = 1e-11
    print(f"minimal rotation, N = {n}: {np.abs(Rm - ref).max():.3e} (bar {bar:.3e})")
    assert np.abs(Rm - ref).max() <= bar
    # the module-level helpers with a context are the same entries
    assert np.array_equal(Q.minimal_rotation(R, t, iterations=3, ctx=ctx), Rm) and np.array_equal(Q.angular_velocity(R, t, ctx=ctx), om)
    # physically: no angular velocity of the result along its own z axis, away from the spline ends (as test_to_coprecessing_frame)
    z_axis = quat.qmul(quat.qmul(Rm, np.array([0.0, 0.0, 0.0, 1.0])), quat.qconj(Rm))[:, 1:]
    along = np.sum(engine.rotor_angular_velocity(t, Rm, ctx=ctx) * z_axis, axis=-1)
    print(f"angular velocity along the own axis: {np.abs(along[100:-100]).max():.3e}")
    assert np.abs(along[100:-100]).max() < 1e-8
    assert np.abs(np.sum(om * z_axis, axis=-1)).min() > 0.1


# --------------------------------------------------------------------------------------------------------------- 6. end to end
def test_coprecessing_frame_of_a_million_steps_device_resident(ctx):
    """the scenario and the assertions of test_to_coprecessing_frame (tests/test_gpu_mode_calculations.py:121-163) at N = 1e6,
    l = 2..8, on the device throughout"""
    import scri_amd
    from scri_amd import quaternions as Q

    n = 1000000
    t = np.linspace(0.0, 2000.0, n)
    LM = np.array([[l, m] for l in range(2, 9) for m in range(-l, l + 1)])
    amp = np.zeros(LM.shape[0], dtype=complex)
    for i, (l, m) in enumerate(LM):
        amp[i] = {(2, 2): 1.0, (2, -2): 1.0, (3, 3): 0.1j, (3, -3): 0.1j, (4, 4): 0.03, (4, -4): 0.03}.get((l, m), 0.0)
    data = np.repeat(amp[None, :], n, axis=0)
    w = _wm(t, data.copy(), 2, 8, ctx).to_device()
    R = Q.multiply(Q.multiply(_about([0, 0, 1], 0.02 * t), _about([0, 1, 0], 0.3 + 0.0 * t)), _about([0, 0, 1], 0.15 * t))
    w.rotate_physical_system(R)
    axis_inertial = Q.multiply(Q.multiply(R, np.array([0.0, 0, 0, 1])), Q.conjugate(R))[:, 1:]
    w.to_coprecessing_frame()
    assert w.is_device_resident and w._host is None
    assert w.frameType == scri_amd.Coprecessing and w.frame.shape == (n, 4)
    R_c = Q.multiply(R, w.frame)
    z_frame = Q.multiply(Q.multiply(R_c, np.array([0.0, 0, 0, 1])), Q.conjugate(R_c))[:, 1:]
    print("z of the frame vs the axis:", np.abs(z_frame - axis_inertial).max())
    assert np.abs(z_frame - axis_inertial).max() < 1e-9
    omega = Q.angular_velocity(R_c, t, ctx=ctx)
    print("angular velocity about the axis:", np.abs(np.sum(omega * z_frame, axis=-1))[100:-100].max())
    assert np.abs(np.sum(omega * z_frame, axis=-1))[100:-100].max() < 1e-8
    assert np.abs(np.sum(Q.angular_velocity(R, t, ctx=ctx) * axis_inertial, axis=-1)).min() > 0.1
    dpa = w.LLDominantEigenvector()
    assert w.is_device_resident
    assert np.abs(np.abs(dpa[:, 2]) - 1).max() < 1e-9
    assert np.abs(np.abs(w.data) - np.abs(data)).max() < 1e-9
    w.to_inertial_frame()
    assert w.frameType == scri_amd.Inertial


def test_corotating_frame_of_a_million_steps_device_resident(ctx):
    """the constant-waveform case of test_reference_corotating_frame_case (tests/test_gpu_mode_calculations.py:61-78) at N = 1e6"""
    import scri_amd

    n = 1000000
    t = np.linspace(-10.0, 10.0, n)
    LM = np.array([[l, m] for l in range(2, 9) for m in range(-l, l + 1)])
    data = np.repeat((LM[:, 1] - 1j * LM[:, 1])[None, :], n, axis=0).astype(complex)
    omega = 2 * math.pi / 5.0
    R0 = np.array([1.0, 2, 3, 4]) / math.sqrt(30)
    half = np.zeros((n, 4))
    half[:, 3] = omega / 2 * t
    R_in = quat.qmul(R0[None, :], quat.qexp(half))
    w_rot = _wm(t, data.copy(), 2, 8, ctx).to_device()
    w_rot.rotate_physical_system(R_in)
    R_out = scri_amd.mode_calculations.corotating_frame(w_rot, R0=R_in[0], tolerance=1e-12)
    assert w_rot.is_device_resident and w_rot._host is None
    print("corotating frame vs the rotors put in:", np.abs(R_in - R_out).max())
    assert np.allclose(R_in, R_out, atol=1e-10, rtol=0.0)
    w_rot.to_corotating_frame(R0=R_in[0], tolerance=1e-12)
    assert w_rot.is_device_resident and w_rot._host is None
    assert np.allclose(w_rot.data, data, atol=1e-8, rtol=1e-5)
    assert w_rot.frameType == scri_amd.Corotating


# ------------------------------------------------------------------------------------------------------------ 7. ABI hostility
def test_new_exports_refuse_bad_arguments():
    """in a child process, as tests/test_gpu_abi_robustness.py: a crash is a failure with the name of the call that died"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "frame_chain_abi_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=900)
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert out.returncode == 0 and lines and lines[-1].startswith("done"), (
        f"the child died (exit {out.returncode}) in: {lines[-1] if lines else '(nothing printed)'}\n{out.stderr[-1500:]}")
    assert int(lines[-1].split()[1]) >= 40
    for l in lines[:-1]:
        label, want, rc = l.rsplit(" ", 2)
        assert (int(rc) == 0) if want == "want0" else (int(rc) < 0), l
