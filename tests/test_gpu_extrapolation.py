"""The extrapolation fit on the GPU (bms_extrapolate through scri_amd._Extrapolate / extrapolate_waveforms) against the reference's
own outputs (g29, tests/golden/make_golden_extrapolation.py), a per-step numpy.polynomial.polynomial.polyfit restatement, and the
exact limit of data that are polynomials in 1/r.  Bar of the fit comparisons, per time step: |delta| <= C kappa eps max|y|, kappa the
condition number of the scaled Vandermonde matrix of the step (both solvers are backward stable)."""
import os
import warnings

import numpy as np
import pytest
from numpy.polynomial.polynomial import polyfit, polyvander

from tests.golden.make_golden_extrapolation import ORDERS, ROW_STEP, common_time_inputs, fit_inputs

pytestmark = pytest.mark.gpu

G29 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g29_ref_extrapolation.npz")
EPS = np.finfo(float).eps
C_BAR = 16.0


@pytest.fixture(scope="module")
def g29():
    return np.load(G29)


def _wms(t, data, ctx, ell_min=2, ell_max=8):
    import scri_amd

    return [scri_amd.WaveformModes(t=t, data=d, ell_min=ell_min, ell_max=ell_max, frameType=scri_amd.Corotating, dataType=scri_amd.h,
                                   r_is_scaled_out=True, m_is_scaled_out=True, history=["# input"], ctx=ctx) for d in data]


def _bar(radii, data, rows, N):
    """C kappa eps max|y| for each of `rows`"""
    out = []
    for t in rows:
        V = polyvander(1.0 / radii[:, t], N)
        V = V / np.linalg.norm(V, axis=0)
        out.append(C_BAR * np.linalg.cond(V) * EPS * np.abs(data[:, t]).max())
    return np.array(out)


@pytest.mark.parametrize("kind", ["poly", "noisy"])
def test_fit_matches_g29_polyfit_and_the_exact_limit(ctx, g29, kind):
    from scri_amd import _Extrapolate

    t, radii, data, c0 = fit_inputs(kind)
    Ws = _wms(t, data, ctx)
    out = _Extrapolate(Ws, list(radii), ORDERS)
    head = Ws[-1].history  # (the outermost waveform's history, then the line of the order)
    rows = np.arange(0, t.size, ROW_STEP)
    every = np.arange(0, t.size, 7)
    for N, W in zip(ORDERS, out):
        assert W.data.shape == (t.size, 77)
        if N < 0:
            np.testing.assert_array_equal(W.data, data[N])
            assert W.history[: len(head)] == head and W.history[-1] == f"### Extrapolating with N={N}\n"
            continue
        assert W.history[: len(head)] == head and W.history[len(head)] == f"### Extrapolating with N={N}\n"
        assert (W.ell_min, W.ell_max, W.dataType, W.frameType) == (2, 8, Ws[-1].dataType, Ws[-1].frameType)
        got = W.data
        # the reference's own outputs
        err = np.abs(got[rows] - g29[f"{kind}_N{N}"]).max(axis=1)
        assert np.all(err <= _bar(radii, data, rows, N)), (N, err.max())
        # a per-step polyfit restatement on every 7th step
        ref = np.array([polyfit(1.0 / radii[:, s], data[:, s, :], N)[0] for s in every])
        err = np.abs(got[every] - ref).max(axis=1)
        assert np.all(err <= _bar(radii, data, every, N)), (N, err.max())
        if kind == "poly" and N >= 3:  # data of degree 3 in 1/r: the limit itself
            rel = np.abs(got - c0).max(axis=1) / np.abs(c0).max(axis=1)
            assert rel.max() <= 1e-12, (N, rel.max())


def test_host_device_and_blocks_are_bit_identical(ctx):
    import torch

    from scri_amd import device_series, engine

    t, radii, data, _ = fit_inputs("noisy")
    orders = [0, 2, 3, 4, 5, 1, 6, 7, 8]  # (more than one launch's worth of orders, in any order)
    host, counts = engine.extrapolate(list(data), radii, orders, ctx=ctx)
    assert not counts.any()
    # every order against the per-step polyfit: orders 6..8 go through the kernel built for up to 16 columns, and 8 through the
    # second launch of the call (a launch takes at most 8 orders)
    every = np.arange(0, t.size, 7)
    for k, N in enumerate(orders):
        ref = np.array([polyfit(1.0 / radii[:, s], data[:, s, :], N)[0] for s in every])
        err = np.abs(host[k, every] - ref).max(axis=1)
        assert np.all(err <= _bar(radii, data, every, N)), (N, err.max())
    for blocks in (3, 7, 16):
        again, _ = engine.extrapolate(list(data), radii, orders, ctx=ctx, blocks=blocks)
        np.testing.assert_array_equal(again, host)
    # strided host views (row stride > n_modes) are read in place
    wide = np.zeros((data.shape[0], data.shape[1], 90), dtype=complex)
    wide[:, :, 5:82] = data
    strided, _ = engine.extrapolate([w[:, 5:82] for w in wide], radii, orders, ctx=ctx, blocks=4)
    np.testing.assert_array_equal(strided, host)
    dev = device_series.attach(ctx)
    srcs = [device_series.to_device(ctx, d) for d in data]
    r_dev = torch.from_numpy(np.ascontiguousarray(radii)).to(dev)
    out = device_series.empty(ctx, (len(orders),) + data.shape[1:])
    _, counts = engine.extrapolate([s.data_ptr() for s in srcs], (r_dev.data_ptr(), data.shape[1], data.shape[2]), orders, ctx=ctx,
                                   device=True, out=out.data_ptr())
    np.testing.assert_array_equal(out.cpu().numpy(), host)
    # and _Extrapolate on device-resident waveforms keeps its results there
    from scri_amd import _Extrapolate

    Ws = [w.to_device() for w in _wms(t, data, ctx)]
    res = _Extrapolate(Ws, list(radii), [-2, 3, 5])
    assert all(W.is_device_resident for W in res)
    np.testing.assert_array_equal(res[1].data, host[2])
    np.testing.assert_array_equal(res[2].data, host[4])
    np.testing.assert_array_equal(res[0].data, data[-2])


def test_rank_deficient_steps_are_nan_and_counted(ctx):
    from scri_amd import _Extrapolate, engine

    rng = np.random.default_rng(9)
    n_r, n_t = 6, 300
    t = np.linspace(0.0, 1.0, n_t)
    radii = np.geomspace(50.0, 500.0, n_r)[:, None] * np.ones((1, n_t))
    bad = np.array([17, 18, 150, 299])
    radii[3, bad] = radii[2, bad]  # two equal radii at these steps: the fit of order n_radii - 1 has no unique answer
    radii[1, 200] = np.nan  # and no radius at all at this one: every fit of order >= 1 is undefined (order 0 never looks at r)
    data = rng.normal(size=(n_r, n_t, 21)) + 1j * rng.normal(size=(n_r, n_t, 21))
    out, counts = engine.extrapolate(list(data), radii, [n_r - 1, n_r - 2, 2, 0], ctx=ctx)
    assert list(counts) == [bad.size + 1, 1, 1, 0]
    assert np.all(np.isnan(out[0, bad])) and np.all(np.isnan(out[:3, 200]))
    assert np.all(np.isfinite(np.delete(out[0], np.append(bad, 200), axis=0)))
    assert np.all(np.isfinite(np.delete(out[1:3], 200, axis=1))) and np.all(np.isfinite(out[3]))
    np.testing.assert_allclose(out[3], data.mean(axis=0), rtol=0, atol=1e-14)
    with pytest.warns(np.exceptions.RankWarning, match="N=5 is rank deficient at 5 of 300"):
        res = _Extrapolate(_wms(t, data, ctx, 2, 4), list(radii), [n_r - 1])
    assert np.all(np.isnan(res[0].data[bad]))


def test_extrapolate_waveforms_against_composed_steps(ctx):
    """The driver's steps composed from existing scri_amd calls, with the CPU polyfit in the middle."""
    import scri_amd
    from scri_amd import extrapolate_waveforms
    from scri_amd.extrapolation import intersection

    rng = np.random.default_rng(12)
    n_r, ell_max = 5, 4
    items = []
    for i in range(n_r):
        t = np.linspace(-10.0 + 0.5 * i, 400.0 + 0.3 * i, 1500 + 13 * i)
        phase = 0.02 * t + 0.00004 * t**2
        data = np.zeros((t.size, 21), dtype=complex)
        data[:, 4 + 2] = 0.1 * np.exp(1j * phase)  # (2, 0)
        data[:, 4 + 4] = np.exp(-2j * phase) * (1 + 10.0 / (100.0 * (i + 1)))  # (2, 2)
        data[:, 4 + 0] = np.exp(2j * phase) * (1 + 10.0 / (100.0 * (i + 1)))  # (2, -2)
        data += 1e-3 * (rng.normal(size=data.shape) + 1j * rng.normal(size=data.shape))
        r = 100.0 * (i + 1) * (1.0 + 0.001 * np.sin(0.01 * t))
        items.append((scri_amd.WaveformModes(t=t, data=data, ell_min=2, ell_max=ell_max, frameType=scri_amd.Inertial,
                                             dataType=scri_amd.h, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx), r))
    Ws, Radii = [w for w, _ in items], [r for _, r in items]
    orders = [-1, 2, 3]
    got = extrapolate_waveforms(Ws, Radii, orders)
    got_c = extrapolate_waveforms(Ws, Radii, orders, OutputFrame=scri_amd.Corotating)
    # the same steps by hand
    T = intersection([-3e300, 3e300], Ws[0].t, 0.005, -3e300, 3e300)
    for w in Ws[1:]:
        T = intersection(T, w.t)
    R = np.array([scri_amd.engine.cubic_spline(w.t, r.astype(complex), T, ctx=ctx).real for w, r in items])
    V = [w.interpolate(T) for w in Ws]
    V[-1].to_corotating_frame(z_alignment_region=(0.1, 0.8))
    for w in V[:-1]:
        w.rotate_decomposition_basis(V[-1].frame)
    Y = np.array([w.data for w in V])
    for N, W, Wc in zip(orders, got, got_c):
        if N < 0:
            exp = V[N].data
        else:
            exp = np.array([polyfit(1.0 / R[:, s], Y[:, s, :], N)[0] for s in range(T.size)])
        e = scri_amd.WaveformModes(t=T, data=exp, frame=V[-1].frame, ell_min=2, ell_max=ell_max, frameType=scri_amd.Corotating,
                                   dataType=scri_amd.h, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
        e.to_inertial_frame()
        assert W.frameType == scri_amd.Inertial and np.array_equal(W.t, T)
        assert np.abs(W.data - e.data).max() <= 1e-10 * np.abs(e.data).max(), N
        e.to_corotating_frame()
        assert Wc.frameType == scri_amd.Corotating
        assert np.abs(Wc.data - e.data).max() <= 1e-10 * np.abs(e.data).max(), N
    # device-resident inputs: device-resident results, the same numbers
    dev = extrapolate_waveforms([w.copy().to_device() for w in Ws], Radii, orders)
    for W, D in zip(got, dev):
        assert D.is_device_resident
        assert np.abs(D.data - W.data).max() <= 1e-12 * np.abs(W.data).max()


def test_set_common_time_matches_g29(ctx, g29):
    import scri_amd
    from scri_amd.extrapolation import set_common_time

    items = common_time_inputs()
    Ws = [scri_amd.WaveformModes(t=t, data=d, ell_min=2, ell_max=3, frameType=scri_amd.Corotating, dataType=scri_amd.h, ctx=ctx)
          for t, _, d in items]
    Radii = [r for _, r, _ in items]
    set_common_time(Ws, Radii, 0.005, -3e300, 3e300)
    np.testing.assert_array_equal(Ws[0].t, g29["common_t"])
    assert np.abs(np.array(Radii) - g29["common_radii"]).max() <= 1e-12 * np.abs(g29["common_radii"]).max()
    assert np.abs(np.array([w.data for w in Ws]) - g29["common_data"]).max() <= 1e-12 * np.abs(g29["common_data"]).max()
