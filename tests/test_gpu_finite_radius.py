"""Raw finite-radius series retarded to tortoise time on the GPU (bms_finite_radius_retard: kernels_retard.hip, engine_retard.hip;
scri_amd.extrapolation.finite_radius_waveform / finite_radius_data) against the numpy yardstick of tests/helpers/finite_radius_ref.py,
whose sums are exactly rounded, and the reference's own outputs (g33, tests/golden/make_golden_finite_radius.py).

Bars.  Times: 4 ulp of max(|T_cum|, |r*|) against the exact-sum yardstick -- one for the rounded sum, one for the subtraction, one each
for the two logarithms, whose libraries document <= 1 ulp, scaled by 2E < r*; against g33 and numpy's cumsum n 2^-53 T_max more, the
standard bound of a sequential sum.  Radii: equal bits.  Data: (p + 2) 2^-52 relative per component, p - 1 products and one by the unit
factor in either arithmetic plus the final product.  Kept indices: equal."""
import ctypes
import os

import numpy as np
import pytest

from tests.golden.make_golden_finite_radius import CH_MASS, COORD_RADIUS, DATA_TYPES, INITIAL_ADM_ENERGY, ROW_STEP, inputs
from tests.helpers import finite_radius_ref as ref

pytestmark = pytest.mark.gpu

G33 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g33_ref_finite_radius.npz")


@pytest.fixture(scope="module")
def g33():
    return np.load(G33)


@pytest.fixture(scope="module")
def TILE():
    from scri_amd import engine

    return engine.retard_tile()


def kept_indices(ctx, t, min_step):
    """the kept indices of the axis t as the entry finds them: column 0 carries the sample number through a factor of exactly 1"""
    from scri_amd import engine

    n = len(t)
    data = np.arange(n, dtype=float).astype(complex).reshape(n, 1)
    t_out, radii, rows, _ = engine.finite_radius_retard(t, np.full(n, 100.0), np.ones(n), data, 100.0, 1.0, 1.0, 1.0, 1, min_time_step=min_step,
                                                        ctx=ctx)
    assert t_out.shape == radii.shape == (rows.shape[0],)
    return rows[:, 0].real.astype(int)


def axes_of(n, TILE, step):
    """the axes of n samples the keep mask is held to: restarts, ties and steps of `step`, placed by the tile"""
    rng = np.random.default_rng(3310 + n)
    out = [ref.restarting_axis(rng, n, step) for _ in range(2)]
    rising = np.cumsum(rng.choice([step, 0.05, 0.3], n)) + 3.0
    out.append(rising)
    out.append(rising[::-1].copy())  # only the last sample survives
    out.append(np.full(n, 7.0))  # ties throughout
    if n > 4:
        k = min(n - 2, max(2, (n // TILE) * TILE - 1 + 3))  # a restart whose dropped stretch straddles a tile edge (or the middle)
        a = rising.copy()
        a[k:] -= a[k] - a[max(k - 9, 0)]
        out.append(a)
        b = rising.copy()  # a restart to before the first time
        b[n // 2:] -= b[n // 2] - b[0] + 1.0
        out.append(b)
        c = rising.copy()  # a late restart that reaches back over several tiles
        c[n - 2:] -= c[n - 2] - c[n // 5]
        out.append(c)
    return out


@pytest.mark.parametrize("tiles, extra", [(0, 1), (0, 2), (1, -1), (1, 0), (1, 1), (2, 1), (70, 3)])
def test_keep_mask_equals_monotonic_indices(ctx, TILE, tiles, extra):
    from scri_amd.extrapolation import monotonic_indices

    n = tiles * TILE + extra
    for step in (0.0, 1e-3, 0.2):
        for t in axes_of(n, TILE, step):
            for min_step in ((1e-3,) if n > 4 * TILE else (0.0, 1e-3, 0.2)):
                np.testing.assert_array_equal(kept_indices(ctx, t, min_step), monotonic_indices(t, min_step))


def test_more_tiles_than_one_workgroup_scans_at_once(ctx, TILE):
    """300 tiles and seven samples: the scans of the tile totals walk two chunks.  With 1 - 2E/R = 1/4 and a lapse of 1 the integrand is
    exactly 2, and on a dyadic axis every term and every sum is exact: the retarded time is known in closed form."""
    from scri_amd import engine
    from scri_amd.extrapolation import monotonic_indices

    n = 300 * TILE + 7
    rng = np.random.default_rng(3320)
    t = np.cumsum(rng.integers(1, 400, n)) / 1024.0
    t[n // 3:] -= t[n // 3] - t[n // 3 - 5 * TILE - 11]
    t[n - 40:] -= 2.0
    idx = monotonic_indices(t)
    R, E = 128.0, 48.0
    data = np.arange(n, dtype=float).astype(complex).reshape(n, 1)
    t_out, radii, rows, _ = engine.finite_radius_retard(t, np.full(n, R), np.ones(n), data, R, E, 1.0, 1.0, 1, ctx=ctx)
    np.testing.assert_array_equal(rows[:, 0].real.astype(int), idx)
    T = t[idx]
    log = np.log((R / (2.0 * E)) - 1.0)
    r_star = R + (2.0 * E) * log
    expected = (T[0] + 2.0 * (T - T[0])) - r_star
    # the sum is exact on both sides.  Here 2E > r*, so the bar is written out: the two libraries' logarithms (<= 1 ulp each) times 2E,
    # and on either side the roundings of the product, of r* and of the final difference
    bar = 2.0 * E * 2 * np.spacing(abs(log)) + 2 * np.spacing(2.0 * E * abs(log)) + 2 * np.spacing(abs(r_star)) + 2 * np.spacing(np.abs(expected))
    dist = np.abs(t_out - expected) / bar
    print("closed form, 300 tiles: distance in units of the bar", dist.max())
    assert dist.max() <= 1
    np.testing.assert_array_equal(radii, np.full(idx.size, R))


def times_bar(y):
    return 4 * np.spacing(np.maximum(np.abs(y["t_cum"]), np.abs(y["r_star"])))


@pytest.mark.parametrize("data_type", DATA_TYPES)
def test_reference_cases_times_radii_and_data(ctx, g33, data_type):
    import scri_amd
    from scri_amd.extrapolation import finite_radius_waveform

    t, areal, lapse, data = inputs(data_type)
    y = ref.retard(t, areal, lapse, data, COORD_RADIUS, INITIAL_ADM_ENERGY, CH_MASS, data_type)
    W, Radii = finite_radius_waveform(t, data, areal, lapse, COORD_RADIUS, INITIAL_ADM_ENERGY, CH_MASS, getattr(scri_amd, data_type), ctx=ctx)
    assert (W.frameType, W.dataType, W.r_is_scaled_out, W.m_is_scaled_out) == (scri_amd.Inertial, getattr(scri_amd, data_type), True, True)
    assert (W.ell_min, W.ell_max, W.n_times) == (2, 8, t.size)
    assert len(W.history) == 1 and W.history[0].startswith("# extrapolation.read_finite_radius_waveform(")
    bar = times_bar(y)
    d_exact = np.abs(W.t - y["t"]) * abs(CH_MASS)
    print(data_type, "times: distance to the exact-sum yardstick in units of the bar", (d_exact / bar).max())
    assert np.all(d_exact <= bar)
    wider = bar + t.size * 2.0**-53 * np.abs(y["t_cum"]).max()
    for name, other in (("cumsum", y["t_cumsum"]), ("g33", g33[f"{data_type}_t"])):
        d = np.abs(W.t - other) * abs(CH_MASS)
        print(data_type, "times: distance to", name, "in ulp of the largest time", (d / np.spacing(np.abs(y["t_cum"]).max())).max())
        assert np.all(d <= wider)
    np.testing.assert_array_equal(Radii, y["radii"])
    np.testing.assert_array_equal(Radii, g33[f"{data_type}_radii"])
    tol = (y["exponent"] + 2) * 2.0**-52
    for got, want in ((W.data, y["data"]), (W.data[::ROW_STEP], g33[f"{data_type}_data"])):
        assert np.all(np.abs(got.real - want.real) <= tol * np.abs(want.real))
        assert np.all(np.abs(got.imag - want.imag) <= tol * np.abs(want.imag))


def restarting_case(TILE, n_cols, seed=3330):
    """3 TILE + 5 samples with two restarts (one across a tile edge), varying radius and lapse, a frame"""
    rng = np.random.default_rng(seed)
    n = 3 * TILE + 5
    t = np.cumsum(rng.uniform(0.05, 0.6, n)) - 40.0
    t[TILE + 2:] -= t[TILE + 2] - t[TILE - 6]
    t[2 * TILE + 40:] -= 3.7
    areal = 248.3 * (1.0 + 1e-3 * np.sin(0.01 * t + 0.4))
    lapse = 0.99 * (1.0 + 1e-3 * np.cos(0.013 * t))
    data = rng.normal(size=(n, n_cols)) + 1j * rng.normal(size=(n, n_cols))
    frame = rng.normal(size=(n, 4))
    return t, areal, lapse, data, frame


@pytest.mark.parametrize("n_cols", [1, 5, 77])
def test_restarting_axis_shapes_strides_and_memories(ctx, TILE, n_cols):
    import torch

    from scri_amd import device_series, engine

    t, areal, lapse, data, frame = restarting_case(TILE, n_cols)
    n = t.size
    E, M, unit, p = 0.9921, 0.9873, 1.0 / 0.9873**2, 4
    y = ref.retard(t, areal, lapse, data, 247.0, E, M, "psi1", frame=frame)
    assert 0 < y["idx"].size < n - 8
    args = (247.0, E, M, unit, p)
    t_out, radii, rows, frame_out = engine.finite_radius_retard(t, areal, lapse, data, *args, frame=frame, ctx=ctx)
    K = y["idx"].size
    assert t_out.shape == radii.shape == (K,) and rows.shape == (K, n_cols) and frame_out.shape == (K, 4)
    bar = times_bar(y)
    d = np.abs(t_out - y["t"]) * abs(M)
    print(n_cols, "columns, restarting axis: times in units of the bar", (d / bar).max())
    assert np.all(d <= bar)
    np.testing.assert_array_equal(radii, y["radii"])
    np.testing.assert_array_equal(frame_out, y["frame"])
    tol = (p + 2) * 2.0**-52
    assert np.all(np.abs(rows.real - y["data"].real) <= tol * np.abs(y["data"].real))
    assert np.all(np.abs(rows.imag - y["data"].imag) <= tol * np.abs(y["data"].imag))
    # two calls: the same bits
    again = engine.finite_radius_retard(t, areal, lapse, data, *args, frame=frame, ctx=ctx)
    for a, b in zip((t_out, radii, rows, frame_out), again):
        np.testing.assert_array_equal(a, b)
    # padded rows on both sides, host arrays
    wide_in = np.full((n, n_cols + 3), np.nan + 0j)
    wide_in[:, :n_cols] = data
    wide_out = np.full((n, n_cols + 2), 5.0 + 0j)
    res = engine.finite_radius_retard(t, areal, lapse, wide_in[:, :n_cols], *args, out=wide_out, ctx=ctx)
    np.testing.assert_array_equal(res[0], t_out)
    np.testing.assert_array_equal(wide_out[:K, :n_cols], rows)
    assert np.all(wide_out[:, n_cols:] == 5.0)
    # device tensors, dense and padded: the bits of the host call; the source is unchanged, the padding and the rows beyond K untouched
    dev = device_series.attach(ctx)
    src = torch.from_numpy(wide_in).to(dev)
    src[:, n_cols:] = 3.0
    before = src.clone()
    d_frame = torch.from_numpy(frame).to(dev)
    for padded in (False, True):
        source = src[:, :n_cols] if padded else src[:, :n_cols].contiguous()
        out = torch.full((n, n_cols + (2 if padded else 0)), 5.0 + 0j, dtype=torch.complex128, device=dev)
        dt_out, d_radii, d_rows, d_frame_out = engine.finite_radius_retard(t, areal, lapse, source, *args, frame=d_frame, out=out, ctx=ctx)
        np.testing.assert_array_equal(dt_out, t_out)
        np.testing.assert_array_equal(d_radii, radii)
        np.testing.assert_array_equal(d_rows.cpu().numpy(), rows)
        np.testing.assert_array_equal(d_frame_out.cpu().numpy(), frame_out)
        full = out.cpu().numpy()
        assert np.all(full[K:] == 5.0) and np.all(full[:, n_cols:] == 5.0)
        assert torch.equal(src, before) and torch.equal(d_frame, torch.from_numpy(frame).to(dev))
    new = engine.finite_radius_retard(t, areal, lapse, src[:, :n_cols], *args, ctx=ctx)[2]  # a new tensor beside the source
    assert new.is_cuda and np.array_equal(new.cpu().numpy(), rows)


def test_waveform_of_a_device_tensor_is_device_resident(ctx, TILE):
    import torch

    import scri_amd
    from scri_amd import device_series
    from scri_amd.extrapolation import finite_radius_waveform

    t, areal, lapse, data, frame = restarting_case(TILE, 21)
    host, Rh = finite_radius_waveform(t, data, areal, lapse, 247.0, 0.9921, 0.9873, scri_amd.psi4, ell_max=4, frame=frame, ctx=ctx)
    tensor = torch.from_numpy(data).to(device_series.attach(ctx))
    W, R = finite_radius_waveform(t, tensor, areal, lapse, 247.0, 0.9921, 0.9873, scri_amd.psi4, frame=frame, ctx=ctx)
    assert W.is_device_resident and not host.is_device_resident and W.ell_max == 4
    np.testing.assert_array_equal(W.t, host.t)
    np.testing.assert_array_equal(R, Rh)
    np.testing.assert_array_equal(W.data, host.data)
    np.testing.assert_array_equal(W.frame, host.frame)
    assert host.frame.shape == (host.n_times, 4) and np.all(np.diff(host.t) > 0)


def raw_call(ctx, **change):
    """the status of the C entry on a small well-formed host call with the named arguments replaced"""
    from scri_amd import _lib

    n = 12
    a = dict(t=np.arange(n, dtype=float), areal=np.full(n, 100.0), lapse=np.ones(n), n_raw=n, data=np.ones((n, 3), dtype=complex), ld=3, n_cols=3,
             mem=_lib.BMS_HOST, coord_radius=99.0, energy=1.0, ch_mass=1.0, unit=1.0, exponent=1, min_step=1e-3, ld_out=3)
    a.update(change)
    keep = _lib.c_i64(-7)
    t_out, r_out, out = np.zeros(n), np.zeros(n), np.zeros((n, 4), dtype=complex)
    rc = _lib.load().bms_finite_radius_retard(
        ctx.handle, _lib.dptr(a["t"]), _lib.dptr(a["areal"]), _lib.dptr(a["lapse"]), a["n_raw"], _lib.vptr(a["data"]), a["ld"], a["n_cols"], a["mem"],
        None, a["coord_radius"], a["energy"], a["ch_mass"], a["unit"], a["exponent"], a["min_step"], ctypes.byref(keep), _lib.dptr(t_out),
        _lib.dptr(r_out), _lib.vptr(out), a["ld_out"], None)
    return rc, int(keep.value)


def test_refusals(ctx):
    from scri_amd import _lib, engine

    assert raw_call(ctx) == (0, 12)
    inf, nan = float("inf"), float("nan")
    for change in (dict(n_raw=0), dict(n_raw=-3), dict(n_cols=0), dict(exponent=0), dict(exponent=6), dict(ch_mass=0.0), dict(coord_radius=0.0),
                   dict(coord_radius=-1.0), dict(coord_radius=inf), dict(coord_radius=nan), dict(energy=0.0), dict(energy=-1.0), dict(energy=inf),
                   dict(energy=nan), dict(min_step=-1e-3), dict(ld=2), dict(ld_out=2), dict(mem=7)):
        rc, kept = raw_call(ctx, **change)
        assert rc == _lib.BMS_ERR_INVALID and kept == -7, change  # (found before anything is launched: the outputs are untouched)
    assert raw_call(ctx) == (0, 12)  # the context still serves
    # a kept radius that is not beyond 2E, not finite: refused, by the first one's name; the same radius at a dropped sample: not read
    n = 40
    t = np.arange(n, dtype=float)
    t[20:] -= 5.0  # samples 15 .. 19 are dropped
    data = np.ones((n, 2), dtype=complex)
    for bad in (2.0, 1.5, -3.0, nan, inf):
        areal = np.full(n, 100.0)
        areal[[25, 31]] = bad
        with pytest.raises(ValueError, match=r"2 kept radii .* the first is areal_radius\[25\]"):
            engine.finite_radius_retard(t, areal, np.ones(n), data, 99.0, 1.0, 1.0, 1.0, 1, ctx=ctx)
        areal = np.full(n, 100.0)
        areal[15:20] = bad
        t_out, _, rows, _ = engine.finite_radius_retard(t, areal, np.ones(n), data, 99.0, 1.0, 1.0, 1.0, 1, ctx=ctx)
        assert rows.shape == (35, 2) and np.all(np.isfinite(t_out))
    with pytest.raises(ValueError, match="not finite"):
        engine.finite_radius_retard(np.array([0.0, nan, 2.0]), np.full(3, 100.0), np.ones(3), data[:3], 99.0, 1.0, 1.0, 1.0, 1, ctx=ctx)
    with pytest.raises(ValueError):
        engine.finite_radius_retard(t, np.full(n, 100.0), np.ones(n), data, 99.0, 1.0, 1.0, 1.0, 7, ctx=ctx)


def test_timing_tag(ctx):
    """the launches are timed under an existing tag: the list of tags is fixed by other tests"""
    from scri_amd import engine

    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        kept_indices(ctx, np.arange(50.0), 1e-3)
        ctx.synchronize()
        timing = ctx.get_timing(reset=True)
    finally:
        ctx.enable_timing(False)
    assert timing["pointwise"][1] == 3 and all(v[1] == 0 for k, v in timing.items() if k != "pointwise")
    assert engine.retard_tile() == 256


def test_pipeline_from_the_file_writers_data(ctx):
    """fake_finite_radius_data -> finite_radius_data -> extrapolate_waveforms against the same chain on the yardstick's tables, at the
    bar of the chain in tests/test_gpu_extrapolation.py (1e-10 of the largest mode).  The distance to h0 is set by the truncation of
    the splines of the writer and of set_common_time, not by rounding: it is printed, and no bar is set on it."""
    import scri_amd
    from scri_amd import extrapolate_waveforms
    from scri_amd.extrapolation import finite_radius_data
    from scri_amd.sample_waveforms import fake_finite_radius_data, fake_precessing_waveform

    kw = dict(t_1=700.0, dt=0.5, r_min=100.0, r_max=300.0, n_radii=6, ell_max=4)
    groups = fake_finite_radius_data(ctx=ctx, **kw)
    assert list(groups)[0] == "R0100.dir" and len(groups) == 6 and groups["R0100.dir"]["data"].shape == (2001, 21)
    Ws, Radii, coord = finite_radius_data(groups, 1.0, ctx=ctx)
    assert [float(c) for c in coord] == [float(g["CoordRadius"]) for g in groups.values()]
    Ys, YR = [], []
    for W, R, g in zip(Ws, Radii, groups.values()):
        y = ref.retard(g["t"], g["ArealRadius"], g["AverageLapse"], g["data"], g["CoordRadius"], g["InitialAdmEnergy"], 1.0, "h")
        assert W.n_times == y["idx"].size == 2001
        assert np.all(np.abs(W.t - y["t"]) <= times_bar(y))
        np.testing.assert_array_equal(R, y["radii"])
        Ys.append(scri_amd.WaveformModes(t=y["t"], data=y["data"], ell_min=2, ell_max=4, frameType=scri_amd.Inertial, dataType=scri_amd.h,
                                         r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx))
        YR.append(y["radii"])
    orders = [-1, 2, 3]
    got = extrapolate_waveforms(Ws, Radii, orders)
    want = extrapolate_waveforms(Ys, YR, orders)
    for N, a, b in zip(orders, got, want):
        assert a.n_times == b.n_times
        dist = np.abs(a.data - b.data).max() / np.abs(b.data).max()
        print("pipeline, N =", N, ": distance to the chain on the yardstick's tables", dist)
        assert np.abs(a.t - b.t).max() <= 4 * np.spacing(np.abs(b.t).max() + 400.0)
        assert dist <= 1e-10, N
    h0 = fake_precessing_waveform(t_0=0.0, t_1=700.0, dt=0.5, ell_max=4, mass_ratio=1.0, precession_opening_angle=0.0, ctx=ctx)
    for N, a in zip(orders, got):
        inside = (a.t > h0.t[0] + 50.0) & (a.t < h0.t[-1] - 50.0)
        ref_rows = scri_amd.engine.cubic_spline(h0.t, h0.data, a.t[inside], ctx=ctx)
        print("pipeline, N =", N, ": distance to h0 on the inner axis", np.abs(a.data[inside] - ref_rows).max() / np.abs(ref_rows).max())
