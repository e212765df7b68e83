"""GPU parity of the alignment kernels (bms_align_moments, bms_align_residual) and of the device route of
scri_amd.alignment.align2d built on them.

The yardstick is never the code under test: the moments and the cost are the sums of the module's docstring written out on scipy's
CubicSpline(ta, A)(t + dt, nu), and the optimum is compared with the unchanged host route of align2d run in the test."""
import ctypes

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

pytestmark = pytest.mark.gpu

T1, T2 = -50.0, 50.0
BARS = (5e-13, 5e-12, 2e-10)  # orders 0, 1, 2: the bars of the same spline evaluation in tests/test_gpu_series.py, times max(1, max|ref|)


class _Modes:
    def __init__(self, t, data, ell_min, ell_max):
        self.t, self.data, self.ell_min, self.ell_max = t, data, ell_min, ell_max

    def copy(self):
        return _Modes(self.t.copy(), self.data.copy(), self.ell_min, self.ell_max)


def _lm(ell_min, ell_max):
    return [(l, m) for l in range(ell_min, ell_max + 1) for m in range(-l, l + 1)]


def _chirp(t, ell_min, ell_max, seed=1):
    rng = np.random.default_rng(seed)
    LM = _lm(ell_min, ell_max)
    amp = rng.normal(size=len(LM)) + 1j * rng.normal(size=len(LM))
    phase = 0.07 * t + 2e-5 * t**2
    return np.stack([a * np.exp(-1j * m * phase) * (1 + 0.001 * t) for a, (l, m) in zip(amp, LM)], axis=1)


def _weights(t):
    w = np.zeros_like(t)
    w[:-1] += 0.5 * np.diff(t)
    w[1:] += 0.5 * np.diff(t)
    return w


def _axis(kind, lo, hi, n):
    if kind == "uniform":
        return np.linspace(lo, hi, n)
    steps = np.random.default_rng(5).uniform(0.5, 1.5, n - 1)  # steps x [0.5, 1.5]
    t = np.concatenate([[0.0], np.cumsum(steps)])
    return lo + (hi - lo) * t / t[-1]


class _Case:
    """One pair of series with its column tables, and the literal sums"""

    def __init__(self, ta, A, col_a, tw, B, col_b, m_of):
        self.ta, self.A, self.col_a, self.tw, self.B, self.col_b = ta, A, np.asarray(col_a), tw, B, np.asarray(col_b)
        self.m_of = np.asarray(m_of)
        self.ms = np.unique(self.m_of)
        self.m_slot = np.searchsorted(self.ms, self.m_of)
        self.w = _weights(tw)
        self.spline = CubicSpline(ta, A[:, self.col_a])
        self.Bc = B[:, self.col_b]

    def reference(self, dts, order):
        """[order + 1, len(dts), 1 + 2 n_slots] from scipy's spline and its derivatives, the sums written out"""
        x = (self.tw[None, :] + np.asarray(dts)[:, None]).ravel()
        V = [self.spline(x, nu).reshape(len(dts), self.tw.size, -1) for nu in range(order + 1)]
        N = [np.abs(V[0]) ** 2]
        if order >= 1:
            N.append(2 * (V[0].conj() * V[1]).real)
        if order >= 2:
            N.append(2 * (np.abs(V[1]) ** 2 + (V[0].conj() * V[2]).real))
        out = np.zeros((order + 1, len(dts), 1 + 2 * self.ms.size))
        for o in range(order + 1):
            out[o, :, 0] = np.einsum("i,dic->d", self.w, N[o])
            cross = np.einsum("i,dic->dc", self.w, V[o] * self.Bc.conj()[None])
            for s in range(self.ms.size):
                C = cross[:, self.m_slot == s].sum(axis=1)
                out[o, :, 1 + 2 * s], out[o, :, 2 + 2 * s] = C.real, C.imag
        return out

    def slopes(self, ctx, Y):
        from scri_amd import engine

        return engine.knot_slopes(self.ta, Y, ctx=ctx)

    def on_device(self, ctx, pad=0):
        """(Y, S, B) as device tensors; pad > 0: views of rows `pad` columns wider than the data (ld != n_cols)"""
        import torch

        from scri_amd import device_series

        Y = device_series.to_device(ctx, self.A)
        S = self.slopes(ctx, Y)
        B = device_series.to_device(ctx, self.B)
        if pad:
            wide = lambda x: torch.cat([x, torch.full((x.shape[0], pad), float("nan"), dtype=x.dtype, device=x.device)], dim=1)[:, : x.shape[1]]  # noqa: E731
            Y, S, B = wide(Y), wide(S), wide(B)
            assert Y.stride(0) == self.A.shape[1] + pad
        return Y, S, B

    def moments(self, ctx, dts, order, bulk=None):
        from scri_amd import engine

        Y, S, B = bulk if bulk is not None else self.on_device(ctx)
        return engine.align_moments(self.ta, Y, S, self.col_a, self.tw, self.w, B, self.col_b, self.m_slot, self.ms.size, dts, order, ctx=ctx)


def _window(tb):
    rows = (tb >= T1) & (tb <= T2)
    return tb[rows], rows


def _trimmed_case(kind):
    """l = 2..4 on both sides; wa trimmed so that both bounds of dt are set by ta[0] and ta[-1]: the first and the last spline
    interval are hit exactly"""
    ta = _axis(kind, -120.0, 130.0, 1400)
    tb = np.linspace(-150.0, 150.0, 1501)
    tw, rows = _window(tb)
    assert tw.size == 501
    m_of = [m for _, m in _lm(2, 4)]
    case = _Case(ta, _chirp(ta - 3.217, 2, 4), np.arange(21), tw, _chirp(tb, 2, 4)[rows], np.arange(21), m_of)
    lower, upper = max(T1 - T2, ta[0] - T1), min(T2 - T1, ta[-1] - T2)
    assert lower == ta[0] - T1 and upper == ta[-1] - T2
    return case, np.linspace(lower, upper, 203)


_cache = {}


def _trimmed(kind):
    """the case, its 203 offsets and the reference at orders 0..2, computed once"""
    if kind not in _cache:
        case, dts = _trimmed_case(kind)
        _cache[kind] = (case, dts, case.reference(dts, 2))
    return _cache[kind]


def _check(got, ref):
    assert got.shape == ref.shape
    for o in range(ref.shape[0]):
        scale = max(1.0, np.abs(ref[o]).max())
        dev = np.abs(got[o] - ref[o]).max() / scale
        print(f"order {o}: max deviation {dev:.2e} of max(1, max|ref|) = {scale:.3e} (bar {BARS[o]:.0e})")
        assert dev < BARS[o], (o, dev)


@pytest.mark.parametrize("kind", ["uniform", "jittered"])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_moments_match_the_literal_sums(ctx, kind, order):
    case, dts, ref = _trimmed(kind)
    _check(case.moments(ctx, dts, order), ref[: order + 1])


def test_moments_with_different_column_tables_and_padded_rows(ctx):
    """wa l = 2..8 (77 columns), wb l = 3..6, an include_modes subset: different column tables on the two sides, row strides that are not
    the number of columns, more columns in wa than one chunk"""
    ta = _axis("jittered", -120.0, 130.0, 1400)
    tb = np.linspace(-150.0, 150.0, 1501)
    tw, rows = _window(tb)
    subset = [lm for lm in _lm(3, 6) if lm[1] in (-3, -2, 0, 1, 2, 4, 6)]
    assert len(subset) > 16
    col = lambda ell_min: [l * (l + 1) - ell_min**2 + m for l, m in subset]  # noqa: E731
    case = _Case(ta, _chirp(ta + 1.5, 2, 8, seed=3), col(2), tw, _chirp(tb, 3, 6, seed=4)[rows], col(3), [m for _, m in subset])
    assert case.A.shape[1] == 77
    dts = np.linspace(ta[0] - T1, ta[-1] - T2, 37)
    _check(case.moments(ctx, dts, 2, bulk=case.on_device(ctx, pad=3)), case.reference(dts, 2))


def test_an_offset_has_the_same_bits_alone_and_among_others(ctx):
    case, dts, _ = _trimmed("jittered")
    bulk = case.on_device(ctx)
    full = case.moments(ctx, dts, 2, bulk=bulk)
    for k in (0, 1, 101, 202):
        alone = case.moments(ctx, dts[k : k + 1], 2, bulk=bulk)
        assert np.array_equal(alone[:, 0], full[:, k]), k


def test_host_and_device_memory_give_the_same_bits(ctx):
    from scri_amd import _lib, engine

    case, dts, _ = _trimmed("uniform")
    Y, S, B = case.on_device(ctx)
    on_device = case.moments(ctx, dts, 1, bulk=(Y, S, B))
    Yh, Sh, Bh = (np.ascontiguousarray(x.cpu().numpy()) for x in (Y, S, B))
    # host arrays through the Python interface (uploaded once) ...
    uploaded = engine.align_moments(case.ta, Yh, Sh, case.col_a, case.tw, case.w, Bh, case.col_b, case.m_slot, case.ms.size, dts, 1, ctx=ctx)
    assert np.array_equal(uploaded, on_device)
    # ... and through the C entry with mem = BMS_HOST
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    ca, cb, sl = i32(case.col_a), i32(case.col_b), i32(case.m_slot)
    p32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))  # noqa: E731
    out = np.empty_like(on_device)
    rc = _lib.load().bms_align_moments(
        ctx.handle, _lib.dptr(case.ta), case.ta.size, _lib.vptr(Yh), _lib.vptr(Sh), Yh.shape[1], p32(ca), _lib.dptr(case.tw), _lib.dptr(case.w),
        case.tw.size, _lib.vptr(Bh), Bh.shape[1], p32(cb), ca.size, p32(sl), case.ms.size, _lib.BMS_HOST, _lib.dptr(dts), dts.size, 1, _lib.dptr(out))
    ctx.check(rc, "bms_align_moments")
    assert np.array_equal(out, on_device)


def test_staged_and_unstaged_tiles_give_the_same_bits(ctx):
    """A time axis 40 x finer than the offset spacing: the knots a tile of 16 offsets reaches do not fit the LDS stage and are read through
    L2, while the same offsets scanned one at a time are staged"""
    ta = np.linspace(-110.0, 110.0, 1467)  # steps of 0.15
    tb = np.linspace(-150.0, 150.0, 1501)
    tw, rows = _window(tb)
    m_of = [m for _, m in _lm(2, 4)]
    case = _Case(ta, _chirp(ta - 1.0, 2, 4), np.arange(21), tw, _chirp(tb, 2, 4)[rows], np.arange(21), m_of)
    dts = -57.0 + 6.0 * np.arange(20)
    assert (dts[1] - dts[0]) / (ta[1] - ta[0]) > 39.9 and ta[0] <= T1 + dts[0] and T2 + dts[-1] <= ta[-1]
    assert 63 * 0.2 / 0.15 + 2 < 112 < 15 * 6.0 / 0.15  # knots of a tile: one offset | sixteen (kernels.h: ALIGN_STRETCH_KNOTS)
    bulk = case.on_device(ctx)
    together = case.moments(ctx, dts, 2, bulk=bulk)
    _check(together, case.reference(dts, 2))
    for k in range(dts.size):
        assert np.array_equal(case.moments(ctx, dts[k : k + 1], 2, bulk=bulk)[:, 0], together[:, k]), k


def test_long_offset_lists(ctx):
    """70 001 offsets cross any 16-bit launch dimension"""
    ta = np.linspace(-40.0, 40.0, 600)
    tw = -1.5 + 0.2 * np.arange(16)
    rng = np.random.default_rng(8)
    A = _chirp(ta, 2, 2, seed=6)
    B = _chirp(tw, 2, 2, seed=7) + 0.1 * rng.normal(size=(16, 5))
    case = _Case(ta, A, np.arange(5), tw, B, np.arange(5), [-2, -1, 0, 1, 2])
    dts = np.linspace(-30.0, 30.0, 70001)
    _check(case.moments(ctx, dts, 0), case.reference(dts, 0))


def test_offset_lists_longer_than_one_launch(ctx):
    """501 rows, 77 columns, 17 slots, order 2: the partial sums of one launch (128 MiB: scri_amd/csrc/engine_align.hip) hold
    19 968 offsets -- 8 row tiles x 3 orders x 35 numbers x 8 bytes each, whole tiles of 16 -- so 25 000 offsets go through as two
    launches into one result.  Offsets on both sides of the cut have the bits they have alone, and match the literal sums."""
    ta = _axis("jittered", -120.0, 130.0, 1400)
    tb = np.linspace(-150.0, 150.0, 1501)
    tw, rows = _window(tb)
    m_of = [m for _, m in _lm(2, 8)]
    case = _Case(ta, _chirp(ta - 0.5, 2, 8, seed=3), np.arange(77), tw, _chirp(tb, 2, 8, seed=3)[rows], np.arange(77), m_of)
    assert case.ms.size == 17
    per_launch = (128 << 20) // (8 * 3 * 35 * 8) // 16 * 16
    dts = np.linspace(ta[0] - T1, ta[-1] - T2, 25000)
    assert per_launch == 19968 < dts.size
    bulk = case.on_device(ctx)
    full = case.moments(ctx, dts, 2, bulk=bulk)
    ks = [0, per_launch - 17, per_launch - 1, per_launch, per_launch + 1, per_launch + 16, dts.size - 1]
    for k in ks:
        assert np.array_equal(case.moments(ctx, dts[k : k + 1], 2, bulk=bulk)[:, 0], full[:, k]), k
    _check(full[:, ks], case.reference(dts[ks], 2))


def test_residual_entry_matches_the_direct_sum(ctx):
    from scri_amd import engine

    case, _, _ = _trimmed("jittered")
    Y, S, B = case.on_device(ctx)
    for dt, dphi in [(0.0, 0.0), (3.217, 1.234), (-69.3, 5.0), (case.ta[-1] - T2, 0.3)]:
        res, nb = engine.align_residual(case.ta, Y, S, case.col_a, case.tw, case.w, B, case.col_b, case.m_of, dt, dphi, ctx=ctx)
        Aw = case.spline(case.tw + dt) * np.exp(1j * case.m_of * dphi)
        bar = 5e-13 * (case.w @ np.sum((np.abs(Aw) + np.abs(case.Bc)) ** 2, axis=1))
        assert res >= 0.0
        assert abs(res - case.w @ np.sum(np.abs(Aw - case.Bc) ** 2, axis=1)) < bar
        assert abs(nb - case.w @ np.sum(np.abs(case.Bc) ** 2, axis=1)) < bar


# ------------------------------------------------------------------------------------------------ align2d(ctx=ctx)


def _pair(dt, dphi, ell_min_a=2, ell_max_a=4):
    """wb = the chirp on its own times; wa = the waveform that the offset (dt, dphi) carries onto wb (tests/test_alignment.py)"""
    tb = np.linspace(-150.0, 150.0, 1501)
    ta = np.linspace(-160.0, 170.0, 1400)
    wb = _Modes(tb, _chirp(tb, 2, 4), 2, 4)
    m = np.array([m for _, m in _lm(2, 4)])
    full = _chirp(ta - dt, 2, 4) * np.exp(-1j * m * dphi)
    keep = [i for i, (l, _) in enumerate(_lm(2, 4)) if ell_min_a <= l <= ell_max_a]
    return _Modes(ta, full[:, keep], ell_min_a, ell_max_a), wb


def _direct_cost(wa, wb, include_modes, x):
    ell_min, ell_max = max(wa.ell_min, wb.ell_min), min(wa.ell_max, wb.ell_max)
    LM = [lm for lm in _lm(ell_min, ell_max) if include_modes is None or lm in {tuple(y) for y in include_modes}]
    col = lambda w: [l * (l + 1) - w.ell_min**2 + m for l, m in LM]  # noqa: E731
    m_of = np.array([m for _, m in LM], dtype=float)
    t, rows = _window(wb.t)
    w = _weights(t)
    B = wb.data[rows][:, col(wb)]
    A = CubicSpline(wa.t, wa.data[:, col(wa)])(t + x[0]) * np.exp(1j * m_of * x[1])
    return 0.5 * (w @ np.sum(np.abs(A - B) ** 2, axis=1)) / (w @ np.sum(np.abs(B) ** 2, axis=1))


def _both_routes(ctx, wa, wb, n, include_modes=None):
    from scri_amd.alignment import align2d

    err, wa_prime, res = align2d(wa, wb, T1, T2, n_brute_force_δt=n, include_modes=include_modes, ctx=ctx)
    host = align2d(wa, wb, T1, T2, n_brute_force_δt=n, include_modes=include_modes)[2]
    cost_new, cost_host = _direct_cost(wa, wb, include_modes, res.x), _direct_cost(wa, wb, include_modes, host.x)
    print(f"x = {res.x} (host route {host.x}), cost {cost_new:.3e} (host route {cost_host:.3e}), reported {res.cost:.3e}, nfev {res.nfev}")
    assert err == res.cost and res.success and not hasattr(res, "fun") and not hasattr(res, "jac")
    assert cost_new <= cost_host * (1 + 1e-9) + 1e-13
    assert abs(res.cost - cost_new) <= 1e-9 * cost_new + 1e-15
    return err, wa_prime, res


@pytest.mark.parametrize("dt,dphi", [(3.217, 1.234), (-7.5, 5.9), (0.0, 0.0)])
def test_align2d_recovers_offset(ctx, dt, dphi):
    wa, wb = _pair(dt, dphi)
    err, wa_prime, res = _both_routes(ctx, wa, wb, 200)
    assert abs(res.x[0] - dt) < 1e-5
    assert abs((res.x[1] - dphi + np.pi) % (2 * np.pi) - np.pi) < 1e-6
    assert err < 1e-12 and err == res.cost
    t = np.linspace(-50, 50, 77)
    assert np.abs(CubicSpline(wa_prime.t, wa_prime.data)(t) - CubicSpline(wb.t, wb.data)(t)).max() < 1e-5


def test_align2d_include_modes_and_different_ell_ranges(ctx):
    from scri_amd.alignment import align2d

    wa, wb = _pair(2.5, 0.7, ell_min_a=2, ell_max_a=3)
    err, _, res = _both_routes(ctx, wa, wb, 100)
    assert abs(res.x[0] - 2.5) < 1e-5 and abs(res.x[1] - 0.7) < 1e-6
    err, _, res = _both_routes(ctx, wa, wb, 100, include_modes=[(2, 2), (2, -2), (3, 2)])
    assert abs(res.x[0] - 2.5) < 1e-5
    assert abs((res.x[1] - 0.7 + np.pi / 2) % np.pi - np.pi / 2) < 1e-6
    with pytest.raises(ValueError, match="no common modes"):
        align2d(wa, wb, -50.0, 50.0, include_modes=[(7, 0)], ctx=ctx)


def test_align2d_cost_is_half_the_normalised_squared_distance(ctx):
    wa, wb = _pair(1.0, 0.3)
    wb.data = wb.data.copy()
    wb.data[:, 2] += 0.5  # the (2, 0) mode
    err, wa_prime, res = _both_routes(ctx, wa, wb, 100)
    t, rows = _window(wb.t)
    diff = CubicSpline(wa_prime.t, wa_prime.data)(t) - wb.data[rows]
    trap = lambda y: 0.5 * np.sum((y[1:] + y[:-1]) * np.diff(t))  # noqa: E731
    expected = 0.5 * trap(np.sum(np.abs(diff) ** 2, axis=1)) / trap(np.sum(np.abs(wb.data[rows]) ** 2, axis=1))
    assert abs(err - expected) < 1e-9 * expected
    assert err > 1e-4


def test_align2d_keeps_resident_waveforms_resident(ctx):
    import scri_amd
    from scri_amd.alignment import align2d

    a, b = _pair(3.217, 1.234)
    make = lambda w: scri_amd.WaveformModes(t=w.t, data=w.data, ell_min=2, ell_max=4, dataType=scri_amd.h, frameType=scri_amd.Inertial,  # noqa: E731
                                            r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    wa, wb = make(a), make(b)
    _, _, on_host = align2d(wa, wb, T1, T2, n_brute_force_δt=200, ctx=ctx)
    assert not wa.is_device_resident and not wb.is_device_resident
    wa.to_device(), wb.to_device()
    err, wa_prime, res = align2d(wa, wb, T1, T2, n_brute_force_δt=200)  # (no ctx=: the residency selects the route)
    assert wa.is_device_resident and wb.is_device_resident and wa_prime.is_device_resident
    assert np.array_equal(res.x, on_host.x) and res.cost == on_host.cost == err
    m = np.array([m for _, m in _lm(2, 4)], dtype=float)
    assert np.abs(wa_prime.t - (a.t - res.x[0])).max() <= 4e-15 * np.abs(a.t).max()
    expected = a.data * np.exp(1j * m * res.x[1])[None, :]
    assert np.abs(wa_prime.data - expected).max() <= 4e-15 * np.abs(expected).max()
    assert wa.is_device_resident and wb.is_device_resident  # (reading wa_prime.data moved wa_prime alone)
    # a resident wa whose rows are wider than its columns (a padded view) is aligned too, to the same bits
    import torch

    padded = make(a).to_device()
    padded._dev = torch.cat([padded._dev, torch.zeros((a.t.size, 3), dtype=padded._dev.dtype, device=padded._dev.device)], dim=1)[:, :21]
    assert padded._dev.stride(0) == 24
    assert np.array_equal(align2d(padded, wb, T1, T2, n_brute_force_δt=200)[2].x, res.x) and padded.is_device_resident
    other = scri_amd.Context(ctx.device)
    try:
        with pytest.raises(ValueError, match="two different contexts"):
            align2d(wa, wb, T1, T2, ctx=other)
    finally:
        other.close()


def test_align2d_errors_and_degenerate_window(ctx, monkeypatch):
    from scri_amd import engine
    from scri_amd.alignment import align2d

    wa, wb = _pair(0.0, 0.0)
    scans = []
    real = engine.align_moments

    def spy(*args, **kwargs):
        scans.append((np.array(args[10]), args[11]))
        return real(*args, **kwargs)

    monkeypatch.setattr(engine, "align_moments", spy)
    with pytest.raises(ValueError, match="out of order"):
        align2d(wa, wb, 10.0, -10.0, ctx=ctx)
    with pytest.raises(ValueError, match="not contained in wb"):
        align2d(wa, wb, -200.0, 0.0, ctx=ctx)
    short = _Modes(wa.t[300:], wa.data[300:], wa.ell_min, wa.ell_max)
    with pytest.raises(ValueError, match="not contained in wa"):
        align2d(short, wb, -150.0, 150.0, ctx=ctx)
    with pytest.raises(ValueError, match="no common modes"):
        align2d(wa, wb, T1, T2, include_modes=[(7, 0)], ctx=ctx)
    assert not scans  # every refusal came before any GPU work
    # wa exactly as long as the window: no offset is possible, the scan is the single offset 0 and only the turn is refined
    ta = np.linspace(T1, T2, 700)
    m = np.array([m for _, m in _lm(2, 4)])
    exact = _Modes(ta, _chirp(ta, 2, 4) * np.exp(-1j * m * 0.7), 2, 4)
    err, _, res = align2d(exact, wb, T1, T2, ctx=ctx)
    assert scans[0][1] == 0 and np.array_equal(scans[0][0], [0.0])
    assert all(order == 2 and np.array_equal(d, [0.0]) for d, order in scans[1:])
    assert res.x[0] == 0.0 and abs(res.x[1] - 0.7) < 1e-6 and err < 1e-12
