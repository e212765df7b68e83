"""Brackets of two waveforms in one pass over the modes (bms_pair_brackets, kernels_flux.hip) and the three operations of
device-resident waveforms built on it (inner_product, LVector, LLComparisonMatrix), at the shapes where the kernel can go wrong: one
column with every ladder term clipped (0, 0), ranges where m +- 2 exists only at the ends of a block (0, 1), (2, 2), one-sided clips
(2, 3), (3, 5), a row just past one pass of a wave (2, 8: 77 columns) and of several (2, 16: 285 columns); series of 1 and 2 steps, around
one workgroup's share of a pass and around one pass of the whole grid (both read from the launcher: bms_pair_launch_shape).

Yardstick and bars: tests/helpers/pair_cases.py (the reference's sums in long double, (n_terms + 16) 2^-53 S per time step and bracket),
pinned without a GPU by tests/test_pair_brackets_host.py."""
import os

import numpy as np
import pytest

from tests.helpers import pair_cases as pc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANGES = ((0, 0), (0, 1), (2, 2), (2, 3), (3, 5), (2, 8), (2, 16))
WANT = ("inner", "L", "LL")


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, np.ascontiguousarray(a))


def _brackets(ctx, a, b, lmin, lmax, want=WANT, **kw):
    """engine.pair_brackets, results as host arrays by name"""
    from scri_amd import engine

    out = engine.pair_brackets(a, b, lmin, lmax, want=want, ctx=ctx, **kw)
    return {k: (o.cpu().numpy() if hasattr(o, "cpu") else o) for k, o in zip(want, out)}


def _lengths(lmin, lmax):
    from scri_amd import engine

    waves, groups = engine.pair_launch_shape(engine.LM_total_size(lmin, lmax))
    n = {1, 2, waves - 1, waves, waves + 1}
    if lmax <= 3:
        n |= {waves * groups - 1, waves * groups, waves * groups + 1}
    return sorted(k for k in n if k >= 1)


def _waveform(ctx, t, data, lmin, lmax, data_type=None):
    import scri_amd

    return scri_amd.WaveformModes(t=t, data=np.array(data), ell_min=lmin, ell_max=lmax, dataType=scri_amd.h if data_type is None else data_type,
                                  frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)


def _assert_within_the_bar(got, f, g, lmin, lmax, where=""):
    y = pc.yardstick(f, g, lmin, lmax)
    worst = {}
    for which in got:
        value, bar = pc.group(y, which)
        assert got[which].shape == value.shape and got[which].dtype == np.complex128, (which, where)
        worst[which] = pc.ratio(got[which], value, bar)
        assert worst[which] <= 1.0, (which, where, worst[which])
    return worst


# ---- 1. yardstick
@pytest.mark.parametrize("lmin,lmax", RANGES)
def test_brackets_within_the_bar_of_the_long_double_sums(ctx, lmin, lmax):
    worst = {}
    for n in _lengths(lmin, lmax):
        f, g = pc.pair(lmin, lmax, n, n % 11)
        got = _brackets(ctx, _dev(ctx, f), _dev(ctx, g), lmin, lmax)
        for k, r in _assert_within_the_bar(got, f, g, lmin, lmax, n).items():
            worst[k] = max(worst.get(k, 0.0), r)
    print(f"l = {lmin}..{lmax}, N in {_lengths(lmin, lmax)}: largest |error| / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- 2. the reference's numbers, on device-resident waveforms
@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(G, "g13_ref_mode_calculations.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def g11():
    return np.load(os.path.join(G, "g11_ref_mode_operators.npz"), allow_pickle=False)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_resident_vector_and_matrix_equal_the_reference(ctx, g13, tag):
    import scri_amd
    from scri_amd import mode_calculations as mcalc

    t = g13[f"{tag}_t"]
    lmin, lmax = (int(x) for x in g13[f"{tag}_ells"])
    dt = scri_amd.h if tag == "a" else scri_amd.psi2
    w = _waveform(ctx, t, g13[f"{tag}_data"], lmin, lmax, dt).to_device()
    other = _waveform(ctx, t, g13[f"{tag}_other"], lmin, lmax, dt).to_device()
    lv, llc = g13[f"{tag}_LVector"], g13[f"{tag}_LLComparisonMatrix"]
    got_v, got_m = mcalc.LVector(w, other), mcalc.LLComparisonMatrix(w, other)
    assert w.is_device_resident and other.is_device_resident
    assert isinstance(got_v, np.ndarray) and got_v.shape == lv.shape and got_v.dtype == np.complex128
    assert isinstance(got_m, np.ndarray) and got_m.shape == llc.shape and got_m.dtype == np.complex128
    assert np.abs(got_v - lv).max() < 1e-13 * np.abs(lv).max()
    assert np.abs(got_m - llc).max() < 1e-13 * np.abs(llc).max()
    assert np.all(got_m[:, 1, 2] == 0)
    # the grafted forms are the same calls
    assert np.array_equal(w.LVector(other), got_v) and np.array_equal(w.LLComparisonMatrix(other), got_m) and np.array_equal(scri_amd.LVector(w, other), got_v)
    assert w.is_device_resident and other.is_device_resident


def test_resident_inner_product_equals_the_reference(ctx, g11):
    from oracle import waveform_modes_ref as ref
    from oracle.containers import WM
    from tests.test_golden import G11_TYPES

    t = g11["t"]
    for name, dt in G11_TYPES.items():
        lmin, lmax = (int(x) for x in g11[f"{name}_ells"])
        a = _waveform(ctx, t, g11[f"{name}_in"], lmin, lmax, dt).to_device()
        b = _waveform(ctx, t, g11[f"{name}_other"], lmin, lmax, dt).to_device()
        got = np.array([a.inner_product(b), a.inner_product(b, t1=2.0, t2=7.0)])
        assert a.is_device_resident and b.is_device_resident
        fixture = g11[f"{name}_inner"]
        oa, ob = (WM(t=t, data=g11[f"{name}_{k}"], ell_min=lmin, ell_max=lmax, dataType=dt) for k in ("in", "other"))
        oracle = np.array([ref.inner_product(oa, ob), ref.inner_product(oa, ob, t1=2.0, t2=7.0)])
        for k in range(2):
            assert abs(got[k] - fixture[k]) < 1e-12 * abs(fixture[k]), (name, k)
            assert abs(got[k] - oracle[k]) < 1e-12 * abs(oracle[k]), (name, k)


# ---- 3. residency
def _pair_of_waveforms(ctx, n=40, lmin=2, lmax=6, seed=3):
    t = np.linspace(0.0, 10.0, n) + 0.01 * np.cos(np.arange(n))
    f, g = pc.pair(lmin, lmax, n, seed)
    smooth = np.exp(-0.03 * t)[:, None]  # (a spline stands between the two sides of the inner product: smooth in time)
    f, g = f[:1] * smooth * np.exp(0.2j * t)[:, None], g[:1] * smooth * np.exp(0.17j * t)[:, None]
    return t, f, g


def test_resident_waveforms_stay_resident(ctx):
    from scri_amd import mode_calculations as mcalc

    t, f, g = _pair_of_waveforms(ctx)
    a, b = _waveform(ctx, t, f, 2, 6).to_device(), _waveform(ctx, t, g, 2, 6).to_device()
    host_a, host_b = _waveform(ctx, t, f, 2, 6), _waveform(ctx, t, g, 2, 6)
    for call in (lambda x, y: x.inner_product(y), lambda x, y: x.inner_product(y, t1=2.0, t2=7.0), mcalc.LVector, mcalc.LLComparisonMatrix):
        got = call(a, b)
        assert a.is_device_resident and b.is_device_resident
        expect = call(host_a, host_b)  # the route of two host-resident waveforms
        assert not host_a.is_device_resident and not host_b.is_device_resident
        assert np.abs(np.asarray(got) - np.asarray(expect)).max() <= 1e-12 * np.abs(np.asarray(expect)).max()
        # one host, one resident: neither changes residence, and the numbers are those of the resident pair
        for x, y in ((a, host_b), (host_a, b)):
            mixed = call(x, y)
            assert a.is_device_resident and b.is_device_resident and not host_a.is_device_resident and not host_b.is_device_resident
            assert np.array_equal(np.asarray(mixed), np.asarray(got))


def test_residency_with_differing_modes_and_times(ctx):
    from oracle import waveform_modes_ref as ref
    from oracle.containers import WM, h
    from scri_amd.mode_operators import time_intersection

    t, f, g = _pair_of_waveforms(ctx)
    a = _waveform(ctx, t, f, 2, 6).to_device()
    low = _waveform(ctx, t, g[:, :25], 0, 4).to_device()  # l = 0..4 against l = 2..6: the common range 2..4 read in place
    with pytest.raises(ValueError, match="ell_min and ell_max must match in inner_product"):
        a.inner_product(low)
    got = a.inner_product(low, allow_LM_differ=True)
    assert a.is_device_resident and low.is_device_resident
    expect = ref.inner_product(WM(t=t, data=f[:, :21], ell_min=2, ell_max=4, dataType=h), WM(t=t, data=g[:, 4:25], ell_min=2, ell_max=4, dataType=h))
    assert abs(got - expect) < 1e-12 * abs(expect)
    assert abs(got - _waveform(ctx, t, f, 2, 6).inner_product(_waveform(ctx, t, g[:, :25], 0, 4), allow_LM_differ=True)) < 1e-12 * abs(expect)
    with pytest.raises(ValueError, match="Intersection of \\(ell,m\\) modes is empty"):
        a.inner_product(_waveform(ctx, t, g[:, :4], 0, 1).to_device(), allow_LM_differ=True)

    t2 = t * 0.9 + 0.3
    shifted = _waveform(ctx, t2, g, 2, 6).to_device()
    with pytest.raises(ValueError, match="Time samples must match in inner_product"):
        a.inner_product(shifted)
    got = a.inner_product(shifted, allow_times_differ=True)
    assert a.is_device_resident and shifted.is_device_resident
    expect = _waveform(ctx, t, f, 2, 6).inner_product(_waveform(ctx, t2, g, 2, 6), allow_times_differ=True)
    assert abs(got - expect) < 1e-11 * abs(expect)  # (the bar tests/test_gpu_mode_operators.py holds the interpolated product to)
    both = a.inner_product(_waveform(ctx, t2, g[:, :25], 0, 4).to_device(), allow_LM_differ=True, allow_times_differ=True)
    tc = time_intersection(t, t2)
    assert a.is_device_resident and np.isfinite(both) and tc.size > 4
    with pytest.raises(ValueError, match="Spin weights must match in inner_product"):
        import scri_amd

        a.inner_product(_waveform(ctx, t, g, 2, 6, scri_amd.psi2).to_device())


def test_two_contexts_are_refused(ctx):
    from scri_amd import _lib, mode_calculations as mcalc

    t, f, g = _pair_of_waveforms(ctx, n=8)
    second = _lib.Context(ctx.device)
    try:
        a, b = _waveform(ctx, t, f, 2, 6).to_device(), _waveform(second, t, g, 2, 6).to_device()
        for call in (mcalc.LVector, mcalc.LLComparisonMatrix, lambda x, y: x.inner_product(y)):
            with pytest.raises(ValueError, match="different contexts"):
                call(a, b)
        assert a.is_device_resident and b.is_device_resident
    finally:
        second.close()


def test_host_resident_waveforms_keep_their_route_and_bits(ctx):
    """the statements of the route before the kernel, written out: bms_mode_map per ladder operator and a host contraction"""
    from scri_amd import engine, mode_calculations as mcalc

    t, f, g = _pair_of_waveforms(ctx, n=12)
    a, b = _waveform(ctx, t, f, 2, 6), _waveform(ctx, t, g, 2, 6)
    braket = lambda x, y: np.einsum("ij, ij -> i", np.conjugate(x.data), y.data)  # noqa: E731
    Lp, Lm, Lz = (braket(a, mcalc._ladder_applied(b, w)) for w in "+-z")
    assert np.array_equal(mcalc.LVector(a, b), np.stack([0.5 * (Lp + Lm), -0.5j * (Lp - Lm), Lz], axis=1))
    T = {x + y: braket(a, mcalc._ladder_applied(mcalc._ladder_applied(b, y), x)) for y in "+-z" for x in "+-z"}
    LL = mcalc.LLComparisonMatrix(a, b)
    assert np.array_equal(LL[:, 0, 0], (T["++"] + T["+-"] + T["-+"] + T["--"]) / 4)
    assert np.array_equal(LL[:, 1, 1], -(T["++"] - T["+-"] - T["-+"] + T["--"]) / 4 - 1j * (T["+z"] - T["-z"]) / 2)
    assert np.array_equal(LL[:, 2, 1], -1j * (T["z+"] - T["z-"]) / 2) and np.array_equal(LL[:, 2, 2], T["zz"]) and np.all(LL[:, 1, 2] == 0)
    integrand = np.sum(np.conjugate(a.data) * b.data, axis=1)
    ends = engine.spline_derivative(t, integrand[:, np.newaxis], np.array([t[0], t[-1]]), order=-1, ctx=ctx)
    assert a.inner_product(b) == complex(ends[1, 0] - ends[0, 0])
    assert not a.is_device_resident and not b.is_device_resident


# ---- 4. bits
def test_same_bits_in_slices_memories_and_one_by_one(ctx):
    from scri_amd import engine

    lmin, lmax, n = 2, 8, 1000
    f, g = pc.pair(lmin, lmax, n, 4)
    df, dg = _dev(ctx, f), _dev(ctx, g)
    whole = _brackets(ctx, df, dg, lmin, lmax)
    host = _brackets(ctx, f, g, lmin, lmax)
    for i0, i1 in ((137, 611), (0, 7), (993, 1000)):
        part = _brackets(ctx, df[i0:i1], dg[i0:i1], lmin, lmax)
        for name in WANT:
            assert np.array_equal(part[name], whole[name][i0:i1]), (name, i0, i1)
    for name in WANT:
        assert np.array_equal(host[name], whole[name]), name
        single = engine.pair_brackets(df, dg, lmin, lmax, want=name, ctx=ctx).cpu().numpy()
        assert np.array_equal(single, whole[name]), name
        others = tuple(k for k in WANT if k != name)
        for k, v in _brackets(ctx, df, dg, lmin, lmax, want=others).items():
            assert np.array_equal(v, whole[k]), (k, others)


def test_column_blocks_of_wider_tensors(ctx):
    """ld > n_modes: a and b are column blocks of wider NaN-filled tensors with different row strides and column offsets"""
    import torch

    lmin, lmax, n = 2, 8, 37
    f, g = pc.pair(lmin, lmax, n, 5)
    nm = f.shape[1]
    wide_f = torch.full((n, nm + 9), float("nan"), dtype=torch.complex128, device=_dev(ctx, f).device)
    wide_g = torch.full((n, nm + 4), float("nan"), dtype=torch.complex128, device=wide_f.device)
    wide_f[:, 5:5 + nm], wide_g[:, 1:1 + nm] = _dev(ctx, f), _dev(ctx, g)
    got = _brackets(ctx, wide_f[:, 5:5 + nm], wide_g[:, 1:1 + nm], lmin, lmax)
    plain = _brackets(ctx, _dev(ctx, f), _dev(ctx, g), lmin, lmax)
    _assert_within_the_bar(got, f, g, lmin, lmax)
    for name in WANT:
        assert np.array_equal(got[name], plain[name]), name


@pytest.mark.parametrize("memory", ["device", "host"])
def test_common_range_read_in_place(ctx, memory):
    """a holds l = 2..6, b holds l = 0..4: the common range 2..4 read where it lies equals the call on sliced contiguous copies"""
    n = 29
    f, _ = pc.pair(2, 6, n, 6)
    _, g = pc.pair(0, 4, n, 7)
    move = (lambda x: _dev(ctx, x)) if memory == "device" else np.ascontiguousarray
    in_place = _brackets(ctx, move(f), move(g), 2, 4, ell_min_a=2, ell_min_b=0)
    fs, gs = f[:, :21], g[:, 4:25]
    sliced = _brackets(ctx, move(fs), move(gs), 2, 4)
    _assert_within_the_bar(in_place, fs, gs, 2, 4)
    for name in WANT:
        assert np.array_equal(in_place[name], sliced[name]), name
    with pytest.raises(ValueError, match="b has 24 columns"):
        _brackets(ctx, move(f), move(g[:, :24]), 2, 4, ell_min_a=2, ell_min_b=0)


def test_one_tensor_on_both_sides(ctx):
    lmin, lmax, n = 2, 5, 19
    f, _ = pc.pair(lmin, lmax, n, 8)
    df = _dev(ctx, f)
    got = _brackets(ctx, df, df, lmin, lmax)
    _assert_within_the_bar(got, f, f, lmin, lmax)
    assert np.array_equal(got["inner"], _brackets(ctx, df, df.clone(), lmin, lmax)["inner"])
    assert np.all(got["inner"].real > 0) and np.abs(got["inner"].imag).max() <= 1e-15 * got["inner"].real.max()


# ---- 5. edges
def test_nan_poisons_one_step_and_zeros_stay_zeros(ctx):
    lmin, lmax, n = 2, 8, 50
    f, g = pc.pair(lmin, lmax, n, 9)
    clean = _brackets(ctx, _dev(ctx, f), _dev(ctx, g), lmin, lmax)
    bad = g.copy()
    bad[23, 40] = np.nan
    got = _brackets(ctx, _dev(ctx, f), _dev(ctx, bad), lmin, lmax)
    keep = np.arange(n) != 23
    for name in WANT:
        assert np.array_equal(got[name][keep], clean[name][keep]), name
    assert np.isnan(got["inner"][23]) and np.isnan(got["L"][23, 2]) and np.isnan(got["LL"][23, 8])
    zero = _brackets(ctx, _dev(ctx, np.zeros_like(f)), _dev(ctx, g), lmin, lmax)
    for name in WANT:
        assert np.array_equal(zero[name], np.zeros_like(clean[name])), name


def _launches(ctx):
    return ctx.get_timing(reset=True)["pointwise"][1]


def test_guard_values_around_the_outputs_stay_intact(ctx):
    import ctypes
    import torch

    from scri_amd import _lib

    lmin, lmax, n = 2, 8, 67
    f, g = pc.pair(lmin, lmax, n, 10)
    df, dg = _dev(ctx, f), _dev(ctx, g)
    guard = complex(-7.0, 3.0)
    pad = 4
    bufs = {k: torch.full((pad + n * w + pad,), guard, dtype=torch.complex128, device=df.device) for k, w in (("inner", 1), ("L", 3), ("LL", 9))}
    ptr = lambda k: ctypes.c_void_p(bufs[k].data_ptr() + 16 * pad)  # noqa: E731
    torch.cuda.synchronize()
    rc = _lib.load().bms_pair_brackets(ctx.handle, ctypes.c_void_p(df.data_ptr()), f.shape[1], lmin, ctypes.c_void_p(dg.data_ptr()), g.shape[1], lmin, n, lmin,
                                       lmax, _lib.BMS_DEVICE, ptr("inner"), ptr("L"), ptr("LL"))
    assert rc == 0
    ctx.synchronize()
    plain = _brackets(ctx, df, dg, lmin, lmax)
    for k, w in (("inner", 1), ("L", 3), ("LL", 9)):
        host = bufs[k].cpu().numpy()
        assert np.all(host[:pad] == guard) and np.all(host[pad + n * w:] == guard), k
        assert np.array_equal(host[pad:pad + n * w], plain[k].reshape(-1)), k


def test_refusals_launch_nothing(ctx):
    from scri_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, nm = 6, 12  # l = 2..3
    a, b = np.ones((n, nm), dtype=complex), np.ones((n, nm), dtype=complex)
    inner, L, LL = np.full(n, -1.0 + 0j), np.full((n, 3), -1.0 + 0j), np.full((n, 9), -1.0 + 0j)
    vp = _lib.vptr

    def call(a=vp(a), ld_a=nm, lmin_a=2, b=vp(b), ld_b=nm, lmin_b=2, n_times=n, lmin=2, lmax=3, mem=_lib.BMS_HOST, inner=vp(inner), L=vp(L), LL=vp(LL)):
        return lib.bms_pair_brackets(ctx.handle, a, ld_a, lmin_a, b, ld_b, lmin_b, n_times, lmin, lmax, mem, inner, L, LL)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        assert call(a=None) == INVALID and says("NULL waveform")
        assert call(b=None) == INVALID and says("NULL waveform")
        assert call(inner=None, L=None, LL=None) == INVALID and says("every output is NULL")
        assert call(lmin=3, lmax=2) == INVALID and says("bad ell range [3, 2]")
        assert call(lmin_a=3) == INVALID and says("below a row's first ell")
        assert call(lmin_b=3) == INVALID and says("below a row's first ell")
        assert call(lmin_a=-1) == INVALID
        assert call(ld_a=nm - 1) == INVALID and says("row stride")
        assert call(ld_b=nm - 1) == INVALID and says("row stride")
        assert call(lmin_b=1, ld_b=nm + 2) == INVALID and says("row stride")  # (three more columns lie before l = 2)
        assert call(n_times=-1) == INVALID and says("negative n_times")
        assert call(mem=7) == INVALID and says("mem is BMS_HOST or BMS_DEVICE, got 7")
        assert lib.bms_pair_brackets(None, vp(a), nm, 2, vp(b), nm, 2, n, 2, 3, 0, vp(inner), vp(L), vp(LL)) == INVALID
        import ctypes

        odd = ctypes.c_void_p(a.ctypes.data + 8)  # (refused by its value before anything reads it)
        assert call(a=odd, mem=_lib.BMS_DEVICE) == INVALID and says("aligned")
        assert call(n_times=0) == 0
        # an l range whose row does not fit in LDS
        wide = np.ones((1, 102 * 102), dtype=complex)
        assert call(a=vp(wide), ld_a=wide.shape[1], lmin_a=0, b=vp(wide), ld_b=wide.shape[1], lmin_b=0, n_times=1, lmin=0, lmax=101) == UNSUPPORTED
        assert says("does not fit in LDS")
        assert _launches(ctx) == 0
        assert np.all(inner == -1.0) and np.all(L == -1.0) and np.all(LL == -1.0)
        assert call(L=None, LL=None) == 0 and _launches(ctx) == 1 and np.array_equal(inner, np.full(n, 12.0 + 0j)) and np.all(L == -1.0)
        assert call() == 0 and np.array_equal(LL[:, 8], np.full(n, 2.0 * (4 + 1) + 2.0 * (9 + 4 + 1) + 0j))  # sum of m^2 over l = 2, 3
    finally:
        ctx.enable_timing(False)
    from scri_amd import engine

    with pytest.raises(ValueError, match="want names"):
        engine.pair_brackets(a, b, 2, 3, want=("inner", "M"), ctx=ctx)
    empty = engine.pair_brackets(np.zeros((0, nm), dtype=complex), np.zeros((0, nm), dtype=complex), 2, 3, ctx=ctx)
    assert [x.shape for x in empty] == [(0,), (0, 3), (0, 9)]
