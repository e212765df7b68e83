"""The four fluxes of a device-resident waveform in one launch (bms_poincare_fluxes, kernels_flux.hip) and the sparse expectation value
(bms_expectation_values), at the shapes where the kernel can go wrong: l ranges without a neighbour in l on either side (2, 2), with
one-sided clips (2, 3), (3, 5), a row of one pass (2, 8) and of more than one pass of a wave (2, 16: 285 columns); series of the
derivative's minimum length (4, 5), around one workgroup's share of a pass and around one pass of the whole grid (both read from the
launcher: bms_flux_launch_shape); a column block of a wider tensor.

Yardstick and bars: tests/helpers/flux_cases.py (the reference's sums in long double, (n_terms + 16) 2^-53 S per time step and
component), pinned without a GPU by tests/test_flux_operators.py."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests.helpers import flux_cases as fc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANGES = ((2, 2), (2, 3), (3, 5), (2, 8), (2, 16))


@pytest.fixture(scope="module")
def g32():
    return np.load(os.path.join(G, "g32_ref_flux_operators.npz"), allow_pickle=False)


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, a)


def _fused(ctx, t, h, hdot, lmin, lmax, want=fc.FLUXES):
    """engine.poincare_fluxes on device tensors, results as host arrays by name"""
    from scri_amd import engine

    out = engine.poincare_fluxes(t, h, hdot, lmin, lmax, want=want, ctx=ctx)
    return {k: o.cpu().numpy() for k, o in zip(want, out)}


def _lengths(ctx, lmin, lmax):
    """the series lengths of a range: the derivative's minimum, one workgroup's share of a pass +-1 and, for the narrow ranges (the
    yardstick of a long series of wide rows takes too long), one pass of the whole grid +-1"""
    from scri_amd import engine

    waves, groups, _ = engine.flux_launch_shape(engine.LM_total_size(lmin, lmax))
    n = {4, 5, waves - 1, waves, waves + 1}
    if lmax <= 3:
        n |= {waves * groups - 1, waves * groups, waves * groups + 1}
    return sorted(k for k in n if k >= 1)


def _waveform(ctx, t, data, lmin, lmax, data_type=None):
    import scri_amd

    return scri_amd.WaveformModes(t=t, data=data.copy(), ell_min=lmin, ell_max=lmax, dataType=scri_amd.h if data_type is None else data_type,
                                  frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)


# ---- 1. yardstick
@pytest.mark.parametrize("lmin,lmax", RANGES)
def test_fused_fluxes_within_the_bar_of_the_long_double_sums(ctx, lmin, lmax):
    worst = {}
    for n in _lengths(ctx, lmin, lmax):
        t, h, hdot = fc.chirp_pair(lmin, lmax, n, 3 * lmax + n % 13)
        got = _fused(ctx, t, _dev(ctx, h), _dev(ctx, hdot), lmin, lmax)
        for name, (value, bar) in fc.yardstick(t, h, hdot, lmin, lmax).items():
            assert got[name].shape == value.shape and got[name].dtype == np.float64
            r = fc.ratio(got[name], value, bar)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (name, n, r)
    print(f"l = {lmin}..{lmax}, N in {_lengths(ctx, lmin, lmax)}: largest |error| / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_column_block_of_a_wider_tensor(ctx):
    """ld > n_modes: h and hdot are column blocks of wider tensors with different row strides"""
    import torch

    lmin, lmax, n = 2, 8, 37
    t, h, hdot = fc.chirp_pair(lmin, lmax, n, 5)
    nm = h.shape[1]
    wide_h = torch.full((n, nm + 9), float("nan"), dtype=torch.complex128, device=_dev(ctx, h).device)
    wide_n = torch.full((n, nm + 4), float("nan"), dtype=torch.complex128, device=wide_h.device)
    wide_h[:, 5:5 + nm], wide_n[:, 1:1 + nm] = _dev(ctx, h), _dev(ctx, hdot)
    got = _fused(ctx, t, wide_h[:, 5:5 + nm], wide_n[:, 1:1 + nm], lmin, lmax)
    plain = _fused(ctx, t, _dev(ctx, h), _dev(ctx, hdot), lmin, lmax)
    for name, (value, bar) in fc.yardstick(t, h, hdot, lmin, lmax).items():
        assert fc.ratio(got[name], value, bar) <= 1.0, name
        assert np.array_equal(got[name], plain[name]), name  # (the row stride changes no bit)


# ---- 2. the reference's numbers
@pytest.mark.parametrize("lmin,lmax", RANGES[:4])
def test_fused_fluxes_equal_the_reference(ctx, g32, lmin, lmax):
    """fixture (b): the reference sums the same terms in double in another order, so twice the bar; hdot derived: handed over from
    oracle.flux_ref.data_dot (the derivative has its own tests)"""
    from oracle import flux_ref

    tag = f"{lmin}_{lmax}"
    t, (h, given), fluxes = g32[f"b_{tag}_t"], g32[f"b_{tag}_modes"], g32[f"b_{tag}_fluxes"]
    for k, hdot in enumerate((flux_ref.data_dot(t, h), given)):
        got = _fused(ctx, t, _dev(ctx, h), _dev(ctx, hdot), lmin, lmax)
        y = fc.yardstick(t, h, hdot, lmin, lmax)
        for name, cols in (("energy", 0), ("momentum", slice(1, 4)), ("angular", slice(4, 7)), ("boost", slice(7, 10))):
            r = fc.ratio(got[name], fluxes[k][:, cols].astype(fc.LD), 2 * y[name][1])
            print(f"l = {lmin}..{lmax} {'derived' if k == 0 else 'given'} {name}: {r:.3f} of twice the bar")
            assert r <= 1.0, (name, k, r)


# ---- 3. residency
def test_device_resident_waveforms_stay_resident(ctx):
    import scri_amd
    from scri_amd import flux

    lmin, lmax, n = 2, 6, 41
    t, h, hdot = fc.chirp_pair(lmin, lmax, n, 9)
    w = _waveform(ctx, t, h, lmin, lmax).to_device()
    wd = _waveform(ctx, t, hdot, lmin, lmax, scri_amd.hdot).to_device()
    results = {"poincare": flux.poincare_fluxes(w), "poincare_given": flux.poincare_fluxes(w, wd), "energy": w.energy_flux(), "momentum": w.momentum_flux(),
               "angular": w.angular_momentum_flux(), "boost": w.boost_flux(), "angular_given": flux.angular_momentum_flux(w, wd),
               "boost_given": flux.boost_flux(w, wd), "energy_of_hdot": flux.energy_flux(wd), "momentum_of_hdot": flux.momentum_flux(wd)}
    assert w.is_device_resident and wd.is_device_resident
    for r in results.values():
        for a in (r if isinstance(r, tuple) else (r,)):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape[0] == n
    # the values: the given pair against the yardstick, the derived one against the host route at the existing tests' tolerance
    y = fc.yardstick(t, h, hdot, lmin, lmax)
    for name, got in zip(fc.FLUXES, results["poincare_given"]):
        assert fc.ratio(got, *y[name]) <= 1.0, name
    host = flux.host_poincare_fluxes(_waveform(ctx, t, h, lmin, lmax))
    for got, ref, tol in zip(results["poincare"], host, (1e-12, 1e-12, 1e-12, 1e-11)):
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max()
    for short in (4, 5):  # the derivative's minimum
        ts, hs, _ = fc.chirp_pair(lmin, lmax, short, 1)
        ws = _waveform(ctx, ts, hs, lmin, lmax).to_device()
        for got, ref, tol in zip(ws.poincare_fluxes(), flux.host_poincare_fluxes(_waveform(ctx, ts, hs, lmin, lmax)), (1e-12, 1e-12, 1e-12, 1e-11)):
            assert got.shape == ref.shape and np.abs(got - ref).max() <= tol * np.abs(ref).max()
        assert ws.is_device_resident
    # a host-resident hdot beside a device-resident h is staged, and stays where it was
    wh = _waveform(ctx, t, hdot, lmin, lmax, scri_amd.hdot)
    assert np.array_equal(flux.boost_flux(w, wh), results["boost_given"]) and not wh.is_device_resident and w.is_device_resident
    with pytest.raises(ValueError, match="expected to have data of type `h`"):
        flux.angular_momentum_flux(wd)
    assert wd.is_device_resident


def test_host_resident_waveforms_keep_their_route_and_bits(ctx):
    import scri_amd
    from scri_amd import flux

    lmin, lmax, n = 2, 5, 23
    t, h, hdot = fc.chirp_pair(lmin, lmax, n, 2)
    w, wd = _waveform(ctx, t, h, lmin, lmax), _waveform(ctx, t, hdot, lmin, lmax, scri_amd.hdot)
    pairs = ((flux.energy_flux(w), flux.host_energy_flux(w)), (flux.momentum_flux(w), flux.host_momentum_flux(w)),
             (flux.angular_momentum_flux(w), flux.host_angular_momentum_flux(w)), (flux.boost_flux(w, wd), flux.host_boost_flux(w, wd)),
             (w.boost_flux(), flux.host_boost_flux(w)))
    for got, ref in pairs:
        assert np.array_equal(got, ref)
    for got, ref in zip(flux.poincare_fluxes(w, wd), flux.host_poincare_fluxes(w, wd)):
        assert np.array_equal(got, ref)
    assert not w.is_device_resident and not wd.is_device_resident
    # a device-resident waveform that starts below l = 2 goes through that route as well
    low = _waveform(ctx, t, np.concatenate([np.zeros((n, 3)), h], axis=1), 1, lmax)
    expect = flux.host_momentum_flux(low)
    assert np.array_equal(flux.momentum_flux(low.to_device()), expect)


# ---- 4. determinism
def test_same_bits_twice_in_slices_and_one_by_one(ctx):
    from scri_amd import engine

    lmin, lmax, n = 2, 8, 1000
    t, h, hdot = fc.chirp_pair(lmin, lmax, n, 4)
    dh, dn = _dev(ctx, h), _dev(ctx, hdot)
    whole, again = _fused(ctx, t, dh, dn, lmin, lmax), _fused(ctx, t, dh, dn, lmin, lmax)
    for i0, i1 in ((137, 611), (0, 7), (993, 1000)):
        part = _fused(ctx, t[i0:i1], dh[i0:i1], dn[i0:i1], lmin, lmax)
        for name in fc.FLUXES:
            assert np.array_equal(part[name], whole[name][i0:i1]), (name, i0, i1)
    for name in fc.FLUXES:
        assert np.array_equal(whole[name], again[name]), name
        single = engine.poincare_fluxes(t, dh, dn, lmin, lmax, want=name, ctx=ctx).cpu().numpy()
        assert np.array_equal(single, whole[name]), name
    # energy and momentum read hdot alone
    alone = _fused(ctx, None, None, dn, lmin, lmax, want=("energy", "momentum"))
    assert np.array_equal(alone["energy"], whole["energy"]) and np.array_equal(alone["momentum"], whole["momentum"])


# ---- 5. exact zeros and symmetry
def test_constant_single_mode_radiates_nothing(ctx):
    import scri_amd

    t = fc.axis(30)
    single = scri_amd.WaveformModes(t=t, data=np.zeros((30, 45), dtype=complex), ell_min=2, ell_max=6, dataType=scri_amd.h, frameType=scri_amd.Inertial, ctx=ctx)
    single.data[:, single.index(5, 3)] = 1.0
    single.to_device()
    e, p, j, b = single.poincare_fluxes()
    zero = np.zeros((30, 3))
    assert np.array_equal(p, zero) and np.array_equal(j, zero) and np.array_equal(b, zero) and np.array_equal(e, np.zeros(30))
    assert np.array_equal(single.boost_flux(), zero) and single.is_device_resident


def test_fluxes_of_a_device_resident_waveform_rotate_as_vectors(ctx):
    """the rotation test of tests/test_gpu_flux.py on a device-resident waveform, at its tolerance"""
    from oracle import quat
    from scri_amd import quaternions, synthetic

    n = 50
    t = np.linspace(2.0, 30.0, n) + 0.03 * np.cos(np.arange(n))
    h = _waveform(ctx, t, synthetic.chirp_modes(t, 2, 6, 4) * (1 + 0.02 * t[:, None]), 2, 6).to_device()
    R = np.array([1.0, 4.0, 3.0, 2.0]) / np.sqrt(30.0)
    Rinv = quat.qconj(R)

    def rotated(v):
        q = np.concatenate([np.zeros((v.shape[0], 1)), v], axis=1)
        return quaternions.multiply(quaternions.multiply(R, q), Rinv)[:, 1:]

    before = [h.momentum_flux(), h.angular_momentum_flux(), h.boost_flux()]
    e_before = h.energy_flux()
    g = h.copy()
    g.rotate_decomposition_basis(Rinv)
    assert g.is_device_resident and h.is_device_resident
    for a, b in zip(before, (g.momentum_flux(), g.angular_momentum_flux(), g.boost_flux())):
        assert np.allclose(rotated(a), b, rtol=1e-12, atol=1e-12 * np.abs(a).max())
    assert np.allclose(e_before, g.energy_flux(), rtol=1e-13, atol=0)


# ---- 6. bms_expectation_values
def _expectation_yardstick(a, rows, cols, values, b, conj_a):
    A = np.conj(a.astype(fc.CLD)) if conj_a else a.astype(fc.CLD)
    v = values.astype(fc.CLD)
    value = (A[:, rows] * v * b.astype(fc.CLD)[:, cols]).sum(axis=1)
    S = (np.abs(A[:, rows]) * np.abs(v) * np.abs(b[:, cols])).sum(axis=1)
    return value, (len(rows) + 16) * fc.U * S  # (the bound of a complex sum holds for its real and imaginary parts)


@pytest.mark.parametrize("memory", ["device", "host"])
def test_expectation_values_within_the_bar(ctx, memory):
    from scri_amd import engine, flux

    lmin, lmax, n = 3, 5, 19
    t, a, b = fc.chirp_pair(lmin, lmax, n, 8)
    rows, cols, values = flux.p_plus(lmin, lmax, s=-3)
    move = (lambda x: _dev(ctx, x)) if memory == "device" else (lambda x: x)
    for conj_a in (True, False):
        got = engine.expectation_values(move(a), rows, cols, values, move(b), conj_a=conj_a, ctx=ctx)
        got = got.cpu().numpy() if memory == "device" else got
        value, bar = _expectation_yardstick(a, rows, cols, values, b, conj_a)
        r = max(fc.ratio(got.real, value.real, bar), fc.ratio(got.imag, value.imag, bar))
        print(f"{memory}, conj_a = {conj_a}: {r:.3f} of the bar")
        assert got.shape == (n,) and r <= 1.0
    # the reference's helper takes <a| already conjugated, as arrays or as waveforms
    abar = np.conj(a)
    assert np.array_equal(flux.sparse_expectation_value(abar, rows, cols, values, b), engine.expectation_values(abar, rows, cols, values, b, ctx=ctx))


def test_expectation_values_reproduce_the_fused_momentum_flux(ctx):
    from scri_amd import engine, flux

    lmin, lmax, n = 2, 8, 33
    t, h, hdot = fc.chirp_pair(lmin, lmax, n, 6)
    dn = _dev(ctx, hdot)
    ev = [engine.expectation_values(dn, *gen(lmin, lmax, s=-2), dn, conj_a=True, ctx=ctx).cpu().numpy() for gen in (flux.p_plus, flux.p_minus, flux.p_z)]
    by_triplets = np.stack([0.5 * (ev[0].real + ev[1].real), 0.5 * (ev[0].imag - ev[1].imag), ev[2].real], axis=1) / (16 * np.pi)
    fused = _fused(ctx, None, None, dn, lmin, lmax, want=("momentum",))["momentum"]
    value, bar = fc.yardstick(t, None, hdot, lmin, lmax, want=("momentum",))["momentum"]
    assert fc.ratio(by_triplets, fused.astype(fc.LD), 2 * bar) <= 1.0  # (each side within one bar of the exact sum)
    assert fc.ratio(by_triplets, value, bar) <= 1.0


def _launches(ctx):
    return ctx.get_timing(reset=True)["pointwise"][1]


def test_out_of_range_triplet_is_refused_without_a_launch(ctx):
    from scri_amd import engine

    a = np.ones((4, 7), dtype=complex)
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        for rows, cols in (([0, 7, 1], [0, 1, 2]), ([0, 1, 2], [0, -1, 2])):
            with pytest.raises(ValueError, match=r"element 1 couples row -?\d+ and column -?\d+, outside \[0, 7\)"):
                engine.expectation_values(a, rows, cols, [1.0, 1.0, 1.0], a, ctx=ctx)
        assert _launches(ctx) == 0
        engine.expectation_values(a, [0, 6], [6, 0], [1.0, 1.0], a, ctx=ctx)
        assert _launches(ctx) == 1
    finally:
        ctx.enable_timing(False)


def test_matrix_expectation_value_on_device_resident_waveforms(ctx, g32):
    """fixture (c).  Equal times: the sum's own bar, twice (two double-precision sums).  Different times: both sides evaluate the same
    not-a-knot cubic spline through 9 and 11 samples in double first; its diagonally dominant solve and the cubic's evaluation leave the
    interpolated modes a few tens of roundings apart, and the sum passes that on with the condition S / |value| of the cases here (below
    10): 1e-12 of the largest value, the figure the existing flux tests use wherever a spline stands between the two sides."""
    import scri_amd
    from scri_amd import flux

    ta, tb = g32["c_ta"], g32["c_tb"]
    a = _waveform(ctx, ta, g32["c_a"], 2, 4).to_device()
    M = functools.partial(flux.p_plus, s=-2)
    cases = {"lm": (_waveform(ctx, ta, g32["c_b_on_ta"], 3, 5), dict(allow_LM_differ=True)), "times": (_waveform(ctx, tb, g32["c_b_same_ells"], 2, 4), dict(allow_times_differ=True)),
             "both": (_waveform(ctx, tb, g32["c_b"], 3, 5), dict(allow_LM_differ=True, allow_times_differ=True))}
    for name, (b, kw) in cases.items():
        b.to_device()
        times, values = flux.matrix_expectation_value(a, M, b, **kw)
        assert a.is_device_resident and b.is_device_resident
        ref_t, ref = g32[f"c_{name}_times"], g32[f"c_{name}_values"]
        assert np.array_equal(times, ref_t) and values.shape == ref.shape and values.dtype == np.complex128
        if name == "lm":
            rows, cols, vals = M(3, 4)
            _, bar = _expectation_yardstick(g32["c_a"][:, 5:], rows, cols, vals, g32["c_b_on_ta"][:, :16], True)
            assert max(fc.ratio(values.real, ref.real.astype(fc.LD), 2 * bar), fc.ratio(values.imag, ref.imag.astype(fc.LD), 2 * bar)) <= 1.0
        else:
            assert np.abs(values - ref).max() <= 1e-12 * np.abs(ref).max(), name
    # host-resident waveforms go through the same entry
    times, values = flux.matrix_expectation_value(_waveform(ctx, ta, g32["c_a"], 2, 4), M, _waveform(ctx, ta, g32["c_b_on_ta"], 3, 5), allow_LM_differ=True)
    assert np.abs(values - g32["c_lm_values"]).max() <= 1e-13 * np.abs(g32["c_lm_values"]).max()


# ---- 7. argument errors: every one comes back with its status and a message, and nothing is launched
def test_refusals_of_both_entries(ctx):
    from scri_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, nm = 6, 12  # l = 2..3
    t = np.linspace(0.0, 1.0, n)
    h, hd = np.ones((n, nm), dtype=complex), np.ones((n, nm), dtype=complex)
    e, p, j, b = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    vp, dp = _lib.vptr, _lib.dptr

    def fluxes(t=dp(t), h=vp(h), ld_h=nm, hd=vp(hd), ld_hd=nm, n_times=n, lmin=2, lmax=3, mem=_lib.BMS_HOST, e=vp(e), p=vp(p), j=vp(j), b=vp(b)):
        return lib.bms_poincare_fluxes(ctx.handle, t, h, ld_h, hd, ld_hd, n_times, lmin, lmax, mem, e, p, j, b)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        assert fluxes(hd=None) == INVALID and says("NULL hdot")
        assert fluxes(h=None) == INVALID and says("need h")
        assert fluxes(t=None) == INVALID and says("needs the times")
        assert fluxes(e=None, p=None, j=None, b=None) == INVALID and says("every output is NULL")
        assert fluxes(ld_h=nm - 1) == INVALID and says("row stride smaller than the number of modes (12)")
        assert fluxes(ld_hd=nm - 1) == INVALID and says("row stride")
        assert fluxes(lmin=1) == UNSUPPORTED and says("ell_min = 1")
        assert fluxes(lmin=0, lmax=3) == UNSUPPORTED
        assert fluxes(lmin=3, lmax=2) == INVALID and says("bad ell range [3, 2]")
        assert fluxes(n_times=-1) == INVALID and says("negative n_times")
        assert fluxes(mem=7) == INVALID and says("mem is BMS_HOST or BMS_DEVICE, got 7")
        assert lib.bms_poincare_fluxes(None, dp(t), vp(h), nm, vp(hd), nm, n, 2, 3, 0, vp(e), vp(p), vp(j), vp(b)) == INVALID
        e[:] = -1.0
        assert fluxes(n_times=0) == 0 and np.all(e == -1.0)
        # energy and momentum need neither h nor the times
        assert fluxes(t=None, h=None, j=None, b=None) == 0 and _launches(ctx) == 1 and np.all(e > 0)

        rows, cols = np.array([0, 1], dtype=np.int32), np.array([1, 0], dtype=np.int32)
        vals, out = np.ones(2, dtype=complex), np.zeros(n, dtype=complex)
        i32 = ctypes.POINTER(ctypes.c_int32)

        def expect(a=vp(h), ld_a=nm, b=vp(hd), ld_b=nm, n_times=n, n_cols=nm, rows=rows.ctypes.data_as(i32), cols=cols.ctypes.data_as(i32), vals=vp(vals),
                   n_el=2, mem=_lib.BMS_HOST, out=vp(out)):
            return lib.bms_expectation_values(ctx.handle, a, ld_a, 1, b, ld_b, n_times, n_cols, rows, cols, vals, n_el, mem, out)

        for kw in (dict(a=None), dict(b=None), dict(out=None), dict(rows=None), dict(vals=None)):
            assert expect(**kw) == INVALID and says("NULL argument"), kw
        assert expect(ld_a=nm - 1) == INVALID and says("row stride smaller than the number of columns (12)")
        assert expect(ld_b=nm - 1) == INVALID
        assert expect(n_cols=0) == INVALID and says("bad sizes")
        assert expect(n_times=-1) == INVALID and expect(n_el=-1) == INVALID
        assert expect(mem=5) == INVALID and says("got 5")
        assert expect(n_cols=1, ld_a=1, ld_b=1) == INVALID and says("outside [0, 1)")
        out[:] = -1.0
        assert expect(n_times=0) == 0 and np.all(out == -1.0)
        assert _launches(ctx) == 0
        assert expect() == 0 and np.array_equal(out, np.full(n, 2.0 + 0j)) and _launches(ctx) == 1
    finally:
        ctx.enable_timing(False)
