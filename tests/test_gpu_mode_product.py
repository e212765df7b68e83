"""Products of two mode rows on Gauss-Legendre rows (bms_mode_product, bms_supermomenta: product_kernel in kernels_product.hip) at the shapes
where the kernel can go wrong: odd and even degree sums, l_out = 0 and l_out = l_a + l_b, unequal operands, every sign of the spins, the bar
of either operand, one array as both operands, garbage below l = |s|, l = 16 and 24; series around one pass of a workgroup and of the whole
grid (read from the launcher: bms_product_launch_shape), the largest size that fits in LDS and the first that does not; slices, repeats,
host arrays, row strides and single outputs bit for bit; the methods of a device-resident AsymptoticBondiData against the host-resident
object, the oracle and the reference's recorded supermomenta (g25); the refusals.

Yardstick and bars: tests/helpers/product_cases.py (the three sums in long double, (K + 16) 2^-53 S per entry), pinned without a GPU by
tests/test_mode_product_host.py.  Where a comparison is with the oracle's double-precision grid route, four times that route's recorded
distance from the yardstick is added (product_cases.ORACLE_DISTANCE).  Observed on the MI355X: the device lies within 0.10 of the bar on
the products (0.001 at l = 16, 24 and 28) and 0.08 on the supermomenta; every test prints its own share."""
import os

import numpy as np
import pytest

from tests.helpers import product_cases as pc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRID_TAGS = ("gemm_synthesis", "gemm_analysis", "theta_quadrature", "analysis_fused", "analysis_large")


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, a)


def _product(ctx, a, sa, la, b, sb, lb, lout, **kw):
    """engine.mode_product on device tensors, the result as a host array"""
    from scri_amd import engine

    da = _dev(ctx, a)
    db = da if b is a else _dev(ctx, b)
    return engine.mode_product(da, sa, la, db, sb, lb, lout, ctx=ctx, **kw).cpu().numpy()


def _within(got, value, bar, what, extra=0.0):
    r = pc.ratio(got, value, bar * (1 + extra))
    assert r <= 1.0, (what, r)
    return r


# ---- 1. values
@pytest.mark.parametrize("case", pc.ELL_CASES)
def test_products_within_the_bar_of_the_long_double_sums(ctx, case):
    la, lb, lout = case
    worst = 0.0
    for sa, sb in pc.SPIN_CASES:
        a, b = pc.operands(la, lb, sa, sb)
        got = _product(ctx, a, sa, la, b, sb, lb, lout)
        value, bar = pc.yardstick(a, sa, la, False, b, sb, lb, False, lout)
        assert got.shape == value.shape and got.dtype == np.complex128
        S = abs(sa + sb)
        assert np.all(got[:, : min(S * S, got.shape[1])] == 0)  # exact zeros below l = |S|
        worst = max(worst, _within(got, value, bar, (case, sa, sb)))
    print(f"(l_a, l_b, l_out) = {case}: largest |error| / bar {worst:.3f}")


@pytest.mark.parametrize("conj", [(True, False), (False, True), (True, True)])
def test_bar_of_either_operand_at_load(ctx, conj):
    ca, cb = conj
    for (la, lb, lout), (sa, sb) in (((3, 2, 2), (2, 1)), ((2, 3, 5), (-2, 2)), ((4, 4, 1), (1, -3)), ((5, 3, 4), (0, 2))):
        a, b = pc.operands(la, lb, sa, sb)
        got = _product(ctx, a, sa, la, b, sb, lb, lout, conj_a=ca, conj_b=cb)
        value, bar = pc.yardstick(a, sa, la, ca, b, sb, lb, cb, lout)
        _within(got, value, bar, (la, lb, lout, sa, sb, conj))
        # the flag is the bar of the modes: the same bits as the barred rows passed plain
        plain = _product(ctx, pc.bar(a, sa) if ca else a, -sa if ca else sa, la, pc.bar(b, sb) if cb else b, -sb if cb else sb, lb, lout)
        assert np.array_equal(got, plain), (la, lb, lout, sa, sb, conj)


def test_one_array_as_both_operands_and_garbage_below_the_spin(ctx):
    from scri_amd import engine

    la, lout = 4, 5
    a, _ = pc.operands(la, la, 2, 2)
    d = _dev(ctx, a)
    for ca, cb in ((False, False), (False, True), (True, True)):
        got = engine.mode_product(d, 2, la, d, 2, la, lout, conj_a=ca, conj_b=cb, ctx=ctx).cpu().numpy()
        value, bar = pc.yardstick(a, 2, la, ca, a, 2, la, cb, lout)
        _within(got, value, bar, ("same array", ca, cb))
        assert np.array_equal(got, _product(ctx, a, 2, la, a.copy(), 2, la, lout, conj_a=ca, conj_b=cb))
    for (sa, sb), garbage in (((2, -2), 1e300 + 3j), ((-1, -3), np.nan), ((2, 2), np.inf)):
        clean = _product(ctx, *_interleave(pc.operands(3, 4, sa, sb), sa, sb, 3, 4), 4)
        dirty = _product(ctx, *_interleave(pc.operands(3, 4, sa, sb, garbage=garbage), sa, sb, 3, 4), 4)
        assert np.all(np.isfinite(dirty)) and np.array_equal(clean, dirty), (sa, sb)


def _interleave(ab, sa, sb, la, lb):
    a, b = ab
    return a, sa, la, b, sb, lb


@pytest.mark.parametrize("ell", [16, 24])
def test_wide_rows(ctx, ell):
    from scri_amd import engine

    shape = engine.product_launch_shape(ell, ell, ell)
    a, b = pc.operands(ell, ell, 2, 2, n_times=5)
    got = _product(ctx, a, 2, ell, b, 2, ell, ell, conj_b=True)
    value, bar = pc.yardstick(a, 2, ell, False, b, 2, ell, True, ell)
    r = _within(got, value, bar, ell)
    print(f"l = {ell}: {pc.n_nodes(ell, ell, ell)} rows, launch shape {shape}, largest |error| / bar {r:.3f}")


# ---- 2. the edges of the launch
def test_lengths_around_one_pass(ctx):
    from scri_amd import engine

    steps, groups, _ = engine.product_launch_shape(2, 2, 2)
    lengths = sorted({1, 2, steps + 1, steps * groups + 1} | ({steps - 1} if steps > 1 else set()) | {steps})
    a, b = pc.operands(2, 2, 2, -2, n_times=max(lengths))
    whole = _product(ctx, a, 2, 2, b, -2, 2, 2)
    value, bar = pc.yardstick(a, 2, 2, False, b, -2, 2, False, 2)
    _within(whole, value, bar, "second turn of a persistent workgroup")
    for n in lengths:
        assert np.array_equal(_product(ctx, a[:n], 2, 2, b[:n], -2, 2, 2), whole[:n]), n
    assert _product(ctx, a[:0], 2, 2, b[:0], -2, 2, 2).shape == (0, 9)
    print(f"l = 2: {steps} step(s) per pass, {groups} workgroups; lengths {lengths}")


def test_largest_that_fits_and_first_that_does_not(ctx):
    from scri_amd import engine

    ell = 2
    while engine.product_launch_shape(ell + 1, ell + 1, ell + 1) is not None:
        ell += 1
    a, b = pc.operands(ell, ell, 2, -1, n_times=3)
    got = _product(ctx, a, 2, ell, b, -1, ell, ell)
    value, bar = pc.yardstick(a, 2, ell, False, b, -1, ell, False, ell)
    r = _within(got, value, bar, ell)
    print(f"largest (l, l, l) whose time step fits in LDS: l = {ell}, largest |error| / bar {r:.3f}")
    big = np.zeros((3, (ell + 2) ** 2), dtype=complex)
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):
            engine.mode_product(big, 2, ell + 1, big, -1, ell + 1, ell + 1, ctx=ctx)
        with pytest.raises(NotImplementedError, match="do not fit in LDS"):
            engine.supermomenta(big, big, big, ell + 1, ctx=ctx)
        assert sum(v[1] for v in ctx.get_timing(reset=True).values()) == 0
    finally:
        ctx.enable_timing(False)


# ---- 3. bits
def test_same_bits_in_slices_twice_from_host_arrays_and_in_wider_tensors(ctx):
    import torch

    from scri_amd import engine

    la, lb, lout, n = 5, 3, 4, 200
    a, b = pc.operands(la, lb, 2, -1, n_times=n)
    da, db = _dev(ctx, a), _dev(ctx, b)
    run = lambda x, y: engine.mode_product(x, 2, la, y, -1, lb, lout, conj_b=True, ctx=ctx)  # noqa: E731
    whole = run(da, db).cpu().numpy()
    assert np.array_equal(run(da, db).cpu().numpy(), whole)
    for i0, i1 in ((37, 111), (0, 7), (193, 200)):
        assert np.array_equal(run(da[i0:i1], db[i0:i1]).cpu().numpy(), whole[i0:i1]), (i0, i1)
    host = run(a, b)
    assert isinstance(host, np.ndarray) and np.array_equal(host, whole)
    blocks = []
    for k, x in enumerate((da, db)):
        wide = torch.full((n, x.shape[1] + 3 + 2 * k), float("nan"), dtype=torch.complex128, device=x.device)
        wide[:, k + 1:k + 1 + x.shape[1]] = x
        blocks.append(wide[:, k + 1:k + 1 + x.shape[1]])
    assert np.array_equal(run(*blocks).cpu().numpy(), whole)
    # a row stride of the output wider than its columns, through the C entry (the wrapper writes dense rows)
    from scri_amd import _lib

    n_out, ld_out = (lout + 1) ** 2, (lout + 1) ** 2 + 5
    out = torch.full((n, ld_out), float("nan"), dtype=torch.complex128, device=da.device)
    rc = _lib.load().bms_mode_product(ctx.handle, _lib.c_vp(da.data_ptr()), da.stride(0), 2, la, 0, _lib.c_vp(db.data_ptr()), db.stride(0), -1, lb, 1, n, lout,
                                      _lib.BMS_DEVICE, _lib.c_vp(out.data_ptr()), ld_out)
    assert rc == 0
    out = out.cpu().numpy()
    assert np.array_equal(out[:, :n_out], whole) and np.all(np.isnan(out[:, n_out:]))
    hout = np.full((n, ld_out), np.nan, dtype=complex)
    rc = _lib.load().bms_mode_product(ctx.handle, _lib.vptr(a), a.shape[1], 2, la, 0, _lib.vptr(b), b.shape[1], -1, lb, 1, n, lout, _lib.BMS_HOST, _lib.vptr(hout), ld_out)
    assert rc == 0 and np.array_equal(hout[:, :n_out], whole) and np.all(np.isnan(hout[:, n_out:]))
    value, bar = pc.yardstick(a, 2, la, False, b, -1, lb, True, lout)
    _within(whole, value, bar, "whole")


def _abd_on_device(ctx, ell_max, graded):
    """(t, psi2, sigma, sigma_dot as the route derives it in HBM, device tensors of the three)"""
    from scri_amd import engine

    t, psi2, sigma = pc.abd_case(ell_max, graded)
    d2, ds = _dev(ctx, psi2), _dev(ctx, sigma)
    dd = engine.spline_derivative(t, ds, t, 1, ctx=ctx)
    return t, psi2, sigma, dd.cpu().numpy(), (d2, ds, dd)


def test_supermomenta_one_by_one_and_integrated(ctx):
    from scri_amd import engine

    ell_max = 8
    t, psi2, sigma, sigma_dot, dev = _abd_on_device(ctx, ell_max, True)
    for lout in (ell_max, 5):
        together = [o.cpu().numpy() for o in engine.supermomenta(*dev, ell_max, lout, ctx=ctx)]
        integrated = [o.cpu().numpy() for o in engine.supermomenta(*dev, ell_max, lout, integrated=True, ctx=ctx)]
        for k, name in enumerate(pc.SUPERMOMENTA):
            alone = engine.supermomenta(*dev, ell_max, lout, want=name, ctx=ctx).cpu().numpy()
            assert np.array_equal(alone, together[k]), (name, lout)
            assert np.array_equal(engine.supermomenta(*dev, ell_max, lout, want=name, integrated=True, ctx=ctx).cpu().numpy(), integrated[k]), (name, lout)
        assert np.array_equal(integrated[4], together[4])  # the mass aspect is never altered
        for k in range(4):  # -bar / (2 sqrt(pi)) of the plain output: negation, conjugation and halving are exact, the division rounds once
            barred = -0.5 * pc.bar(together[k], 0)
            for got, expect in ((integrated[k].real, barred.real / np.sqrt(np.pi)), (integrated[k].imag, barred.imag / np.sqrt(np.pi))):
                assert np.all(np.abs(got - expect) <= pc.U * np.abs(expect)), (k, lout)
        host = engine.supermomenta(psi2, sigma, sigma_dot, ell_max, lout, ctx=ctx)
        for k in range(5):
            assert isinstance(host[k], np.ndarray) and np.array_equal(host[k], together[k]), (k, lout)
        i0, i1 = 11, 40
        part = engine.supermomenta(*(x[i0:i1] for x in dev), ell_max, lout, ctx=ctx)
        for k in range(5):
            assert np.array_equal(part[k].cpu().numpy(), together[k][i0:i1]), (k, lout)


# ---- 4. bms_supermomenta and the methods
def _abd(ctx, t, psi2, sigma, ell_max):
    import scri_amd

    a = scri_amd.AsymptoticBondiData(t, ell_max, ctx=ctx)
    a._raw_data[2], a._raw_data[5] = psi2, sigma
    return a


@pytest.mark.parametrize("case", pc.ABD_CASES)
def test_supermomenta_and_the_methods(ctx, case):
    from oracle import bms_charges_ref as cref
    from scri_amd import engine
    from scri_amd.device_series import DeviceModesTimeSeries

    ell_max, graded = case
    t, psi2, sigma, sigma_dot, dev = _abd_on_device(ctx, ell_max, graded)
    grid = 4 * pc.ORACLE_DISTANCE["supermomenta"]
    host = _abd(ctx, t, psi2, sigma, ell_max)
    resident = host.to_device()
    worst = 0.0
    for integrated in (False, True):
        y = pc.supermomenta_yardstick(psi2, sigma, sigma_dot, ell_max, ell_max, integrated)
        got = dict(zip(pc.SUPERMOMENTA, (o.cpu().numpy() for o in engine.supermomenta(*dev, ell_max, integrated=integrated, ctx=ctx))))
        four = resident.supermomenta(integrated=integrated)
        for k, (name, definition) in enumerate(pc.DEFINITIONS.items()):
            value, bar = y[name]
            worst = max(worst, _within(got[name], value, bar, (name, integrated)))
            _within(got[name], cref.supermomentum(t, psi2, sigma, definition, integrated=integrated), bar, (name, integrated, "oracle"), extra=grid)
            one = resident.supermomentum(definition, integrated=integrated)
            ref = host.supermomentum(definition, integrated=integrated)
            assert isinstance(one, DeviceModesTimeSeries) and isinstance(four[k], DeviceModesTimeSeries)
            assert (one.spin_weight, one.ell_min, one.ell_max, one._truncator) == (ref.spin_weight, ref.ell_min, ref.ell_max, host._truncator)
            assert np.array_equal(one.ndarray, got[name]) and np.array_equal(four[k].ndarray, got[name]), (name, integrated)
            _within(one.ndarray, np.asarray(ref.ndarray), bar, (name, integrated, "host-resident"), extra=grid)
        worst = max(worst, _within(got["mass_aspect"], *y["mass_aspect"], "mass_aspect"))
    for truncate in (max, ell_max, max(ell_max - 1, 1)):
        lout = ell_max if callable(truncate) else truncate
        value, bar = pc.supermomenta_yardstick(psi2, sigma, sigma_dot, ell_max, lout)["mass_aspect"]
        m, ref = resident.mass_aspect(truncate), host.mass_aspect(truncate)
        assert isinstance(m, DeviceModesTimeSeries) and (m.spin_weight, m.ell_min, m.ell_max) == (ref.spin_weight, ref.ell_min, ref.ell_max) == (0, 0, lout)
        worst = max(worst, _within(m.ndarray, value, bar, ("mass_aspect", lout)))
        _within(m.ndarray, cref.mass_aspect(t, psi2, sigma, lout), bar, ("mass_aspect", lout, "oracle"), extra=grid)
        _within(m.ndarray, np.asarray(ref.ndarray), bar, ("mass_aspect", lout, "host-resident"), extra=grid)
    assert resident.is_device_resident and not host.is_device_resident
    for got, name in zip(host.supermomenta(), pc.DEFINITIONS.values()):  # a host-resident object: the four methods, as they were
        assert np.array_equal(np.asarray(got.ndarray), np.asarray(host.supermomentum(name).ndarray))
    print(f"l_max = {ell_max}, {'graded' if graded else 'uniform'} axis: largest |error| / bar {worst:.3f}")


def _grid_launches(ctx):
    timing = ctx.get_timing(reset=True)
    return sum(timing[k][1] for k in GRID_TAGS), timing["pointwise"][1]


def test_recorded_supermomenta_of_the_reference_and_the_route_each_case_takes(ctx):
    """g25 within the tolerance tests/test_golden_reference_algebra.py holds it to; the aliasing working_ell_max, a widening truncator, an
    output band other than the fields' are seen to keep the grid route, by the context's launch counts; a host-resident object keeps its
    host series"""
    import scri_amd

    g = np.load(os.path.join(G, "g25_ref_supermomenta.npz"))
    L = int(g["ell_max"])
    host = scri_amd.AsymptoticBondiData(g["u"], L, ctx=ctx)
    host._raw_data[:] = g["raw"]
    abd = host.to_device()
    ctx.enable_timing(True)
    try:
        for name in ("Bondi-Sachs", "Moreschi", "Geroch", "GW"):
            for tag, kw in (("plain", {}), ("integrated", dict(integrated=True)), ("wide", dict(working_ell_max=6)),
                            ("integrated_wide", dict(integrated=True, working_ell_max=6))):
                ref = g[f"{name}_{tag}"]
                _grid_launches(ctx)
                r = abd.supermomentum(name, **kw)
                on_grid, pointwise = _grid_launches(ctx)
                assert (on_grid > 0) == ("wide" in tag) and pointwise >= 1, (name, tag, on_grid, pointwise)
                assert [r.spin_weight, r.ell_min, r.ell_max] == list(g[f"{name}_{tag}_meta"]), (name, tag)
                assert np.abs(np.asarray(r.ndarray) - ref).max() < 1e-12 * max(1.0, np.abs(ref).max()), (name, tag)
        routes = (("exact working_ell_max", lambda: abd.supermomentum("M", working_ell_max=2 * L), False),
                  ("narrower output", lambda: abd.supermomentum("M", output_ell_max=L - 1), True),
                  ("wider output", lambda: abd.supermomentum("M", output_ell_max=L + 1), True),
                  ("mass_aspect()", lambda: abd.mass_aspect(), False), ("mass_aspect(L - 1)", lambda: abd.mass_aspect(L - 1), False),
                  ("mass_aspect(sum)", lambda: abd.mass_aspect(sum), True), ("mass_aspect(L + 1)", lambda: abd.mass_aspect(L + 1), True),
                  ("mass_aspect(min)", lambda: abd.mass_aspect(min), False), ("supermomenta()", lambda: abd.supermomenta(), False),
                  ("CWWY_angular_momentum()", lambda: abd.CWWY_angular_momentum(), True))
        for what, call, grid in routes:
            _grid_launches(ctx)
            call()
            assert (_grid_launches(ctx)[0] > 0) == grid, what
    finally:
        ctx.enable_timing(False)
    with pytest.raises(ValueError) as e:
        abd.supermomentum("Bondi")
    assert str(e.value) == str(g["unknown_name_error"])
    assert abd.is_device_resident
    from scri_amd.device_series import DeviceModesTimeSeries

    for r in (host.supermomentum("M"), host.mass_aspect(), *host.supermomenta()):  # a host-resident object: host series from the grid route, as before
        assert not isinstance(r, DeviceModesTimeSeries) and not host.is_device_resident


# ---- 5. argument errors: every one comes back with its status and a message, and nothing is launched
def test_refusals(ctx):
    from scri_amd import _lib, engine

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, nm = 4, 16  # l = 3
    x = np.ones((n, nm), dtype=complex)
    out = np.full((n, nm), -1.0 + 0j)
    vp = _lib.vptr

    def product(c=ctx.handle, a=vp(x), ld_a=nm, sa=2, la=3, ca=0, b=vp(x), ld_b=nm, sb=-2, lb=3, cb=0, n_times=n, lout=3, mem=_lib.BMS_HOST, o=vp(out), ld_o=nm):
        return lib.bms_mode_product(c, a, ld_a, sa, la, ca, b, ld_b, sb, lb, cb, n_times, lout, mem, o, ld_o)

    def supermomenta(c=ctx.handle, p=vp(x), ld_p=nm, s=vp(x), ld_s=nm, d=vp(x), ld_d=nm, n_times=n, lmax=3, lout=3, mem=_lib.BMS_HOST, integrated=0,
                     outs=(vp(out),) * 5, ld_o=nm):
        return lib.bms_supermomenta(c, p, ld_p, s, ld_s, d, ld_d, n_times, lmax, lout, mem, integrated, *outs, ld_o)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    dx = _dev(ctx, x)
    dptr = lambda off=0: _lib.c_vp(dx.data_ptr() + off)  # noqa: E731
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        assert product(c=None) == INVALID and supermomenta(c=None) == INVALID
        assert product(mem=7) == INVALID and says("bms_mode_product: mem is BMS_HOST or BMS_DEVICE, got 7")
        assert supermomenta(mem=7) == INVALID and says("bms_supermomenta: mem is BMS_HOST or BMS_DEVICE, got 7")
        assert product(a=None) == INVALID and says("NULL") and product(b=None) == INVALID and product(o=None) == INVALID
        assert product(ld_a=nm - 1) == INVALID and says("row stride of a or b") and product(ld_b=nm - 1) == INVALID and says("row stride of a or b")
        assert product(ld_o=nm - 1) == INVALID and says("row stride of out")
        assert product(n_times=-1) == INVALID and says("negative n_times")
        assert product(la=-1) == INVALID and product(lb=-1) == INVALID and product(lout=-1) == INVALID and says("negative ell_max")
        assert product(lout=7, ld_o=64) == INVALID and says("ell_max_out = 7 is beyond ell_max_a + ell_max_b = 6")
        device = dict(a=dptr(), b=dptr(), o=dptr(), mem=_lib.BMS_DEVICE)
        for k in ("a", "b", "o"):
            assert product(**{**device, k: dptr(8)}) == INVALID and says("device arrays must be aligned")
        assert product(sa=5) == UNSUPPORTED and says("up to |s| = 4") and product(sa=-3, sb=-2) == UNSUPPORTED
        assert product(sa=3, ca=1, sb=-2) == UNSUPPORTED  # the effective spins count: -3 - 2
        assert product(sa=-3, ca=1, sb=-2) == 0
        assert product(la=9000, ld_a=1 << 40) == UNSUPPORTED and says("beyond")
        assert supermomenta(p=None) == INVALID and says("NULL psi2, sigma or sigma_dot") and supermomenta(s=None) == INVALID and supermomenta(d=None) == INVALID
        assert supermomenta(outs=(None,) * 5) == INVALID and says("every output is NULL")
        assert supermomenta(ld_s=nm - 1) == INVALID and says("row stride of sigma or sigma_dot") and supermomenta(ld_d=nm - 1) == INVALID
        assert supermomenta(ld_p=nm - 1) == INVALID and says("row stride of psi2 or of the outputs") and supermomenta(ld_o=nm - 1) == INVALID
        assert supermomenta(ld_p=9, lout=2, ld_o=9) == 0  # psi2 and the outputs are as wide as the band asked for
        assert supermomenta(n_times=-1) == INVALID and supermomenta(lmax=-1) == INVALID and supermomenta(lout=-1) == INVALID
        assert supermomenta(lout=4, ld_o=25, ld_p=25) == INVALID and says("ell_max_out = 4 is beyond ell_max = 3")
        assert supermomenta(lmax=1, lout=1) == UNSUPPORTED and says("ell_max = 1")
        assert supermomenta(p=dptr(8), s=dptr(), d=dptr(), outs=(dptr(),) * 5, mem=_lib.BMS_DEVICE) == INVALID and says("aligned")
        launched = ctx.get_timing(reset=True)["pointwise"][1]
        assert launched == 2  # the two calls above that were in order
        out[:] = -1.0
        assert product(n_times=0) == 0 and supermomenta(n_times=0) == 0 and np.all(out == -1.0)
        assert ctx.get_timing(reset=True)["pointwise"][1] == 0
        assert supermomenta(outs=(None, None, vp(out), None, None)) == 0 and ctx.get_timing(reset=True)["pointwise"][1] == 1 and not np.any(out == -1.0)
    finally:
        ctx.enable_timing(False)
    with pytest.raises(ValueError, match="want names"):
        engine.supermomenta(x, x, x, 3, want=("energy",), ctx=ctx)
    with pytest.raises(ValueError, match="same memory"):
        engine.mode_product(x, 2, 3, dx, -2, 3, 3, ctx=ctx)
    with pytest.raises(ValueError, match="beyond"):
        engine.mode_product(x, 2, 3, x, -2, 3, 7, ctx=ctx)
