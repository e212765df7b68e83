"""The six Bondi-gauge violations and their norms in one launch (bms_bondi_constraints: constraint_kernel in kernels_product.hip) and the
methods of a device-resident AsymptoticBondiData that run on it: parity with the long-double yardstick at ell_max = 2 (most product columns
below |S|), 3 (odd, five nodes), 8, and 17, 18, 20 (18 is the first size whose time step passes 64 kB of LDS), garbage below every spin; slices, row
strides, host arrays, repeats, single outputs and norms-only calls bit for bit, on a series longer than the grid of persistent workgroups;
every refusal; bondi_gauge_check, bondi_violations and bondi_violation_norms of resident objects against the yardstick, the
host-resident object, the reference's recorded norms (g26) and the reference's own bounds (tests/test_gpu_abd_ivp.py), with the route each
object takes read from the context's launch counts.

Yardstick and bars: tests/helpers/constraint_cases.py (derived, not measured), pinned without a GPU by
tests/test_constraint_yardstick_host.py.  Every test prints its own share of the bar.  Observed on the MI355X over the
whole file: v0, v1, v2 at most 0.12 of the bar, v3 0.37, v4 0.49, v5 0.13, the norms 0.14; the host-resident route within 0.49 of a bar of the yardstick."""
import os

import numpy as np
import pytest

from tests.helpers import constraint_cases as cc
from tests.helpers import product_cases as pc

pytestmark = pytest.mark.gpu

G26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_ref_initial_values.npz")
GRID_TAGS = ("gemm_synthesis", "gemm_analysis", "theta_quadrature", "analysis_fused", "analysis_large")


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, a)


def _inputs(ctx, ell_max, graded=False, n_times=cc.STEPS):
    """(host rows, device rows) of one case: (fields [6], psi_dot [3], sigma_dot, sigma_ddot)"""
    t, raw = cc.fields_case(ell_max, graded, n_times)
    psi_dot, sigma_dot, sigma_ddot = cc.host_derivatives(t, raw)
    host = (list(raw), psi_dot, sigma_dot, sigma_ddot)
    return host, ([_dev(ctx, x) for x in raw], [_dev(ctx, x) for x in psi_dot], _dev(ctx, sigma_dot), _dev(ctx, sigma_ddot))


def _run(ctx, rows, ell_max, **kw):
    """engine.bondi_constraints, everything as host arrays"""
    from scri_amd import engine

    v, norms = engine.bondi_constraints(*rows, ell_max, ctx=ctx, **kw)
    return [x.cpu().numpy() if hasattr(x, "cpu") else x for x in v], norms


def _shares(v, norms, yard):
    """the largest |error| / bar of the six violations and of the norms; every one must be within its bar"""
    (values, (norm_values, norm_bars)) = yard
    shares = [pc.ratio(v[k], *values[k]) for k in range(6)]
    shares.append(cc.norm_ratio(norms, norm_values, norm_bars))
    assert max(shares) <= 1.0, shares
    return shares


# ---- 1. values
@pytest.mark.parametrize("case", cc.ELL_CASES)
def test_entry_within_the_bars_of_the_long_double_yardstick(ctx, case):
    ell_max, graded = case
    host, dev = _inputs(ctx, ell_max, graded)
    v, norms = _run(ctx, dev, ell_max)
    assert all(x.shape == (cc.STEPS, (ell_max + 1) ** 2) and x.dtype == np.complex128 for x in v) and norms.shape == (cc.STEPS, 6) and norms.dtype == np.float64
    shares = _shares(v, norms, cc.yardstick(*host, ell_max))
    print(f"l_max = {ell_max}, {'graded' if graded else 'uniform'} axis: |error| / bar of v0 .. v5 and the norms: {', '.join(f'{r:.3f}' for r in shares)}")


@pytest.mark.parametrize("ell_max", [17, 18, 20])
def test_sizes_around_64_kb_of_lds(ctx, ell_max):
    """a time step of ell_max = 17 holds 59 232 bytes of rows and panels, 18 is the first beyond 64 kB (67 056) and 20 holds 82 176: beyond it
    the launcher has to ask for the dynamic LDS"""
    from scri_amd import engine

    lds = 16 * (3 * (ell_max + 1) ** 2 + 3 * pc.n_nodes(ell_max, ell_max, ell_max) * (2 * ell_max + 1))
    assert (lds > 64 * 1024) == (ell_max >= 18) and engine.product_launch_shape(ell_max, ell_max, ell_max) is not None
    host, dev = _inputs(ctx, ell_max, n_times=2)
    shares = _shares(*_run(ctx, dev, ell_max), cc.yardstick(*host, ell_max))
    print(f"l_max = {ell_max} ({lds} bytes of LDS): |error| / bar of v0 .. v5 and the norms: {', '.join(f'{r:.3f}' for r in shares)}")


def test_product_columns_below_the_spin_and_garbage_below_the_operands(ctx):
    """v0, v1, v2 and v5 read sigma, psi3, psi4 and sigma_dot through the products alone: whatever is stored below those spins changes no
    bit; with the diagonal terms zero the columns with l < |S| are exact zeros"""
    ell_max, n = 3, 5
    (raw, psi_dot, sigma_dot, sigma_ddot), _ = _inputs(ctx, ell_max, n_times=n)
    clean = _run(ctx, (raw, psi_dot, sigma_dot, sigma_ddot), ell_max, want=(0, 1, 2), norms=False)[0]
    for garbage in (np.nan, np.inf, 1e300 + 3j):
        dirty = [x.copy() for x in raw]
        for i in (3, 4, 5):
            dirty[i][:, : cc.SPINS[i] ** 2] = garbage
        got = _run(ctx, (dirty, psi_dot, sigma_dot, sigma_ddot), ell_max, want=(0, 1, 2), norms=False)[0]
        keep = [slice(None), slice(None), slice(1, None)]  # (v2 reads psi3 (0, 0) as stored, times a zero factor)
        assert all(np.array_equal(got[k][:, keep[k]], clean[k][:, keep[k]]) for k in range(3)), garbage
    # sigma_dot below l = 2 reaches v5 through the product alone (sigma itself is read as stored, times zero factors)
    five = _run(ctx, (raw, psi_dot, sigma_dot, sigma_ddot), ell_max, want=(5,), norms=False)[0][0]
    dirty_dot = sigma_dot.copy()
    dirty_dot[:, :4] = np.nan
    assert np.array_equal(_run(ctx, (raw, psi_dot, dirty_dot, sigma_ddot), ell_max, want=(5,), norms=False)[0][0], five)
    zero = np.zeros_like(raw[0])
    v0 = _run(ctx, ([None, zero, raw[2], None, None, raw[5]], [zero, None, None], None, None), ell_max, want=(0,), norms=False)[0][0]
    v1 = _run(ctx, ([None, None, zero, raw[3], None, raw[5]], [None, zero, None], None, None), ell_max, want=(1,), norms=False)[0][0]
    assert np.all(v0[:, :4] == 0) and np.all(v1[:, :1] == 0) and np.all(v0[:, 4:] != 0) and np.all(v1[:, 1:] != 0)
    value, bar = pc.yardstick(raw[5], 2, ell_max, False, raw[2], 0, ell_max, False, ell_max)
    assert pc.ratio(v0, -3 * value, 3 * bar + cc.U * np.abs(3 * value)) <= 1.0  # (one rounding more: the weight)


# ---- 2. bits
def test_same_bits_in_slices_strides_memories_repeats_and_single_outputs(ctx):
    import torch

    from scri_amd import _lib, engine

    ell_max, nm = 2, 9
    _, groups, _ = engine.product_launch_shape(ell_max, ell_max, ell_max)
    n = groups + 3  # some workgroups take a second pass
    host, dev = _inputs(ctx, ell_max, n_times=n)
    whole, norms = _run(ctx, dev, ell_max)
    shares = _shares(whole, norms, cc.yardstick(*host, ell_max))
    again, norms_again = _run(ctx, dev, ell_max)
    assert all(np.array_equal(a, b) for a, b in zip(again, whole)) and np.array_equal(norms_again, norms)
    cut = lambda rows, i0, i1: ([x[i0:i1] for x in rows[0]], [x[i0:i1] for x in rows[1]], rows[2][i0:i1], rows[3][i0:i1])  # noqa: E731
    for i0, i1 in ((0, 1), (n - 1, n), (37, 111), (groups - 2, n)):  # (n_times = 1 among them)
        part, part_norms = _run(ctx, cut(dev, i0, i1), ell_max)
        assert all(np.array_equal(part[k], whole[k][i0:i1]) for k in range(6)) and np.array_equal(part_norms, norms[i0:i1]), (i0, i1)
    from_host, host_norms = _run(ctx, cut(host, 0, 300), ell_max)
    assert all(isinstance(x, np.ndarray) and np.array_equal(x, w[:300]) for x, w in zip(from_host, whole)) and np.array_equal(host_norms, norms[:300])
    for k in range(6):  # each output alone, and the norms alone
        alone, no_norms = _run(ctx, dev, ell_max, want=(k,), norms=False)
        assert no_norms is None and len(alone) == 1 and np.array_equal(alone[0], whole[k]), k
    nothing, norms_only = _run(ctx, dev, ell_max, want=())
    assert nothing == [] and np.array_equal(norms_only, norms)

    def wide(x, k):  # the rows inside a wider tensor of NaN
        w = torch.full((x.shape[0], nm + 3 + k), float("nan"), dtype=torch.complex128, device=x.device)
        w[:, 1:1 + nm] = x
        return w[:, 1:1 + nm]

    padded = ([wide(x, k) for k, x in enumerate(dev[0])], [wide(x, 6 + k) for k, x in enumerate(dev[1])], wide(dev[2], 9), wide(dev[3], 10))
    strided, strided_norms = _run(ctx, padded, ell_max)
    assert all(np.array_equal(a, b) for a, b in zip(strided, whole)) and np.array_equal(strided_norms, norms)
    # a row stride of the outputs wider than their columns, and n_times = 0, through the C entry
    ld_out, m = nm + 5, 40
    out = torch.full((6, m, ld_out), float("nan"), dtype=torch.complex128, device=dev[2].device)
    vp, i64 = _lib.c_vp, _lib.c_i64
    fields = (vp * 6)(*(vp(x.data_ptr()) for x in dev[0]))
    dots = (vp * 3)(*(vp(x.data_ptr()) for x in dev[1]))
    homes = (vp * 6)(*(vp(out[k].data_ptr()) for k in range(6)))
    call = lambda n_times: _lib.load().bms_bondi_constraints(  # noqa: E731
        ctx.handle, fields, (i64 * 6)(*[nm] * 6), dots, (i64 * 3)(*[nm] * 3), vp(dev[2].data_ptr()), nm, vp(dev[3].data_ptr()), nm, n_times, ell_max,
        _lib.BMS_DEVICE, homes, ld_out, None)
    assert call(0) == 0 and bool(torch.isnan(out).all())
    assert call(m) == 0
    out = out.cpu().numpy()
    assert all(np.array_equal(out[k][:, :nm], whole[k][:m]) for k in range(6)) and np.all(np.isnan(out[:, :, nm:]))
    print(f"l_max = 2, {n} steps on {groups} workgroups: |error| / bar of v0 .. v5 and the norms: {', '.join(f'{r:.3f}' for r in shares)}")


# ---- 3. refusals: every one comes back with its status and a message, nothing is launched and no output is touched
def test_refusals(ctx):
    from scri_amd import _lib, engine

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, L = 4, 3
    nm = (L + 1) ** 2
    x = np.ones((n, 900), dtype=complex)  # (wide enough for the strides of ell_max = 29)
    out = np.full((n, 900), -1.0 + 0j)
    norms = np.full((n, 6), -1.0)
    vp, i64 = _lib.c_vp, _lib.c_i64
    X, O = _lib.vptr(x), _lib.vptr(out)

    def entry(c=ctx.handle, fields=(X,) * 6, ld_f=(900,) * 6, dots=(X,) * 3, ld_d=(900,) * 3, sd=X, ld_sd=900, sdd=X, ld_sdd=900, n_times=n, lmax=L,
              mem=_lib.BMS_HOST, outs=(O,) * 6, ld_o=900, nrm=_lib.vptr(norms)):
        return lib.bms_bondi_constraints(c, (vp * 6)(*fields), (i64 * 6)(*ld_f), (vp * 3)(*dots), (i64 * 3)(*ld_d), sd, ld_sd, sdd, ld_sdd, n_times, lmax, mem,
                                         (vp * 6)(*outs) if outs is not None else None, ld_o, nrm)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    only = lambda k: tuple(O if j == k else None for j in range(6))  # noqa: E731
    without = lambda i: tuple(None if j == i else X for j in range(6))  # noqa: E731
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        assert entry(c=None) == INVALID
        assert entry(mem=7) == INVALID and says("bms_bondi_constraints: mem is BMS_HOST or BMS_DEVICE, got 7")
        assert entry(outs=(None,) * 6, nrm=None) == INVALID and says("every output is NULL")
        assert entry(outs=None, nrm=None) == INVALID and says("every output is NULL")
        for i, name in ((1, "psi1"), (2, "psi2"), (3, "psi3"), (4, "psi4"), (5, "sigma")):  # the norms read everything but psi0
            assert entry(fields=without(i)) == INVALID and says(f"NULL {name}"), name
        assert entry(dots=(None, X, X)) == INVALID and says("NULL psi0_dot") and entry(dots=(X, X, None)) == INVALID and says("NULL psi2_dot")
        assert entry(sd=None) == INVALID and says("NULL sigma_dot") and entry(sdd=None) == INVALID and says("NULL sigma_ddot")
        assert entry(outs=only(3), nrm=None, sd=None) == INVALID and entry(outs=only(4), nrm=None, sdd=None) == INVALID
        assert entry(ld_f=(900, 900, nm - 1, 900, 900, 900)) == INVALID and says("row stride of psi2")
        assert entry(ld_d=(900, nm - 1, 900)) == INVALID and says("row stride of psi1_dot")
        assert entry(ld_sd=nm - 1) == INVALID and says("row stride of sigma_dot") and entry(ld_sdd=nm - 1) == INVALID and says("row stride of sigma_ddot")
        assert entry(ld_o=nm - 1) == INVALID and says("row stride of the violations")
        assert entry(n_times=-1) == INVALID and says("negative n_times")
        assert entry(lmax=-1) == INVALID and says("negative ell_max")
        assert entry(lmax=1) == UNSUPPORTED and says("ell_max = 1") and entry(lmax=0) == UNSUPPORTED
        assert entry(lmax=29) == UNSUPPORTED and says("do not fit in LDS")
        assert entry(lmax=9000, ld_f=(1 << 40,) * 6, ld_d=(1 << 40,) * 3, ld_sd=1 << 40, ld_sdd=1 << 40, ld_o=1 << 40) == UNSUPPORTED and says("beyond")
        dx = _dev(ctx, x)
        D = lambda off=0: vp(dx.data_ptr() + off)  # noqa: E731
        device = dict(fields=(D(),) * 6, dots=(D(),) * 3, sd=D(), sdd=D(), outs=(D(),) * 6, nrm=D(), mem=_lib.BMS_DEVICE)
        for key, bad in (("fields", (D(),) * 5 + (D(8),)), ("dots", (D(), D(8), D())), ("sd", D(8)), ("sdd", D(8)), ("outs", (D(8),) + (D(),) * 5), ("nrm", D(4))):
            assert entry(**{**device, key: bad}) == INVALID and says("device arrays must be aligned"), key
        assert sum(v[1] for v in ctx.get_timing(reset=True).values()) == 0  # nothing was launched
        assert np.all(out == -1.0) and np.all(norms == -1.0)
        # what is not needed may be NULL: psi0 always, and whatever only outputs not asked for read
        assert entry(fields=without(0)) == 0
        assert entry(outs=only(3), nrm=None, fields=(None, None, None, X, None, None), dots=(None,) * 3, sdd=None) == 0
        assert entry(outs=only(4), nrm=None, fields=(None, None, None, None, X, None), dots=(None,) * 3, sd=None) == 0
        assert entry(outs=only(0), nrm=None, fields=(None, X, X, None, None, X), dots=(X, None, None), sd=None, sdd=None) == 0
        assert entry(outs=only(5), nrm=None, fields=(None, None, X, None, None, X), dots=(None,) * 3, sdd=None) == 0
        timing = ctx.get_timing(reset=True)
        assert timing["constraints"][1] == 5 and sum(v[1] for k, v in timing.items() if k != "constraints") == 0
        out[:], norms[:] = -1.0, -1.0
        assert entry(n_times=0) == 0 and np.all(out == -1.0) and np.all(norms == -1.0)
        assert sum(v[1] for v in ctx.get_timing(reset=True).values()) == 0
    finally:
        ctx.enable_timing(False)
    y = np.ones((n, nm), dtype=complex)
    with pytest.raises(ValueError, match="want names"):
        engine.bondi_constraints([y] * 6, [y] * 3, y, y, L, want=(6,), ctx=ctx)
    with pytest.raises(ValueError, match="neither"):
        engine.bondi_constraints([y] * 6, [y] * 3, y, y, L, want=(), norms=False, ctx=ctx)
    with pytest.raises(ValueError, match="need sigma_ddot"):
        engine.bondi_constraints([y] * 6, [y] * 3, y, None, L, ctx=ctx)
    with pytest.raises(ValueError, match="same memory"):
        engine.bondi_constraints([y] * 5 + [_dev(ctx, y)], [y] * 3, y, y, L, ctx=ctx)
    with pytest.raises(NotImplementedError, match="ell_max = 1"):
        engine.bondi_constraints([y[:, :4]] * 6, [y[:, :4]] * 3, y[:, :4], y[:, :4], 1, ctx=ctx)


# ---- 4. the methods of AsymptoticBondiData
def _abd(ctx, t, raw, ell_max, truncator=max):
    import scri_amd

    a = scri_amd.AsymptoticBondiData(t, ell_max, multiplication_truncator=truncator, ctx=ctx)
    a._raw_data[:] = raw
    return a


def _launches(ctx):
    timing = ctx.get_timing(reset=True)
    return timing["constraints"][1], sum(timing[k][1] for k in GRID_TAGS)


@pytest.mark.parametrize("case", [(3, False), (8, True)])
def test_gauge_check_and_the_properties_of_a_resident_object(ctx, case):
    from scri_amd import engine
    from scri_amd.device_series import DeviceModesTimeSeries

    ell_max, graded = case
    t, raw = cc.fields_case(ell_max, graded)
    host = _abd(ctx, t, raw, ell_max)
    resident = host.to_device()
    # the yardstick is fed with the derivatives the route takes in HBM
    d = lambda i, order: engine.spline_derivative(t, resident._raw_dev[i], t, order, ctx=ctx).cpu().numpy()  # noqa: E731
    yard = cc.yardstick(list(raw), [d(0, 1), d(1, 1), d(2, 1)], d(5, 1), d(5, 2), ell_max)
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        series, norms = resident.bondi_gauge_check()
        assert _launches(ctx) == (1, 0)
        assert all(isinstance(s, DeviceModesTimeSeries) for s in series) and len(series) == len(norms) == 6
        assert [(s.spin_weight, s.ell_min, s.ell_max, s._truncator) for s in series] == [(sw, 0, ell_max, max) for sw in cc.VIOLATION_SPINS]
        assert all(isinstance(x, np.ndarray) and x.shape == (cc.STEPS,) for x in norms)
        shares = _shares([s.ndarray for s in series], np.stack(norms, axis=1), yard)
        only_norms = resident.bondi_gauge_check(violations=False)
        assert only_norms[0] is None and all(np.array_equal(a, b) for a, b in zip(only_norms[1], norms))
        only_series = resident.bondi_gauge_check(norms=False)
        assert only_series[1] is None and all(np.array_equal(v.ndarray, s.ndarray) for v, s in zip(only_series[0], series))
        _launches(ctx)
        # the properties of the resident object take the same route: one launch each and no grid product, the bits of the method
        violations = resident.bondi_violations
        assert _launches(ctx) == (1, 0)
        by_norms = resident.bondi_violation_norms
        assert _launches(ctx) == (1, 0)
        assert all(np.array_equal(v.ndarray, s.ndarray) for v, s in zip(violations, series)) and all(np.array_equal(a, b) for a, b in zip(by_norms, norms))
        assert resident.is_device_resident and not host.is_device_resident
        # the host-resident object keeps its route; the resident one lies within the bar plus that route's own distance from the yardstick
        on_host, host_norms = host.bondi_violations, host.bondi_violation_norms
        assert _launches(ctx)[0] == 0
    finally:
        ctx.enable_timing(False)
    (values, (norm_values, norm_bars)) = yard
    distance = []
    for k in range(6):
        value, bar = values[k]
        h = np.asarray(on_host[k].ndarray)
        assert not isinstance(on_host[k], DeviceModesTimeSeries) and (on_host[k].spin_weight, on_host[k].ell_max) == (cc.VIOLATION_SPINS[k], ell_max)
        away = np.abs(h.astype(cc.CLD) - value)
        distance.append(pc.ratio(h, value, bar))
        assert np.all(np.abs(violations[k].ndarray.astype(cc.CLD) - h) <= bar + away), k
        away = np.abs(np.asarray(host_norms[k]).astype(cc.LD) - norm_values[:, k])
        assert np.all(np.abs(by_norms[k].astype(cc.LD) - np.asarray(host_norms[k])) <= norm_bars[:, k] + away), k
    print(f"l_max = {ell_max}: resident |error| / bar of v0 .. v5 and the norms: {', '.join(f'{r:.3f}' for r in shares)}; "
          f"the host-resident route's distance from the yardstick, in bars, v0 .. v5: {', '.join(f'{r:.2f}' for r in distance)}")


def test_recorded_norms_of_the_reference_and_the_route_each_object_takes(ctx):
    """g26 moved to the device: the norms within the 1e-10 tests/test_golden_reference_algebra.py holds the host route to; the resident
    properties make one launch each and no grid product; ell_max = 1, another truncator and a host-resident object make none of the new
    launch, by the context's launch counts"""
    g = np.load(G26)
    u, L = g["u"], int(g["ell_max"])
    ctx.enable_timing(True)
    try:
        for tag in ("exact", "numeric"):
            resident = _abd(ctx, u, g[f"{tag}_raw"], L).to_device()
            _launches(ctx)
            norms = np.array(resident.bondi_violation_norms)
            assert _launches(ctx) == (1, 0)
            assert norms.shape == g[f"{tag}_violation_norms"].shape and np.abs(norms - g[f"{tag}_violation_norms"]).max() < 1e-10, tag
            assert resident.is_device_resident
        t, raw = cc.fields_case(3, n_times=20)
        for what, abd, one_launch in (("host-resident", _abd(ctx, t, raw, 3), False), ("sum truncator", _abd(ctx, t, raw, 3, sum).to_device(), False),
                                      ("ell_max = 1", _abd(ctx, t, raw[:, :, :4], 1).to_device(), False), ("resident", _abd(ctx, t, raw, 3).to_device(), True)):
            _launches(ctx)
            norms, violations = abd.bondi_violation_norms, abd.bondi_violations
            new, on_grid = _launches(ctx)
            assert (new == 2 and on_grid == 0) if one_launch else new == 0, (what, new, on_grid)
            assert len(norms) == len(violations) == 6 and abd.is_device_resident == (what != "host-resident")
            both = abd.bondi_gauge_check()  # of every object: the route its properties take
            assert _launches(ctx)[0] == (1 if one_launch else 0), what
            assert all(np.array_equal(np.asarray(a.ndarray), np.asarray(b.ndarray)) for a, b in zip(both[0], violations)), what
            assert all(np.array_equal(a, b) for a, b in zip(both[1], norms)), what
    finally:
        ctx.enable_timing(False)


def test_violations_beyond_the_measured_gain_keep_the_grid_products(ctx):
    """at ell_max = 17 (two workgroups per compute unit by LDS; the one launch was measured slower than the grid products at ell_max = 24,
    quicker at 16) bondi_violations keeps its route and bondi_violation_norms, which gains at every size, makes the one launch; the
    norms are those of the kept route to the norm bar plus that route's distance from the yardstick"""
    from scri_amd import engine

    ell_max, n = 17, 6
    t, raw = cc.fields_case(ell_max, n_times=n)
    resident = _abd(ctx, t, raw, ell_max).to_device()
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        violations = resident.bondi_violations
        new, on_grid = _launches(ctx)
        assert new == 0 and on_grid > 0
        norms = resident.bondi_violation_norms
        assert _launches(ctx) == (1, 0)
    finally:
        ctx.enable_timing(False)
    d = lambda i, order: engine.spline_derivative(t, resident._raw_dev[i], t, order, ctx=ctx).cpu().numpy()  # noqa: E731
    _, (norm_values, norm_bars) = cc.yardstick(list(raw), [d(0, 1), d(1, 1), d(2, 1)], d(5, 1), d(5, 2), ell_max)
    for k in range(6):
        kept = violations[k].norm()
        away = np.abs(np.asarray(kept).astype(cc.LD) - norm_values[:, k])
        assert np.all(np.abs(norms[k].astype(cc.LD) - kept) <= norm_bars[:, k] + away), k


def _nonsense(sigma, sigmadot, sigmaddot, psi2, psi1, psi0):
    from tests.test_gpu_abd_ivp import nonsense

    nonsense(sigma, sigmadot, sigmaddot, psi2, psi1, psi0)


def _entries(**entries):
    """a modifier of tests/test_gpu_abd_ivp.py: `nonsense` below the spins, then field[(l, m)] = value"""
    order = ("sigma", "sigmadot", "sigmaddot", "psi2", "psi1", "psi0")

    def modifier(*a):
        _nonsense(*a)
        for name, values in entries.items():
            for (l, m), value in values.items():
                a[order.index(name)][l * (l + 1) + m] = value

    return modifier


def _random(sigma, sigmadot, sigmaddot, psi2, psi1, psi0):
    rng = np.random.default_rng(1234)
    nm = sigma.size
    sigma[:] = 0.01 * rng.random(2 * nm).view(complex)
    sigmadot[:] = (0.01 / 100) * rng.random(2 * nm).view(complex)
    sigmaddot[:] = (0.01 / 100**2) * rng.random(2 * nm).view(complex)
    psi2[:] = 0.3 * rng.random(2 * nm).view(complex)
    psi1[:] = 0.1 * rng.random(2 * nm).view(complex)


# the seven constructions of the reference's test_abd_ivp (tests/test_gpu_abd_ivp.py) with the bounds it holds their violations to
IVP_CASES = {
    "test0": (_nonsense, 8, 0.0),
    "test1": (_entries(psi2={(0, 0): 0.234}), 3, 1e-13),
    "test2_and_3": (_entries(psi2={(0, 0): 0.234, (1, -1): 0.345, (2, -2): 0.456}), 4, 4e-11),
    "test4": (_entries(psi2={(0, 0): 0.234}, sigma={(2, 2): 0.5678}), 6, 2e-10),
    "test5": (_entries(sigma={(2, 2): 0.5678}, sigmadot={(2, 2): 0.6789}), 6, 7e-9),
    "test6": (_entries(sigmaddot={(2, 2): 0.1 / 10_000**2}), 7, 5e-8),
    "test7": (_random, 8, 4.5e-6),
}


@pytest.mark.parametrize("name", list(IVP_CASES))
def test_bounds_of_the_reference_on_resident_copies(ctx, name):
    from tests.test_gpu_abd_ivp import construct_and_validate, viol

    modifier, ell_max, limit = IVP_CASES[name]
    seen = {}

    def validator(abd):
        resident = abd.to_device()
        seen["viol"] = viol(resident)
        assert resident.is_device_resident and (seen["viol"] <= limit if limit else seen["viol"] == 0.0), (name, seen["viol"], limit)

    construct_and_validate(ctx, modifier, validator, ell_max=ell_max)
    print(f"{name}: largest violation norm of the resident copy {seen['viol']:.3e} (bound {limit:.1e})")
