"""The Bondi charges of device-resident AsymptoticBondiData rows in one launch (bms_bondi_charges, charge_kernel in kernels_flux.hip) at
the shapes where the kernel can go wrong: l_max = 2 (sigma has no neighbour in l), 3 (one-sided), 5, 8 (81 columns: a second turn of the
wave with most lanes idle), 16 (289 columns) and 24 (the coefficient image read through L2); series of the derivative's minimum length
(4, 5), around one workgroup's share of a pass and, for the narrow rows, around one pass of the whole grid (both read from the launcher:
bms_charge_launch_shape); slices, single outputs and column blocks of wider tensors bit for bit; the public methods of a device-resident
object against the host-resident one; the reference's recorded charges (g12); the refusals.

Yardstick and bars: tests/helpers/charge_cases.py (the product rule's sums in long double, (n_terms + 16) 2^-53 S per time step and
component), pinned without a GPU by tests/test_bondi_charges_host.py."""
import os

import numpy as np
import pytest

from tests.helpers import charge_cases as cc

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, a)


def _charges(ctx, t, psi1, psi2, sigma, sigma_dot, ell_max, want=cc.CHARGES):
    """engine.bondi_charges on device tensors, results as host arrays by name"""
    from scri_amd import engine

    out = engine.bondi_charges(t, psi1, psi2, sigma, sigma_dot, ell_max, want=want, ctx=ctx)
    return {k: o.cpu().numpy() for k, o in zip(want, out)}


def _lengths(ell_max):
    """the series lengths of an l_max: the derivative's minimum, one workgroup's share of a pass +-1 and, for the narrow rows (the
    yardstick of a long series of wide rows takes too long), one pass of the whole grid +-1"""
    from scri_amd import engine

    waves, groups, _ = engine.charge_launch_shape((ell_max + 1) ** 2)
    n = {4, 5, waves - 1, waves, waves + 1}
    if ell_max <= 3:
        n |= {waves * groups - 1, waves * groups, waves * groups + 1}
    return sorted(k for k in n if k >= 1)


def _abd(ctx, t, psi1, psi2, sigma, ell_max):
    """a host-resident AsymptoticBondiData with these three fields (the charges read no other) and a mass monopole that keeps the
    four-momentum timelike"""
    import scri_amd

    a = scri_amd.AsymptoticBondiData(t, ell_max, ctx=ctx)
    a._raw_data[1], a._raw_data[2], a._raw_data[5] = psi1, psi2, sigma
    a._raw_data[2, :, 0] -= 5.0 * np.sqrt(4 * np.pi)
    return a


# ---- 1. yardstick
@pytest.mark.parametrize("ell_max", [2, 3, 5, 8, 16, 24])
def test_charges_within_the_bar_of_the_long_double_sums(ctx, ell_max):
    from scri_amd import engine

    in_lds = engine.charge_launch_shape((ell_max + 1) ** 2)[2]
    if ell_max == 24 and in_lds:
        return  # (the case is the branch that reads the image through L2: the smaller ones cover the other)
    worst = {}
    for n in _lengths(ell_max):
        t, psi1, psi2, sigma, sigma_dot = cc.chirp_fields(ell_max, n, 3 * ell_max + n % 13)
        got = _charges(ctx, t, *(_dev(ctx, x) for x in (psi1, psi2, sigma, sigma_dot)), ell_max)
        for name, (value, bar) in cc.yardstick(t, psi1, psi2, sigma, sigma_dot, ell_max).items():
            assert got[name].shape == value.shape and got[name].dtype == np.float64
            r = cc.ratio(got[name], value, bar)
            worst[name] = max(worst.get(name, 0.0), r)
            assert r <= 1.0, (name, n, r)
    print(f"l_max = {ell_max} (image in {'LDS' if in_lds else 'L2'}), N in {_lengths(ell_max)}: largest |error| / bar " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- 2. independence
def test_same_bits_in_slices_one_by_one_in_wider_tensors_and_twice(ctx):
    import torch

    from scri_amd import engine

    ell_max, n = 8, 1000
    t, *fields = cc.chirp_fields(ell_max, n, 4)
    d1, d2, ds, dd = (_dev(ctx, x) for x in fields)
    whole, again = _charges(ctx, t, d1, d2, ds, dd, ell_max), _charges(ctx, t, d1, d2, ds, dd, ell_max)
    for i0, i1 in ((137, 611), (0, 7), (993, 1000)):
        part = _charges(ctx, t[i0:i1], d1[i0:i1], d2[i0:i1], ds[i0:i1], dd[i0:i1], ell_max)
        for name in cc.CHARGES:
            assert np.array_equal(part[name], whole[name][i0:i1]), (name, i0, i1)
    for name in cc.CHARGES:
        assert np.array_equal(whole[name], again[name]), name
        single = engine.bondi_charges(t, d1, d2, ds, dd, ell_max, want=name, ctx=ctx).cpu().numpy()
        assert np.array_equal(single, whole[name]), name
    # the angular momentum and the centre-of-mass charge read neither sigma_dot, psi2 nor the times
    alone = _charges(ctx, None, d1, None, ds, None, ell_max, want=("angular", "com"))
    assert np.array_equal(alone["angular"], whole["angular"]) and np.array_equal(alone["com"], whole["com"])
    # column blocks of wider tensors, each with a row stride of its own
    nm = (ell_max + 1) ** 2
    blocks = []
    for k, x in enumerate((d1, d2, ds, dd)):
        wide = torch.full((n, nm + 3 + 2 * k), float("nan"), dtype=torch.complex128, device=x.device)
        wide[:, k + 1:k + 1 + nm] = x
        blocks.append(wide[:, k + 1:k + 1 + nm])
    strided = _charges(ctx, t, *blocks, ell_max)
    for name in cc.CHARGES:
        assert np.array_equal(strided[name], whole[name]), name
    for name, (value, bar) in cc.yardstick(t, *fields, ell_max).items():
        assert cc.ratio(whole[name], value, bar) <= 1.0, name


# ---- 3. the public route
@pytest.mark.parametrize("ell_max", [4, 8])
def test_methods_of_a_device_resident_object(ctx, ell_max):
    """the host-resident object takes the grid products; each side is held against the yardstick on the host's own derivative of sigma
    (both derive it with the same spline kernel): |dev - host| <= the bar + the host's own distance from the yardstick"""
    n = 300
    t, psi1, psi2, sigma, _ = cc.chirp_fields(ell_max, n, 20 + ell_max)
    host = _abd(ctx, t, psi1, psi2, sigma, ell_max)
    dev = host.to_device()
    sigma_dot = np.asarray(host.sigma.dot.ndarray)
    y = cc.yardstick(t, host._raw_data[1], host._raw_data[2], host._raw_data[5], sigma_dot, ell_max)
    together = dev.bondi_charges()
    singles = (dev.bondi_four_momentum(), dev.bondi_angular_momentum(), dev.bondi_boost_charge(), dev.bondi_CoM_charge())
    hosts = (host.bondi_four_momentum(), host.bondi_angular_momentum(), host.bondi_boost_charge(), host.bondi_CoM_charge())
    assert dev.is_device_resident and not host.is_device_resident
    for name, got, one, ref in zip(cc.CHARGES, together, singles, hosts):
        value, bar = y[name]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == ref.shape == value.shape
        assert np.array_equal(got, one), name
        host_distance = np.abs(ref.astype(cc.LD) - value)
        share = cc.ratio(got, value, bar)
        print(f"l_max = {ell_max} {name}: device {share:.3f} of the bar; the host route at most {float((host_distance / bar).max()):.2f} bars from the yardstick")
        assert np.all(np.abs(got.astype(cc.LD) - ref.astype(cc.LD)) <= bar + host_distance), name
    for got, ref in zip(host.bondi_charges(), hosts):  # a host-resident object: the four methods, as they were
        assert np.array_equal(got, ref)
    P = together[0]
    assert np.allclose(dev.bondi_rest_mass() ** 2, P[:, 0] ** 2 - (P[:, 1:] ** 2).sum(axis=1), rtol=1e-14, atol=0)
    chi_dev, chi_host = dev.bondi_dimensionless_spin(), host.bondi_dimensionless_spin()
    assert chi_dev.shape == (n, 3) and np.abs(chi_dev - chi_host).max() <= 5e-13 * max(1.0, np.abs(chi_host).max())
    assert dev.is_device_resident


# ---- 4. the reference's numbers
def test_recorded_charges_of_the_reference(ctx):
    """g12: the reference summed the same products on a grid in double and differentiated sigma-bar with scipy's spline; the yardstick
    takes the oracle's restatement of that derivative, and the recorded route's distance from it is measured here"""
    import scri_amd
    from oracle import modes_time_series_ref as mref

    g = np.load(os.path.join(G, "g12_ref_bms_charges.npz"), allow_pickle=False)
    u, raw, L = g["u"], g["raw"], int(g["ell_max"])
    a = scri_amd.AsymptoticBondiData(u, L, ctx=ctx)
    a._raw_data[:] = raw
    a = a.to_device()
    y = cc.yardstick(u, raw[1], raw[2], raw[5], mref.interpolate(u, raw[5], u, 1), L)
    recorded = dict(four_momentum="bondi_four_momentum", angular="bondi_angular_momentum", boost="bondi_boost_charge", com="bondi_CoM_charge")
    for name, got in zip(cc.CHARGES, a.bondi_charges()):
        value, bar = y[name]
        ref = g[recorded[name]].astype(cc.LD)
        distance = np.abs(ref - value)
        print(f"g12 {name}: device {cc.ratio(got, value, bar):.3f} of the bar, the recorded route at most {float((distance / bar).max()):.2f} bars from the yardstick")
        assert np.all(np.abs(got.astype(cc.LD) - ref) <= 2 * bar + distance), name


# ---- 5. argument errors: every one comes back with its status and a message, and nothing is launched
def _launches(ctx):
    return ctx.get_timing(reset=True)["pointwise"][1]


def test_refusals(ctx):
    from scri_amd import _lib

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, nm = 6, 16  # l_max = 3
    t = np.linspace(0.0, 1.0, n)
    x = np.ones((n, nm), dtype=complex)
    P, J, N, Gc = np.zeros((n, 4)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    vp, dp = _lib.vptr, _lib.dptr

    def charges(c=ctx.handle, t=dp(t), p1=vp(x), ld1=nm, p2=vp(x), ld2=nm, s=vp(x), lds=nm, sd=vp(x), ldd=nm, n_times=n, lmax=3, mem=_lib.BMS_HOST,
                P=vp(P), J=vp(J), N=vp(N), Gc=vp(Gc)):
        return lib.bms_bondi_charges(c, t, p1, ld1, p2, ld2, s, lds, sd, ldd, n_times, lmax, mem, P, J, N, Gc)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    d = _dev(ctx, x)
    ctx.enable_timing(True)
    try:
        _launches(ctx)
        assert charges(c=None) == INVALID
        assert charges(mem=7) == INVALID and says("mem is BMS_HOST or BMS_DEVICE, got 7")
        device = dict(p1=_lib.c_vp(d.data_ptr()), p2=_lib.c_vp(d.data_ptr()), s=_lib.c_vp(d.data_ptr()), sd=_lib.c_vp(d.data_ptr()), mem=_lib.BMS_DEVICE)
        assert charges(**{**device, "s": _lib.c_vp(d.data_ptr() + 8)}) == INVALID and says("device arrays must be aligned")
        assert charges(sd=None) == INVALID and says("need sigma_dot")
        assert charges(sd=None, J=None, N=None, Gc=None) == INVALID and says("need sigma_dot")
        assert charges(p2=None) == INVALID and says("need psi2")
        assert charges(p1=None) == INVALID and says("need psi1")
        assert charges(s=None) == INVALID and says("NULL sigma")
        assert charges(t=None) == INVALID and says("needs the times")
        assert charges(P=None, J=None, N=None, Gc=None) == INVALID and says("every output is NULL")
        assert charges(lds=nm - 1) == INVALID and says("row stride smaller than the number of modes (16)")
        assert charges(ldd=nm - 1) == INVALID and says("row stride")
        assert charges(ld1=3) == INVALID and says("four columns")
        assert charges(n_times=-1) == INVALID and says("negative n_times")
        assert charges(lmax=1) == UNSUPPORTED and says("ell_max = 1")
        assert charges(lmax=-1) == INVALID
        # beyond the LDS rule: two rows of (71 + 1)^2 columns are more than a workgroup has (nothing is read before the refusal)
        assert charges(lmax=71, ld1=5184, ld2=5184, lds=5184, ldd=5184) == UNSUPPORTED and says("do not fit in LDS")
        P[:] = -1.0
        assert charges(n_times=0) == 0 and np.all(P == -1.0)
        assert _launches(ctx) == 0
        # the angular momentum and the centre-of-mass charge need neither sigma_dot, psi2 nor the times
        assert charges(t=None, p2=None, sd=None, P=None, N=None) == 0 and _launches(ctx) == 1 and np.all(P == -1.0)
        assert charges() == 0 and _launches(ctx) == 1 and np.all(np.isfinite(P)) and not np.any(P == -1.0)
    finally:
        ctx.enable_timing(False)
    from scri_amd import engine

    with pytest.raises(ValueError, match="need sigma_dot"):
        engine.bondi_charges(t, x, x, x, None, 3, ctx=ctx)
    with pytest.raises(ValueError, match="want names"):
        engine.bondi_charges(t, x, x, x, x, 3, want=("energy",), ctx=ctx)
    host = engine.bondi_charges(t, x, x, x, x, 3, ctx=ctx)  # host arrays in, host arrays out, the bits of device memory
    on_device = _charges(ctx, t, d, d, d, d, 3)
    for name, got in zip(cc.CHARGES, host):
        assert isinstance(got, np.ndarray) and np.array_equal(got, on_device[name]), name
