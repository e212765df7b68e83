"""AsymptoticBondiData.from_initial_values for a shear series resident in HBM, and the entry it runs on (bms_bianchi_rhs: bianchi_kernel
in kernels_product.hip): one stage of the Bianchi identities run forwards, rhs_k = eth a + (3 - k) sigma b, with psi4 and psi3 formed by
the head.

The entry is compared BIT FOR BIT with its composition -- the product of bms_mode_product and a numpy epilogue in the kernel's order -- at
ell_max = 2 (most product columns below |S|), 3 (odd), 8 and the largest size whose time step fits in LDS, on 1 and 5 steps and on a
series longer than the grid of persistent workgroups; then slices, memories, row strides and garbage below the spins, and every refusal.
The resident route is held to the reference's recorded values (g26) with the bound the host route is held to, and to the unchanged host
route on the inputs of tests/test_gpu_abd_ivp.py::test7_random_and_the_numerical_branch.

Host route against resident route (ell_max = 8, 2001 steps), largest |difference| / max(1, |ref|.max()) per field, measured on the MI355X:
see ROUTE_DIFFERENCE below.  The two routes differ by the rounding of the products (Gauss-Legendre rows against the grid) carried through
three integrals, in psi3 by the rounding of its factor (sqrt(x / 2) there, sqrt(x) / sqrt(2) here) and in sigma and psi4 by nothing."""
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_ref_initial_values.npz")
FIELDS = ("psi0", "psi1", "psi2", "psi3", "psi4", "sigma")
# Measured on the MI355X by test_resident_route_against_the_host_route, which prints them: psi0 9.43e-16, psi1 7.79e-16, psi2 2.29e-16,
# psi3 1.53e-19, psi4 0, sigma 0.  The bar is four times the largest, and never looser than the 1e-9 test7 allows between the branches.
ROUTE_DIFFERENCE = 9.43e-16
ROUTE_BAR = min(4 * ROUTE_DIFFERENCE, 1e-9)


def _dev(ctx, a):
    from scri_amd import device_series

    return device_series.to_device(ctx, a)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _ell(L):
    return np.concatenate([np.full(2 * l + 1, l) for l in range(L + 1)])


def _f(L, s):
    """the factor of the GHP eth on spin s as the kernel forms it: sqrt((l - s)(l + s + 1)) / sqrt(2), zero for l < max(|s|, |s + 1|)"""
    l = _ell(L)
    return np.where(l >= max(abs(s), abs(s + 1)), np.sqrt(np.maximum((l - s) * (l + s + 1), 0).astype(float)) / np.sqrt(2.0), 0.0)


def _bar(a, s, L):
    out = np.empty_like(a)
    for l in range(L + 1):
        for m in range(-l, l + 1):
            out[..., l * (l + 1) + m] = (-1.0) ** (s + m) * np.conj(a[..., l * (l + 1) - m])
    return out


def _rows(L, n, seed):
    """smooth random rows [n, (L + 1)^2]: random modes with a slow drift and a phase in time"""
    rng = np.random.default_rng(seed)
    nm = (L + 1) ** 2
    t = np.linspace(-1.0, 1.0, n)[:, None] if n > 1 else np.zeros((1, 1))
    c = rng.normal(size=(3, nm)) + 1j * rng.normal(size=(3, nm))
    return np.ascontiguousarray((c[0] + 0.3 * t * c[1] + 0.1 * t * t * c[2]) * np.exp(0.7j * t))


def _epilogue(k, L, a, product):
    """f_l * a + (3 - k) * product, per real and imaginary part in the kernel's order"""
    f = _f(L, 1 - k)
    times = float(3 - k)
    out = np.empty_like(product)
    out.real = f * a.real + times * product.real
    out.imag = f * a.imag + times * product.imag
    return out


def _composition(ctx, k, L, sigma, a, b):
    """what engine.bianchi_rhs(k, ...) must equal, from engine.mode_product on device tensors and numpy: rhs, or (rhs, psi3, psi4)"""
    from scri_amd import engine

    if k < 2:
        return _epilogue(k, L, a, _host(engine.mode_product(_dev(ctx, sigma), 2, L, _dev(ctx, b), -k, L, L, ctx=ctx)))
    psi4 = -_bar(b, 2, L)
    psi3 = -(_f(L, -2) * _bar(a, 2, L))
    return _epilogue(2, L, psi3, _host(engine.mode_product(_dev(ctx, sigma), 2, L, _dev(ctx, psi4), -2, L, L, ctx=ctx))), psi3, psi4


@functools.lru_cache(maxsize=None)
def _largest_ell_max():
    from scri_amd import engine

    return max(L for L in range(2, 25) if engine.product_launch_shape(L, L, L) is not None)


def _same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    want = want if isinstance(want, tuple) else (want,)
    return len(got) == len(want) and all(np.array_equal(_host(g), w) for g, w in zip(got, want))


# ---- 1. bits against the composition
@pytest.mark.parametrize("n_times", [1, 5])
@pytest.mark.parametrize("ell_max", [2, 3, 8, "largest"])
def test_bits_of_the_composition(ctx, ell_max, n_times):
    from scri_amd import engine

    L = _largest_ell_max() if ell_max == "largest" else ell_max
    sigma, a, b = (_rows(L, n_times, seed) for seed in (L, 100 + L, 200 + L))
    for k in (0, 1, 2):
        got = engine.bianchi_rhs(k, _dev(ctx, sigma), _dev(ctx, a), _dev(ctx, b), L, ctx=ctx)
        want = _composition(ctx, k, L, sigma, a, b)
        assert _same(got, want), (L, n_times, k)
        rhs = _host(got[0] if k == 2 else got)
        assert rhs.shape == (n_times, (L + 1) ** 2) and rhs.dtype == np.complex128 and np.all(np.isfinite(rhs)) and np.abs(rhs[:, 4:]).min() > 0


def test_bits_on_the_second_pass_of_the_persistent_loop(ctx):
    from scri_amd import engine

    L = 2
    n = engine.product_launch_shape(L, L, L)[1] + 3
    sigma, a, b = (_rows(L, n, seed) for seed in (1, 2, 3))
    for k in (0, 1, 2):
        assert _same(engine.bianchi_rhs(k, _dev(ctx, sigma), _dev(ctx, a), _dev(ctx, b), L, ctx=ctx), _composition(ctx, k, L, sigma, a, b)), k


# ---- 2. independence
def test_same_bits_in_memories_slices_strides_and_with_garbage_below_the_spins(ctx):
    import torch

    from scri_amd import engine

    L, n = 3, 5
    nm = (L + 1) ** 2
    sigma, a, b = (_rows(L, n, seed) for seed in (11, 12, 13))
    dev = [_dev(ctx, x) for x in (sigma, a, b)]

    def wide(x, k):  # the rows inside a wider tensor of NaN
        w = torch.full((x.shape[0], nm + 2 + k), float("nan"), dtype=torch.complex128, device=x.device)
        w[:, 1:1 + nm] = x
        return w[:, 1:1 + nm]

    for k in (0, 1, 2):
        whole = engine.bianchi_rhs(k, *dev, L, ctx=ctx)
        whole = tuple(_host(x) for x in whole) if k == 2 else (_host(whole),)
        assert _same(engine.bianchi_rhs(k, *dev, L, ctx=ctx), whole)  # two calls
        from_host = engine.bianchi_rhs(k, sigma, a, b, L, ctx=ctx)
        assert all(isinstance(x, np.ndarray) for x in (from_host if k == 2 else (from_host,))) and _same(from_host, whole)
        part = engine.bianchi_rhs(k, *(x[2:5] for x in dev), L, ctx=ctx)
        assert _same(part, tuple(w[2:5] for w in whole))
        assert _same(engine.bianchi_rhs(k, *(x[2:5] for x in (sigma, a, b)), L, ctx=ctx), tuple(w[2:5] for w in whole))
        # inputs as column slices of wider tensors, outputs into the slices of a [6, N, nm] tensor (and a wider one: ld > nm)
        for pad in (0, 5):
            raw = torch.full((6, n, nm + pad), float("nan"), dtype=torch.complex128, device=dev[0].device)
            home = (raw[0, :, :nm], raw[3, :, :nm], raw[4, :, :nm]) if k == 2 else raw[k + 1, :, :nm]
            back = engine.bianchi_rhs(k, *(wide(x, j) for j, x in enumerate(dev)), L, ctx=ctx, out=home)
            written = (0, 3, 4) if k == 2 else (k + 1,)
            raw = raw.cpu().numpy()
            assert _same(back, whole) and all(np.array_equal(raw[i][:, :nm], w) for i, w in zip(written, whole))
            assert np.all(np.isnan(raw[:, :, nm:])) and all(np.all(np.isnan(raw[i])) for i in range(6) if i not in written)
        # the product reads nothing below the spins of its operands: sigma below l = 2, b below |spin of b|
        for garbage in (np.nan, np.inf, 1e300 + 3j):
            dirty_s, dirty_b = sigma.copy(), b.copy()
            dirty_s[:, :4] = garbage
            if k < 2:
                dirty_b[:, : k * k] = garbage  # (k = 1: psi3 (0, 0); k = 0: psi2 has nothing below its spin)
                assert _same(engine.bianchi_rhs(k, dirty_s, a, dirty_b, L, ctx=ctx), whole), (k, garbage)
            else:  # the head stores psi4 and psi3 as formed, garbage included: rhs alone is the product's
                dirty_b[:, :4] = garbage
                rhs, _, psi4 = engine.bianchi_rhs(2, dirty_s, a, dirty_b, L, ctx=ctx)
                assert np.array_equal(rhs, whole[0]) and np.array_equal(psi4[:, 4:], whole[2][:, 4:]), garbage
        # the diagonal term reads `a` as stored, below its spin too, where the factor is an exact zero
        dirty_a = a.copy()
        dirty_a[:, : (1 - k) ** 2] = 1e300 + 3j
        assert _same(engine.bianchi_rhs(k, sigma, dirty_a, b, L, ctx=ctx), whole), k
    # product columns below l = |2 - k| are exact zeros: with a = 0 so is rhs there, and nowhere else
    zero = np.zeros_like(a)
    for k in (0, 1):
        rhs = engine.bianchi_rhs(k, sigma, zero, b, L, ctx=ctx)
        assert np.all(rhs[:, : (2 - k) ** 2] == 0) and np.all(rhs[:, (2 - k) ** 2:] != 0)


# ---- 3. refusals: every one comes back with its status and a message that names the entry, nothing is launched, no output is touched
def test_refusals(ctx):
    from scri_amd import _lib, engine

    lib = _lib.load()
    INVALID, UNSUPPORTED = _lib.BMS_ERR_INVALID, _lib.BMS_ERR_UNSUPPORTED
    n, L = 4, 3
    nm = (L + 1) ** 2
    x = np.ones((n, 900), dtype=complex)  # (wide enough for the strides of ell_max = 29)
    out = np.full((3, n, 900), -7.0 + 0j)
    X, R, P3, P4 = _lib.vptr(x), _lib.vptr(out[0]), _lib.vptr(out[1]), _lib.vptr(out[2])

    def entry(c=ctx.handle, k=1, sigma=X, ld_s=900, a=X, ld_a=900, b=X, ld_b=900, n_times=n, lmax=L, mem=_lib.BMS_HOST, rhs=R, ld_r=900, psi3=None,
              psi4=None, ld_p=0):
        return lib.bms_bianchi_rhs(c, k, sigma, ld_s, a, ld_a, b, ld_b, n_times, lmax, mem, rhs, ld_r, psi3, psi4, ld_p)

    says = lambda text: text in lib.bms_last_error(ctx.handle).decode() and "bms_bianchi_rhs" in lib.bms_last_error(ctx.handle).decode()  # noqa: E731
    head = dict(k=2, psi3=P3, psi4=P4, ld_p=900)
    ctx.enable_timing(True)
    try:
        ctx.get_timing(reset=True)
        assert entry(c=None) == INVALID
        assert entry(mem=7) == INVALID and says("mem is BMS_HOST or BMS_DEVICE, got 7")
        assert entry(k=3) == INVALID and says("names no stage") and entry(k=-1) == INVALID and says("names no stage")
        for name in ("sigma", "a", "b", "rhs"):
            assert entry(**{name: None}) == INVALID and says("NULL sigma, a, b or rhs"), name
            assert entry(**{**head, name: None}) == INVALID and says("NULL sigma, a, b or rhs"), name
        assert entry(**{**head, "psi3": None}) == INVALID and says("NULL psi3 or psi4")
        assert entry(**{**head, "psi4": None}) == INVALID and says("NULL psi3 or psi4")
        for k in (0, 1):
            assert entry(k=k, psi3=P3) == INVALID and says(f"must be NULL at k = {k}") and entry(k=k, psi4=P4) == INVALID and says(f"must be NULL at k = {k}")
        for key in ("ld_s", "ld_a", "ld_b"):
            assert entry(**{key: nm - 1}) == INVALID and says("columns read"), key
        assert entry(ld_r=nm - 1) == INVALID and says("columns written") and entry(**{**head, "ld_p": nm - 1}) == INVALID and says("columns written")
        assert entry(n_times=-1) == INVALID and says("negative n_times")
        assert entry(lmax=-1) == INVALID and says("negative ell_max")
        assert entry(lmax=1) == UNSUPPORTED and says("ell_max = 1") and entry(lmax=0) == UNSUPPORTED
        assert entry(lmax=29) == UNSUPPORTED and says("do not fit in LDS")
        assert entry(lmax=9000, ld_s=1 << 40, ld_a=1 << 40, ld_b=1 << 40, ld_r=1 << 40) == UNSUPPORTED and says("beyond")
        dx = _dev(ctx, x)
        D = lambda off=0: _lib.c_vp(dx.data_ptr() + off)  # noqa: E731
        device = dict(k=2, sigma=D(), a=D(), b=D(), rhs=D(), psi3=D(), psi4=D(), ld_p=900, mem=_lib.BMS_DEVICE)
        for key in ("sigma", "a", "b", "rhs", "psi3", "psi4"):
            assert entry(**{**device, key: D(8)}) == INVALID and says("device arrays must be aligned"), key
        assert sum(v[1] for v in ctx.get_timing(reset=True).values()) == 0  # nothing was launched
        assert np.all(out == -7.0)
        # an empty series is BMS_OK at any ell_max the library carries, and writes nothing
        assert entry(n_times=0) == 0 and entry(**{**head, "n_times": 0}) == 0 and entry(n_times=0, lmax=29) == 0 and np.all(out == -7.0)
        assert sum(v[1] for v in ctx.get_timing(reset=True).values()) == 0
        assert entry() == 0 and entry(**head) == 0
        timing = ctx.get_timing(reset=True)
        assert timing["constraints"][1] == 2 and sum(v[1] for k, v in timing.items() if k != "constraints") == 0
        assert np.all(out[:, :, :nm] != -7.0) and np.all(out[:, :, nm:] == -7.0)
    finally:
        ctx.enable_timing(False)
    y = np.ones((n, nm), dtype=complex)
    with pytest.raises(ValueError, match="same memory"):
        engine.bianchi_rhs(1, y, _dev(ctx, y), y, L, ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        engine.bianchi_rhs(1, y, y[:3], y, L, ctx=ctx)
    with pytest.raises(ValueError, match="out= names device arrays"):
        engine.bianchi_rhs(1, y, y, y, L, ctx=ctx, out=_dev(ctx, y))
    with pytest.raises(ValueError, match="writes 3"):
        engine.bianchi_rhs(2, _dev(ctx, y), _dev(ctx, y), _dev(ctx, y), L, ctx=ctx, out=_dev(ctx, y))
    with pytest.raises(NotImplementedError, match="ell_max = 1"):
        engine.bianchi_rhs(1, y[:, :4], y[:, :4], y[:, :4], 1, ctx=ctx)


# ---- 4. the resident route of from_initial_values against the reference's recorded values
def _relative(got, ref):
    return [float(np.abs(got[f] - ref[f]).max() / max(1.0, np.abs(ref[f]).max())) for f in range(6)]


def test_resident_route_against_the_values_of_the_reference(ctx):
    import torch

    import scri_amd

    g = np.load(G26)
    u, L = g["u"], int(g["ell_max"])
    abd = scri_amd.AsymptoticBondiData.from_initial_values(u, L, sigma0=_dev(ctx, g["sigma_of_u"]), psi2=g["psi2"], psi1=g["psi1"], psi0=g["psi0"], ctx=ctx)
    assert abd.is_device_resident and isinstance(abd._raw_dev, torch.Tensor) and abd._raw_dev.is_cuda and tuple(abd._raw_dev.shape) == g["numeric_raw"].shape
    shares = _relative(abd._raw_data, g["numeric_raw"])
    print("resident route against the reference (g26), |difference| / max(1, |ref|): " + ", ".join(f"{n} {s:.2e}" for n, s in zip(FIELDS, shares)))
    assert all(s < 2e-12 for s in shares), shares


# ---- 5. ... and against the unchanged host route
@pytest.fixture(scope="module")
def case7(ctx):
    """the inputs of the numerical branch in tests/test_gpu_abd_ivp.py::test7_random_and_the_numerical_branch -- the shear of the
    polynomial branch on its random coefficients (ell_max = 8, 2001 steps) and that branch's psi2, psi1, psi0 at time[0] -- and the
    host route on them, computed once: (u, ell_max, sigma, psi2, psi1, psi0, raw of the host route)"""
    import scri_amd

    ell_max = 8
    rng = np.random.default_rng(1234)
    nm = (ell_max + 1) ** 2
    u = np.linspace(-100, 100, num=2001)
    sigma = 0.01 * rng.random(2 * nm).view(complex)
    sigmadot = (0.01 / 100) * rng.random(2 * nm).view(complex)
    sigmaddot = (0.01 / 100**2) * rng.random(2 * nm).view(complex)
    psi2 = 0.3 * rng.random(2 * nm).view(complex)
    psi1 = 0.1 * rng.random(2 * nm).view(complex)
    a = scri_amd.AsymptoticBondiData.from_initial_values(u, ell_max, sigma, sigmadot, sigmaddot, psi2, psi1, np.zeros(nm, dtype=complex), ctx=ctx)
    inputs = (a.sigma.ndarray.copy(), a.psi2.ndarray[0].copy(), a.psi1.ndarray[0].copy(), a.psi0.ndarray[0].copy())
    host = scri_amd.AsymptoticBondiData.from_initial_values(u, ell_max, sigma0=inputs[0], psi2=inputs[1], psi1=inputs[2], psi0=inputs[3], ctx=ctx)
    assert not host.is_device_resident
    raw = host._raw_data
    raw.setflags(write=False)
    return (u, ell_max) + inputs + (raw,)


def test_resident_route_against_the_host_route(ctx, case7):
    import scri_amd

    u, L, sigma, psi2, psi1, psi0, host_route = case7
    abd = scri_amd.AsymptoticBondiData.from_initial_values(u, L, sigma0=_dev(ctx, sigma), psi2=psi2, psi1=psi1, psi0=psi0, ctx=ctx)
    assert abd.is_device_resident
    shares = _relative(abd._raw_data, host_route)
    print("resident route against the host route, |difference| / max(1, |ref|): " + ", ".join(f"{n} {s:.2e}" for n, s in zip(FIELDS, shares)))
    assert max(shares) <= ROUTE_BAR, shares
    norms = abd.bondi_violation_norms
    print(f"largest violation norm of the resident result: {np.max(norms):.3e}")
    assert np.max(norms) <= 4.5e-6


# ---- 6. edges
def _parent_statements(ctx, u, L, sigma0, psi2, psi1, psi0):
    """the spline branch of from_initial_values as it stood before the resident route, with engine.grid_multiply: [6, N, nm]"""
    from scri_amd import engine

    nm = (L + 1) ** 2
    lfac = lambda f: np.concatenate([np.full(2 * l + 1, f(l)) for l in range(L + 1)])  # noqa: E731
    eth = lambda a, s: a * lfac(lambda l: math.sqrt((l - s) * (l + s + 1) / 2.0) if l >= abs(s) and l >= abs(s + 1) else 0.0)  # noqa: E731
    real = lambda a: 0.5 * (a + _bar(a, 0, L))  # noqa: E731
    imag = lambda a: -0.5j * (a - _bar(a, 0, L))  # noqa: E731

    def mul(a, sa, b, sb):
        a, b = np.atleast_2d(a), np.atleast_2d(b)
        n = max(a.shape[0], b.shape[0])
        a = np.ascontiguousarray(np.broadcast_to(a, (n, a.shape[1])))
        b = np.ascontiguousarray(np.broadcast_to(b, (n, b.shape[1])))
        return engine.grid_multiply(a, sa, L, b, sb, L, 2 * L, L, ctx=ctx)

    def row(x, s):
        x = np.array(x, dtype=complex)[np.newaxis, :]
        x[..., : s * s] = 0
        return x

    psi2, psi1, psi0 = row(psi2, 0), row(psi1, 1), row(psi0, 2)
    d = lambda x, k: engine.spline_derivative(u, x, u, k, ctx=ctx)  # noqa: E731
    sig = np.array(sigma0, dtype=complex)
    sig[..., :4] = 0
    sb = _bar(sig, 2, L)
    p4 = -d(sb, 2)
    sbdot = d(sb, 1)
    p3 = -eth(sbdot, -2)
    adjust = real(psi2) - 1j * imag(eth(eth(sb[:1], -2), -1) + mul(sig[:1], 2, sbdot[:1], -2))
    p2 = d(eth(p3, -1) + mul(sig, 2, p4, -2), -1) + adjust
    p1 = d(eth(p2, 0) + 2 * mul(sig, 2, p3, -1), -1) + psi1
    p0 = d(eth(p1, 1) + 3 * mul(sig, 2, p2, 0), -1) + psi0
    assert p0.shape == (u.size, nm)
    return np.stack([p0, p1, p2, p3, p4, sig])


def _small_case(L, n, seed=5):
    rng = np.random.default_rng(seed)
    nm = (L + 1) ** 2
    u = np.linspace(0.0, 3.0, n)
    c = 0.05 * (rng.normal(size=(3, nm)) + 1j * rng.normal(size=(3, nm)))
    sigma = c[0] + u[:, None] * c[1] + np.sin(u)[:, None] * c[2]
    psi = [0.2 * (rng.normal(size=nm) + 1j * rng.normal(size=nm)) for _ in range(3)]
    return u, sigma, psi


def test_edges_of_the_resident_route(ctx):
    import scri_amd
    from scri_amd.device_series import DeviceModesTimeSeries

    ABD = scri_amd.AsymptoticBondiData
    # the spline's minimum, N = 4, and the composed fallback below the shear's first ell
    for L, n in ((3, 4), (1, 6)):
        u, sigma, (psi2, psi1, psi0) = _small_case(L, n)
        host = ABD.from_initial_values(u, L, sigma0=sigma, psi2=psi2, psi1=psi1, psi0=psi0, ctx=ctx)
        got = ABD.from_initial_values(u, L, sigma0=_dev(ctx, sigma), psi2=psi2, psi1=psi1, psi0=psi0, ctx=ctx)
        assert got.is_device_resident and not host.is_device_resident
        shares = _relative(got._raw_data, host._raw_data)
        print(f"ell_max = {L}, {n} steps, resident against host: " + ", ".join(f"{name} {s:.2e}" for name, s in zip(FIELDS, shares)))
        assert max(shares) <= ROUTE_BAR, (L, n, shares)
        if L == 1:
            assert np.all(got._raw_data[3:] == 0) and np.any(got._raw_data[2] != 0)
    # fewer steps than the spline takes: what the host route raises
    u, sigma, (psi2, psi1, psi0) = _small_case(3, 3)
    with pytest.raises(Exception) as host_error:
        ABD.from_initial_values(u, 3, sigma0=sigma, psi2=psi2, ctx=ctx)
    with pytest.raises(host_error.type):
        ABD.from_initial_values(u, 3, sigma0=_dev(ctx, sigma), psi2=psi2, ctx=ctx)
    # a wrong shape: the text the host route raises
    u, sigma, (psi2, psi1, psi0) = _small_case(3, 6)
    with pytest.raises(ValueError, match=r"Input `sigma0` must have shape \(6, 16\); it has \(5, 16\)"):
        ABD.from_initial_values(u, 3, sigma0=_dev(ctx, sigma[:5]), ctx=ctx)
    with pytest.raises(ValueError, match=r"Input `sigma0` must have shape \(6, 16\); it has \(5, 16\)"):
        ABD.from_initial_values(u, 3, sigma0=sigma[:5], ctx=ctx)
    # a series from ell_min = 2, device=True with a host series and a tensor from l = 0: the same bits
    kw = dict(psi2=psi2, psi1=psi1, psi0=psi0, ctx=ctx)
    tensor_in = ABD.from_initial_values(u, 3, sigma0=_dev(ctx, sigma), **kw)
    series = DeviceModesTimeSeries(_dev(ctx, sigma[:, 4:]), u, 2, 2, 3, ctx=ctx)
    from_series = ABD.from_initial_values(u, 3, sigma0=series, **kw)
    uploaded = ABD.from_initial_values(u, 3, sigma0=sigma, device=True, **kw)
    assert from_series.is_device_resident and uploaded.is_device_resident
    assert np.array_equal(from_series._raw_data, tensor_in._raw_data) and np.array_equal(uploaded._raw_data, tensor_in._raw_data)
    with pytest.raises(ValueError, match="spin weight 2"):
        ABD.from_initial_values(u, 3, sigma0=DeviceModesTimeSeries(_dev(ctx, sigma), u, 0, 0, 3, ctx=ctx), **kw)
    # device=False brings the resident result home; the polynomial branch with device=True is to_device() of its result
    home = ABD.from_initial_values(u, 3, sigma0=_dev(ctx, sigma), device=False, **kw)
    assert not home.is_device_resident and np.array_equal(home._raw_data, tensor_in._raw_data)
    poly = ABD.from_initial_values(u, 3, sigma[0], 0.1 * sigma[1], psi2=psi2, ctx=ctx)
    poly_dev = ABD.from_initial_values(u, 3, sigma[0], 0.1 * sigma[1], psi2=psi2, ctx=ctx, device=True)
    assert not poly.is_device_resident and poly_dev.is_device_resident and np.array_equal(poly_dev._raw_data, poly._raw_data)
    # a host series with `device` unset: a host object, the bits of the statements as they stood
    host = ABD.from_initial_values(u, 3, sigma0=sigma, **kw)
    assert not host.is_device_resident and isinstance(host._raw_data, np.ndarray)
    assert np.array_equal(host._raw_data, _parent_statements(ctx, u, 3, sigma, psi2, psi1, psi0))


# ---- 7. WM_to_MT of a resident waveform
def test_wm_to_mt_of_a_resident_waveform(ctx):
    import scri_amd
    from scri_amd import map_to_superrest_frame as m
    from scri_amd.device_series import DeviceModesTimeSeries

    u, sigma, _ = _small_case(4, 7)
    data = np.ascontiguousarray(sigma[:, 4:])
    make = lambda: scri_amd.WaveformModes(t=u, data=data.copy(), ell_min=2, ell_max=4, dataType=scri_amd.h, frameType=scri_amd.Inertial,  # noqa: E731
                                          r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    on_host = m.WM_to_MT(make())
    w = make().to_device()
    got = m.WM_to_MT(w)
    assert isinstance(got, DeviceModesTimeSeries) and not isinstance(on_host, DeviceModesTimeSeries)
    assert w.is_device_resident and got.buf.data_ptr() == w._dev.data_ptr()
    assert (got.ell_min, got.ell_max, got.spin_weight) == (on_host.ell_min, on_host.ell_max, on_host.spin_weight) == (2, 4, -2)
    assert got._truncator is max and np.array_equal(got.t, on_host.t)
    assert np.array_equal(got.ndarray, np.asarray(on_host)) and w.is_device_resident
