"""GPU parity of bms_polar / bms_count_nonfinite (kernels_polar.hip; engine.abs_arg, engine.count_nonfinite) with the reference's
statements np.abs, np.angle and np.unwrap(np.angle(.), axis=0) on the inputs of tests/test_polar_host.py.

Bars (none of them set from what the kernels give):
  abs, arg     |gpu - numpy| <= (B + 1) spacing(|numpy|): 1 for glibc's own distance from exact, B the bound the device math library is
               specified to (OpenCL: hypot 4 ulp, atan2 6 ulp).  Special values and signed zeros are compared exactly.
  K            rint((unwrapped_gpu - arg_gpu) / 2 pi) equals the integer rule's count (test_polar_host.wrap_counts) at every element; the
               inputs keep min| |d| - pi | >= 1e-6, asserted on numpy's angles and on the GPU's.
  value        |unwrapped_gpu - float64(longdouble(arg_gpu) + K 2pi_longdouble)| <= 1 ulp of the result (a correctly rounded sum, or plain
               float64 whose extra |K| 2.45e-16 is below ulp(2 pi |K| - pi)); skipped where long double has fewer than 63 mantissa bits.
  whole        |gpu - np.unwrap(np.angle(z))| <= |np.unwrap(...) - exact| + (B + 2) ulp, exact = longdouble(np.angle(z)) + K 2pi: numpy's
               own drift comes from its float cumsum.
  NaN          a NaN planted at row 0, T-1, T, 2T+1 (different columns) makes that column NaN from there on and leaves the others'
               bits; an infinite part gives a finite angle and does not poison.
Host and device memory, abs-only / arg-only / both, a column-sliced view (ld > n_cols) and a wide output (ld_out > n_cols) give the
same bits; the counts and first rows of bms_count_nonfinite are exact; every refusal returns a negative status and leaves the context
giving the same bits."""
import ctypes

import numpy as np
import pytest

from tests import test_polar_host as ph

pytestmark = pytest.mark.gpu

B_HYPOT, B_ATAN2 = 4, 6  # OpenCL bounds of the device math library, in ulp
TWO_PI_LD = np.longdouble("6.283185307179586476925286766559005768394")
HAVE_LD = np.finfo(np.longdouble).nmant >= 63
N_ROWS = lambda T: (1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5)  # noqa: E731
N_COLS = (1, 5, 63, 64, 65, 77)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ulps(got, ref):
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(got - ref) / np.spacing(np.abs(ref)), initial=0.0))


def _dev(ctx, z):
    import torch

    from scri_amd import device_series

    return torch.from_numpy(np.array(z, order="C")).to(device_series.attach(ctx))  # (a copy: the shared blocks are read-only)


def _check_block(ctx, shape, z):
    """every bar of the module docstring on one clean block; returns (abs ulps, arg ulps) seen"""
    from scri_amd import engine

    a, p = engine.abs_arg(z, ctx=ctx)
    u = engine.abs_arg(z, unwrap=True, want="arg", ctx=ctx)
    assert isinstance(a, np.ndarray) and a.shape == p.shape == u.shape == z.shape and a.dtype == p.dtype == u.dtype == np.float64
    ref_a, ref_p = np.abs(z), np.angle(z)
    ua, up = _ulps(a, ref_a), _ulps(p, ref_p)
    print(f"polar {shape}: abs {ua:.2f} ulp, arg {up:.2f} ulp from numpy")
    assert ua <= B_HYPOT + 1, (shape, ua)
    assert up <= B_ATAN2 + 1, (shape, up)
    # K and the value
    assert ph.margin(ref_p) >= ph.MARGIN and ph.margin(p) >= ph.MARGIN, shape
    K = ph.wrap_counts(ref_p)
    assert np.array_equal(ph.wrap_counts(p), K), shape
    assert np.array_equal(np.rint((u - p) / ph.TWO_PI).astype(np.int64), K), shape
    assert _same_bits(u[:1], p[:1]), shape  # row 0 is p[0]
    if HAVE_LD:
        exact = (p.astype(np.longdouble) + K * TWO_PI_LD).astype(np.float64)
        assert np.all(np.abs(u - exact) <= np.spacing(np.abs(exact))), shape
    # against numpy as a whole
    whole = np.unwrap(ref_p, axis=0)
    exact_np = ref_p.astype(np.longdouble) + K * TWO_PI_LD
    drift = np.abs(whole - exact_np).astype(np.float64)
    bar = drift + (B_ATAN2 + 2) * np.spacing(np.abs(exact_np.astype(np.float64)))
    assert np.all(np.abs(u - whole) <= bar), shape
    # memory kinds, and the outputs asked for one at a time
    d = _dev(ctx, z)
    da, dp = engine.abs_arg(d, ctx=ctx)
    du = engine.abs_arg(d, unwrap=True, want="arg", ctx=ctx)
    assert da.is_cuda and str(da.dtype) == "torch.float64" and tuple(du.shape) == z.shape
    assert _same_bits(da.cpu().numpy(), a) and _same_bits(dp.cpu().numpy(), p) and _same_bits(du.cpu().numpy(), u), shape
    return ua, up


@pytest.mark.parametrize("n_cols", N_COLS)
def test_abs_arg_and_unwrapped_against_numpy(ctx, n_cols):
    from scri_amd import engine

    T = engine.POLAR_TILE_ROWS
    worst = [_check_block(ctx, (n_rows, n_cols), ph.cases()[n_rows, n_cols]) for n_rows in N_ROWS(T)]
    print(f"polar n_cols = {n_cols}: worst abs {max(w[0] for w in worst):.2f} ulp, arg {max(w[1] for w in worst):.2f} ulp")


def test_count_running_to_the_hundreds_and_back(ctx):
    from scri_amd import engine

    T = engine.POLAR_TILE_ROWS
    z = ph.cases()[16 * T + 3, 6]
    _check_block(ctx, z.shape, z)
    p, u = engine.abs_arg(z, want="arg", ctx=ctx), engine.abs_arg(z, unwrap=True, want="arg", ctx=ctx)
    assert np.abs(np.rint((u - p) / ph.TWO_PI)).max() >= 100


def test_one_output_at_a_time_and_both_give_the_same_bits(ctx):
    from scri_amd import engine

    T = engine.POLAR_TILE_ROWS
    for shape in ((2 * T + 1, 77), (3, 5), (T, 64)):
        z = ph.cases()[shape]
        for source in (z, _dev(ctx, z)):
            host = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()  # noqa: E731
            for unwrap in (False, True):
                a, p = (host(x) for x in engine.abs_arg(source, unwrap=unwrap, ctx=ctx))
                p2, a2 = (host(x) for x in engine.abs_arg(source, unwrap=unwrap, want=("arg", "abs"), ctx=ctx))
                assert _same_bits(host(engine.abs_arg(source, unwrap=unwrap, want="abs", ctx=ctx)), a), (shape, unwrap)
                assert _same_bits(host(engine.abs_arg(source, unwrap=unwrap, want=("arg",), ctx=ctx)[0]), p), (shape, unwrap)
                assert _same_bits(a2, a) and _same_bits(p2, p), (shape, unwrap)


def test_row_strides_of_input_and_output(ctx):
    """ld > n_cols: a column-sliced tensor view; ld_out > n_cols: a wide output through the C ABI, in device and in host memory"""
    import torch

    from scri_amd import _lib, engine

    T = engine.POLAR_TILE_ROWS
    z = ph.cases()[2 * T + 1, 77]
    n_rows, n_cols = z.shape
    a, p = engine.abs_arg(z, ctx=ctx)
    u = engine.abs_arg(z, unwrap=True, want="arg", ctx=ctx)
    wide = np.full((n_rows, n_cols + 9), complex(np.nan, np.nan))
    wide[:, 3 : 3 + n_cols] = z
    view = _dev(ctx, wide)[:, 3 : 3 + n_cols]
    assert view.stride(0) == n_cols + 9
    va, vp_ = engine.abs_arg(view, ctx=ctx)
    assert _same_bits(va.cpu().numpy(), a) and _same_bits(vp_.cpu().numpy(), p)
    assert _same_bits(engine.abs_arg(view, unwrap=True, want="arg", ctx=ctx).cpu().numpy(), u)
    assert engine.count_nonfinite(view, ctx=ctx) == (0, -1)
    lib, ld_out = _lib.load(), n_cols + 5
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)  # noqa: E731
    d = _dev(ctx, z)
    for unwrap, want_arg in ((0, p), (1, u)):
        oa = torch.full((n_rows, ld_out), float("nan"), dtype=torch.float64, device=d.device)
        op = torch.full((n_rows, ld_out), float("nan"), dtype=torch.float64, device=d.device)
        assert lib.bms_polar(ctx.handle, vp(d), n_cols, n_rows, n_cols, _lib.BMS_DEVICE, unwrap, vp(oa), vp(op), ld_out) == 0
        ha, hp = np.full((n_rows, ld_out), np.nan), np.full((n_rows, ld_out), np.nan)
        assert lib.bms_polar(ctx.handle, vp(z), n_cols, n_rows, n_cols, _lib.BMS_HOST, unwrap, vp(ha), vp(hp), ld_out) == 0
        for got_a, got_p in ((oa.cpu().numpy(), op.cpu().numpy()), (ha, hp)):
            assert _same_bits(np.ascontiguousarray(got_a[:, :n_cols]), a) and _same_bits(np.ascontiguousarray(got_p[:, :n_cols]), want_arg)
            assert np.isnan(got_a[:, n_cols:]).all() and np.isnan(got_p[:, n_cols:]).all()  # (nothing beyond the columns)


def test_special_values_and_signed_zeros_exactly(ctx):
    from scri_amd import engine

    inf, nan, pi = np.inf, np.nan, np.pi
    table = [  # (re, im, |z|, arg)
        (0.0, 0.0, 0.0, 0.0), (-1.0, 0.0, 1.0, pi), (-1.0, -0.0, 1.0, -pi), (1.0, -0.0, 1.0, -0.0), (-0.0, 0.0, 0.0, pi), (-0.0, -0.0, 0.0, -pi),
        (0.0, -0.0, 0.0, -0.0), (0.0, 2.0, 2.0, pi / 2), (0.0, -2.0, 2.0, -pi / 2), (-0.0, 2.0, 2.0, pi / 2), (nan, 1.0, nan, nan),
        (1.0, nan, nan, nan), (nan, nan, nan, nan), (inf, nan, inf, nan), (nan, -inf, inf, nan), (inf, 1.0, inf, 0.0), (inf, -1.0, inf, -0.0),
        (-inf, 1.0, inf, pi), (-inf, -1.0, inf, -pi), (1.0, inf, inf, pi / 2), (1.0, -inf, inf, -pi / 2), (3e200, 4e200, 5e200, None),
        (3e-200, 4e-200, 5e-200, None), (3e-320, 4e-320, 5e-320, None),
    ]
    z = np.array([[complex(r, i)] for r, i, _, _ in table])
    for source in (z, np.ascontiguousarray(z.T)):  # one column: the pointwise kernel; one row: with unwrap, the tiled kernels (row 0 is p[0])
        for unwrap in (False, True):
            a, p = engine.abs_arg(source, unwrap=unwrap and source.shape[0] == 1, ctx=ctx)
            a, p = a.reshape(-1), p.reshape(-1)
            for k, (r, i, want_a, want_p) in enumerate(table):
                if want_p is None:  # no spurious overflow or underflow
                    assert abs(a[k] - want_a) <= (B_HYPOT + 1) * np.spacing(want_a), (r, i, a[k])
                    continue
                assert _same_bits(a[k : k + 1], np.array([want_a])) or (np.isnan(want_a) and np.isnan(a[k])), (r, i, a[k])
                assert _same_bits(p[k : k + 1], np.array([want_p])) or (np.isnan(want_p) and np.isnan(p[k])), (r, i, p[k])
                # ... which is what numpy gives
                assert (np.isnan(want_a) and np.isnan(np.abs(z[k, 0]))) or np.abs(z[k, 0]) == want_a
                assert (np.isnan(want_p) and np.isnan(np.angle(z[k, 0]))) or _same_bits(np.array([np.angle(z[k, 0])]), np.array([want_p]))
    # infinite parts on the diagonals: finite angles within the bar
    d = np.array([[complex(inf, inf), complex(-inf, inf), complex(inf, -inf), complex(-inf, -inf)]])
    a, p = engine.abs_arg(d, ctx=ctx)
    assert np.isinf(a).all() and _ulps(p, np.angle(d)) <= B_ATAN2 + 1


def test_nan_poisons_its_column_from_there_on_and_inf_does_not(ctx):
    from scri_amd import engine

    T = engine.POLAR_TILE_ROWS
    clean = ph.cases()[3 * T + 5, 77]
    u_clean = engine.abs_arg(clean, unwrap=True, want="arg", ctx=ctx)
    z = clean.copy()
    planted = {12: 0, 3: T - 1, 5: T, 10: 2 * T + 1}  # column: row
    for k, (col, row) in enumerate(planted.items()):
        z[row, col] = complex(np.nan, 1.0) if k % 2 else complex(1.0, np.nan)
    z[T, 1] = complex(np.inf, 1.0)   # (column of kind "no wrap": the angle 0 of the infinite element keeps every step small)
    z[T - 1, 7] = complex(-2.0, np.inf)  # angle pi / 2
    for source in (z, _dev(ctx, z)):
        a, u = engine.abs_arg(source, unwrap=True, ctx=ctx)
        if not isinstance(u, np.ndarray):
            a, u = a.cpu().numpy(), u.cpu().numpy()
        untouched = np.ones(z.shape[1], dtype=bool)
        for col, row in planted.items():
            assert np.isnan(u[row:, col]).all() and _same_bits(u[:row, col], u_clean[:row, col]), (col, row)
            untouched[col] = False
        for col in (1, 7):
            assert np.isfinite(u[:, col]).all() and np.isinf(a[:, col]).sum() == 1, col
            assert np.array_equal(u[:, col], ph.unwrap_by_rule(engine.abs_arg(z[:, col : col + 1], want="arg", ctx=ctx))[:, 0]), col
            untouched[col] = False
        assert _same_bits(np.ascontiguousarray(u[:, untouched]), np.ascontiguousarray(u_clean[:, untouched]))
        assert np.array_equal(np.isnan(u), np.isnan(np.unwrap(np.angle(z), axis=0)))  # numpy poisons the same elements
    count, first = engine.count_nonfinite(z, ctx=ctx)
    assert (count, first) == (6, 0)


def test_count_nonfinite_is_exact(ctx):
    from scri_amd import engine

    T = engine.POLAR_TILE_ROWS
    clean = ph.cases()[3 * T + 5, 77]
    last = clean.shape[0] - 1
    bad = (complex(np.nan, 1.0), complex(1.0, np.nan), complex(np.inf, 1.0), complex(1.0, -np.inf), complex(np.nan, np.inf))
    plans = [[], [(0, 0)], [(T - 1, 76)], [(T, 5)], [(last, 76)], [(last, 0), (T, 3), (T, 4), (T - 1, 2)], [(2 * T, 63), (2 * T, 64), (5, 1)],
             [(r, c) for r in (0, T - 1, T, last) for c in (0, 31, 76)]]
    for k, plan in enumerate(plans):
        z = clean.copy()
        for m, (r, c) in enumerate(plan):
            z[r, c] = bad[(k + m) % len(bad)]
        want = (len(plan), min((r for r, _ in plan), default=-1))
        assert engine.count_nonfinite(z, ctx=ctx) == want, plan
        assert engine.count_nonfinite(_dev(ctx, z), ctx=ctx) == want, plan
        assert engine.count_nonfinite(_dev(ctx, z)[1:, 2:70], ctx=ctx) == (
            sum(1 for r, c in plan if r >= 1 and 2 <= c < 70), min((r - 1 for r, c in plan if r >= 1 and 2 <= c < 70), default=-1)), plan
    for shape in ((1, 1), (3, 5), (T + 1, 64)):
        assert engine.count_nonfinite(ph.cases()[shape], ctx=ctx) == (0, -1)
    assert engine.count_nonfinite(np.empty((0, 7), dtype=complex), ctx=ctx) == (0, -1)


def test_refusals_leave_the_context_as_it_was(ctx):
    from scri_amd import _lib, engine

    T = engine.POLAR_TILE_ROWS
    z = ph.cases()[T + 1, 65]
    n_rows, n_cols = z.shape
    baseline = engine.abs_arg(z, unwrap=True, ctx=ctx)
    lib, H = _lib.load(), _lib.BMS_HOST
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    a, p = np.full(z.shape, np.nan), np.full(z.shape, np.nan)
    count, first = ctypes.c_int64(-7), ctypes.c_int64(-7)
    polar = lambda **kw: lib.bms_polar(*[{**dict(c=ctx.handle, data=vp(z), ld=n_cols, n_rows=n_rows, n_cols=n_cols, mem=H, unwrap=1,  # noqa: E731
                                               a=vp(a), p=vp(p), ld_out=n_cols), **kw}[k]
                                         for k in ("c", "data", "ld", "n_rows", "n_cols", "mem", "unwrap", "a", "p", "ld_out")])
    count_ = lambda **kw: lib.bms_count_nonfinite(*[{**dict(c=ctx.handle, data=vp(z), ld=n_cols, n_rows=n_rows, n_cols=n_cols, mem=H,  # noqa: E731
                                                            count=ctypes.byref(count), first=ctypes.byref(first)), **kw}[k]
                                                    for k in ("c", "data", "ld", "n_rows", "n_cols", "mem", "count", "first")])
    refusals = [dict(data=None), dict(a=None, p=None), dict(mem=7), dict(mem=-1), dict(n_rows=-1), dict(n_cols=-1), dict(ld=n_cols - 1),
                dict(ld_out=n_cols - 1), dict(c=None)]
    for kw in refusals:
        rc = polar(**kw)
        assert rc < 0, (kw, rc)
        if kw.get("c", 1) is not None:
            assert rc == _lib.BMS_ERR_INVALID, (kw, rc)
        assert np.isnan(a).all() and np.isnan(p).all(), kw  # (nothing was written)
        again = engine.abs_arg(z, unwrap=True, ctx=ctx)
        assert _same_bits(again[0], baseline[0]) and _same_bits(again[1], baseline[1]), kw
    for kw in (dict(data=None), dict(mem=7), dict(n_rows=-1), dict(n_cols=-1), dict(ld=n_cols - 1), dict(count=None), dict(first=None), dict(c=None)):
        rc = count_(**kw)
        assert rc < 0 and (count.value, first.value) == (-7, -7), (kw, rc)
        assert engine.count_nonfinite(z, ctx=ctx) == (0, -1)
    # nothing to do: BMS_OK with nothing written
    assert polar(n_rows=0) == 0 and polar(n_cols=0, ld=0, ld_out=0) == 0 and np.isnan(a).all() and np.isnan(p).all()
    assert count_(n_rows=0) == 0 and count_(n_cols=0) == 0 and (count.value, first.value) == (-7, -7)
    # one output absent is no refusal
    assert polar(a=None) == 0 and np.isnan(a).all() and _same_bits(p, baseline[1])
    assert polar(p=None) == 0 and _same_bits(a, baseline[0])
    with pytest.raises(ValueError):
        engine.abs_arg(z, want=("abs", "phase"), ctx=ctx)
    with pytest.raises(ValueError):
        engine.abs_arg(_dev(ctx, z).real, ctx=ctx)
