"""GPU parity of the spline calculus (bms_spline_derivative, bms_cubic_spline, bms_angular_velocity: kernels_series.hip and
kernels_spline.hip) at the edges of its tiles, blocks, grids and LDS budgets, against the extended-precision reference
oracle/spline_exact.py.

One rule serves every case (tests/helpers/spline_cases.py): with E_got = max|got - exact|, E_ref = max|fp64 oracle - exact| (scipy
through oracle/modes_time_series_ref.py; oracle/mode_calculations_ref.py for the angular velocity) and scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured.
The comparison is against the reference and scipy's distance from it, never against the kernels' own output.

MEASURED on an MI355X, every call of this module (F and G of tests/helpers/spline_cases.py are the next power of two above twice
the first two columns; second column only over calls with E_ref < 4 eps scale):
  family   worst E_got/E_ref                      worst E_got/(eps scale)              worst E_got/scale: E_got, E_ref, shape
  anti     4.02  a, n=5, order -12                5.64  d, 255 columns, order -3       1.8e-15: 7.2e-13, 1.1e-12, b n=1025 uniform order -3
  value    1.73  a, n=8                           2.62  a, n=4                         7.2e-16: 2.6e-14, 4.3e-14, a n=6
  d1       2.18  b, n=640 uniform                 5.59  b, n=320 jittered              2.3e-15: 1.2e-14, 1.1e-14, b n=353 jittered
  d2       5.09  d, 63 columns (column 43)        4.46  d, 513 columns                 1.8e-13: 1.7e-12, 7.5e-13, b n=640 uniform
  d3       2.05  b, n=320 jittered                4.95  a, n=8                         1.8e-11: 3.4e-10, 3.2e-10, b n=1025 jittered
  cubic    1.48  i, n=4                           2.82  i, n=4                         6.3e-16: 4.8e-15, 3.3e-15, i n=4
  av       1.42  <Ldt>, ell 0..21, n=12           3.19  <Ldt>, ell 0..35, n=12         7.8e-16: 6.5e-12, 1.5e-11, <Ldt> ell 0..50 n=11
No case needed the caps, and none needed a change of a kernel.  The sizes up to 1225 modes pass with the four-wave launcher of before
the 4 / 2 / 1-wave choice as well (measured once, on the library built from the parent commit).

Cases (letters as in the lists of the functions below):
  bms_spline_derivative  a shortest series  b tile seams (slope tiles of 320 with a run-in of 32, prefix tiles of 512)  c knot ownership
                         d column blocks  e the stride loop over more than 32768 evaluation points  f axes at the mesh guard
                         g row stride wider than the columns  h column independence
  bms_cubic_spline       i shortest series  j ring overflow (more than 16 samples of an interval between two flushes)
                         k two and three tiles  l agreement with bms_spline_derivative(order = 0)
  bms_angular_velocity   every LDS size class of the launcher, a wide row stride, the <LL>-only caller, the refusal beyond one wave
Every device-memory call hands over an output tensor filled with NaN, and every host call of bms_cubic_spline follows a call of the
same shape on other data: a row that no lane writes shows as NaN or as the other data's row.
"""
import numpy as np
import pytest

from oracle import mode_calculations_ref as mc_ref
from oracle import modes_time_series_ref as mref
from oracle import spline_exact as sx
from tests.helpers import spline_cases as sc

pytestmark = pytest.mark.gpu

ALL_ORDERS = list(range(-16, 4))


# ------------------------------------------------------------------------------------------------------------- calls
def _entry(ctx, entry, t, y_ptr, ld, n_cols, mem, u, order, out_ptr):
    from scri_amd import _lib

    lib = _lib.load()
    if entry == "derivative":
        rc = lib.bms_spline_derivative(ctx.handle, _lib.dptr(t), t.shape[0], y_ptr, ld, n_cols, mem, _lib.dptr(u), u.shape[0], int(order), out_ptr)
    else:
        rc = lib.bms_cubic_spline(ctx.handle, _lib.dptr(t), t.shape[0], y_ptr, ld, n_cols, mem, _lib.dptr(u), u.shape[0], out_ptr)
    ctx.check(rc, entry)


def _host_call(ctx, entry, t, y, u, order=0, pad=0):
    """The C entry on host memory; pad > 0: rows of n_cols + pad columns, the padding NaN"""
    from scri_amd import _lib

    t, u = np.ascontiguousarray(t, dtype=float), np.ascontiguousarray(u, dtype=float)
    n, n_cols = y.shape
    buf = np.full((n, n_cols + pad), complex(np.nan, np.nan))
    buf[:, :n_cols] = y
    out = np.full((u.shape[0], n_cols), complex(np.nan, np.nan))
    _entry(ctx, entry, t, _lib.vptr(buf), n_cols + pad, n_cols, _lib.BMS_HOST, u, order, _lib.vptr(out))
    return out


def _device_call(ctx, entry, t, y, u, order=0, pad=0):
    """The C entry on device memory, as scri_amd/device_series.py passes it: a tensor view of row stride n_cols + pad (the padding NaN)
    and an output tensor that starts as NaN"""
    import torch

    from scri_amd import _lib, device_series

    dev = device_series.attach(ctx)
    t, u = np.ascontiguousarray(t, dtype=float), np.ascontiguousarray(u, dtype=float)
    n, n_cols = y.shape
    nan = complex(float("nan"), float("nan"))
    buf = torch.full((n, n_cols + pad), nan, dtype=torch.complex128, device=dev)
    view = buf[:, :n_cols]
    view.copy_(torch.from_numpy(np.ascontiguousarray(y, dtype=np.complex128)))
    assert view.stride(0) == n_cols + pad and view.stride(1) == 1
    out = torch.full((u.shape[0], n_cols), nan, dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    _entry(ctx, entry, t, _lib.c_vp(view.data_ptr()), view.stride(0), n_cols, _lib.BMS_DEVICE, u, order, _lib.c_vp(out.data_ptr()))
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _derivative(ctx, t, y, u, order):
    from scri_amd import engine

    return engine.spline_derivative(t, y, u, order, ctx=ctx)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _refs(t, y, u, order):
    return sx.evaluate(t, y, u, order), mref.interpolate(t, y, u, order)


def _parity(ctx, t, y, u, order, what, call=_derivative):
    exact, ref = _refs(t, y, u, order)
    got = call(ctx, t, y, u, order)
    sc.check(sc.family_of(order), got, exact, ref, f"{what} order={order}")
    return got


def _cubic(ctx, t, y, u, what):
    """bms_cubic_spline from host memory (after a call of the same shape on other data) and from device memory (into NaN): both under
    the rule, and the same bits.  Returns (result, bar)."""
    exact, ref = _refs(t, y, u, 0)
    _host_call(ctx, "cubic", t, y * (-1.7 + 0.3j) + 0.5, u)
    got = _host_call(ctx, "cubic", t, y, u)
    bar = sc.check("cubic", got, exact, ref, f"{what} host")
    got_dev = _device_call(ctx, "cubic", t, y, u)
    sc.check("cubic", got_dev, exact, ref, f"{what} device")
    assert _same_bits(got, got_dev), what
    return got, bar


# ------------------------------------------------------------------------------------------------ bms_spline_derivative
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8, 9])
def test_a_shortest_series(ctx, n):
    """the 4-knot unrolled loops and their tails, the first and last rows of the system; every order"""
    t = sc.jittered_axis(n, seed=n)
    y = sc.signal(t, 3, seed=n)
    u = np.concatenate([t, 0.5 * (t[1:] + t[:-1]), [t[0] - (t[1] - t[0]), t[-1] + (t[-1] - t[-2])]])
    for order in ALL_ORDERS:  # (orders -5 .. 3 at these lengths are what the older sweep could reach)
        _parity(ctx, t, y, u, order, f"a n={n}")


def _seam_points(t, seed):
    n = t.shape[0]
    pts = [t]
    for period in (320, 512):
        for s in range(period, n + 3, period):
            for j in range(s - 3, s + 3):  # the six intervals around the seam
                if 0 <= j <= n - 2:
                    pts.append([0.5 * (t[j] + t[j + 1])])
            if s <= n - 1:
                pts.append([np.nextafter(t[s], -np.inf), np.nextafter(t[s], np.inf)])
    pts.append(np.random.default_rng(seed).uniform(t[0], t[-1], 100))
    u = np.concatenate(pts)
    np.random.default_rng(seed + 1).shuffle(u)
    return u


@pytest.mark.parametrize("axis", ["uniform", "jittered"])
@pytest.mark.parametrize("n", [319, 320, 321, 352, 353, 511, 512, 513, 640, 641, 1025])
def test_b_tile_seams(ctx, n, axis):
    t = sc.uniform_axis(n) if axis == "uniform" else sc.jittered_axis(n, seed=n)
    y = sc.signal(t, 5, seed=n)
    u = _seam_points(t, n)
    for order in (-16, -3, -2, -1, 0, 1, 2, 3):  # (-3 .. 3 at n = 700 is what the older sweep could reach)
        _parity(ctx, t, y, u, order, f"b n={n} {axis}")


@pytest.mark.parametrize("n", [9, 353, 513])
def test_c_knot_ownership(ctx, n):
    """Order 3 is piecewise constant: the interval a sample is evaluated in is visible.  The interval is that of the last knot <= u."""
    t = sc.jittered_axis(n, seed=n)
    y = sc.signal(t, 3, seed=n)
    mid = 0.5 * (t[1:] + t[:-1])
    below = np.nextafter(t[1:], -np.inf)  # just under the knots 1 .. n-1
    outside = np.array([t[0] - 0.1, np.nextafter(t[0], -np.inf), np.nextafter(t[-1], np.inf), t[-1] + 0.1])
    u = np.concatenate([t, below, mid, outside])
    got = _parity(ctx, t, y, u, 3, f"c n={n}")
    at_knot, under_knot, at_mid, out = got[:n], got[n : 2 * n - 1], got[2 * n - 1 : 3 * n - 2], got[3 * n - 2 :]
    # (the value is 6 c3 of the interval and does not depend on the offset: the same interval gives the same bits)
    assert _same_bits(at_knot[: n - 1], at_mid)  # x_j belongs to [x_j, x_{j+1})
    assert _same_bits(under_knot, at_mid)  # nextafter(x_j, -inf) to the interval below
    assert _same_bits(at_knot[n - 1], at_mid[n - 2])  # the last knot and beyond: the last interval
    assert _same_bits(out[2], at_mid[n - 2]) and _same_bits(out[3], at_mid[n - 2])
    assert _same_bits(out[0], at_mid[0]) and _same_bits(out[1], at_mid[0])  # below x_0: the first interval
    # and the neighbouring interval's value is another one (not at x_1 and x_{n-2}: not-a-knot makes f''' continuous there)
    differs = np.any(at_mid[1:] != at_mid[:-1], axis=1)  # [k]: intervals k and k + 1
    assert np.all(differs[1 : n - 3]), np.nonzero(~differs[1 : n - 3])[0]


def _check_columns(family, got, exact, ref, what):
    """the rule column by column"""
    assert got.shape == exact.shape and np.isfinite(got).all(), what
    e_got = np.abs(got - exact).max(axis=0).astype(float)
    e_ref = np.abs(ref - exact).max(axis=0).astype(float)
    scale = np.maximum(1.0, np.abs(exact).max(axis=0).astype(float))
    F, G = sc.RULE[family]
    bar = np.maximum(F * e_ref, G * sc.EPS * scale)
    c = int(np.argmax(e_got / bar))
    print(f"RULE {family} E_got={e_got[c]:.3e} E_ref={e_ref[c]:.3e} scale={scale[c]:.3e} got/ref={e_got[c] / max(e_ref[c], 1e-300):.3g} "
          f"got/eps={e_got[c] / (sc.EPS * scale[c]):.3g} | {what} worst column {c}")
    # (for the record of the measured ratios: the worst of each over the columns, which need not be column c)
    print(f"RULECOLS {family} got/ref={np.max(e_got / np.maximum(e_ref, 1e-300)):.3g} "
          f"got/eps={np.max(np.where(e_ref < 4 * sc.EPS * scale, e_got / (sc.EPS * scale), 0.0)):.3g} | {what}")
    bad = np.nonzero(e_got > bar)[0]
    assert bad.size == 0, f"{what}: columns {bad[:8]} beyond the bar, e.g. E_got = {e_got[bad[0]]:.3e} > {bar[bad[0]]:.3e}"


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 255, 256, 257, 513])
def test_d_column_blocks(ctx, n_cols):
    """both evaluation kernels go from ceil(n_cols / 64) * 64 threads to blocks of 256 at 256 columns; partial last waves at 65 and 257"""
    n = 70
    t = sc.jittered_axis(n, seed=n_cols)
    y = sc.signal(t, n_cols, seed=n_cols)
    u = np.concatenate([t, np.random.default_rng(n_cols).uniform(t[0] - 0.05, t[-1] + 0.05, 150)])
    for order in (-3, -1, 0, 2):
        exact, ref = _refs(t, y, u, order)
        got = _derivative(ctx, t, y, u, order)
        _check_columns(sc.family_of(order), got, exact, ref, f"d n_cols={n_cols} order={order} host")
        got_dev = _device_call(ctx, "derivative", t, y, u, order)
        assert _same_bits(got, got_dev), (n_cols, order)


@pytest.mark.parametrize("shuffled", [False, True])
def test_e_more_samples_than_grid_rows(ctx, shuffled):
    """the evaluation grids stop at 32768 rows and stride over the rest"""
    n, n_new = 8, 32768 + 7
    t = sc.jittered_axis(n, seed=1)
    y = sc.signal(t, 3, seed=1)
    rng = np.random.default_rng(31)
    u = np.sort(rng.uniform(t[0] - 0.5, t[-1] + 0.5, n_new))
    if shuffled:
        rng.shuffle(u)
    for order in (-3, -2, 0, 1):
        exact, ref = _refs(t, y, u, order)
        for where, call in (("host", _derivative), ("device", lambda c, *a: _device_call(c, "derivative", *a))):
            got = call(ctx, t, y, u, order)
            fam = sc.family_of(order)
            sc.check(fam, got[:32768], exact[:32768], ref[:32768], f"e rows < 32768 shuffled={shuffled} order={order} {where}")
            sc.check(fam, got[32768:], exact[32768:], ref[32768:], f"e rows >= 32768 shuffled={shuffled} order={order} {where}")


def _mesh_guard_axis(kind):
    n = 700
    j = np.arange(n - 1)
    if kind == "wave794":  # max/min step 794 within 96 knots: still classified regular, so it is tiled
        return sc.axis_from_steps(0.05 * 10.0 ** (-1.45 * (1 + np.sin(2 * np.pi * j / 96))))
    if kind == "wave1e5":  # the same with amplitude 2.5: graded, one tile
        return sc.axis_from_steps(0.05 * 10.0 ** (-2.5 * (1 + np.sin(2 * np.pi * j / 96))))
    if kind in ("drop320", "drop512"):  # one drop of the step by 900 at a tile seam
        k = int(kind[4:])
        h0 = 12.0 / (k + (n - 1 - k) / 900.0)
        return sc.axis_from_steps(np.where(j < k, h0, h0 / 900.0))
    assert kind == "t1e5"  # the magnitude of a real waveform's time axis
    return 1e5 + np.cumsum(np.random.default_rng(41).uniform(0.05, 0.2, n))


@pytest.mark.parametrize("kind", ["wave794", "wave1e5", "drop320", "drop512", "t1e5"])
def test_f_axes_at_the_mesh_guard(ctx, kind):
    t = _mesh_guard_axis(kind)
    y = sc.signal(t, 5, seed=7)
    u = np.concatenate([t, 0.5 * (t[1:] + t[:-1]), np.random.default_rng(43).uniform(t[0], t[-1], 100)])
    for order in (-2, -1, 0, 1):  # (the older sweep reached graded axes of a step ratio up to 30, and random ones far beyond the guard)
        _parity(ctx, t, y, u, order, f"f {kind}")


@pytest.mark.parametrize("entry", ["derivative", "cubic"])
def test_g_row_stride_wider_than_the_columns(ctx, entry):
    n, n_cols = 353, 65
    t = sc.jittered_axis(n, seed=2)
    y = sc.signal(t, n_cols, seed=2)
    u = np.sort(_seam_points(t, 3))
    for order in (-3, -1, 0, 1) if entry == "derivative" else (0,):
        dense = _host_call(ctx, entry, t, y, u, order)
        if order == 0:
            exact, ref = _refs(t, y, u, 0)
            sc.check("value" if entry == "derivative" else "cubic", dense, exact, ref, f"g {entry} dense rows")
        assert np.isfinite(dense).all()
        assert _same_bits(_host_call(ctx, entry, t, y, u, order, pad=3), dense), (entry, order, "host")
        assert _same_bits(_device_call(ctx, entry, t, y, u, order, pad=3), dense), (entry, order, "device")


def test_h_column_independence(ctx):
    n, n_cols, sick = 353, 65, 17
    t = sc.jittered_axis(n, seed=4)
    y = sc.signal(t, n_cols, seed=4)
    y_nan = y.copy()
    y_nan[100, sick] = np.nan
    u = _seam_points(t, 5)
    others = np.arange(n_cols) != sick
    for order in (-2, 0, 1):
        clean = _derivative(ctx, t, y, u, order)
        got = _derivative(ctx, t, y_nan, u, order)
        assert np.isnan(got[:, sick]).any()
        assert _same_bits(got[:, others], clean[:, others]), order


# ------------------------------------------------------------------------------------------------ bms_cubic_spline
@pytest.mark.parametrize("n", [4, 5, 6, 7, 8])
def test_i_cubic_shortest_series(ctx, n):
    t = sc.jittered_axis(n, seed=10 + n)
    y = sc.signal(t, 3, seed=10 + n)
    h0, h1 = t[1] - t[0], t[-1] - t[-2]
    u = np.sort(np.concatenate([[t[0] - 0.5 * h0, t[0] - 0.1 * h0], t, t, 0.5 * (t[1:] + t[:-1]), [t[-1] + 0.1 * h1, t[-1] + 0.5 * h1]]))
    _cubic(ctx, t, y, u, f"i n={n}")  # (lengths the older sweep could reach, though not duplicated samples or a single one)
    for k, single in enumerate((0.5 * (t[1] + t[2]), t[0], t[-1] + 0.2 * h1)):
        _cubic(ctx, t, y, np.array([single]), f"i n={n} single sample {k}")


@pytest.mark.parametrize("n_cols", [1, 64, 65, 130])
def test_j_cubic_ring_overflow(ctx, n_cols):
    """more samples in an interval than the LDS ring has rows: the oldest row goes out early"""
    n = 40
    t = sc.jittered_axis(n, seed=20)
    y = sc.signal(t, n_cols, seed=20 + n_cols)
    everywhere = np.concatenate([np.linspace(t[j], t[j + 1], 50, endpoint=False) for j in range(n - 1)])
    _cubic(ctx, t, y, everywhere, f"j n_cols={n_cols} 50 per interval")
    crowded = np.concatenate([np.linspace(t[j], t[j + 1], 200, endpoint=False) for j in (3, 20, 37)])
    _cubic(ctx, t, y, crowded, f"j n_cols={n_cols} three crowded intervals")


def _tile_sample_sets(t):
    n = t.shape[0]
    inside = lambda j, count: np.linspace(t[j], t[j + 1], count, endpoint=False)  # noqa: E731
    sets = {}
    # (1) 40 samples in each of the intervals 317 .. 322, one elsewhere, and stretches of 7 knots without any
    dense = [j for j in range(317, 323) if j <= n - 2]
    sparse = [j for j in range(n - 1) if j not in dense and j % 40 >= 7]
    sets["seam crowd"] = np.sort(np.concatenate([inside(j, 40) for j in dense] + [inside(j, 1) + 0.3 * (t[j + 1] - t[j]) for j in sparse]))
    # (2) on the knots 319, 320, 321 and one ulp either side of knot 320 (of the last knot where the series ends before it)
    k = min(320, n - 1)
    sets["on the seam"] = np.sort(np.concatenate([t[[j for j in (319, 320, 321) if j <= n - 1]], [np.nextafter(t[k], -np.inf), np.nextafter(t[k], np.inf)]]))
    # (3) all inside one interval of the second tile (the last interval where there is none)
    sets["one interval"] = inside(min(330, n - 2), 30)
    # (4) beyond the last knot, (5) before the first
    sets["beyond"] = t[-1] + np.linspace(0.0, 0.02, 20)
    sets["before"] = t[0] - np.linspace(0.02, 0.0, 20)
    return sets


@pytest.mark.parametrize("n", [320, 321, 353, 700])
def test_k_l_cubic_across_tiles_and_agreement_of_the_two_forms(ctx, n):
    t = sc.jittered_axis(n, seed=30 + n)
    y = sc.signal(t, 65, seed=30 + n)
    for name, u in _tile_sample_sets(t).items():
        got, bar = _cubic(ctx, t, y, u, f"k n={n} {name}")
        # l: the slope form with the ring and the knot-data form agree within the sum of their tolerances
        exact, ref = _refs(t, y, u, 0)
        other = _derivative(ctx, t, y, u, 0)
        bar_other = sc.check("value", other, exact, ref, f"l n={n} {name}")
        assert float(np.abs(got - other).max()) <= bar + bar_other, (n, name)


# ------------------------------------------------------------------------------------------------ bms_angular_velocity
def _modes(t, ell_min, ell_max, seed):
    n_modes = (ell_max + 1) ** 2 - ell_min**2
    return sc.signal(t, n_modes, seed=seed)


def _check_av(got, t, data, ell_min, ell_max, what):
    ldt, ll, om = sx.ldt_ll_omega(t, data, ell_min, ell_max)
    ldt64 = mc_ref.LdtVector(data, mc_ref.data_dot(t, data), ell_min, ell_max)
    ll64 = mc_ref.LLMatrix(data, ell_min, ell_max)
    om64 = -np.linalg.solve(ll64, ldt64[..., None])[..., 0]
    for name, g, e, r in (("<Ldt>", got[0], ldt, ldt64), ("<LL>", got[1], ll, ll64), ("omega", got[2], om, om64)):
        sc.check("av", g, e, r, f"{what} {name}")


# (ell_min, ell_max, time-step counts): modes, what the size reaches.  The step counts are the remainders modulo the waves of a block.
AV_CASES = [
    (0, 21, (9, 10, 11, 12)),  # 484: the last static size (ell <= 16 is what the older tests reach)
    (0, 22, (9, 10, 11, 12)),  # 528: the first opt-in size
    (2, 22, (9, 10, 11, 12)),  # 525
    (0, 34, (9, 10, 11, 12)),  # 1225: the last that fits four waves in 160 KB
    (0, 35, (9, 10, 11, 12)),  # 1296: two waves
    (0, 49, (9, 10, 11, 12)),  # 2500: the last two-wave size
    (0, 50, (9, 10, 11, 12)),  # 2601: one wave
    (0, 70, (5,)),  # 5041: the last that fits at all
]


@pytest.mark.parametrize("ell_min,ell_max,steps", AV_CASES, ids=[f"ell{a}-{b}" for a, b, _ in AV_CASES])
def test_angular_velocity_at_the_lds_sizes(ctx, ell_min, ell_max, steps):
    from scri_amd import engine

    for n in steps:
        t = sc.jittered_axis(n, seed=n)
        data = _modes(t, ell_min, ell_max, seed=ell_max + n)
        got = engine.angular_velocity(t, data, ell_min, ell_max, ctx=ctx, parts=True)
        _check_av(got, t, data, ell_min, ell_max, f"av ell={ell_min}..{ell_max} n={n}")


def test_angular_velocity_from_a_wide_device_row(ctx):
    import torch

    from scri_amd import device_series, engine

    ell_min, ell_max, n = 2, 22, 11
    t = sc.jittered_axis(n, seed=n)
    data = _modes(t, ell_min, ell_max, seed=3)
    dev = device_series.attach(ctx)
    buf = torch.full((n, data.shape[1] + 5), complex(float("nan"), float("nan")), dtype=torch.complex128, device=dev)
    view = buf[:, : data.shape[1]]
    view.copy_(torch.from_numpy(data))
    assert view.stride(0) == data.shape[1] + 5
    torch.cuda.synchronize(dev)
    got = engine.angular_velocity(t, view, ell_min, ell_max, ctx=ctx, parts=True)
    _check_av(got, t, data, ell_min, ell_max, "av wide device row")
    dense = engine.angular_velocity(t, data, ell_min, ell_max, ctx=ctx, parts=True)
    assert all(_same_bits(a, b) for a, b in zip(got, dense))


def _principal_axis(ll, like):
    """Unit eigenvector of the largest eigenvalue of the symmetric positive matrices ll[n, 3, 3] by power iteration in the precision
    of ll, its sign that of `like`"""
    v = np.asarray(like).astype(ll.dtype)
    for _ in range(600):
        v = np.einsum("nij,nj->ni", ll, v)
        v /= np.sqrt((v * v).sum(axis=1))[:, None]
    return v


def test_ll_only_caller_at_a_two_wave_size(ctx):
    """engine_frames' <LL>-only launch (the dominant-axis path of the coprecessing frame) at 1296 modes"""
    from scri_amd import engine

    ell_min, ell_max, n = 0, 35, 10
    t = sc.jittered_axis(n, seed=n)
    data = _modes(t, ell_min, ell_max, seed=5)
    m = np.concatenate([np.arange(-l, l + 1) for l in range(ell_min, ell_max + 1)])
    data = data * (1.0 + 0.25 * np.abs(m))[None, :]  # weight towards |m| = l: <LL> gets a principal axis well apart from the others
    _, got = engine.coprecessing_frame(t, data, ell_min, ell_max, rough=(0.0, 0.0, 1.0), rough_index=0, want_axis=True, ctx=ctx)
    _, ll, _ = sx.ldt_ll_omega(t, data, ell_min, ell_max)
    ll64 = mc_ref.LLMatrix(data, ell_min, ell_max)
    lam, vec = np.linalg.eigh(ll64)
    assert np.min((lam[:, 2] - lam[:, 1]) / lam[:, 2]) >= 0.3  # the input condition, on the oracle's own numbers
    ref = vec[:, :, 2] * np.sign(np.sum(vec[:, :, 2] * got, axis=1))[:, None]
    assert np.all(got[:, 2] > 0.5)  # the rough direction decides the sign
    sc.check("av", got, _principal_axis(ll, got), ref, "av <LL>-only caller, principal axis")


def test_angular_velocity_refuses_what_one_wave_cannot_hold(ctx):
    """5184 modes: refused with the limit in words before anything is launched, by all three entries"""
    from scri_amd import _lib, engine

    ell_min, ell_max, n = 0, 71, 5
    t = sc.uniform_axis(n)
    data = np.zeros((n, (ell_max + 1) ** 2), dtype=complex)
    calls = (
        lambda: engine.angular_velocity(t, data, ell_min, ell_max, ctx=ctx),
        lambda: engine.coprecessing_frame(t, data, ell_min, ell_max, want_axis=True, ctx=ctx),
        lambda: engine.corotating_frame(t, data, ell_min, ell_max, _frame_tensor(ctx, n), want_omega=True, ctx=ctx),
    )
    for call in calls:
        with pytest.raises(NotImplementedError, match=rf"5184 modes.*at most 5120 modes.*status {_lib.BMS_ERR_UNSUPPORTED}\b"):
            call()
    ctx.synchronize()  # and the context is as usable as before
    small = sc.signal(t, 9, seed=1)
    assert np.isfinite(engine.angular_velocity(t, small, 0, 2, ctx=ctx)).all()


def _frame_tensor(ctx, n):
    import torch

    from scri_amd import device_series

    return torch.zeros((n, 4), dtype=torch.float64, device=device_series.attach(ctx))
