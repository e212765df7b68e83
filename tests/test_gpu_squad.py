"""GPU parity of the rotor interpolation bms_squad (kernels_frames.hip: squad_control_kernel, squad_eval_kernel; engine.squad) with the
statement `scri_amd.quaternions.squad`, measured against the long-double truth of tests/test_squad_statement.py on that module's inputs.

The rule is the project's (tests/test_gpu_spline_edges.py:7) with scale 1 -- the components of a unit rotor:
    E_got <= max(F * E_ref, G * eps),   E_got = max|GPU - truth|,  E_ref = max|float64 statement - truth|,   F <= 32 and G <= 256 whatever
is measured.  The margin covers the device's atan2, sin, cos, log, exp differing from the host's by an ulp or two through three nested
slerps; every other operation is the statement's, in its order and without contraction.  F and G below are the next power of two
above twice the worst ratio measured.

MEASURED on an MI355X (E in units of eps; every ordered and shuffled call of this module, host and device memory give the same bits):
  axis     n      E_got   E_ref   E_got/E_ref   | |R| - 1 |   max|GPU - statement|
  uniform  2      2.10    2.66    0.79          2.0           1.5
  uniform  3      2.36    2.36    1.00          2.5           1.5
  uniform  4      2.26    2.44    0.92          4.0           1.0
  uniform  5      1.48    1.81    0.82          2.0           1.0
  uniform  255    2.68    2.89    0.92          3.0           1.5      (256 and 257: the same figures)
  uniform  1025   2.68    2.89    0.92          4.0           1.5
  graded   2      0.80    0.80    1.00          1.0           0.5
  graded   3      1.29    1.48    0.87          2.0           0.5
  graded   4      1.23    1.23    1.00          1.5           0.5
  graded   5      1.35    1.60    0.84          1.5           0.5
  graded   255    2.23    2.70    0.83          3.0           1.5      (256 and 257: the same figures)
  graded   1025   2.48    2.78    0.89          3.0           1.5
  sign-flipped series (uniform 257, graded 256, uniform 4): | |R| - 1 | = 3.0, 3.0, 4.0 eps
Worst E_got / E_ref = 1.00 and worst E_got / eps = 2.68, so F = 4 and G = 8; the caps were not needed.

Also asserted: host and device memory give identical bits; ascending and shuffled arguments give the same value per argument; a series
whose sign flips half way (no accuracy input: tests/test_squad_statement.py) comes out finite and of norm 1 within G eps; every refusal of
include/scri_amd.h returns BMS_ERR_INVALID with a message and leaves the context giving the same bits afterwards; one rotor, no rotors
and no arguments answer as the numpy statement does."""
import numpy as np
import pytest

from scri_amd import quaternions
from tests import test_squad_statement as st

pytestmark = [pytest.mark.gpu, st.pytestmark]

EPS = st.EPS
F, G = 4.0, 8.0  # worst measured: 1.00 and 2.68 (the table above)
assert F <= 32.0 and G <= 256.0


def _device(ctx, R, t, u):
    """engine.squad on device memory, into a tensor that starts as NaN; back as numpy"""
    import torch

    from scri_amd import device_series, engine

    dev = device_series.attach(ctx)
    out = torch.full((len(u), 4), float("nan"), dtype=torch.float64, device=dev)
    got = engine.squad(torch.from_numpy(np.array(R, dtype=float)).to(dev), t, u, ctx=ctx, out=out)
    assert got is out
    return out.cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", st.AXES)
def test_squad_against_the_long_double_truth(ctx, kind):
    from scri_amd import engine

    worst_f = worst_g = 0.0
    for n in st.SIZES:
        c = st.cases()[kind, n]
        t, R, u, p = c["t"], c["R"], c["u"], c["perm"]
        got = engine.squad(R, t, u, ctx=ctx)
        assert got.shape == (u.size, 4) and np.isfinite(got).all(), (kind, n)
        assert _same_bits(got, _device(ctx, R, t, u)), (kind, n)
        shuffled = engine.squad(R, t, u[p], ctx=ctx)
        assert _same_bits(shuffled, got[p]), (kind, n)
        assert _same_bits(_device(ctx, R, t, u[p]), shuffled), (kind, n)
        e_got, e_ref = st.error(got, c["truth"]), st.error(c["ref"], c["truth"])
        drift = float(np.abs(np.linalg.norm(got, axis=1) - 1).max())
        print(f"RULE squad {kind} n={n}: E_got = {e_got / EPS:.2f} eps, E_ref = {e_ref / EPS:.2f} eps, got/ref = {e_got / e_ref:.2f}, "
              f"| |R| - 1 | = {drift / EPS:.2f} eps, max|GPU - statement| = {np.abs(got - c['ref']).max() / EPS:.2f} eps")
        worst_f, worst_g = max(worst_f, e_got / e_ref), max(worst_g, e_got / EPS)
        assert e_ref <= 8 * EPS
        assert e_got <= max(F * e_ref, G * EPS), (kind, n, e_got, e_ref)
        assert drift <= G * EPS
    print(f"RULE squad {kind}: worst E_got / E_ref = {worst_f:.2f}, worst E_got / eps = {worst_g:.2f}")


def test_sign_flipped_series_is_finite_and_unit(ctx):
    from scri_amd import engine

    for kind, n in (("uniform", 257), ("graded", 256), ("uniform", 4)):
        c = st.cases()[kind, n]
        R = st.sign_flipped(c["R"])
        got = engine.squad(R, c["t"], c["u"], ctx=ctx)
        drift = float(np.abs(np.linalg.norm(got, axis=1) - 1).max())
        print(f"sign-flipped {kind} n={n}: | |R| - 1 | = {drift / EPS:.2f} eps")
        assert np.isfinite(got).all() and drift <= G * EPS
        assert _same_bits(got, _device(ctx, R, c["t"], c["u"]))


def test_refusals_leave_the_context_as_it_was(ctx):
    from scri_amd import _lib, engine

    lib = _lib.load()
    c = st.cases()["graded", 5]
    t, R, u = c["t"].copy(), c["R"].copy(), c["u"].copy()
    baseline = engine.squad(R, t, u, ctx=ctx)
    out = np.full((u.size, 4), np.nan)
    H, dp, vp = _lib.BMS_HOST, _lib.dptr, _lib.vptr
    equal, falling, t_nan, t_inf, u_nan, u_inf = t.copy(), t.copy(), t.copy(), t.copy(), u.copy(), u.copy()
    equal[3] = equal[2]
    falling[1], falling[2] = t[2], t[1]
    t_nan[4], t_inf[0], u_nan[7], u_inf[-1] = np.nan, -np.inf, np.nan, np.inf
    n, m = t.size, u.size
    refused = {
        "NULL t_in": lambda: lib.bms_squad(ctx.handle, None, n, vp(R), H, dp(u), m, vp(out)),
        "NULL R_in": lambda: lib.bms_squad(ctx.handle, dp(t), n, None, H, dp(u), m, vp(out)),
        "NULL t_out": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, None, m, vp(out)),
        "NULL out": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, dp(u), m, None),
        "mem = 7": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), 7, dp(u), m, vp(out)),
        "n = 1": lambda: lib.bms_squad(ctx.handle, dp(t), 1, vp(R), H, dp(u), m, vp(out)),
        "n = 0": lambda: lib.bms_squad(ctx.handle, dp(t), 0, vp(R), H, dp(u), m, vp(out)),
        "n = -3": lambda: lib.bms_squad(ctx.handle, dp(t), -3, vp(R), H, dp(u), m, vp(out)),
        "m = -1": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, dp(u), -1, vp(out)),
        "equal knots": lambda: lib.bms_squad(ctx.handle, dp(equal), n, vp(R), H, dp(u), m, vp(out)),
        "falling knots": lambda: lib.bms_squad(ctx.handle, dp(falling), n, vp(R), H, dp(u), m, vp(out)),
        "NaN knot": lambda: lib.bms_squad(ctx.handle, dp(t_nan), n, vp(R), H, dp(u), m, vp(out)),
        "infinite knot": lambda: lib.bms_squad(ctx.handle, dp(t_inf), n, vp(R), H, dp(u), m, vp(out)),
        "NaN argument": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, dp(u_nan), m, vp(out)),
        "infinite argument": lambda: lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, dp(u_inf), m, vp(out)),
    }
    for what, call in refused.items():
        rc = call()
        message = lib.bms_last_error(ctx.handle)
        assert rc == _lib.BMS_ERR_INVALID and message, (what, rc, message)
        assert np.isnan(out).all(), what  # (nothing was written)
        assert _same_bits(engine.squad(R, t, u, ctx=ctx), baseline), what
    assert lib.bms_squad(None, dp(t), n, vp(R), H, dp(u), m, vp(out)) == _lib.BMS_ERR_INVALID
    assert lib.bms_squad(ctx.handle, dp(t), n, vp(R), H, dp(u), 0, vp(out)) == 0 and np.isnan(out).all()  # no arguments: nothing to do
    with pytest.raises(ValueError, match="strictly increasing"):
        engine.squad(R, equal, u, ctx=ctx)
    with pytest.raises(ValueError):
        engine.squad(R, t[:-1], u, ctx=ctx)
    assert _same_bits(engine.squad(R, t, u, ctx=ctx), baseline)


def test_degenerate_sizes_answer_as_the_statement_does(ctx):
    import torch

    from scri_amd import device_series, engine

    dev = device_series.attach(ctx)
    c = st.cases()["uniform", 5]
    t, R, u = c["t"], c["R"], c["u"]
    for Rk, tk, uk in ((R[:1], t[:1], u), (R[:0], t[:0], u), (R, t, u[:0]), (R[:1], t[:1], u[:0]), (np.zeros((0, 4)), [], [])):
        want = quaternions.squad(Rk, tk, uk)
        got = engine.squad(Rk, tk, uk, ctx=ctx)
        assert isinstance(got, np.ndarray) and _same_bits(got, want), (Rk.shape, np.shape(uk))
        got_dev = engine.squad(torch.from_numpy(np.array(Rk, dtype=float)).to(dev), tk, uk, ctx=ctx)
        assert got_dev.is_cuda and _same_bits(got_dev.cpu().numpy(), want), (Rk.shape, np.shape(uk))
    # two rotors: the smallest series the kernels take, and a single argument
    want = quaternions.squad(R[:2], t[:2], u[:1])
    assert np.abs(engine.squad(R[:2], t[:2], u[:1], ctx=ctx) - want).max() <= G * EPS
