"""Seeded sweep of the time-series calculus and the grid product (bms_spline_derivative,
bms_cubic_spline, bms_grid_multiply) against the oracle at RANDOM sizes: series of 4 .. 40 000 samples on
uniform, jittered and graded axes (the spline kernels work in 320-knot tiles with a 32-knot run-in: the sizes in the suite are a few
fixed ones), derivative orders -16 .. 3, 1 .. 300 columns, evaluation points inside, on the knots, outside and unordered; grid products
of random spins, l ranges, working and output l, 1 .. 3 000 rows.
The spline results are held to the rule of tests/helpers/spline_cases.py: their distance from the extended-precision reference
(oracle/spline_exact.py) against F times scipy's own distance from it, or G eps of the scale -- no widening by the mesh, no factor per
order -- with F = 32 and G = 256, the caps of the rule (the constants of the suite are measured on the suite's shapes).  The worst
ratios of the run are printed per family at the end.
Usage: python tools/series_sweep.py [last_seed [first_seed]]   (prints failures; exit code = their number)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import scri_amd
from oracle import modes_time_series_ref as mref
from oracle import spline_exact as sx
from scri_amd import engine
from tests.helpers import spline_cases as sc

DONE = {"spline calculus cases": 0, "cubic spline cases": 0, "grid products": 0}
WORST = {}  # family -> [worst E_got / E_ref, worst E_got / (eps scale) over calls with E_ref < 4 eps scale, where]


def _rule(family, got, exact, ref, what):
    """None if `got` is within the rule, else the complaint; keeps the worst ratios"""
    if got.shape != exact.shape or not np.isfinite(got).all():
        return f"{family}: shape or non-finite values"
    e_got, e_ref, scale = sc.errors(got, exact, ref)
    w = WORST.setdefault(family, [0.0, 0.0, "", ""])
    if e_ref > 0 and e_got / e_ref > w[0]:
        w[0], w[2] = e_got / e_ref, what
    if e_ref < 4 * sc.EPS * scale and e_got / (sc.EPS * scale) > w[1]:
        w[1], w[3] = e_got / (sc.EPS * scale), what
    bar = sc.bar(family, e_ref, scale, at_the_caps=True)
    return None if e_got <= bar else f"{family}: E_got {e_got:.2e} > bar {bar:.2e} (E_ref {e_ref:.2e}, scale {scale:.2e})"


def _axis(rng, n):
    kind = int(rng.integers(4))
    if kind == 0:
        t = np.linspace(-3.0, 9.0, n)
    elif kind == 1:  # jittered
        t = np.linspace(-3.0, 9.0, n)
        if n > 1:
            t = t + rng.uniform(-0.3, 0.3, n) * (t[1] - t[0])
    elif kind == 2:  # random samples
        t = np.sort(rng.uniform(-3.0, 9.0, n)) + np.arange(n) * 1e-6
    else:  # steps shrinking geometrically by up to 30x
        r = rng.uniform(3.0, 30.0) ** (-1.0 / max(n - 1, 1))
        t = -3.0 + np.concatenate([[0.0], np.cumsum(r ** np.arange(n - 1))])
        t = -3.0 + (t + 3.0) * 12.0 / max(t[-1] + 3.0, 1e-300)
    return t, kind


def _signal(rng, t, ncols):
    w = rng.uniform(0.3, 2.0, ncols)
    a = rng.normal(size=ncols) + 1j * rng.normal(size=ncols)
    return a[None, :] * np.exp(1j * w[None, :] * t[:, None]) * (1 + 0.05 * t[:, None])


def one(seed, ctx):
    rng = np.random.default_rng(55_000 + seed)
    bad = []
    # ---- spline calculus
    ncols = int(rng.integers(1, 301))
    n = int(10 ** rng.uniform(np.log10(4), np.log10(40_000)))
    n = max(4, min(n, 400_000 // ncols))  # (the extended reference keeps 16 levels of knot values: bounded memory)
    t, kind = _axis(rng, n)
    y = _signal(rng, t, ncols)
    order = int(rng.integers(-16, 4))
    n_new = int(rng.integers(1, 3_000))
    # (samples up to two steps outside the data: extrapolation, as scipy does it)
    tn = rng.uniform(t[0] - 2 * (t[1] - t[0]), t[-1] + 2 * (t[-1] - t[-2]), n_new)
    tn[: min(n_new, 20)] = t[rng.integers(0, n, min(n_new, 20))]  # on knots
    what = f"seed {seed}: n={n} cols={ncols} axis={kind} order={order} n_new={n_new}"
    try:
        got = engine.spline_derivative(t, y, tn, order, ctx=ctx)
        ref = mref.interpolate(t, y, tn, order)
        DONE["spline calculus cases"] += 1
        complaint = _rule(sc.family_of(order), got, sx.evaluate(t, y, tn, order), ref, what)
        if complaint:
            bad.append("spline_derivative " + complaint)
    except Exception as e:  # noqa: BLE001
        # the oracle (scipy) and the engine must agree on what they refuse: both raise, or neither
        try:
            mref.interpolate(t, y, tn, order)
            bad.append(f"spline_derivative raised {type(e).__name__}: {str(e)[:120]}")
        except Exception:  # noqa: BLE001
            pass
    # ---- cubic spline (interpolation only, its own entry point)
    try:
        ts = np.sort(tn)
        got = engine.cubic_spline(t, y, ts, ctx=ctx)
        ref = mref.interpolate(t, y, ts, 0)
        DONE["cubic spline cases"] += 1
        complaint = _rule("cubic", got, sx.evaluate(t, y, ts, 0), ref, what)
        if complaint:
            bad.append("cubic_spline " + complaint)
    except Exception as e:  # noqa: BLE001
        try:
            mref.interpolate(t, y, np.sort(tn), 0)
            bad.append(f"cubic_spline raised {type(e).__name__}: {str(e)[:120]}")
        except Exception:  # noqa: BLE001
            pass
    # ---- grid product
    sa, sb = int(rng.integers(-2, 3)), int(rng.integers(-2, 3))
    la, lb = int(rng.integers(abs(sa), 11)), int(rng.integers(abs(sb), 11))
    rows = int(10 ** rng.uniform(0, np.log10(3_000)))
    a = rng.normal(size=(rows, (la + 1) ** 2)) + 1j * rng.normal(size=(rows, (la + 1) ** 2))
    b = rng.normal(size=(rows, (lb + 1) ** 2)) + 1j * rng.normal(size=(rows, (lb + 1) ** 2))
    a[:, : sa * sa] = 0
    b[:, : sb * sb] = 0
    W = max(1, int(rng.integers(max(la, lb), la + lb + 1)))  # (a working l of 0 is a one-point grid: refused by the engine)
    Lout = int(rng.integers(min(abs(sa + sb), W), W + 1))  # (0 <= output l <= working l is the engine's precondition)
    if rows * (2 * W + 1) ** 2 < 3e6:
        got = engine.grid_multiply(a, sa, la, b, sb, lb, W, Lout, ctx=ctx)
        ref = mref.grid_multiply(a, sa, la, b, sb, lb, W, Lout)
        DONE["grid products"] += 1
        err = np.abs(got - ref).max()
        if got.shape != ref.shape or not err < 3e-13 * max(1.0, np.abs(ref).max()):
            bad.append(f"grid_multiply s=({sa},{sb}) l=({la},{lb}) W={W} Lout={Lout} rows={rows}: {err:.2e}")
    return bad, what


def main():
    last = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    ctx = scri_amd.Context(0)
    failures = 0
    for seed in range(first, last):
        try:
            bad, what = one(seed, ctx)
        except Exception as e:  # noqa: BLE001
            bad, what = [f"{type(e).__name__}: {str(e)[:300]}"], f"seed {seed}"
        if bad:
            failures += 1
            print("FAILED", what, "|", "; ".join(bad), flush=True)
    print("checked:", DONE)
    for family, (r_ref, r_eps, at_ref, at_eps) in sorted(WORST.items()):
        print(f"worst {family}: E_got / E_ref = {r_ref:.3g} ({at_ref}); E_got / (eps scale) = {r_eps:.3g} ({at_eps})")
    print("done, failures:", failures)
    return failures


if __name__ == "__main__":
    sys.exit(min(main(), 100))
