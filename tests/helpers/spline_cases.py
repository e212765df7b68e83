"""Inputs and the tolerance rule shared by tests/test_oracle_spline_exact.py, tests/test_gpu_spline_edges.py and
tools/series_sweep.py: time axes, the column signal, and the bar a result of the series calculus is held to.

The rule.  For one call with result `got`, the extended-precision result `exact` (oracle/spline_exact.py) and the fp64 yardstick
`ref` (scipy through oracle/modes_time_series_ref.py, or oracle/mode_calculations_ref.py):
    E_got = max|got - exact|,  E_ref = max|ref - exact|,  scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale).
F and G are set per family from the measured worst ratios (next power of two above twice the worst), under the caps F <= 32 and
G <= 256, which are conditions and not measurements: two fp64 evaluations of one conditioned quantity by equivalent formulas differ by
a modest factor, while the defects looked for are orders of magnitude larger (a run-in cut short >= 2e-10 relative; a lost tile
carry, a neighbouring column or a stale row O(1))."""
import numpy as np

EPS = float(np.finfo(float).eps)
F_CAP, G_CAP = 32.0, 256.0

# family -> (F, G): the next power of two above twice the worst ratio measured on an MI355X over every call of
# tests/test_gpu_spline_edges.py (its docstring has the figures and where they occurred).  "anti": bms_spline_derivative of order
# -16 .. -1, "value": order 0, "d1" .. "d3": orders 1 .. 3, "cubic": bms_cubic_spline, "av": <Ldt>, <LL>, omega and the principal
# axis of bms_angular_velocity and its callers.
#                 worst E_got / E_ref    worst E_got / (eps scale) where E_ref < 4 eps scale
RULE = {
    "anti": (16.0, 16.0),   # 4.02                   5.64
    "value": (4.0, 8.0),    # 1.73                   2.62
    "d1": (8.0, 16.0),      # 2.18                   5.59
    "d2": (16.0, 16.0),     # 5.09                   4.46
    "d3": (8.0, 16.0),      # 2.05                   4.95
    "cubic": (4.0, 8.0),    # 1.48                   2.82
    "av": (4.0, 8.0),       # 1.42                   3.19
}


def family_of(order):
    return "anti" if order < 0 else ("value" if order == 0 else f"d{order}")


def errors(got, exact, ref):
    """(E_got, E_ref, scale) of the rule, as floats"""
    exact = np.asarray(exact)
    e_got = float(np.abs(np.asarray(got) - exact).max())
    e_ref = float(np.abs(np.asarray(ref) - exact).max())
    return e_got, e_ref, max(1.0, float(np.abs(exact).max()))


def bar(family, e_ref, scale, at_the_caps=False):
    """The rule's bar.  at_the_caps: with F and G at their caps instead of the family's measured constants (tools/series_sweep.py, whose
    random shapes are not the ones the constants were measured on)."""
    F, G = (F_CAP, G_CAP) if at_the_caps else RULE[family]
    assert F <= F_CAP and G <= G_CAP
    return max(F * e_ref, G * EPS * scale)


def check(family, got, exact, ref, what):
    """Assert the rule for one call; prints the figures first (pytest -s shows them) and returns the bar."""
    got = np.asarray(got)
    assert got.shape == np.asarray(exact).shape, (what, got.shape, np.asarray(exact).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result (a row or column nobody wrote?)"
    e_got, e_ref, scale = errors(got, exact, ref)
    b = bar(family, e_ref, scale)
    print(f"RULE {family} E_got={e_got:.3e} E_ref={e_ref:.3e} scale={scale:.3e} got/ref={e_got / max(e_ref, 1e-300):.3g} "
          f"got/eps={e_got / (EPS * scale):.3g} | {what}")
    assert e_got <= b, f"{what}: E_got = {e_got:.3e} > bar {b:.3e} (E_ref = {e_ref:.3e}, scale = {scale:.3e})"
    return b


# ---- axes (span about 12, so that the 16-fold antiderivative stays near 1e4)
def uniform_axis(n):
    return np.linspace(-3.0, 9.0, n)


def jittered_axis(n, seed=0):
    t = np.linspace(-3.0, 9.0, n)
    return t + np.random.default_rng(1000 + seed).uniform(-0.3, 0.3, n) * (t[1] - t[0])


def axis_from_steps(steps, t0=-3.0):
    return t0 + np.concatenate([[0.0], np.cumsum(np.asarray(steps, dtype=float))])


def signal(t, n_cols, seed=0):
    """Column c carries a_c exp(i w_c t) (1 + 0.05 t) with distinct w_c in [0.3, 2]: a swapped or shared column shows."""
    rng = np.random.default_rng(2000 + seed)
    w = rng.permutation(np.linspace(0.3, 2.0, n_cols)) if n_cols > 1 else np.array([1.1])
    a = rng.normal(size=n_cols) + 1j * rng.normal(size=n_cols)
    t = np.asarray(t, dtype=float)[:, None]
    return a[None, :] * np.exp(1j * w[None, :] * t) * (1 + 0.05 * t)
