"""Case tables, the exact reference, the launchers' arithmetic restated and the rule's constants of
tests/test_oracle_time_spline_exact.py (no GPU) and tests/test_gpu_time_spline_edges.py: the per-pixel not-a-knot spline along time
of the BMS transformation, evaluated OFF its knots at each pixel's own skewed time, held to oracle/waveform_grid_ref.py from_modes
restated in extended precision.

The rule is the project's (tests/helpers/spline_cases.py).  For one call with result `got`, the extended-precision result `exact`
(exact_from_modes below) and the fp64 yardstick `ref` (oracle/waveform_grid_ref.py from_modes itself, scipy's splines included):
    E_got = max|got - exact|,  E_ref = max|ref - exact|,  scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured,
and the bar of every case stays below BAR_CAP = 1e-12 scale, half of what the transforms were held to before (a loose E_ref must not
hide a defect; the bar depends on E_ref only, so tests/test_oracle_time_spline_exact.py checks it without a GPU)."""
import functools
import warnings

import numpy as np

from oracle import containers, quat, wigner
from oracle import spline_exact as sx
from oracle import waveform_grid_ref as grid_ref
from tests.helpers import synthesis_cases as sy
from tests.helpers.spline_cases import EPS, F_CAP, G_CAP, errors

LD, CLD = np.longdouble, np.clongdouble
BAR_CAP = 1e-12

# family -> (F, G): the next power of two above twice the worst ratio measured on an MI355X over every call of
# tests/test_gpu_time_spline_edges.py (its docstring has the figures and where they occurred).  The family is the ROUTE of the call
# (ROUTES below; A3'' counts under A3, whose kernels it runs, and group C under A1); "graded": every route on the axes of the family
# "graded under the guard", on the rows beside the seam (graded_rows); "modes": group B; "abd": group D.
# No family needs the caps and no kernel was changed.  The graded family stays within 7.4 eps x scale at its seams (6.6 next to the
# run-in of the 320-knot elimination tile, on the stretch of ratio 1.15 over 47 steps): a halo of 32 knots has forgotten its start
# on every axis the guard lets through that these tables hold.
#                     worst E_got / E_ref    worst E_got / (eps scale) where E_ref < 4 eps scale
RULE = {
    "A1": (16.0, 32.0),      # 4.92                   9.21
    "A2": (8.0, 16.0),       # 2.76                   6.79
    "A3": (8.0, 16.0),       # 2.02                   5.90
    "A3'": (8.0, 16.0),      # 2.02                   5.90
    "A4": (4.0, 16.0),       # 1.97                   5.70
    "A5": (4.0, 8.0),        # 1.42                   2.61
    "A5'": (4.0, 16.0),      # 1.87                   4.20
    "A6": (4.0, 8.0),        # 1.11                   3.73
    "A6b": (8.0, 32.0),      # 2.25                   8.53
    "graded": (8.0, 16.0),   # 2.32                   6.59
    "modes": (4.0, 16.0),    # 1.76                   5.51
    "abd": (8.0, 16.0),      # 2.20                   5.36
}


def bar(family, e_ref, scale):
    F, G = RULE[family]
    assert F <= F_CAP and G <= G_CAP
    return max(F * e_ref, G * EPS * scale)


def check(family, got, exact, ref, what):
    """Assert the rule for one call; prints the figures first (pytest -s shows them) and returns the bar."""
    got = np.asarray(got)
    assert got.shape == np.asarray(exact).shape, (what, got.shape, np.asarray(exact).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result (a row or pixel nobody wrote?)"
    e_got, e_ref, scale = errors(got, exact, ref)
    b = bar(family, e_ref, scale)
    print(f"RULE {family} E_got={e_got:.3e} E_ref={e_ref:.3e} scale={scale:.3e} got/ref={e_got / max(e_ref, 1e-300):.3g} "
          f"got/eps={e_got / (EPS * scale):.3g} | {what}")
    assert b < BAR_CAP * scale, f"{what}: the bar {b:.3e} is not below {BAR_CAP:g} x scale -- change the case's inputs, not the rule"
    if e_got > b:
        r, p = np.unravel_index(int(np.argmax(np.abs(got - np.asarray(exact)))), got.shape)
        raise AssertionError(f"{what}: E_got = {e_got:.3e} > bar {b:.3e} (E_ref = {e_ref:.3e}, scale = {scale:.3e}); worst at row {r}, column {p}")
    return b


# ------------------------------------------------------------------------------------------------ the launchers' arithmetic
SPLINE_TILE, SPLINE_HALO = 320, 32   # bspline_forward_modes_kernel / bspline_backward_modes_kernel as the engine launches them
SOLVE_TILE, SOLVE_RUN_IN = 48, 32    # bspline_solve_modes_kernel<48, 32>
BACKWARD_TILES = (96, 160, 320, 640)
RING = 8                             # rows a wave of bspline_backward_eval_kernel parks before its lanes' stores
GUARD_RATIO, GUARD_BLOCK = 1e3, 16   # spline_tile_for / walk_time_axis: step range over three blocks of 16 steps


def backward_tile(n_cols, n_rows, cus):
    """launch_bspline_backward_eval's cost model (kernels_bspline.hip): the cheapest of 96 / 160 / 320 / 640, ties to the first"""
    slots = 16 * cus
    best, tile = 1e300, None
    for t in BACKWARD_TILES:
        waves = ((n_cols + 63) // 64) * ((n_rows + t - 1) // t)
        cost = ((waves + slots - 1) // slots + 0.25) * (t + SPLINE_HALO)
        if cost < best:
            best, tile = cost, t
    return tile


def solve_tiles(n_rows, n_modes=12, with_ones=1):
    """(row tiles, tiles per XCD, workgroups) of launch_bspline_solve_modes"""
    ncb = (2 * (n_modes + with_ones) + 63) // 64
    n_tiles = (n_rows + SOLVE_TILE - 1) // SOLVE_TILE
    per_xcd = (n_tiles + 7) // 8
    return n_tiles, per_xcd, 8 * per_xcd * ncb


def forward_tiles(n_rows):
    return (n_rows + SPLINE_TILE - 1) // SPLINE_TILE


def eval_blocks(rows, step=64):
    """row tiles of the evaluating product and, with 64-row steps, the boundaries between them (tests/test_gpu_dense_product_small.py)"""
    return 2 * ((rows + 63) // 64) - 1 if step == 64 else (rows - 3 + 60) // 61


def regular_axis(t):
    """spline_tile_for (engine_tables.hip): False where the steps vary more than 1e3-fold within three consecutive blocks of 16 --
    such an axis takes the exact single-tile recurrences"""
    h = np.diff(np.asarray(t, dtype=float))
    mins, maxs = [], []
    for b0 in range(0, h.size, GUARD_BLOCK):
        blk = h[b0 : b0 + GUARD_BLOCK]
        mins.append(blk.min())
        maxs.append(blk.max())
        if max(maxs[-3:]) > GUARD_RATIO * min(mins[-3:]):
            return False
    return True


def window_variation(t, width=48):
    """largest ratio of two steps within `width` consecutive steps"""
    h = np.diff(np.asarray(t, dtype=float))
    return max(h[i : i + width].max() / h[i : i + width].min() for i in range(max(1, h.size - width + 1)))


def skews(alpha, k, gamma, tt):
    """(skew_a, skew_b) per pixel: output sample i of pixel p is the spline at x_i + skew_a (x_i - tt) + skew_b, i.e. at
    uprm_i / k_p + alpha_p with uprm_i = (x_i - tt) / gamma"""
    return 1.0 / (gamma * np.asarray(k, dtype=float)) - 1.0, np.asarray(alpha, dtype=float) - tt


def skew_spread(skew_a, skew_b):
    """skew_spread (engine_tables.hip): the largest range of the skew rate and of the skew offset within a block of 64 columns"""
    ra = rb = 0.0
    for c0 in range(0, len(skew_a), 64):
        ra = max(ra, float(np.ptp(skew_a[c0 : c0 + 64])))
        rb = max(rb, float(np.ptp(skew_b[c0 : c0 + 64])))
    return ra, rb


def fits(x, tt, rate_range, offset_range, tile, y, g0=0, n_rows=None):
    """launch_bspline_backward_eval's `fits` for tile y: may the march read its abscissae from the staged window?"""
    n_rows = len(x) - g0 if n_rows is None else n_rows
    jA = g0 + y * tile
    jB = min(g0 + n_rows, jA + tile)
    if jB - jA < 2:
        return False
    xm = max(abs(x[jA] - tt), abs(x[jB - 1] - tt))
    dx = (x[jB - 1] - x[jA]) / (jB - 1 - jA)
    return bool(dx > 0 and rate_range * xm + offset_range <= 10.0 * dx)


def backward_launches(x, tt, rate_range, offset_range, tile, g0=0, n_rows=None):
    """(launches of bspline_backward_eval_kernel, fits() per tile): one launch per run of tiles with the same answer"""
    n_rows = len(x) - g0 if n_rows is None else n_rows
    f = [fits(x, tt, rate_range, offset_range, tile, y, g0, n_rows) for y in range((n_rows + tile - 1) // tile)]
    return 1 + sum(a != b for a, b in zip(f, f[1:])), f


# ------------------------------------------------------------------------------------------------ inputs
ELL_MIN, ELL_MAX = 2, 3
N_MODES = 12
def base_step(n):
    return min(0.1, 20.0 / (n - 1))


def axis(kind, n):
    """|t| of order 10: starts at -8, steps of 0.1 (less from 200 rows on, so that the axis ends at 12).  Fewer than 40 rows start at
    -0.2 instead: under a boost the pixels' own times k (t - alpha) differ by 2 % of |t|, and at |t| = 8 that is more than such a
    series is long -- no output row would be left."""
    dt = base_step(n)
    T0 = -8.0 if n >= 40 else -0.2
    if kind == "uniform":
        h = np.full(n - 1, dt)
    elif kind == "jitter":
        x = T0 + dt * np.arange(n) + np.random.default_rng(3000 + n).uniform(-0.3, 0.3, n) * dt
        return x
    elif kind == "alternating":
        h = np.where(np.arange(n - 1) % 2 == 0, 0.2, 0.01) * (dt / 0.105)
    else:
        raise ValueError(kind)
    return T0 + np.concatenate([[0.0], np.cumsum(h)])


def graded_axis(n, seam, ratio, steps, grow):
    """Family "graded under the guard": steps of `big` = 0.1 on one side of row `seam`, of big / ratio^steps on the other, and a
    geometric stretch of `steps` steps between them that ends (grow: the forward run-in sees it) or begins (the backward run-in)
    at the seam.  t = 0 at the seam, so that |t| is small where the steps are."""
    big = 0.1
    small = big / ratio**steps
    j = np.arange(n - 1)  # step j lies between rows j and j + 1
    if grow:
        e = np.clip(j - (seam - steps), 0, steps)       # small ... growing over rows seam - steps .. seam ... big
    else:
        e = np.clip((seam + steps) - 1 - j, 0, steps)   # big ... shrinking over rows seam .. seam + steps ... small
    h = small * ratio**e.astype(float)
    x = np.concatenate([[0.0], np.cumsum(h)])
    return x - x[seam]


def rough_signal(t, n_modes, seed):
    """the signal of test_bspline_path_on_short_and_irregular_time_axes: oscillations of order one plus 5 % noise per sample, so that a
    wrong row, a neighbour's column or a sample one row off is an O(0.05) error"""
    rng = np.random.default_rng(seed)
    n = len(t)
    data = (np.sin(np.outer(t, rng.uniform(0.5, 3.0, size=n_modes))) + 1j * np.cos(np.outer(t, rng.uniform(0.5, 3.0, size=n_modes)))) * rng.normal(size=n_modes)
    return data + 0.05 * (rng.normal(size=(n, n_modes)) + 1j * rng.normal(size=(n, n_modes)))


def real_supertranslation(coeffs):
    """alpha_lm of a real function from arbitrary complex coefficients (l = 0 .. L)"""
    a = np.array(coeffs, dtype=complex)
    L = int(round(np.sqrt(a.size))) - 1
    for ell in range(L + 1):
        for m in range(ell + 1):
            ip, im = wigner.LM_index(ell, m, 0), wigner.LM_index(ell, -m, 0)
            a[ip] = (a[ip] + (-1.0) ** m * np.conj(a[im])) / 2
            a[im] = (-1.0) ** m * np.conj(a[ip])
    return a


@functools.lru_cache(maxsize=None)
def _unit_supertranslation():
    """l = 1, 2 coefficients of a real function whose range over the sphere is 1 (measured on a 61 x 120 grid, to 1e-3)"""
    rng = np.random.default_rng(77)
    a = real_supertranslation(rng.normal(size=9) + 1j * rng.normal(size=9))
    a[0] = 0.0
    th, ph = np.meshgrid(np.linspace(0, np.pi, 61), np.linspace(0, 2 * np.pi, 120, endpoint=False), indexing="ij")
    val = np.tensordot(a, wigner.swsh_grid(quat.from_spherical_coords(th, ph).reshape(-1, 4), 0, 2), axes=([0], [1])).real
    return a / np.ptp(val)


def supertranslation(size, time_shift):
    """l <= 2: a time translation `time_shift` plus a direction-dependent part whose alpha has the range `size` over the sphere"""
    a = size * _unit_supertranslation()
    a[0] = time_shift * np.sqrt(4 * np.pi)
    return a


BOOST = np.array([0.01, -0.02, 0.015])
ROTATION = np.array([0.8, 0.2, -0.5, 0.1]) / np.linalg.norm([0.8, 0.2, -0.5, 0.1])

# route -> (options set to 1 or to the value given, boosted?)
ROUTE_OPTIONS = ("SCRI_AMD_NO_SMALL_DENSE", "SCRI_AMD_NO_SYNTHESIS_EVAL", "SCRI_AMD_SYNTHESIS_EVAL", "SCRI_AMD_TWO_SWEEPS", "SCRI_AMD_GEMM_EVAL_STEP",
                 "SCRI_AMD_NO_GEMM_EVAL", "SCRI_AMD_NO_BSPLINE")
ROUTES = {
    "A1": ({"SCRI_AMD_NO_SMALL_DENSE": 1, "SCRI_AMD_NO_SYNTHESIS_EVAL": 1}, False),
    "A2": ({"SCRI_AMD_NO_SMALL_DENSE": 1, "SCRI_AMD_SYNTHESIS_EVAL": 1}, False),
    "A3": ({}, True),
    "A3'": ({"SCRI_AMD_TWO_SWEEPS": 1}, True),
    "A3''": ({"SCRI_AMD_GEMM_EVAL_STEP": 61}, True),
    "A4": ({"SCRI_AMD_NO_GEMM_EVAL": 1}, True),
    "A5": ({"SCRI_AMD_NO_BSPLINE": 1}, True),
    "A5'": ({}, True),
    "A6": ({}, True),                                # psi3 with its psi4 companion, boosted: elimination on the grid columns
    "A6b": ({"SCRI_AMD_NO_SMALL_DENSE": 1}, False),  # ... without a boost: elimination on the modes
}

# the lengths that are seams of each kernel
N_BACKWARD_96 = (97, 98, 99, 100, 101, 193, 194)
N_SOLVE_48 = (47, 48, 49, 81, 384, 385, 433)
N_FORWARD_320 = (320, 321, 352, 353, 641)
N_GROUPS = tuple(range(8, 16))
N_SLOPE = (4, 5, 6, 7)
GRIDS = (7, 9, 15)
AXES = ("uniform", "jitter", "alternating")

def _second_axis(route, n):
    """the alternating axis, except under a boost from 200 rows on.  There its short steps (0.003 .. 0.006 once the axis is scaled to
    end at 12) put the oracle itself 300 .. 970 eps x scale from the exact result -- the fp64 rounding of k (t - alpha), |t| eps, times
    a slope of 0.05 per short step -- and F x E_ref would pass 1e-12 x scale: those cases take the jittered axis.  The long
    alternating axes stay with the boost-free routes, which run the same elimination (A1) and solve (A2) kernels."""
    return "jitter" if ROUTES[route][1] and n >= 200 else "alternating"


def _two_axes(route, lengths, grid=7, size=0.5):
    return [(route, n, grid, ax, size) for n in lengths for ax in ("uniform", _second_axis(route, n))]


# (route, n, grid, axis kind, supertranslation range in steps)
A_CASES = (
    _two_axes("A1", N_BACKWARD_96 + N_FORWARD_320 + N_GROUPS)
    + [("A1", n, g, "jitter", 0.5) for n in (100, 353) for g in (9, 15)]
    + _two_axes("A2", N_SOLVE_48 + N_GROUPS)
    + [("A2", 385, g, "jitter", 0.5) for g in (9, 15)]
    + _two_axes("A3", N_SOLVE_48 + N_GROUPS)
    + [("A3", n, g, "jitter", 0.5) for n in (81, 433) for g in (9, 15)]
    + _two_axes("A3'", N_FORWARD_320 + (9, 12))
    + [("A3''", n, 15, "jitter", 0.5) for n in (49, 433)]
    + _two_axes("A4", N_BACKWARD_96 + N_GROUPS)
    + [("A4", n, g, "jitter", 0.5) for n in (101, 194) for g in (9, 15)]
    + [c for g in (7, 9) for c in _two_axes("A5", (9, 100, 321), g)]
    + [("A5'", n, 7, ax, 0.5) for n in N_SLOPE for ax in ("uniform", "jitter")]
    + [c for r in ("A6", "A6b") for c in _two_axes(r, (9, 97, 100, 321, 353))]
    # supertranslation sizes: both instances of bspline_backward_eval_kernel and the ring's overflow
    + [(r, n, 9, "uniform", size) for r in ("A1", "A4", "A6", "A6b") for n in (100, 194) for size in (9.0, 30.0)]
)

# family "graded under the guard": (route, n, seam row, ratio, steps, grows towards the seam?)
GRADED = [(r, seam + 70, seam, ratio, steps, grow)
          for r, seam in (("A1", 96), ("A1", 320), ("A3", 48), ("A3'", 320), ("A4", 96))
          for ratio, steps in ((1.3, 25), (1.15, 47))
          for grow in (True, False)]

# the boost under which skew_rate_range |x - tt| crosses 10 dt inside the series (A4): the early tiles fit, the late ones do not
SPLIT_CASE = ("A4", 385, 9, "uniform", 0.5)
SPLIT_BOOST = 25.0 * BOOST


def case_id(c):
    return "-".join(str(v) for v in c)


# ------------------------------------------------------------------------------------------------ the exact reference
def _ld_rotate_z(R):
    w, x, y, z = (R[:, i].astype(LD) for i in range(4))
    n2 = w * w + x * x + y * y + z * z
    return np.stack([2 * (x * z + w * y), 2 * (y * z - w * x), w * w - x * x - y * y + z * z]) / n2  # [3, n_pix]


def _ld_eth(modes, s, ell_min=0):
    """oracle.wigner.eth_GHP with the factors in extended precision"""
    out = np.zeros(len(modes), dtype=CLD)
    L = int(round(np.sqrt(len(modes) + ell_min**2))) - 1
    for ell in range(ell_min, L + 1):
        f = np.sqrt(LD((ell - s) * (ell + s + 1))) if ell >= abs(s) and ell >= abs(s + 1) else LD(0)
        i0 = wigner.LM_index(ell, -ell, ell_min)
        out[i0 : i0 + 2 * ell + 1] = f / np.sqrt(LD(2)) * np.asarray(modes[i0 : i0 + 2 * ell + 1]).astype(CLD)
    return out


def _ld_ethbar(modes, s, ell_min=0):
    out = np.zeros(len(modes), dtype=CLD)
    L = int(round(np.sqrt(len(modes) + ell_min**2))) - 1
    for ell in range(ell_min, L + 1):
        f = -np.sqrt(LD((ell + s) * (ell - s + 1))) if ell >= abs(s) and ell >= abs(s - 1) else LD(0)
        i0 = wigner.LM_index(ell, -ell, ell_min)
        out[i0 : i0 + 2 * ell + 1] = f / np.sqrt(LD(2)) * np.asarray(modes[i0 : i0 + 2 * ell + 1]).astype(CLD)
    return out


def evaluate_per_column(x, y, s, u):
    """The spline through (x[n], y[n, P]) with knot slopes s[n, P] at the abscissae u[m, P], column p at its own u[:, p]: the
    interval's cubic of oracle/spline_exact.py evaluate (order 0), in extended precision."""
    x = x.astype(LD)
    n = x.shape[0]
    j = np.clip(np.searchsorted(x, u.ravel(), side="right").reshape(u.shape) - 1, 0, n - 2)
    h = np.diff(x)[:, None]
    Dh = np.diff(y, axis=0) / h
    c3 = (s[:-1] + s[1:] - 2 * Dh) / (h * h)
    c2 = (Dh - s[:-1]) / h - c3 * h
    tl = u - x[j]
    take = lambda c: np.take_along_axis(c, j, axis=0)  # noqa: E731
    return ((take(c3) * tl + take(c2)) * tl + take(s[:-1])) * tl + take(y[:-1])


def exact_from_modes(w, **kwargs):
    """oracle/waveform_grid_ref.py from_modes (scri/waveform_grid.py:331-613) in extended precision.  The rotors are the oracle's
    (fp64: they are input), the harmonics oracle/wigner.py's with their recurrences in np.longdouble; alpha, k, the grid series with
    its h / sigma term, the psi mixing and k^w are accumulated in np.clongdouble; the per-pixel spline is oracle/spline_exact.py's on
    the INPUT axis t, evaluated at t* = uprm_i' / k_p + alpha_p -- the reference's spline on the knots k (t - alpha) under an affine
    change of variable.  uprm_i' are the fp64 output times the oracle reports.
    Returns (uprm_iprm [N'], exact [N', n_pix] clongdouble, ref [N', n_pix] complex128 (from_modes itself), alpha [n_pix], k [n_pix], gamma, tt)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)  # (a grid that does not resolve the supertranslation: the tests choose it small)
        t_ref, ref, n_theta, n_phi = grid_ref.from_modes(w, **{k_: (v.copy() if hasattr(v, "copy") else v) for k_, v in kwargs.items()})
        (st, lst, ell_max, n_theta, n_phi, v, beta, gamma, varphi, R, rest) = grid_ref.process_transformation_kwargs(w.ell_max, **dict(kwargs))
    R = R.reshape(-1, 4)
    s = w.spin_weight
    t = np.asarray(w.t, dtype=float)
    Y = wigner.swsh_grid(R, s, ell_max)
    SH = wigner.swsh_grid(R, 0, lst)
    vL = v.astype(LD)
    gammaL = 1 / np.sqrt(1 - (vL * vL).sum())
    r = _ld_rotate_z(R)
    k = 1 / (gammaL * (1 - vL @ r))
    alpha = sy.exact_product(st[None, :], SH)[0].real
    lo, hi = wigner.LM_index(w.ell_min, -w.ell_min, 0), wigner.LM_index(w.ell_max, w.ell_max, 0) + 1
    f = sy.exact_product(w.data, Y[:, lo:hi])  # [n, n_pix]
    if beta != 0 or (st[1:] != 0).any():
        n_st = wigner.LM_index(lst, lst, 0) + 1
        if w.dataType == containers.h:
            f = f - sy.exact_product((2 * _ld_ethbar(_ld_ethbar(st, 0), -1))[None, :], Y[:, :n_st])
        elif w.dataType == containers.sigma:
            f = f - sy.exact_product(_ld_eth(_ld_eth(st, 0), 1)[None, :], Y[:, :n_st])
        elif w.dataType in (containers.psi0, containers.psi1, containers.psi2, containers.psi3):
            eth_alpha = sy.exact_product((_ld_eth(st, 0) / np.sqrt(LD(2)))[None, :], wigner.swsh_grid(R, 1, lst))[0]
            pi = wigner._PI
            vdr = np.array([0, (vL[0] + 1j * vL[1]) * np.sqrt(2 * pi / 3), vL[2] * np.sqrt(4 * pi / 3) + 0j, (-vL[0] + 1j * vL[1]) * np.sqrt(2 * pi / 3)], dtype=CLD)
            eth_v = sy.exact_product((vdr / np.sqrt(LD(2)))[None, :], wigner.swsh_grid(R, 1, 1))[0]
            X = (t.astype(LD)[:, None] - alpha[None, :]) * gammaL * k[None, :] * eth_v[None, :] - eth_alpha[None, :]
            for DT in range(w.dataType + 1, containers.psi4 + 1):
                w_tmp = kwargs["psi{}_modes".format(containers.DataNames[DT][-1])]
                Yt = wigner.swsh_grid(R, w_tmp.spin_weight, w_tmp.ell_max)
                ft = sy.exact_product(w_tmp.data, Yt[:, wigner.LM_index(w_tmp.ell_min, -w_tmp.ell_min, 0) : wigner.LM_index(w_tmp.ell_max, w_tmp.ell_max, 0) + 1])
                c = 1
                for q in range(DT - w.dataType):  # comb(5 - dataType, 5 - DT) = comb(5 - dataType, DT - dataType)
                    c = c * (5 - w.dataType - q) // (q + 1)
                f = f + c * ft * X ** (DT - w.dataType)
    f = f * (k ** int(w.conformal_weight))[None, :]
    tt = st[0].real / np.sqrt(4 * float(np.pi))  # (fp64, as the oracle forms it: uprm below is the oracle's)
    u = t_ref.astype(LD)
    tstar = u[:, None] / k[None, :] + alpha[None, :]
    slopes = sx.slopes(t, f)
    exact = evaluate_per_column(t, f, slopes, tstar)
    ref = ref.reshape(t_ref.size, n_theta * n_phi)
    assert exact.shape == ref.shape
    return t_ref, exact, ref, alpha.astype(float), k.astype(float), float(gammaL), float(tt)


# ------------------------------------------------------------------------------------------------ the cases, built once
def transformation_of(route, dt, size, boost=None):
    """(supertranslation, frame rotation, boost velocity) of a case: a time translation by 0.37 steps, a direction-dependent part of
    `size` steps, one frame rotation, and the boost where the route asks for one"""
    st = supertranslation(size * dt, 0.37 * dt)
    v = (BOOST if boost is None else boost) if ROUTES[route][1] else np.zeros(3)
    return st, ROTATION, v


def data_type_of(route):
    return "psi3" if route.startswith("A6") else "h"


@functools.lru_cache(maxsize=None)
def _build(route, n, grid, t_key, size, dt, boost_key):
    t = np.frombuffer(t_key, dtype=float).copy()
    st, rot, v = transformation_of(route, dt, size, boost=None if boost_key is None else np.frombuffer(boost_key, dtype=float))
    name = data_type_of(route)
    data = rough_signal(t, N_MODES, 1000 + n)
    w = containers.WM(t=t, data=data, ell_min=ELL_MIN, ell_max=ELL_MAX, dataType=getattr(containers, name))
    kw = dict(supertranslation=st, frame_rotation=rot, boost_velocity=v, n_theta=grid, n_phi=grid)
    aux = None
    if name == "psi3":
        aux = containers.WM(t=t, data=rough_signal(t, N_MODES, 2000 + n), ell_min=ELL_MIN, ell_max=ELL_MAX, dataType=containers.psi4)
        kw["psi4_modes"] = aux
    t_out, exact, ref, alpha, k, gamma, tt = exact_from_modes(w, **kw)
    for a in (t, data, exact, ref):
        a.setflags(write=False)
    return dict(t=t, data=data, aux=None if aux is None else aux.data, st=st, rot=rot, v=v, w=w, kw=kw, t_out=t_out, exact=exact, ref=ref, alpha=alpha, k=k,
                gamma=gamma, tt=tt, name=name, grid=grid, route=route, n=n)


def build(route, n, grid, t, size, dt, boost=None):
    """One case: inputs, the exact result and the oracle's, computed once per process and left unchanged (read-only arrays)."""
    t = np.ascontiguousarray(t, dtype=float)
    return _build(route, int(n), int(grid), t.tobytes(), float(size), float(dt), None if boost is None else np.ascontiguousarray(boost, dtype=float).tobytes())


def build_case(case, boost=None):
    route, n, grid, ax, size = case
    return build(route, n, grid, axis(ax, n), size, base_step(n), boost=boost)


def build_graded(case):
    route, n, seam, ratio, steps, grow = case
    return build(route, n, 7, graded_axis(n, seam, ratio, steps, grow), 0.5, 0.1)


def other_data(b, which="data"):
    """other data of the same shape: the call a test makes first, so that a row or pixel nobody writes shows as this data's"""
    return rough_signal(b["t"], N_MODES, (5000 if which == "data" else 6000) + b["n"])


def spread_of(b):
    """(rate range, offset range) of the launcher's skew_spread, from the oracle's alpha and k"""
    return skew_spread(*skews(b["alpha"], b["k"], b["gamma"], b["tt"]))


def window_of(b):
    """(i_lo, i_hi): output row r of the case has input index i_lo + r"""
    u = (1 / b["gamma"]) * (b["t"] - b["tt"])
    i_lo = int(np.argmin(np.abs(u - b["t_out"][0])))
    assert np.abs(u[i_lo : i_lo + b["t_out"].size] - b["t_out"]).max() <= 4 * EPS * max(1.0, np.abs(u).max())
    return i_lo, i_lo + b["t_out"].size


ROW_MARGIN = SPLINE_HALO + 2


def needed_rows(t, skew_a, skew_b, tt, c0, c1):
    """needed_rows (engine_tables.hip): the input rows [g0, g1) a launch for output rows [c0, c1) runs on"""
    n = len(t)
    lo = min(t[c0] + (skew_a * (t[c0] - tt) + skew_b))
    hi = max(t[c1 - 1] + (skew_a * (t[c1 - 1] - tt) + skew_b))
    ja = max(int(np.searchsorted(t, lo, side="right")) - 1, 0)
    jb = min(int(np.searchsorted(t, hi, side="left")), n - 1)
    return max(0, ja - ROW_MARGIN), min(n, jb + ROW_MARGIN + 1)


def launch_rows(b):
    """(g0, g1) of the case's one chunk"""
    sa, sb = skews(b["alpha"], b["k"], b["gamma"], b["tt"])
    return needed_rows(b["t"], sa, sb, b["tt"], *window_of(b))


def expected_backward_launches(b, cus=256):
    """(launches of bspline_backward_eval_kernel, fits() per tile, tile) the launcher makes for the case"""
    g0, g1 = launch_rows(b)
    tile = backward_tile(b["grid"] ** 2, g1 - g0, cus)
    return backward_launches(b["t"], b["tt"], *spread_of(b), tile, g0, g1 - g0) + (tile,)


def launches_by_instance(f):
    """(launches of the instance with the abscissa window, launches of the gather instance) for the tiles' answers f: one launch per
    run of tiles with the same answer (a last tile of one row never fits: the gather instance is launched for it and returns)"""
    runs = [v for i, v in enumerate(f) if i == 0 or v != f[i - 1]]
    return sum(runs), len(runs) - sum(runs)


def graded_rows(case, b):
    """output rows of a graded case on the side of the seam where the steps are 0.1 -- (all of them, the 48 next to the seam).  A
    run-in that has not forgotten its start shows there, and there the oracle is within 2 .. 40 eps x scale; where the steps are
    1.4e-4 it is 500 .. 800 away itself (|alpha| eps over such a step, relative to it), so those rows are left to the finite and
    same-bits checks."""
    route, n, seam, ratio, steps, grow = case
    i_lo, i_hi = window_of(b)
    rows = np.arange(i_lo, i_hi)
    side = rows >= seam if grow else rows < seam
    near = side & (np.abs(rows - seam) <= 48)
    return np.nonzero(side)[0], np.nonzero(near)[0]


# ------------------------------------------------------------------------------------------------ mode level (groups B and D)
def exact_modes_of(b, ell_max_out=ELL_MAX):
    """(exact, ref) at mode level: the exact grid followed by the exact analysis (tests/helpers/analysis_cases.py exact_map2salm); the
    oracle's grid followed by its own map2salm"""
    from tests.helpers import analysis_cases as an

    s = b["w"].spin_weight
    g = b["grid"]
    exact = an.exact_map2salm(b["exact"].reshape(-1, g, g), s, ell_max_out, abs(s))
    ref = grid_ref.to_modes(b["t_out"], b["ref"].reshape(-1, g, g), s, ell_max_out)
    return exact, ref


# group B: (route, n, grid, out_i0, out_i1) -- a shard from the middle of the series whose buffer (the rows bms_shard_plan asks for:
# ROW_MARGIN on either side of the knots the outputs read) holds 96 k rows (the last backward tile full) or 96 k + 1 (one row in it)
B_CASES = [("A1", 433, 9, 120, 242), ("A1", 433, 9, 120, 243), ("A3", 433, 9, 120, 240), ("A3", 433, 9, 120, 241), ("A4", 433, 9, 120, 240),
           ("A4", 433, 9, 120, 241)]


def needed_rows_of_case(c):
    route, n, g, o0, o1 = c
    b = build_case((route, n, g, "uniform", 0.5))
    r0, r1 = needed_rows(b["t"], *skews(b["alpha"], b["k"], b["gamma"], b["tt"]), b["tt"], o0, o1)
    return r1 - r0


ABD_ELL_MAX = 2
ABD_GRID = 2 * ABD_ELL_MAX + 1   # working_ell_max = ell_max: the smallest grid the transformation of AsymptoticBondiData accepts
ABD_N = (97, 100, 321, 353)
# route -> (options, boosted?)
ABD_ROUTES = {
    "D5": ({}, True),                                   # abd_mix_forward_kernel<5>, sigma on the evaluating product
    "D6": ({"SCRI_AMD_NO_ABD_SIGMA_EVAL": 1}, True),    # abd_mix_forward_kernel<6>
    "Dfused": ({}, False),                              # elimination on the modes, phi_synthesis_mix6_kernel
    "Dgrid": ({"SCRI_AMD_NO_FUSED_ABD_MIX": 1}, False), # separable synthesis, abd_mix_forward_kernel<6>
}
ABD_OPTIONS = ("SCRI_AMD_NO_ABD_SIGMA_EVAL", "SCRI_AMD_NO_FUSED_ABD_MIX")
D_CASES = [(r, n, ax) for r in ABD_ROUTES for n in ABD_N for ax in ("uniform", "alternating")]


@functools.lru_cache(maxsize=None)
def build_abd(route, n, ax):
    """oracle/abd_ref.py transform (scri/asymptotic_bondi_data/transformations.py:199-431) in extended precision, at mode level: its
    harmonics those of oracle/wigner.py, the Horner mixing in np.clongdouble, the spline oracle/spline_exact.py's on the input axis at
    t* = timeprime / k + alpha, the analysis exact_map2salm."""
    from oracle import abd_ref
    from tests.helpers import analysis_cases as an

    L, g = ABD_ELL_MAX, ABD_GRID
    u = axis(ax, n)
    dt = base_step(n)
    st = supertranslation(0.5 * dt, 0.37 * dt)
    v = BOOST if ABD_ROUTES[route][1] else np.zeros(3)
    nm = (L + 1) ** 2
    raw = np.stack([rough_signal(u, nm, 7000 + 10 * n + f) for f in range(6)])
    for f, s in enumerate(containers.ABD.spins):
        raw[f][:, : s * s] = 0.0  # no modes below l = |s|
    kw = dict(supertranslation=st, frame_rotation=ROTATION, boost_velocity=v, working_ell_max=L, output_ell_max=L)
    ref = abd_ref.transform(containers.ABD(u, raw, L), **{k_: (x.copy() if hasattr(x, "copy") else x) for k_, x in kw.items()})
    R = abd_ref.boosted_grid(ROTATION, v, g, g).reshape(-1, 4)
    vL = v.astype(LD)
    gammaL = 1 / np.sqrt(1 - (vL * vL).sum())
    vr = vL @ _ld_rotate_z(R)
    one_over_k = gammaL * (1 - vr)
    k = 1 / one_over_k
    alpha = sy.exact_product(st[None, :], wigner.swsh_grid(R, 0, 2))[0].real
    eth_alpha = sy.exact_product(_ld_eth(st, 0)[None, :], wigner.swsh_grid(R, 1, 2))[0]
    etheth_alpha = sy.exact_product(_ld_eth(_ld_eth(st, 0), 1)[None, :], wigner.swsh_grid(R, 2, 2))[0]
    pi = wigner._PI
    vdr = np.array([0, (vL[0] + 1j * vL[1]) * np.sqrt(2 * pi / 3), vL[2] * np.sqrt(4 * pi / 3) + 0j, (-vL[0] + 1j * vL[1]) * np.sqrt(2 * pi / 3)], dtype=CLD)
    ethk_over_k = sy.exact_product(vdr[None, :], wigner.swsh_grid(R, 1, 1))[0] / (1 - vr)
    X = ethk_over_k[None, :] * (u.astype(LD)[:, None] - alpha[None, :]) - eth_alpha[None, :]
    p0, p1, p2, p3, p4, sg = (sy.exact_product(raw[f], wigner.swsh_grid(R, s, L)) for f, s in enumerate(containers.ABD.spins))
    ik3 = (one_over_k**3)[None, :]
    fp = [((((p4 * X - 4 * p3) * X + 6 * p2) * X - 4 * p1) * X + p0) * ik3,
          (((-p4 * X + 3 * p3) * X - 3 * p2) * X + p1) * ik3,
          ((p4 * X - 2 * p3) * X + p2) * ik3,
          (-p4 * X + p3) * ik3,
          p4 * ik3,
          (sg - etheth_alpha[None, :]) * one_over_k[None, :]]
    tstar = ref.u.astype(LD)[:, None] / k[None, :] + alpha[None, :]
    exact = []
    for f, s in enumerate(containers.ABD.spins):
        grid = evaluate_per_column(u, fp[f], sx.slopes(u, fp[f]), tstar)
        exact.append(an.exact_map2salm(grid.reshape(-1, g, g), s, L))
    exact = np.stack(exact)
    for a in (u, raw, exact, ref.raw):
        a.setflags(write=False)
    other = np.stack([rough_signal(u, nm, 8000 + 10 * n + f) for f in range(6)])
    return dict(u=u, raw=raw, other=other, st=st, rot=ROTATION, v=v, u_out=ref.u, exact=exact, ref=ref.raw, n=n)
