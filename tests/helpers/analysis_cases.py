"""Case tables, references and the tolerance rule of tests/test_gpu_analysis_edges.py and tests/test_oracle_analysis_exact.py: the
analysis kernels (grid -> modes, scri_amd/csrc/kernels_analysis.hip) held to the quadrature of oracle/spinsfast_ref.py carried in
extended precision.  The counterpart of tests/helpers/synthesis_cases.py.

The rule is the project's (tests/helpers/spline_cases.py).  For one call with result `got`, the extended-precision result `exact` and
the fp64 yardstick `ref`:
    E_got = max|got - exact|,  E_ref = max|ref - exact|,  scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured.
  exact   exact_map2salm() below: the phi transform with k m mod n_phi exact, then one real weight per ring times sLambda_lm(theta_j)
          (oracle/wigner.py swsh_grid at the ring rotors), everything accumulated in np.clongdouble.
  ref     oracle/spinsfast_ref.py map2salm unchanged (fp64; the quadrature as a wrapped convolution assembled into matrices).
  band-limited rows: exact is the mode vector the rows were synthesised from -- no analysis reference at all.
F and G are set per family from the worst ratios measured on an MI355X over every call of tests/test_gpu_analysis_edges.py (next
power of two above twice the worst; the figures stand next to RULE): against exact and ref, never against another route of the
library."""
import collections
import functools

import numpy as np

from oracle import quat, spinsfast_ref, wigner
from tests.helpers import synthesis_cases as sy
from tests.helpers.spline_cases import EPS, F_CAP, G_CAP, errors

# family -> (F, G): the next power of two above twice the worst ratio measured on an MI355X over every call of
# tests/test_gpu_analysis_edges.py.  The family is the kernel the launchers' arithmetic (route_of below) sends a call to:
#   split       analysis_split_kernel                                   fused       analysis_fused_kernel
#   fused_wide  analysis_fused_wide_kernel                              large       phi_dft_folded_kernel + theta_quadrature_mfma_kernel
#   tq_old      phi-DFT product + theta_quadrature_kernel               dense       one product with the quadrature matrix
#   *_1hot      one-hot pixel rows of the same kernel: the analysis matrix itself, entry by entry
# White-noise and band-limited rows run under the family of their kernel.  Shapes as n_theta x n_phi / l_min .. l_max; `band`:
# band-limited rows.  The kernels lie CLOSER to the exact result than the fp64 oracle does in every family but tq_old and dense, so
# most F are 1 or 2, and below 1 for the one-hot rows: there the oracle's matrix entries are off by up to 9e-17 (its theta matrices
# come out of an FFT and two matrix products) and the kernels' by 1e-17 at most, with scale = 1 and entries of 1e-3.
# fused_wide: no call has E_ref < 4 eps scale (the oracle loses more at l >= 17), so nothing was measured for G and every call passes on
# the F term; G is the one-role kernel's, whose body it shares.
#                               worst E_got / E_ref                        worst E_got / (eps scale) where E_ref < 4 eps scale
RULE = {
    "split": (1.0, 4.0),              # 0.360   39 x 9 / 2..8                     1.09    9 x 9 / 2..4, 3 rows
    "fused": (1.0, 2.0),              # 0.337   40 x 47 / 1..6                    0.878   25 x 39 / 1..6
    "fused_wide": (2.0, 2.0),         # 0.701   35 x 35 / 1..17 band              none
    "large": (2.0, 4.0),              # 0.558   5 x 48 / 0..2, 256 rows           1.71    5 x 48 / 0..2, 256 rows
    "tq_old": (4.0, 8.0),             # 1.47    5 x 130 / 0..2, 2100 rows         3.77    5 x 130 / 0..2, 2100 rows
    "dense": (4.0, 16.0),             # 1.41    105 x 13 / 0..6 band              4.90    105 x 6 / 0..6
    "split_1hot": (0.25, 0.125),      # 0.107   25 x 38 / 2..8                    0.0424  25 x 38 / 2..8
    "fused_1hot": (0.25, 0.125),      # 0.107   25 x 38 / 2..8                    0.0424  25 x 38 / 2..8
    "fused_wide_1hot": (0.125, 0.125),  # 0.0484  25 x 38 / 2..17                 0.0459  25 x 38 / 2..17
    "large_1hot": (0.25, 0.0625),     # 0.0810  9 x 48 / 0..4                     0.0295  9 x 48 / 0..4
    "tq_old_1hot": (0.25, 0.03125),   # 0.0750  41 x 48 / 0..8                    0.0136  41 x 48 / 0..8
    "dense_1hot": (4.0, 0.25),        # 1.003   105 x 6 / 0..4                    0.120   105 x 6 / 0..4
}
# worst E_got / (eps scale) of each family over ALL its calls (E_got, E_ref, shape), for the record:
#   split 3.25 (2.5e-15, 1.1e-14, 17 x 17 / 2..8 band)          fused 3.56 (2.7e-15, 1.1e-14, 17 x 17 / 2..8 band)
#   fused_wide 8.42 (7.6e-15, 1.1e-14, 35 x 35 / 1..17 band)    large 3.04 (3.6e-15, 1.8e-14, 41 x 41 / 0..20 band)
#   tq_old 3.77 (8.4e-16, 5.7e-16, 5 x 130 / 0..2)              dense 13.1 (7.5e-15, 5.3e-15, 105 x 13 / 0..6 band)
# Group B (boosted transforms against oracle/waveform_grid_ref.py): at most 9.8e-16 of scale against the bar of 1e-12.


def bar(family, e_ref, scale):
    F, G = RULE[family]
    assert F <= F_CAP and G <= G_CAP
    return max(F * e_ref, G * EPS * scale)


def check(family, got, exact, ref, what):
    """Assert the rule for one call; prints the figures first (pytest -s shows them) and returns the bar."""
    got = np.asarray(got)
    assert got.shape == np.asarray(exact).shape, (what, got.shape, np.asarray(exact).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result (a mode nobody wrote?)"
    e_got, e_ref, scale = errors(got, exact, ref)
    b = bar(family, e_ref, scale)
    print(f"RULE {family} E_got={e_got:.3e} E_ref={e_ref:.3e} scale={scale:.3e} got/ref={e_got / max(e_ref, 1e-300):.3g} "
          f"got/eps={e_got / (EPS * scale):.3g} | {what}")
    if e_got > b:
        r, o = np.unravel_index(int(np.argmax(np.abs(got - np.asarray(exact)))), got.shape)
        raise AssertionError(f"{what}: E_got = {e_got:.3e} > bar {b:.3e} (E_ref = {e_ref:.3e}, scale = {scale:.3e}); worst at row {r}, mode {o}")
    return b


# ------------------------------------------------------------------------------------------------ the launchers' arithmetic
def n_out_of(L, ell_min):
    return (L + 1) ** 2 - ell_min**2


def fused_takes(n_theta, n_phi, L, n_out):
    """fused_analysis_supported (kernels_analysis.hip)"""
    return not (n_theta > 40 or n_phi < 2 or n_phi // 2 + 1 > 24 or n_out > 512 or L < 1 or L > 32)


def split_takes(n_theta, n_phi, L, n_out, n_rows, dedup_poles=False):
    """split_analysis_supported (kernels_analysis.hip) plus the n_rows >= 2 of its caller, launch_analysis_fused (whose other
    condition, a row stride below 2^26 doubles, holds for every grid the kernel takes)"""
    if n_rows < 2 or n_theta < 3 or n_theta > 40 or n_phi < 2 or L < 1 or L > 16 or n_phi // 2 + 1 > 20:
        return False
    nf, nb = (2 * (n_theta - (2 if dedup_poles else 0)) + 15) // 16, (n_out + 63) // 64
    return nf <= 6 and nf + nb <= 10


def large_takes(n_theta, n_phi, L):
    """large_analysis_supported (kernels_analysis.hip)"""
    return n_theta <= 104 and (n_phi // 2 + 1 + 3) // 4 <= 16 and 1 <= L <= 32


def fused_instance(n_theta, n_phi, L, n_out):
    """(wide, NT, KS, EPT, threads, n_sec) of the analysis_fused[_wide]_kernel<NT, KS, EPT> that launch_analysis_fused picks (with
    fused_geometry and fused_ks), or None where it returns hipErrorInvalidValue (more than F_EPT_MAX = 4 items per thread)"""
    nk = n_phi // 2 + 1
    ks = (nk + 3) // 4
    ks = 3 if ks <= 3 else 5 if ks <= 5 else 6
    n_sec = n_out - 256 if 256 < n_out <= 320 else 0
    threads = max(256, 256 if n_sec else (n_out + 63) // 64 * 64)
    ept = (n_theta * nk + threads - 1) // threads
    if ept > 4:
        return None
    return (L > 16, 24 if n_theta <= 24 else 40, ks, max(ept, 2), threads, n_sec)


def split_instance(n_theta, n_phi, L, n_out, dedup_poles=False):
    """(NT, KS, nf, nb) of the analysis_split_kernel<NT, KS> of launch_analysis_fused (with split_analysis_supported)"""
    nk = n_phi // 2 + 1
    nf, nb = (2 * (n_theta - (2 if dedup_poles else 0)) + 15) // 16, (n_out + 63) // 64
    return (24 if n_theta <= 24 else 38 if n_theta <= 38 else 40, 3 if (nk + 3) // 4 <= 3 else 5, nf, nb)


def large_instance(n_theta, n_phi, L, ell_min):
    """(KS, NTC, KQ, NTQ) of launch_analysis_large: phi_dft_folded_kernel<KS, NTC> and theta_quadrature_mfma_kernel<KQ, NTQ>"""
    ks, kq = (n_phi // 2 + 1 + 3) // 4, (n_theta + 3) // 4
    ntq = (L + 1 - ell_min + 15) // 16
    return (7 if ks <= 7 else 10 if ks <= 10 else 13 if ks <= 13 else 16, 1 if L <= 16 else 2,
            11 if kq <= 11 else 18 if kq <= 18 else 26, 1 if ntq <= 1 else 2 if ntq == 2 else 3)


def tq_old_instance(n_theta):
    """NT of the theta_quadrature_kernel<NT, MAXT> of launch_theta_quadrature"""
    return 24 if n_theta <= 24 else 40 if n_theta <= 40 else 72 if n_theta <= 72 else 104


def route_of(n_theta, n_phi, L, ell_min, n_rows, env=None):
    """the family a call of bms_map2salm runs under -- build_analysis and run_analysis (engine_tables.hip), then launch_analysis_fused.
    env: None or the one route option set, "NO_SPLIT" | "NO_LARGE" | "NO_FUSED" (SCRI_AMD_..._ANALYSIS)"""
    n_out = n_out_of(L, ell_min)
    separable = n_theta <= 104  # MAX_THETA_SEPARABLE
    fused = separable and fused_takes(n_theta, n_phi, L, n_out) and env != "NO_FUSED"
    large = separable and not fused and large_takes(n_theta, n_phi, L) and env not in ("NO_LARGE", "NO_FUSED")
    if fused:
        if env != "NO_SPLIT" and split_takes(n_theta, n_phi, L, n_out, n_rows):
            return "split"
        return "fused_wide" if L > 16 else "fused"
    return "large" if large else "tq_old" if separable else "dense"


# the timing tags (scri_amd/_lib.py KERNEL_TAGS) with launches after a call of each family
TAGS = {"split": {"analysis_fused"}, "fused": {"analysis_fused"}, "fused_wide": {"analysis_fused"}, "large": {"analysis_large"},
        "tq_old": {"gemm_analysis", "theta_quadrature"}, "dense": {"gemm_analysis"}}
ANALYSIS_TAGS = {"analysis_fused", "analysis_large", "gemm_analysis", "theta_quadrature"}


# ------------------------------------------------------------------------------------------------ group A: engine.map2salm
Case = collections.namedtuple("Case", "n_theta n_phi L ell_min spin rows env kind", defaults=(None, "noise"))
# kind: "noise" white-noise rows | "one_hot" one-hot pixel rows (`rows` is ignored) | "band" band-limited rows


def case_id(c):
    return f"{c.n_theta}x{c.n_phi}-l{c.ell_min}..{c.L}-s{c.spin}-r{c.rows}-{c.env or 'default'}-{c.kind}"


def _both(cases):
    """each case on the default route and with the split kernel switched off"""
    return [c for c in cases] + [c._replace(env="NO_SPLIT") for c in cases]


# the two-role kernel and, with SCRI_AMD_NO_SPLIT_ANALYSIS or where it refuses, the one-role kernel
A_SMALL_THETA = _both([Case(nt, 9, 8, 2, -2, 5) for nt in (3, 23, 24, 25, 38, 39, 40)])          # every NT, the edges of nf = 1 .. 5
A_SMALL_PHI = _both([Case(9, nph, 8, 2, -2, 5) for nph in (2, 3, 22, 23, 24, 25, 38, 39, 40, 41)])   # KS 3 | 5, both parities; 40, 41: the split refuses
A_SMALL_NT_KS = _both([Case(nt, nph, 6, 1, 1, 4) for nt in (24, 38, 40) for nph in (23, 38)])      # all six analysis_split_kernel<NT, KS>
A_SMALL_NOUT = _both([Case(17, 18, 7, 0, 0, 5), Case(17, 18, 8, 0, 0, 5), Case(33, 34, 16, 0, 0, 5),   # n_out = 64 | 81 | 289: nb = 1 | 2 | 5
                      Case(33, 34, 15, 0, 0, 5), Case(33, 34, 16, 2, -2, 5), Case(33, 34, 16, 6, 1, 5),    # 256 | 285 | 253: n_sec = 0 | 29 | 0
                      Case(17, 18, 12, 2, -2, 5)])                                                       # 165: nb = 3
A_SMALL_ROWS = ([Case(9, 9, 4, 2, -2, r) for r in (1, 2, 3)]                      # one row: the split kernel refuses it
                + [Case(9, 9, 4, 0, 1, r) for r in (1600, 1601)]                  # beyond cus * per_cu pairs: the stride loop, the overlapping last pair
                + [Case(9, 9, 4, 0, 1, 600, "NO_SPLIT")])                         # more rows than 2 x CUs workgroups of the one-role kernel
A_FUSED_PHI = [Case(9, nph, 8, 2, -2, 5) for nph in (46, 47)]                     # nk = 24: the last n_phi the fused kernel takes
# every reachable (NT, KS, EPT) of analysis_fused_kernel that the tables above leave out (n_theta x nk: items of the fold)
A_FUSED_EPT = [Case(24, 47, 6, 1, 1, 3),                       # <24, 6, 3>: 24 x 24 = 576 items
               Case(24, 41, 6, 1, 1, 3),                       # <24, 6, 2>: 24 x 21 = 504
               Case(24, 39, 6, 1, 1, 3, "NO_SPLIT"),           # <24, 5, 2>: 24 x 20 = 480
               Case(40, 23, 6, 1, 1, 3, "NO_SPLIT"),           # <40, 3, 2>: 40 x 12 = 480
               Case(25, 39, 6, 1, 1, 3, "NO_SPLIT"),           # <40, 5, 2>: 25 x 20 = 500
               Case(38, 39, 6, 1, 1, 3, "NO_SPLIT"),           # <40, 5, 3>: 38 x 20 = 760
               Case(40, 39, 6, 1, 1, 3, "NO_SPLIT"),           # <40, 5, 4>: 40 x 20 = 800
               Case(25, 41, 6, 1, 1, 3),                       # <40, 6, 3>: 25 x 21 = 525
               Case(40, 47, 6, 1, 1, 3)]                       # <40, 6, 4>: 40 x 24 = 960
# the wide kernel: (ell_max, ell_min) -> n_out 320 (n_sec 64), 323 (384 threads), 384, 391 (448), 484 (512), 504; l = 32 with few modes
_WIDE_L = [(17, 2), (17, 1), (19, 4), (19, 3), (21, 0), (22, 5), (32, 31), (32, 30)]
A_WIDE = ([Case(9, 10, L, lo, -1 if lo <= 1 else 2, 5) for L, lo in _WIDE_L]                         # <24, 3, 2>
          + [Case(24, 39, L, lo, 1, 3) for L, lo in ((17, 2), (17, 1), (19, 3), (22, 5))]            # <24, 5, 2>
          + [Case(24, 47, L, lo, 1, 3) for L, lo in ((17, 2), (19, 4), (21, 0))] + [Case(17, 47, 32, 30, 1, 3)]   # <24, 6, 3 | 2>
          + [Case(25, 23, L, lo, 1, 3) for L, lo in ((17, 2), (21, 0))]                              # <40, 3, 2>
          + [Case(40, 38, L, lo, 1, 3) for L, lo in ((17, 2), (17, 1), (19, 3), (21, 0))] + [Case(25, 38, 32, 31, 1, 3)]   # <40, 5, 4 | 3 | 2>
          + [Case(40, 46, L, lo, 1, 3) for L, lo in ((17, 2), (17, 1), (19, 3), (22, 5))]            # <40, 6, 4 | 3 | 2>
          + [Case(25, 41, 19, 3, 1, 3)])                                                              # <40, 6, 2>
# the two-kernel route
A_LARGE_SMALL = [Case(9, 10, 22, 4, 2, 5), Case(40, 39, 22, 4, 2, 3)]      # n_out = 513: the fused kernel refuses; mt = 2 | 5, kq <= 11
A_LARGE_THETA = [Case(nt, 48, 4, 0, -2, 5) for nt in (3, 8, 9, 40, 41, 44, 45, 48, 49, 72, 73, 96, 97, 104)]   # ring tiles of 8; KQ edges 44 | 45, 72 | 73
A_LARGE_PHI = [Case(5, nph, 4, 0, -2, 5) for nph in (48, 49, 55, 56, 57, 79, 80, 81, 103, 104, 105, 126, 127)]   # every KS edge, both parities
# (n_theta = 17 from l = 31: on 9 rings the fp64 oracle itself lies 35 .. 42 eps scale from the exact result, on 13 rings 29 .. 31)
A_LARGE_ELL = [Case(9 if L <= 17 else 17, 48, L, lo, -2 if lo == 2 else lo, 5) for L in (1, 15, 16, 17, 31, 32) for lo in (0, 1, 2) if lo <= L]   # NTC 1 | 2, NTQ 1 | 2 | 3
A_LARGE_ROWS = [Case(5, 48, 2, 0, 0, r) for r in (255, 256, 257, 513)] + [Case(3, 48, 2, 0, 0, 4100)]   # rows_per_block = 256; the phi stage's grid stride
A_LARGE_CORNERS = [Case(104, 127, 32, 0, -2, 9), Case(99, 99, 24, 0, 2, 9)]
A_LARGE_SPINS = [Case(41, 48, 8, 0, s, 5) for s in range(-4, 5)]
A_LARGE_PAIRS = ([Case(nt, 48, L, 0, 1, 3) for nt, L in ((45, 16), (45, 20), (45, 32), (73, 16), (73, 20))]   # the (KQ, NTQ) the lists above leave out; <26, 3>: the corner
                 + [Case(5, nph, 17, 0, -1, 3) for nph in (48, 57, 81, 105)])                      # every KS with NTC = 2
# the older pair: one shape per theta_quadrature_kernel<NT>, and the shapes that fall to it by themselves
A_OLD = ([Case(nt, 48, 4, 0, -2, 5, "NO_LARGE") for nt in (24, 40, 72, 104)]
         + [Case(9, 10, 8, 2, -2, 5, "NO_FUSED"), Case(41, 41, 8, 2, -2, 5, "NO_FUSED")]
         + [Case(6, 128, 6, 0, -2, 5), Case(13, 10, 33, 0, -2, 5), Case(5, 130, 2, 0, 0, 2100)])   # ks = 17; l = 33; beyond 2048 row blocks
A_DENSE = [Case(105, 6, 6, 0, -2, 5)]
# one-hot pixel rows, one shape per family at its most awkward geometry: even n_phi, a partial last ring tile, n_theta one above a tile edge
A_ONE_HOT = [Case(25, 38, 8, 2, -2, 0, None, "one_hot"),           # split <38, 5>: a ninth ring in the last 16-row tile, Nyquist column
             Case(25, 46, 8, 2, -2, 0, None, "one_hot"),           # fused <40, 6, 3>: nk = 24
             Case(25, 38, 8, 2, -2, 0, "NO_SPLIT", "one_hot"),     # fused <40, 5, 2>
             Case(25, 38, 17, 2, -2, 0, None, "one_hot"),          # wide, l = 17, n_sec = 64
             Case(41, 48, 17, 1, -1, 0, None, "one_hot"),          # large: one live ring in the sixth tile of 8, NTC = 2
             Case(9, 48, 4, 0, 1, 0, None, "one_hot"),             # large on a small grid: mt = 2, kq = 3, one live ring in the last tile
             Case(41, 48, 8, 0, -2, 0, "NO_LARGE", "one_hot"),     # tq_old <72>
             Case(105, 6, 4, 0, -1, 0, None, "one_hot")]           # dense
# band-limited rows: the grid exactly (2 L + 1)^2 -- the dense quadrature starts at n_theta = 105, where that would be l = 52 (two
# minutes of the fp64 oracle's matrices), so its grid is 105 x (2 L + 1)
A_BAND = [Case(17, 17, 8, 2, -2, 5, None, "band"),                 # split
          Case(17, 17, 8, 2, -2, 5, "NO_SPLIT", "band"),           # fused
          Case(35, 35, 17, 1, 1, 3, None, "band"),                 # wide
          Case(41, 41, 20, 0, 0, 3, None, "band"),                 # large
          Case(41, 41, 20, 0, 0, 3, "NO_LARGE", "band"),           # tq_old
          Case(105, 13, 6, 0, -2, 3, None, "band")]                # dense
A_CASES = (A_SMALL_THETA + A_SMALL_PHI + A_SMALL_NT_KS + A_SMALL_NOUT + A_SMALL_ROWS + A_FUSED_PHI + A_FUSED_EPT + A_WIDE + A_LARGE_SMALL
           + A_LARGE_THETA + A_LARGE_PHI + A_LARGE_ELL + A_LARGE_ROWS + A_LARGE_CORNERS + A_LARGE_SPINS + A_LARGE_PAIRS + A_OLD + A_DENSE
           + A_ONE_HOT + A_BAND)


def family_of(c):
    return route_of(c.n_theta, c.n_phi, c.L, c.ell_min, n_rows_of(c), c.env) + ("_1hot" if c.kind == "one_hot" else "")


def n_rows_of(c):
    return len(one_hot_pixels(c.n_theta, c.n_phi)) if c.kind == "one_hot" else c.rows


# ------------------------------------------------------------------------------------------------ group B: WaveformModes.transform
B_TYPES = ("psi0", "psi1", "psi2", "psi3", "psi4", "h", "sigma", "news")  # spin weights 2, 1, 0, -1, -2, -2, 2, -2
B_GRIDS = [(9, 10), (24, 23), (25, 24), (39, 38), (40, 39)]   # gathered columns, de-duplicated poles: split (closed-form poles) | fused (phases)
B_NOT_FUSED = [(41, 41), (15, 49)]                             # grids the fused analysis does not take: natural column order
B_ELL_MAX, B_STEPS = 4, 40
B_BOOST = (0.01, -0.02, 0.015)


# ------------------------------------------------------------------------------------------------ inputs
def noise_rows(n_rows, n_theta, n_phi, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_rows, n_theta, n_phi)) + 1j * rng.normal(size=(n_rows, n_theta, n_phi))


def one_hot_pixels(n_theta, n_phi):
    """pixel indices j n_phi + k of the one-hot rows: every pixel where the matrix of rows has at most 64 MB, else both pole rings and
    the first and last ring of every 8-ring tile, at k = 0, 1, n_phi / 2, n_phi / 2 + 1, n_phi - 1"""
    n_pix = n_theta * n_phi
    if n_pix * n_pix * 16 <= 64e6:
        return np.arange(n_pix)
    rings = sorted({0, n_theta - 1} | {j for j in range(n_theta) if j % 8 in (0, 7)})
    ks = sorted({0, 1, n_phi // 2, n_phi // 2 + 1, n_phi - 1})
    return np.array([j * n_phi + k for j in rings for k in ks])


def one_hot_rows(pixels, n_theta, n_phi):
    f = np.zeros((len(pixels), n_theta * n_phi), dtype=complex)
    f[np.arange(len(pixels)), pixels] = 1.0
    return f.reshape(len(pixels), n_theta, n_phi)


def band_limited_rows(n_rows, n_theta, n_phi, spin, L, ell_min, seed):
    """(modes a[rows, l = ell_min .. L], grid rows): the rows are the exact syntheses of random modes (synthesis_cases.ring_harmonics and
    exact_product), rounded to fp64; n_theta, n_phi >= 2 L + 1, so the analysis returns a"""
    assert n_theta >= 2 * L + 1 and n_phi >= 2 * L + 1
    a = sy.dense_rows(n_rows, (L + 1) ** 2, seed)
    lm = wigner.LM_range(0, L)
    a[:, lm[:, 0] < max(abs(spin), ell_min)] = 0.0
    Y = sy.ring_harmonics(n_theta, n_phi, spin, L, np.arange(lm.shape[0]))  # [modes, pixels]
    f = sy.exact_product(a, Y.T)
    return a[:, ell_min**2 :], f.astype(complex).reshape(n_rows, n_theta, n_phi), f.reshape(n_rows, n_theta, n_phi)


# ------------------------------------------------------------------------------------------------ the exact reference
_LD, _CLD = np.longdouble, np.clongdouble


def _unit_phases(num, den, sign):
    """e^{sign 2 pi i num / den} in np.clongdouble for integer arrays num (reduced mod den first, so the angle is exact to rounding)"""
    ang = (np.asarray(num) % den).astype(_LD) * (2 * wigner._PI / _LD(den))
    return np.cos(ang) + (1j * sign) * np.sin(ang)


def _w(p):
    """w(p) = int_0^pi e^{i p theta} sin(theta) d theta of oracle/spinsfast_ref.py's docstring, in np.clongdouble"""
    if p == 1 or p == -1:
        return _CLD(1j) * (p * wigner._PI / 2)
    return _CLD(_LD(2) / _LD(1 - p * p)) if p % 2 == 0 else _CLD(0)


@functools.lru_cache(maxsize=None)
def ring_weights(n_theta, nyquist=True):
    """One real weight per ring, np.longdouble [n_theta]: a_lm = sum_j W_j f_m(theta_j) sLambda_lm(theta_j).
    Step (4) of oracle/spinsfast_ref.py's docstring as a real-space multiplication on the theta circle of M = 2 n_theta - 2 samples,
        a_lm = (2 pi / M) sum_{j < M} G_m(theta_j) w_r(theta_j) sLambda_lm(theta_j),  w_r(theta_j) = sum_{-M/2 < p <= M/2} w(p) e^{-i p theta_j}
    (the sign of the exponent is the one that undoes c_n = (1/M) sum_j G_j e^{-i n theta_j} with p = n + m' wrapped), folded over
    the extension: ring M - j carries G_m = (-1)^(m+s) f_m(theta_j) and sLambda_lm(2 pi - theta_j) = (-1)^(m+s) sLambda_lm(theta_j), so
    the two signs cancel and W_j = (2 pi / M) (w_r(theta_j) + w_r(theta_{M-j})) for the inner rings, (2 pi / M) w_r at the poles.
    nyquist=False drops the term p = M / 2 (a deliberately wrong quadrature for the CPU tests of the checks)."""
    M = 2 * n_theta - 2
    ps = [p for p in range(-(M // 2) + 1, M // 2 + 1) if nyquist or p != M // 2]
    w = np.array([_w(p) for p in ps], dtype=_CLD)
    wr = _unit_phases(np.outer(np.arange(M), ps), M, -1) @ w  # [M]
    W = wr[:n_theta].copy()
    W[1 : n_theta - 1] += wr[M - 1 : n_theta - 1 : -1]
    assert np.abs(W.imag).max() <= 64 * np.finfo(_LD).eps * np.abs(W).max()  # (pi sin(theta_j) of p = +-1 cancels between j and M - j)
    out = W.real * (2 * wigner._PI / _LD(M))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=8)
def ring_lambda(n_theta, spin, L, ideal=False):
    """sLambda_lm(theta_j) = sYlm(R(theta_j, 0)), [n_theta, (L + 1)^2] real.  Default: oracle.wigner.swsh_grid at the fp64 ring rotors
    (extended recurrences, rounded to fp64) -- what the library's own table is built from.  ideal=True: the same recurrences
    (wigner.wigner_d_chain) at theta_j = pi j / (n_theta - 1) carried in np.longdouble and NOT rounded: for the round trip to
    extended precision."""
    if not ideal:
        rings = quat.from_spherical_coords(np.pi * np.arange(n_theta) / (n_theta - 1), np.zeros(n_theta))
        Y = wigner.swsh_grid(rings, spin, L)
        assert wigner.EXTENDED and not Y.imag.any()
        out = Y.real.astype(_LD)
    else:
        half = wigner._PI * np.arange(n_theta).astype(_LD) / _LD(2 * (n_theta - 1))
        ra, rb = np.cos(half), np.sin(half)
        out = np.zeros((n_theta, (L + 1) ** 2), dtype=_LD)
        for m in range(-L, L + 1):
            d = wigner.wigner_d_chain(m, -spin, ra, rb, L)
            for ell in range(max(abs(m), abs(spin)), L + 1):
                out[:, wigner.LM_index(ell, m, 0)] = (-1.0) ** spin * np.sqrt(_LD(2 * ell + 1) / (4 * wigner._PI)) * d[:, ell]
    out.setflags(write=False)
    return out


def exact_phi_transform(f, L):
    """step (1): f_m(theta_j) = (1 / n_phi) sum_k f_jk e^{-i m phi_k}, [..., n_theta, 2 L + 1] in np.clongdouble, k m mod n_phi exact"""
    n_phi = f.shape[-1]
    E = _unit_phases(np.outer(np.arange(n_phi), np.arange(-L, L + 1)), n_phi, -1) / _LD(n_phi)
    return np.asarray(f).astype(_CLD) @ E


def exact_map2salm(f, s, ell_max, ell_min=0, weights=None, lam=None):
    """spinsfast.map2salm(f[..., n_theta, n_phi], s, ell_max)[..., ell_min^2:] in np.clongdouble: the exact phi transform, then one real
    weight per ring times sLambda_lm(theta_j).  weights / lam: other ring weights or harmonics than ring_weights() / ring_lambda()."""
    f = np.asarray(f)
    n_theta = f.shape[-2]
    fm = exact_phi_transform(f, ell_max)
    W = ring_weights(n_theta) if weights is None else weights
    lam = ring_lambda(n_theta, s, ell_max) if lam is None else lam
    out = np.zeros(f.shape[:-2] + ((ell_max + 1) ** 2,), dtype=_CLD)
    for m in range(-ell_max, ell_max + 1):
        idx = [wigner.LM_index(ell, m, 0) for ell in range(max(abs(m), abs(s)), ell_max + 1)]
        if idx:
            out[..., idx] = fm[..., :, m + ell_max] @ (W[:, None] * lam[:, idx]).astype(_CLD)
    return out[..., ell_min**2 :]


def exact_matrix(s, ell_max, ell_min, n_theta, n_phi, pixels, weights=None):
    """the analysis matrix entry by entry, [len(pixels), n_out] in np.clongdouble: row r is the analysis of a single 1 at pixel
    pixels[r] -- W_j sLambda_lm(theta_j) e^{-i m phi_k} / n_phi, no sum at all"""
    W = ring_weights(n_theta) if weights is None else weights
    lam = ring_lambda(n_theta, s, ell_max)
    lm = wigner.LM_range(0, ell_max)
    j, k = np.asarray(pixels) // n_phi, np.asarray(pixels) % n_phi
    out = (W[j, None] * lam[j]).astype(_CLD) * _unit_phases(k[:, None] * lm[None, :, 1], n_phi, -1) / _LD(n_phi)
    return out[:, ell_min**2 :]


def fp64_ref(f, s, ell_max, ell_min=0):
    """the fp64 yardstick: oracle/spinsfast_ref.py map2salm unchanged"""
    return spinsfast_ref.map2salm(f, s, ell_max)[..., ell_min**2 :]


def case_inputs(c):
    """(grid rows f [rows, n_theta, n_phi] fp64, exact [rows, n_out], ref [rows, n_out]) of one case of group A"""
    seed = c.n_theta * 1009 + c.n_phi * 31 + c.L * 7 + c.ell_min + 3 * (c.spin + 4)
    if c.kind == "noise":
        f = noise_rows(c.rows, c.n_theta, c.n_phi, seed)
        return f, exact_map2salm(f, c.spin, c.L, c.ell_min), fp64_ref(f, c.spin, c.L, c.ell_min)
    if c.kind == "one_hot":
        pixels = one_hot_pixels(c.n_theta, c.n_phi)
        f = one_hot_rows(pixels, c.n_theta, c.n_phi)
        return f, exact_matrix(c.spin, c.L, c.ell_min, c.n_theta, c.n_phi, pixels), fp64_ref(f, c.spin, c.L, c.ell_min)
    a, f, _ = band_limited_rows(c.rows, c.n_theta, c.n_phi, c.spin, c.L, c.ell_min, seed)
    return f, a.astype(_CLD), fp64_ref(f, c.spin, c.L, c.ell_min)
