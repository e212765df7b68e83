"""Case tables, references and the tolerance rule of tests/test_gpu_synthesis_edges.py: the synthesis kernels (modes -> grid) held to
the oracle's harmonics at the grid level.

The rule is the project's (tests/helpers/spline_cases.py).  For one call with result `got`, the extended-precision result `exact` and
the fp64 yardstick `ref`:
    E_got = max|got - exact|,  E_ref = max|ref - exact|,  scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured.
  dense rows    exact: the input times the oracle's harmonics (oracle/wigner.py swsh_grid, recurrences in np.longdouble, rounded to
                fp64), accumulated in np.clongdouble; ref: the same product in fp64 -- what oracle/spinsfast_ref.py salm2map computes
                (oracle/waveform_grid_ref.py from_modes in group B).
  one-hot rows  row r holds a single 1 at mode r, so the result is the synthesis matrix itself.  exact: swsh_grid; ref: swsh_grid with
                its recurrences in fp64 (fp64_recurrences() below), which loses about l ulp.
F and G are set per family from the worst ratios measured on an MI355X over every call of the module (next power of two above twice
the worst): against exact and ref, never against another route of the library."""
import contextlib
import functools

import numpy as np

from oracle import quat, wigner
from tests.helpers.spline_cases import EPS, F_CAP, G_CAP, errors

# family -> (F, G): the next power of two above twice the worst ratio measured on an MI355X over every call of
# tests/test_gpu_synthesis_edges.py (its docstring has the figures and where they occurred).  The family is the ROUTE a call asks for;
# where a kernel does not take a shape the launcher's next choice runs under the same family.
#   group A (engine.salm2map)          large: theta_synthesis_mfma_kernel + phi_synthesis_folded_kernel    gemm: swsh_kernel<3> + zgemm3m
#                                      *_1hot: the one-hot rows of the same route    large_rings: those against ring_harmonics()
#   group B (WaveformGrid.from_modes)  split / eval / large_b / gemm_b: the route options of B_ROUTES; the time spline takes part
# `large`: the recipe gives F = 64, above the cap, so F stays AT the cap and the shape that asks for it (104 x 127 / l <= 33, dense rows)
# passes on the G term.  The distance is the oracle's, not the kernels': see ring_harmonics() and the `large_rings` row.
#                     worst E_got / E_ref    worst E_got / (eps scale) where E_ref < 4 eps scale
RULE = {
    "large": (32.0, 128.0),      # 30.4                  62.6
    "gemm": (32.0, 64.0),        # 8.23                  16.2
    "large_1hot": (8.0, 16.0),   # 2.69                  5.94
    "gemm_1hot": (1.0, 2.0),     # 0.37                  0.81
    "large_rings": (2.0, 4.0),   # 0.70                  1.79
    "split": (32.0, 64.0),       # 14.3                  24.2
    "eval": (32.0, 64.0),        # 14.0                  25.9
    "large_b": (32.0, 64.0),     # 14.3                  24.2
    "gemm_b": (16.0, 32.0),      # 5.90                  12.0
}


def bar(family, e_ref, scale):
    F, G = RULE[family]
    assert F <= F_CAP and G <= G_CAP
    return max(F * e_ref, G * EPS * scale)


def check(family, got, exact, ref, what):
    """Assert the rule for one call; prints the figures first (pytest -s shows them) and returns the bar."""
    got = np.asarray(got)
    assert got.shape == np.asarray(exact).shape, (what, got.shape, np.asarray(exact).shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values in the result (a pixel nobody wrote?)"
    e_got, e_ref, scale = errors(got, exact, ref)
    b = bar(family, e_ref, scale)
    print(f"RULE {family} E_got={e_got:.3e} E_ref={e_ref:.3e} scale={scale:.3e} got/ref={e_got / max(e_ref, 1e-300):.3g} "
          f"got/eps={e_got / (EPS * scale):.3g} | {what}")
    if e_got > b:
        r, p = np.unravel_index(int(np.argmax(np.abs(got - np.asarray(exact)))), got.shape)
        raise AssertionError(f"{what}: E_got = {e_got:.3e} > bar {b:.3e} (E_ref = {e_ref:.3e}, scale = {scale:.3e}); worst at row {r}, pixel {p}")
    return b


# ------------------------------------------------------------------------------------------------ the launchers' arithmetic
def two_kernel_takes(n_theta, n_phi, ell_max, ell_min=0):
    """large_synthesis_supported (kernels_synthesis_large.hip) and the n_theta >= 3 that every caller of build_synthesis asks for"""
    return 3 <= n_theta <= 104 and n_phi >= 1 and n_phi // 2 + 1 <= 64 and 1 <= ell_max <= 33 and 0 <= ell_min <= ell_max


def one_kernel_takes(n_theta, n_phi, ell_max, ell_min=0):
    """the shape limits of synthesis_split_plan (kernels_synthesis.hip); its list lengths and LDS budget are not restated"""
    return 3 <= n_theta <= 40 and 2 <= n_phi <= 39 and 1 <= ell_max <= 16 and 0 <= ell_min <= ell_max


def branch_of(n_theta, n_phi, L):
    """(KL, NTJ, KM, NTC): the template instances launch_synthesis_large (kernels_synthesis_large.hip) picks with ell_min = 0 --
    theta_synthesis_mfma_kernel<KL, NTJ> and phi_synthesis_folded_kernel<KM, NTC>"""
    kl, km = (L + 4) // 4, (L + 3) // 4  # K-chunks of four l values (theta stage) and of four m pairs (phi stage)
    ntj, ntc = -(-n_theta // 16), -(-(n_phi // 2 + 1) // 16)  # ring tiles of 16, column tiles of 16 over k = 0 .. n_phi / 2
    pick = lambda k: 5 if k <= 5 else (7 if k <= 7 else 9)  # noqa: E731
    return pick(kl), (3 if ntj <= 3 else ntj if ntj <= 5 else 7), pick(km), (2 if ntc <= 2 else 3 if ntc == 3 else 4)


def mix6_branch_of(n_theta, n_phi, L):
    """(KM, NTC) of the phi_synthesis_mix6_kernel<KM, NTC> that launch_phi_synthesis_mix6 picks -- the phi stage's ladder, as in
    branch_of -- or None where abd_mix6_supported (kernels_synthesis_large.hip) declines: a shape the two-kernel route does not take,
    F tiles that do not fit the LDS area of their results (2 L + 1 > n_phi), or six result tiles of 4 n_phi pixels beyond 53 KB"""
    if not (2 <= n_theta <= 104 and n_phi >= 1 and n_phi // 2 + 1 <= 64 and 1 <= L <= 33):
        return None
    if 2 * L + 1 > n_phi or 6 * 4 * n_phi * 16 > 53 * 1024:
        return None
    return branch_of(n_theta, n_phi, L)[2:]


# AsymptoticBondiData without a boost through the fused phi stage (tests/test_gpu_separable_large.py): (L, n_theta, n_phi, time steps)
M6_CASES = [
    (20, 41, 63, 9),    # <5,2>
    (21, 43, 63, 9),    # <7,2>
    (29, 59, 63, 9),    # <9,2>
    (31, 63, 63, 9),    # <9,2>  2 L + 1 = n_phi: the F tiles fill exactly the LDS area their results overwrite
    (20, 44, 64, 9),    # <5,3>  even n_phi; n_theta a multiple of 4
    (28, 57, 95, 9),    # <7,3>
    (33, 67, 95, 9),    # <9,3>
    (20, 42, 96, 9),    # <5,4>  two live rings in the last tile
    (28, 57, 127, 9),   # <7,4>
    (33, 67, 127, 9),   # <9,4>  the instance with scratch
    (20, 41, 63, 120),  # <5,2>  11 ring tiles x 120 steps > 1024 work items: the grid-stride loop and its prefetch of the next item
]


# ------------------------------------------------------------------------------------------------ group A: engine.salm2map
# (n_theta, n_phi, ell_max, spin, dense rows).  One-hot rows come on top: one_hot_modes().
A_ELL = [(9, 10, L, -2, 5) for L in (19, 20, 21, 27, 28, 29, 33)]  # every edge of KL and KM; the grid need not resolve l
A_THETA = [(nt, 6, 9, -2, 5) for nt in (3, 8, 9, 16, 17, 48, 49, 64, 65, 80, 81, 96, 97, 104)]  # ring tiles of 8 (phi stage) and 16 (theta stage)
A_PHI = [(7, nph, 9, -2, 5) for nph in (1, 2, 3, 62, 63, 64, 95, 96, 126, 127)]  # both parities at every edge of NTC
A_ROWS = [(5, 6, 4, -2, r) for r in (1, 7, 8, 9, 255, 256, 257)] + [(104, 11, 8, -2, 158)]  # wave trips of 8 steps, rows_per_block = 256;
#                                                                    13 ring tiles x 158 rows > 2048 items: the phi stage's grid stride
A_SPINS = [(33, 34, 14, s, 5) for s in range(-4, 5)]
A_PAIRS = ([(nt, 6, L, 1, 3) for L in (12, 24, 30) for nt in (40, 60, 72, 100)]      # every (KL, NTJ)
           + [(5, nph, L, -1, 3) for L in (12, 24, 30) for nph in (40, 80, 120)])    # every (KM, NTC)
A_CORNERS = [(99, 99, 24, 2, 9), (104, 127, 33, -2, 9)]  # the AsymptoticBondiData working grid; the largest shape the route takes
A_FALLBACK = [(105, 6, 6, -2, 5), (6, 128, 6, -2, 5), (9, 10, 34, -2, 5), (2, 5, 4, -2, 5)]  # just outside each limit: swsh_kernel + zgemm3m
A_CASES = A_ELL + A_THETA + A_PHI + A_ROWS + A_SPINS + A_PAIRS + A_CORNERS + A_FALLBACK


def case_id(case):
    return "x".join(str(v) for v in case[:2]) + f"-l{case[2]}-s{case[3]}-r{case[4]}"


# ------------------------------------------------------------------------------------------------ group B: WaveformGrid.from_modes
# route options of one call (all others cleared) -> family
B_ROUTES = [
    ("split", {"SCRI_AMD_NO_SYNTHESIS_EVAL": 1}),                                        # synthesis_split_kernel
    ("eval", {"SCRI_AMD_SYNTHESIS_EVAL": 1}),                                            # synthesis_eval_kernel
    ("large_b", {"SCRI_AMD_NO_SPLIT_SYNTHESIS": 1, "SCRI_AMD_NO_SYNTHESIS_EVAL": 1}),    # the two-kernel route with ell_min > 0
    ("gemm_b", {"SCRI_AMD_NO_SEPARABLE_SYNTHESIS": 1}),                                  # the dense (evaluating) product
]
B_OPTIONS = sorted({k for _, o in B_ROUTES for k in o})

# (data type, ell_min, ell_max, n_theta, n_phi, time steps)
B_SWEEP = ([("psi4", 2, L, 2 * L + 1, 2 * L + 1, 9) for L in range(2, 17)]
           + [("psi3", 1, L, 2 * L + 1, 2 * L + 1, 9) for L in range(1, 17)])  # all four list lengths and both NT of synthesis_split_plan
B_GRID_THETA = (3, 23, 24, 25, 39, 40, 41)      # NT = 24 | 40, the last n_theta the one-kernel form takes, the first it does not
B_GRID_PHI = (2, 3, 32, 33, 34, 35, 38, 39, 40)  # the Nyquist column of an even n_phi, the side columns k = 17 .. 19, the last n_phi | the first beyond
B_EDGES = ([("news", 2, L, nt, 2 * L + 1, 9) for L in (6, 16) for nt in B_GRID_THETA]
           + [("news", 2, L, 2 * L + 1, nph, 9) for L in (6, 16) for nph in B_GRID_PHI])
B_ROWS = [("psi4", 2, 6, 13, 14, n) for n in (9, 10, 11)] + [("psi4", 2, 16, 33, 34, n) for n in (10, 11)]  # odd and even row pairs
B_CASES = B_SWEEP + B_EDGES + B_ROWS

# ------------------------------------------------------------------------------------------------ group C: engine.grid_multiply
# (spin_a, ell_max_a, spin_b, ell_max_b, output_ell_max, rows): the library works on the smallest grid that resolves the product,
# W = max((l_a + l_b + output_ell_max + 1) // 2, (l_a + l_b + 2) // 2), n_theta = n_phi = 2 W + 1.
C_CASES = [
    (-2, 8, 1, 8, 16, 5),    # l_a + l_b = 16: 33 x 33, both factors through the one-kernel form with ell_min = 0
    (-2, 10, 1, 10, 20, 5),  # 20: 41 x 41, the two-kernel form
    (-2, 19, 1, 19, 4, 5),   # 38: 43 x 43 and l = 19 > 16, the two-kernel form
    (-2, 8, 1, 8, 16, 1),    # one row: the one-kernel form refuses it (the dense product runs)
    (-2, 8, 1, 8, 16, 2),    # one pair
    (-2, 8, 1, 8, 16, 3),    # a pair and a single row
]


def grid_multiply_working_ell_max(la, lb, out):
    """bms_grid_multiply's choice (engine_blocks.hip) when the caller's working_ell_max is l_a + l_b or more"""
    return max((la + lb + out + 1) // 2, (la + lb + 2) // 2, out, 1)


# ------------------------------------------------------------------------------------------------ inputs and references
def dense_rows(n_rows, n_modes, seed):
    """flat spectrum over ALL modes, l < |s| included (those must not leak into the grid)"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n_rows, n_modes)) + 1j * rng.normal(size=(n_rows, n_modes))


def one_hot_modes(n_pix, spin, ell_max):
    """mode indices (l_min = 0) of the one-hot rows: all where the matrix has at most 4e6 entries, else the edges of the (l, m) triangle"""
    lm = wigner.LM_range(0, ell_max)
    if lm.shape[0] * n_pix <= 4e6:
        return np.arange(lm.shape[0])
    ell, m = lm[:, 0], lm[:, 1]
    return np.nonzero((ell >= ell_max - 1) | (np.abs(m) >= ell_max - 1) | (m == 0) | (ell <= abs(spin) + 1))[0]


def one_hot_rows(modes, n_modes):
    a = np.zeros((len(modes), n_modes), dtype=complex)
    a[np.arange(len(modes)), modes] = 1.0
    return a


@contextlib.contextmanager
def fp64_recurrences():
    """oracle/wigner.py with its recurrences in fp64 for the duration of the block"""
    old = wigner.EXTENDED
    wigner.EXTENDED = False
    try:
        yield
    finally:
        wigner.EXTENDED = old


@functools.lru_cache(maxsize=2)  # (a quarter of a gigabyte at 104 x 127 / l <= 33: the tests of one shape follow each other)
def _harmonics(n_theta, n_phi, spin, ell_max, extended, robust_poles):
    theta = np.pi * np.arange(n_theta) / (n_theta - 1)
    phi = 2 * np.pi * np.arange(n_phi) / n_phi
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    R = quat.from_spherical_coords(th, ph).reshape(n_theta * n_phi, 4)
    with contextlib.nullcontext() if extended else fp64_recurrences():
        Y = wigner.swsh_grid(R, spin, ell_max)
    Y.setflags(write=False)
    return Y


def harmonics(n_theta, n_phi, spin, ell_max, extended=True):
    """oracle.wigner.swsh_grid at the rotors of the equiangular grid, [n_theta n_phi, (ell_max + 1)^2], read-only and cached per
    (grid, s, l); extended=False: with the recurrences in fp64"""
    assert wigner.EXTENDED
    return _harmonics(int(n_theta), int(n_phi), int(spin), int(ell_max), bool(extended), bool(quat.ROBUST_POLES))


def ring_harmonics(n_theta, n_phi, spin, ell_max, modes, extended=True):
    """sYlm of the listed modes (l_min = 0) as a separable synthesis sees the grid, [len(modes), n_theta n_phi]: swsh_grid at the rotors
    R(theta_j, 0) of the rings, times e^{i m phi_k} in np.longdouble with k m mod n_phi exact (extended=False: recurrences and phases in
    fp64).  swsh_grid at the rotors R(theta_j, phi_k) takes the phase from the rotors' fp64 components instead, whose rounding moves
    it by about m eps (2.7e-14 at 104 x 127 / l <= 33): the input's conditioning, which this reference does not carry."""
    rings = quat.from_spherical_coords(np.pi * np.arange(n_theta) / (n_theta - 1), np.zeros(n_theta))
    with contextlib.nullcontext() if extended else fp64_recurrences():
        real = wigner._real_t()
        lm = wigner.LM_range(0, ell_max)[np.asarray(modes)]
        Y = wigner.swsh_grid(rings, spin, ell_max)[:, np.asarray(modes)]  # [n_theta, modes], real up to the sign of zero
        step = 2 * real(wigner._PI) / real(n_phi)
        phase = np.exp(1j * ((lm[:, 1][:, None] * np.arange(n_phi)[None, :]) % n_phi).astype(real) * step)  # [modes, n_phi]
        out = Y.T.astype(phase.dtype)[:, :, None] * phase[:, None, :]
    return out.reshape(len(lm), n_theta * n_phi)


def exact_product(a, Y):
    """a[rows, modes] times Y[pixels, modes] (transposed), accumulated in np.clongdouble; block by block of pixels, so that the
    extended copy of Y stays small"""
    a = a.astype(np.clongdouble)
    out = np.empty((a.shape[0], Y.shape[0]), dtype=np.clongdouble)
    for p0 in range(0, Y.shape[0], 2048):
        out[:, p0 : p0 + 2048] = a @ np.ascontiguousarray(Y[p0 : p0 + 2048].T).astype(np.clongdouble)
    return out


def fp64_product(a, Y):
    """the last line of oracle/spinsfast_ref.py salm2map on harmonics already computed"""
    return np.tensordot(a, Y, axes=([-1], [-1]))
