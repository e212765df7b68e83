"""Operands, references, the two rules and the case tables of tests/test_gpu_dense_product_edges.py and
tests/test_oracle_dense_product_exact.py: the plain dense products (zgemm3m_mfma_kernel<false>, <true> and dgemm_mfma_kernel of
scri_amd/csrc/kernels_gemm.hip, reached through bms_dense_product) held to a reference on operands the TEST owns.

The contract under test is the one include/scri_amd.h states for bms_dense_product.  build() lays the operands out so that every breach
of it shows:
  A   rows at pitch lda, tight (2K doubles; K for the real form) or wide (+6 doubles, the rows entered 2 x 3 doubles into the wider
      matrix, as the rotation hands over `d_data + 2 col`).  Every double that is not one of the M x K entries is NaN: the pitch gaps,
      and GUARD complex numbers before and behind the block.  A read of the rest of a pitch, of a row >= M or of a k >= K poisons a result.
  B   padded to 8 ceil(K / 8) rows x 64 ceil(N / 64) complex columns (real form: 16, 128).  Pad rows and pad columns hold FINITE garbage
      of magnitude 1e3 .. 1e4: they have to exist, they must not reach a result.  NaN guards around the padded block.
  C   pitch ldc tight or +4 doubles, everything prefilled with SENTINEL, guards of GUARD complex numbers of it on either side: after
      the call every double that is not a result must still be the sentinel, bit for bit.
  col_off / col_scale   absent, the scale alone, or both; each array lies between NaN guards.

Two rules, by kind of input:
  integers   every part of A and B an integer of [-2^20, 2^20], col_off integers below 2^40, col_scale +-2^k with |k| <= 8.  Every
      product (< 2^40; for the three-product scheme (ar + ai)(br + bi) < 2^42) and every partial sum in any order (K <= 1024: < 2^52)
      is an integer below 2^53, so the fp64 result has ONE possible value whichever form computes it in whichever order.  Reference:
      int64 arithmetic in numpy.  Rule: EQUAL BITS.  A wrong row, column, panel, k-step or tile owner has no tolerance to hide in.
  rough      standard normal parts; offsets of the size of a column of |B|; scales in [0.5, 2] with random signs.
  graded     the same with column j of B times 10^((j mod 17) - 8) and row i of A times 2^((i mod 13) - 6): under a max-norm bar every
      small column would hide behind the large ones; the bar below is per element.
  For rough and graded the exact result is accumulated in np.longdouble and the rule is a per-element bound that is DERIVED, not
  measured.  With u = 2^-53, eps = 2u, and correctly rounded fused multiply-adds summed in any order, a K-term real product P has
  |fl(P) - P| <= gamma_K sum|a||b|, gamma_n = n u / (1 - n u).  Three-product form: P1 = Ar.Br, P2 = Ai.Bi, P3 = (Ar + Ai).(Br + Bi)
  with the operand sums rounded once each (gamma_{K+2}); Re = P1 - P2 (one more rounding), Im = (P3 - P1) - P2 (two more), so every
  term carries at most gamma_{K+4}, and the terms' magnitudes add up to at most sum|ar br| + sum|ai bi| <= S for Re and to
  sum|sa sb| + sum|ar br| + sum|ai bi| <= 2 S for Im, where
      S_ij = sum_k (|ar| + |ai|)(|br| + |bi|).
  gamma_{K+4} 2 S = (K + 4) eps S to first order; the epilogue (x - off) * scale adds two roundings of a quantity bounded by
  S + |off|: one more eps.  Hence, separately for real and imaginary parts,
      |got - exact|_ij <= (K + 8) eps (S_ij + |off_j|) |scale_j|                            (both complex forms),
  the three units beyond K + 5 absorbing every second-order term (K <= 1024: (K u)^2 < 1e-26).  The four-product form sums 2K terms of total magnitude
  <= S: gamma_{2K} S = K eps S, inside the same bar.  Real form: gamma_K and two roundings: (K + 4) eps (sum|a||b| + |off|) |scale|.
  A dropped k-step or a neighbour's column is of the size of S itself: >= 1e13 bounds.
check() prints the worst ratio |got - exact| / bound of each call (pytest -s); the figures are recorded in DESIGN.md and in the GPU
module's docstring and are not used as a bar.  No constant in this module comes from the code under test."""
import collections
import functools

import numpy as np

EPS = float(np.finfo(float).eps)
GUARD = 4096  # complex numbers on either side, as tests/test_gpu_guard_regions.py
SENTINEL = 12345.0  # the same module's
COMPLEX, REAL, COMPLEX_4M = 0, 1, 2  # BMS_PRODUCT_* of include/scri_amd.h
FORM_NAMES = {COMPLEX: "complex-3M", REAL: "real", COMPLEX_4M: "complex-4M"}
KINDS = ("integers", "rough", "graded")
PITCHES = ("tight", "wide")
EPILOGUES = ("none", "scale", "both")
WIDE_LEAD = 6  # doubles in front of a wide row of A: 2 x 3, three complex columns into the wider matrix
WIDE_C = 4  # doubles behind a wide row of C

_G = 2 * GUARD  # the guards in doubles


def shape_of(form):
    """(doubles per element, tile rows, B panel columns, B rows per turn) of a form, as kernels_gemm.hip has them"""
    return (1, 128, 128, 16) if form == REAL else (2, 64, 64, 8)


# ------------------------------------------------------------------------------------------------ the launchers' arithmetic
Tiling = collections.namedtuple("Tiling", "nbm nbn st_rows_log2 super_rows super_cols n_super grid")


def tiling(form, M, N):
    """launch_zgemm3m / launch_dgemm restated: row and column tiles, the super-tile shape the default build picks, super-tiles per
    direction, the grid"""
    _, bm, bn, _ = shape_of(form)
    nbm, nbn = -(-M // bm), -(-N // bn)
    r = 5 if form == REAL else (6 if nbm >= 512 else 5)
    sr, sc = 1 << r, 64 >> r
    nsm, nsn = -(-nbm // sr), -(-nbn // sc)
    return Tiling(nbm, nbn, r, nsm, nsn, nsm * nsn, -(-(nsm * nsn) // 8) * 8 * 64)


def tile_owners(form, M, N):
    """the kernels' block -> tile map replayed for every block of the grid: {(bm, bn): [blocks that compute it]}, and the largest
    q >> 6 met.  A correct map gives every tile of the result exactly one block."""
    t = tiling(form, M, N)
    b = np.arange(t.grid)
    xcd, q = b & 7, b >> 3
    cl = 6 - t.st_rows_log2
    nsn = (t.nbn + (1 << cl) - 1) >> cl
    S, r = (q >> 6) * 8 + xcd, q & 63
    bm = ((S // nsn) << t.st_rows_log2) + (r >> cl)
    bn = ((S % nsn) << cl) + (r & ((1 << cl) - 1))
    live = (bm < t.nbm) & (bn < t.nbn)
    owners = collections.defaultdict(list)
    for blk, i, j in zip(b[live], bm[live], bn[live]):
        owners[(int(i), int(j))].append(int(blk))
    return owners, int((q >> 6).max())


# ------------------------------------------------------------------------------------------------ operands
class Operands:
    """One call's operands in host memory, laid out as the device buffers will be (build() below)."""

    def flat_result_mask(self):
        mask = np.zeros(self.c_buf.size, dtype=bool)
        rows = self.c_at + self.ldc * np.arange(self.M)[:, None] + np.arange(self.per * self.N)[None, :]
        mask[rows.reshape(-1)] = True
        return mask

    def place(self, D):
        """the C buffer as a correct call that computed D (doubles layout, M x per N) leaves it"""
        out = self.c_buf.copy()
        out[self.flat_result_mask()] = np.asarray(D, dtype=np.float64).reshape(-1)
        return out

    def result_of(self, c_after):
        return np.asarray(c_after)[self.flat_result_mask()].reshape(self.M, self.per * self.N)

    def label(self):
        return (f"{FORM_NAMES[self.form]} {self.M} x {self.N} x {self.K} {self.kind} A {self.pitch} (lda {self.lda}) C ldc {self.ldc} "
                f"epilogue {self.epilogue}")


def _guarded(block, fill):
    g = np.full(_G, fill)
    return np.concatenate([g, np.asarray(block, dtype=np.float64).reshape(-1), g])


def _doubles(Z, real):
    """M x N elements -> M x per N doubles (re, im interleaved)"""
    Z = np.ascontiguousarray(Z)
    return Z if real else Z.view(Z.real.dtype).reshape(Z.shape[0], 2 * Z.shape[1])


@functools.lru_cache(maxsize=None)
def build(form, M, N, K, kind, pitch, epilogue, seed):
    assert form in FORM_NAMES and kind in KINDS and pitch in PITCHES and epilogue in EPILOGUES and M >= 1 and N >= 1 and K >= 1
    assert K <= 1024  # the exactness argument and the second-order terms of the docstring
    per, _, panel, turn = shape_of(form)
    real = form == REAL
    rng = np.random.default_rng([seed, form, M, N, K, KINDS.index(kind), PITCHES.index(pitch), EPILOGUES.index(epilogue)])
    o = Operands()
    o.form, o.M, o.N, o.K, o.kind, o.pitch, o.epilogue, o.seed, o.real, o.per = form, M, N, K, kind, pitch, epilogue, seed, real, per
    o.k_pad, o.n_pad = -(-K // turn) * turn, -(-N // panel) * panel

    def parts(shape):
        if kind == "integers":
            return rng.integers(-(1 << 20), (1 << 20) + 1, size=shape).astype(np.float64)
        return rng.normal(size=shape)

    A = parts((M, K)) if real else parts((M, K)) + 1j * parts((M, K))
    B = parts((K, N)) if real else parts((K, N)) + 1j * parts((K, N))
    if kind == "graded":
        A = A * (2.0 ** ((np.arange(M) % 13) - 6.0))[:, None]
        B = B * (10.0 ** ((np.arange(N) % 17) - 8.0))[None, :]
    o.A, o.B = A, B
    # A: the entries at their pitch, NaN everywhere else
    lead = WIDE_LEAD if pitch == "wide" else 0
    o.lda = per * K + lead
    rows = np.full((M, o.lda), np.nan)
    rows[:, lead:] = _doubles(A, real)
    o.a_buf, o.a_at = _guarded(rows, np.nan), _G + lead
    # B: padded, finite garbage in the pad rows and pad columns
    o.ldb = per * o.n_pad
    garbage = rng.uniform(1e3, 1e4, size=(o.k_pad, o.ldb)) * rng.choice([-1.0, 1.0], size=(o.k_pad, o.ldb))
    garbage[:K, : per * N] = _doubles(B, real)
    o.B_pad = garbage if real else garbage.view(np.complex128)  # k_pad x n_pad elements
    o.b_buf, o.b_at = _guarded(garbage, np.nan), _G
    # C: sentinels
    o.ldc = per * N + (WIDE_C if pitch == "wide" else 0)
    o.c_buf, o.c_at = _guarded(np.full((M, o.ldc), SENTINEL), SENTINEL), _G
    # the epilogue's arrays (per real column)
    n = per * N
    col_size = np.repeat(np.abs(B).sum(axis=0), per)
    if kind == "integers":
        off = rng.integers(-(1 << 40) + 1, 1 << 40, size=n).astype(np.float64)
        scale = rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.integers(-8, 9, size=n)
    else:
        off = rng.normal(size=n) * col_size
        scale = rng.uniform(0.5, 2.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    o.off = off if epilogue == "both" else None
    o.scale = scale if epilogue in ("scale", "both") else None
    o.off_buf = None if o.off is None else _guarded(o.off, np.nan)
    o.scale_buf = None if o.scale is None else _guarded(o.scale, np.nan)
    o.off_at = o.scale_at = _G
    for a in (o.a_buf, o.b_buf, o.c_buf, o.off_buf, o.scale_buf, o.A, o.B, o.B_pad, o.off, o.scale):
        if a is not None:
            a.setflags(write=False)  # shared among the tests that need it, and left unchanged
    return o


# ------------------------------------------------------------------------------------------------ references
def product(A, B, real, three=False):
    """A . B in the dtype of the operands, as M x per N doubles.  three: the three-product scheme of zgemm3m_mfma_kernel<false>, its
    operand sums and recombination in the order the kernel has them."""
    if real:
        return A @ B
    ar, ai, br, bi = A.real, A.imag, B.real, B.imag
    p1, p2 = ar @ br, ai @ bi
    if three:
        re, im = p1 - p2, ((ar + ai) @ (br + bi) - p1) - p2
    else:
        re, im = p1 - p2, ar @ bi + ai @ br
    D = np.empty((A.shape[0], 2 * B.shape[1]), dtype=re.dtype)
    D[:, 0::2], D[:, 1::2] = re, im
    return D


def epilogue(D, off, scale):
    """(D - col_off) * col_scale in the dtype of D; a missing array is no offset / scale 1"""
    if off is not None:
        D = D - off.astype(D.dtype)[None, :]
    if scale is not None:
        D = D * scale.astype(D.dtype)[None, :]
    return D


def fp64_result(o, three=False, A=None, B=None, off="own", scale="own"):
    """numpy's own fp64 product (three: the three-product emulation) with the epilogue: a CORRECT result for the checker's tests, and
    with other operands a defective one"""
    D = product(o.A if A is None else A, o.B if B is None else B, o.real, three)
    return epilogue(D, o.off if isinstance(off, str) else off, o.scale if isinstance(scale, str) else scale)


def exact(o):
    """integers: the one possible fp64 result, from int64 arithmetic.  Otherwise the result accumulated in np.longdouble."""
    if getattr(o, "_exact", None) is None:
        if o.kind == "integers":
            cast = (lambda z: z.astype(np.int64)) if o.real else _IntComplex
            D = product(cast(o.A), cast(o.B), o.real)
            if o.off is not None:
                D = D - o.off.astype(np.int64)[None, :]
            assert np.abs(D).max() < 1 << 53
            D = D.astype(np.float64)  # exact
            E = D if o.scale is None else D * o.scale[None, :]  # a power of two: exact
        else:
            cast = (lambda z: z.astype(np.longdouble)) if o.real else (lambda z: z.astype(np.clongdouble))
            E = epilogue(product(cast(o.A), cast(o.B), o.real), o.off, o.scale)
        E.setflags(write=False)
        o._exact = E
    return o._exact


class _IntComplex:
    """real and imaginary parts of an integer-valued complex matrix as int64 (numpy has no complex integers)"""

    def __init__(self, z):
        self.real, self.imag, self.shape = z.real.astype(np.int64), z.imag.astype(np.int64), z.shape


def bound(o):
    """the per-element bar of the docstring, M x per N, in np.longdouble"""
    if getattr(o, "_bound", None) is None:
        ld = np.longdouble
        if o.real:
            S, c = np.abs(o.A).astype(ld) @ np.abs(o.B).astype(ld), o.K + 4
        else:
            S = (np.abs(o.A.real) + np.abs(o.A.imag)).astype(ld) @ (np.abs(o.B.real) + np.abs(o.B.imag)).astype(ld)
            S, c = np.repeat(S, 2, axis=1), o.K + 8
        off = 0 if o.off is None else np.abs(o.off).astype(ld)[None, :]
        scale = 1 if o.scale is None else np.abs(o.scale).astype(ld)[None, :]
        b = c * ld(EPS) * (S + off) * scale
        b.setflags(write=False)
        o._bound = b
    return o._bound


# ------------------------------------------------------------------------------------------------ the checker
def check(o, c_after, what=""):
    """Hold the C buffer a call left (host copy, guards included) to the contract and to the rule of o.kind.  Prints the figures first
    (pytest -s shows them); returns the worst |got - exact| / bound (0 or inf under the equal-bits rule)."""
    c_after = np.asarray(c_after)
    what = what or o.label()
    assert c_after.shape == o.c_buf.shape and c_after.dtype == np.float64
    mask = o.flat_result_mask()
    untouched = c_after[~mask].view(np.uint64) == o.c_buf[~mask].view(np.uint64)
    if not untouched.all():
        at = int(np.flatnonzero(~mask)[int(np.argmin(untouched))]) - o.c_at
        raise AssertionError(f"{what}: a write outside the results, {at} doubles from C[0][0] (row {at // o.ldc}, double {at % o.ldc} of the pitch)")
    got = o.result_of(c_after)
    if not np.isfinite(got).all():
        r, c = np.argwhere(~np.isfinite(got))[0]
        raise AssertionError(f"{what}: non-finite result at row {r}, double {c}: something outside the operands was read, or a result not written")
    E = exact(o)
    if o.kind == "integers":
        same = got.view(np.uint64) == E.view(np.uint64)
        print(f"RULE {FORM_NAMES[o.form]} equal-bits={bool(same.all())} | {what}")
        if not same.all():
            r, c = np.argwhere(~same)[0]
            raise AssertionError(f"{what}: {int((~same).sum())} results differ from the integer reference, first at row {r}, double {c}: "
                                 f"got {got[r, c]!r}, expected {E[r, c]!r}")
        return 0.0
    ratio = np.abs(got.astype(np.longdouble) - E) / bound(o)
    worst = float(ratio.max())
    r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"RULE {FORM_NAMES[o.form]} got/bound={worst:.3g} at row {r}, double {c} | {what}")
    if not worst <= 1.0:
        raise AssertionError(f"{what}: |got - exact| = {worst:.3g} x the bound at row {r}, double {c} (got {got[r, c]!r}, exact {float(E[r, c])!r})")
    return worst


# ------------------------------------------------------------------------------------------------ the tables
Case = collections.namedtuple("Case", "form M N K pitch epilogue seed")

SWEEPS = {
    # form: (base, M values, N values, K values, corners)
    COMPLEX: ((70, 70, 9),
              (1, 15, 16, 17, 31, 32, 33, 47, 63, 64, 65, 96, 97, 127, 129),
              (1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 97, 128, 129, 197),
              # (6 added to the issue's list: with it every tail of 1 .. 7 k-steps occurs)
              (1, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 24, 25, 33, 50),
              ((1, 1, 1), (33, 33, 1), (65, 65, 8), (129, 197, 33), (64, 64, 16))),
    COMPLEX_4M: ((70, 70, 9), (1, 33, 65), (1, 33, 65), (1, 33, 65),
                 ((1, 1, 1), (33, 33, 1), (65, 65, 8), (129, 197, 33), (64, 64, 16))),
    REAL: ((140, 140, 18),
           (1, 16, 17, 63, 64, 65, 96, 97, 127, 128, 129, 257),
           (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 250),
           (2, 4, 6, 14, 16, 18, 30, 32, 34, 50),
           ()),
}
# where the kernels take another path: staging rows (a_ok1 ...), wave rows and fragments; fragments, wave columns and panels; the K
# turn.  A size of e ends on the edge, e + 1 is the first to cross it.
EDGES = {
    COMPLEX: dict(M=(16, 32, 64, 96), N=(16, 32, 64, 128), K=(8, 16, 24)),
    REAL: dict(M=(16, 64, 96, 128), N=(16, 64, 128), K=(16, 32)),
}
# the XCD super-tile map (integers only): more than one super-tile per direction, more than eight super-tiles (q >> 6 reaches 1), and
# the st_rows_log2 = 6 branch of launch_zgemm3m (512 row tiles or more).  (form, M, N, K): (st_rows_log2, super-tile rows x columns)
MAP_CASES = {
    (COMPLEX, 64 * 33 + 1, 64 * 3 + 5, 9): (5, 2, 2),
    (COMPLEX, 64 * 65 + 1, 64 * 5 + 1, 9): (5, 3, 3),
    (COMPLEX, 64 * 512 + 1, 65, 9): (6, 9, 2),
    (REAL, 128 * 32 + 1, 257, 6): (5, 2, 2),
    (REAL, 128 * 65 + 1, 128 * 5 + 1, 6): (5, 3, 3),
}


def sweep_cases(form):
    """one-at-a-time around the base shape, then the corners; both pitches and the three epilogues dealt round-robin, so that over any
    six consecutive cases every pitch meets every epilogue (and, each case running with all three kinds, every kind)"""
    (m0, n0, k0), Ms, Ns, Ks, corners = SWEEPS[form]
    shapes = [(m, n0, k0) for m in Ms] + [(m0, n, k0) for n in Ns] + [(m0, n0, k) for k in Ks] + list(corners)
    return [Case(form, m, n, k, PITCHES[i % 2], EPILOGUES[i % 3], i) for i, (m, n, k) in enumerate(shapes)]


def map_cases():
    return [Case(form, m, n, k, PITCHES[i % 2], EPILOGUES[(i + 2) % 3], 900 + i) for i, (form, m, n, k) in enumerate(MAP_CASES)]


def case_id(c):
    return f"{FORM_NAMES[c.form]}-{c.M}x{c.N}x{c.K}-{c.pitch}-{c.epilogue}"
