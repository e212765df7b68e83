"""The integer statement of numpy.unwrap that bms_polar scans (kernels_polar.hip), checked on the host against numpy itself, and the
shared inputs of tests/test_gpu_polar.py.

The rule: with p the wrapped angles [n_rows, n_cols] and d = p[i] - p[i-1] in float64,
    k[i] = -1 if d > pi, +1 if d < -pi, else 0 (pi the float64; k[0] = 0),   K = cumsum(k) down the rows (integers),
    unwrapped = p + 2 pi K,   NaN from the first NaN angle of a column on.
It equals numpy's wrap count except where |d| lies within a rounding of pi, where numpy's rounded `mod` decides either way; the inputs
keep away from that edge: every one is built from a prescribed true phase with steps |delta| <= 2.5 rad, so |d| is either <= 2.5 or
>= 2 pi - 2.5 and the margin min| |d| - pi | is about 0.6 (asserted >= 1e-6 here and again in the GPU tests).

Inputs (`cases()`): n_rows in {1, 2, 3, T-1, T, T+1, 2T, 2T+1, 3T+5} x n_cols in {1, 5, 63, 64, 65, 77} with T = engine.POLAR_TILE_ROWS,
and one long block (16T+3 rows, 6 columns) -- with steps of at most 2.5 rad the wrap count grows by at most 0.4 per row, so a count in
the hundreds needs more rows than 3T+5.  Column j of a block is of kind j mod 6:
    0  wraps forced exactly between rows T-1 -> T and T -> T+1 (and 0 -> 1 -> 2, 2T-1 -> 2T -> 2T+1), direction alternating with j
    1  no wrap          2  constant          3  the count runs up (to 196 in the long block) and back
    4  signed zeros on the negative real axis: -1 - 0i at rows 0 and 2T, -1 + 0i at row T (a tile's first row)
    5  random steps in [-2.5, 2.5] with moduli from 1e-150 to 1e150
A single column is of kind 0."""
import functools

import numpy as np

TWO_PI = 2.0 * np.pi
MARGIN = 1e-6


def tile_rows():
    from scri_amd import engine

    return engine.POLAR_TILE_ROWS


def wrap_counts(p):
    """K[i][j] of the rule, int64 (NaN steps count 0)"""
    p = np.asarray(p, dtype=float)
    k = np.zeros(p.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        d = p[1:] - p[:-1]
        k[1:] = np.where(d > np.pi, -1, np.where(d < -np.pi, 1, 0))
    return np.cumsum(k, axis=0)


def unwrap_by_rule(p):
    """p + 2 pi K in float64, NaN from the first NaN of a column on"""
    p = np.asarray(p, dtype=float)
    out = p + TWO_PI * wrap_counts(p)
    out[np.logical_or.accumulate(np.isnan(p), axis=0)] = np.nan
    return out


def margin(p):
    """min | |d| - pi | over the steps of p (inf without steps)"""
    d = np.abs(np.diff(np.asarray(p, dtype=float), axis=0))
    d = d[np.isfinite(d)]
    return float(np.abs(d - np.pi).min()) if d.size else np.inf


def block(n_rows, n_cols, seed):
    """complex128 [n_rows, n_cols] of the kinds in the module docstring"""
    T = tile_rows()
    rng = np.random.default_rng(seed)
    i = np.arange(n_rows)
    z = np.empty((n_rows, n_cols), dtype=np.complex128)
    for j in range(n_cols):
        kind = 0 if n_cols == 1 else j % 6
        mod = np.ones(n_rows)
        if kind == 0:
            phase = np.where((i == 1) | ((i % T == 0) & (i > 0)), 4.0, 3.0) * (1.0 if (j // 6) % 2 == 0 else -1.0)
        elif kind == 1:
            phase = 0.3 * np.sin(0.37 * i + j)
            mod = 1.0 + 0.5 * np.cos(0.11 * i)
        elif kind == 2:
            phase = np.full(n_rows, 2.0)
            mod = np.full(n_rows, 0.7)
        elif kind == 3:
            phase = 0.5 + np.cumsum(np.where(i <= n_rows // 2, 2.4, -2.4))
        elif kind == 4:
            phase = np.full(n_rows, 1.0 - np.pi)
        else:
            phase = np.cumsum(rng.uniform(-2.5, 2.5, size=n_rows))
            mod = 10.0 ** rng.uniform(-150.0, 150.0, size=n_rows)
        z[:, j] = mod * (np.cos(phase) + 1j * np.sin(phase))
        if kind == 4:
            z[0, j] = complex(-1.0, -0.0)
            if n_rows > T:
                z[T, j] = complex(-1.0, 0.0)
            if n_rows > 2 * T:
                z[2 * T, j] = complex(-1.0, -0.0)
    return z


@functools.lru_cache(maxsize=1)
def cases():
    """{(n_rows, n_cols): complex128 block}, built once and shared (read-only)"""
    T = tile_rows()
    out = {}
    for a, n_rows in enumerate((1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5)):
        for b, n_cols in enumerate((1, 5, 63, 64, 65, 77)):
            out[n_rows, n_cols] = block(n_rows, n_cols, 100 * a + b)
    out[16 * T + 3, 6] = block(16 * T + 3, 6, 7)
    for z in out.values():
        z.setflags(write=False)
    return out


def test_tile_rows_is_the_kernels_constant():
    T = tile_rows()
    assert isinstance(T, int) and T >= 4


def test_rule_gives_numpys_wrap_count_on_every_gpu_input():
    worst, top = np.inf, 0
    for shape, z in cases().items():
        p = np.angle(z)
        m = margin(p)
        worst = min(worst, m)
        assert m >= MARGIN, (shape, m)
        K = wrap_counts(p)
        K_numpy = np.rint((np.unwrap(p, axis=0) - p) / TWO_PI).astype(np.int64)
        assert np.array_equal(K, K_numpy), shape
        top = max(top, int(np.abs(K).max()))
        assert np.abs(unwrap_by_rule(p) - np.unwrap(p, axis=0)).max() <= 1e-9, shape  # (numpy's float cumsum drifts; the counts are equal)
    print(f"margin min| |d| - pi | = {worst:.3f}, largest |K| = {top}")
    assert top >= 100  # the long block's count runs to the hundreds


def test_blocks_hold_what_the_gpu_tests_rely_on():
    T = tile_rows()
    z = cases()[2 * T + 1, 77]
    K = wrap_counts(np.angle(z))
    k = np.diff(K, axis=0, prepend=0)
    assert k[T, 0] == 1 and k[T + 1, 0] == -1 and k[T, 6] == -1 and k[T + 1, 6] == 1  # forced at the tile edge, both directions
    assert not k[:, 1].any() and not k[:, 2].any() and np.ptp(np.angle(z[:, 2])) == 0.0  # no wrap; constant
    assert np.signbit(z[0, 4].imag) and z[0, 4].real == -1.0 and not np.signbit(z[T, 4].imag) and z[T, 4].real == -1.0
    assert np.angle(z[0, 4]) == -np.pi and np.angle(z[T, 4]) == np.pi and np.angle(z[2 * T, 4]) == -np.pi
    K_long = wrap_counts(np.angle(cases()[16 * T + 3, 6]))[:, 3]
    assert np.abs(K_long).max() >= 100 and abs(K_long[-1]) <= 2  # to the hundreds and back


def test_numpy_poisons_a_column_from_its_first_nan_on():
    got = np.unwrap(np.array([0.0, 1.0, np.nan, 1.0, 2.0]))
    assert np.array_equal(np.isnan(got), [False, False, True, True, True]) and np.array_equal(got[:2], [0.0, 1.0])
    assert np.array_equal(np.isnan(unwrap_by_rule(np.array([0.0, 1.0, np.nan, 1.0, 2.0]))), np.isnan(got))
    # in two dimensions: only that column
    p = np.array([[0.0, 3.0], [np.nan, -3.0], [1.0, 3.0]])
    got = np.unwrap(p, axis=0)
    assert np.isnan(got[1:, 0]).all() and np.isfinite(got[:, 1]).all()
    assert np.array_equal(np.isnan(unwrap_by_rule(p)), np.isnan(got))


def test_the_pi_edge_is_where_the_rule_and_numpy_part():
    """d = nextafter(pi, 4) > pi: the rule counts a wrap, numpy's rounded mod does not; the inputs avoid it"""
    d = np.nextafter(np.pi, 4.0)
    p = np.array([0.0, d])
    assert np.rint((np.unwrap(p) - p) / TWO_PI)[1] == 0
    assert wrap_counts(p)[1] == -1
    assert margin(p) < MARGIN  # ... and such an input would be refused by the tests' condition
