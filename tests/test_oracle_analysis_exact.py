"""The extended-precision analysis reference of tests/helpers/analysis_cases.py (exact_map2salm, exact_matrix) pinned before
tests/test_gpu_analysis_edges.py leans on it.  No GPU.

  * against the fp64 oracle (oracle/spinsfast_ref.py map2salm: the quadrature as a wrapped convolution assembled into matrices) on fixed
    grids, s = -2 .. 2, both parities of n_phi and of n_theta, one grid with n_theta < 2 L + 1 (frequencies wrap);
  * against the second, FFT-route transcription map2salm_hw_fft of tests/test_oracle_independent_checks.py (sympy's d functions, no
    oracle harmonics) on its three grids;
  * the condition of the GPU module: on EVERY shape of its tables the fp64 oracle lies within 32 eps scale of the exact result -- a
    shape where the yardstick itself is further off could not discriminate;
  * the band-limited round trip in extended precision: synthesis and analysis with unrounded harmonics return the modes to a few
    np.longdouble ulps, so weights, fold and phases are exact and not merely good to fp64;
  * a deliberately wrong analysis is caught: the Nyquist term of the theta weights dropped; the phase of one pole ring flipped; one
    pixel's weight off in the 14th digit, which white noise lets through at the older flat bar and under the rule and the one-hot rows
    reject."""
import numpy as np
import pytest

from oracle import quat, spinsfast_ref, wigner
from tests.helpers import analysis_cases as an
from tests.helpers import synthesis_cases as sy
from tests.helpers.spline_cases import EPS

LD_EPS = float(np.finfo(np.longdouble).eps)
pytestmark = pytest.mark.skipif(LD_EPS > 2e-19, reason="np.longdouble carries no more than fp64 on this platform")


def _scale(x):
    return max(1.0, float(np.abs(x).max()))


# (n_theta, n_phi, ell_max): odd and even n_phi and n_theta; (9, 10, 7) and (6, 7, 5) have n_theta < 2 L + 1: the wrapped case
FIXED = [(9, 9, 3), (8, 7, 3), (7, 10, 3), (17, 18, 8), (9, 10, 7), (6, 7, 5)]


@pytest.mark.parametrize("n_theta,n_phi,L", FIXED)
@pytest.mark.parametrize("s", [-2, -1, 0, 1, 2])
def test_exact_map2salm_agrees_with_the_fp64_oracle(s, n_theta, n_phi, L):
    """bar: the fp64 oracle sums n_phi + 2 n_theta products per mode through two matrix stages, each entry good to a few eps: 32 eps
    scale, the condition the GPU module's tables are held to below"""
    f = an.noise_rows(3, n_theta, n_phi, seed=100 * n_theta + 10 * n_phi + s)
    exact = an.exact_map2salm(f, s, L)
    assert exact.dtype == np.clongdouble and exact.shape == (3, (L + 1) ** 2)
    assert not exact[:, : s * s].any()
    err = float(np.abs(spinsfast_ref.map2salm(f, s, L) - exact).max())
    assert err <= 32 * EPS * _scale(exact), err / (EPS * _scale(exact))
    # ell_min only cuts columns
    assert np.array_equal(an.exact_map2salm(f, s, L, 2), exact[:, 4:])


@pytest.mark.parametrize("n_theta,n_phi", [(9, 9), (8, 7), (7, 10)])
@pytest.mark.parametrize("s", [-2, -1, 0, 1, 2])
def test_exact_map2salm_agrees_with_the_fft_route(s, n_theta, n_phi):
    """map2salm_hw_fft has its harmonics from sympy's d functions evaluated in fp64 and numpy's FFT: the bar of its own test against
    the oracle, 2e-13 max|modes|"""
    ind = pytest.importorskip("tests.test_oracle_independent_checks")
    f = an.noise_rows(1, n_theta, n_phi, seed=100 * n_theta + 10 * n_phi + s)[0]
    expect = ind.map2salm_hw_fft(f, s, 3)
    assert np.abs(an.exact_map2salm(f, s, 3) - expect).max() < 2e-13 * np.abs(expect).max()


def test_the_harmonics_change_sign_across_the_pole_as_the_fold_assumes():
    """sLambda_lm(2 pi - theta) = (-1)^(m+s) sLambda_lm(theta): what lets ring_weights() fold the theta circle onto the rings"""
    n_theta, L = 7, 5
    theta = np.pi * np.arange(n_theta) / (n_theta - 1)
    lm = wigner.LM_range(0, L)
    for s in (-2, -1, 0, 1, 2):
        here = wigner.swsh_grid(quat.from_spherical_coords(theta, np.zeros(n_theta)), s, L)
        there = wigner.swsh_grid(quat.from_spherical_coords(2 * np.pi - theta, np.zeros(n_theta)), s, L)
        assert np.abs(there - (-1.0) ** (lm[:, 1] + s) * here).max() < 8 * EPS
    # the weights are symmetric about the equator and sum to the sphere's area (the constant map is integrated exactly)
    for n in (3, 8, 9, 40, 41, 104):
        W = an.ring_weights(n)
        assert W.dtype == np.longdouble and abs(W.sum() - 4 * wigner._PI) < 64 * n * LD_EPS
        assert np.abs(W - W[::-1]).max() < 64 * LD_EPS


def test_one_hot_matrix_is_the_analysis_of_unit_maps():
    """exact_matrix (no sum) against exact_map2salm on one-hot rows: the same numbers to extended rounding"""
    n_theta, n_phi, L, s = 9, 10, 6, -2
    pixels = an.one_hot_pixels(n_theta, n_phi)
    assert np.array_equal(pixels, np.arange(90))
    f = an.one_hot_rows(pixels, n_theta, n_phi)
    A = an.exact_matrix(s, L, 2, n_theta, n_phi, pixels)
    assert np.abs(A - an.exact_map2salm(f, s, L, 2)).max() < 8 * LD_EPS
    assert np.abs(A - spinsfast_ref.map2salm_matrix(s, L, n_theta, n_phi).T[:, 4:]).max() < 32 * EPS
    # the subset of a grid too large for all pixels: both poles, first and last ring of every 8-ring tile, five columns each
    sub = an.one_hot_pixels(104, 127)
    assert len(sub) == 26 * 5 and {p // 127 for p in sub} == {j for j in range(104) if j % 8 in (0, 7)}
    assert {p % 127 for p in sub} == {0, 1, 63, 64, 126}


# every distinct shape of group A, ordered so that calls sharing the oracle's theta matrices (s, l, n_theta) follow each other
_A_SHAPES = sorted({c._replace(env=None, rows=min(c.rows, 9)) for c in an.A_CASES}, key=lambda c: (c.spin, c.L, c.n_theta, c.n_phi, c.ell_min, c.kind))


@pytest.mark.parametrize("c", _A_SHAPES, ids=an.case_id)
def test_the_fp64_oracle_discriminates_on_every_tabled_shape(c):
    """the condition of tests/test_gpu_analysis_edges.py: E_ref <= 32 eps scale on every shape of its tables (row counts cut to 9:
    the rows are independent)"""
    f, exact, ref = an.case_inputs(c)
    assert exact.shape == ref.shape == (f.shape[0], an.n_out_of(c.L, c.ell_min))
    e_ref, scale = float(np.abs(ref - exact).max()), _scale(exact)
    print(f"E_ref = {e_ref / (EPS * scale):.3g} eps scale | {an.case_id(c)}")
    assert e_ref <= 32 * EPS * scale


@pytest.mark.parametrize("n_theta,n_phi,L,s", [(9, 9, 4, -2), (17, 18, 8, 1), (33, 33, 16, 0), (13, 12, 5, 2)])
def test_band_limited_round_trip_is_exact_in_extended_precision(n_theta, n_phi, L, s):
    """modes -> grid -> modes with unrounded harmonics (ring_lambda(ideal=True)) and exact phases, all in np.longdouble.  bar: the
    recurrences lose about l ulp (oracle/wigner.py) and a mode is a sum over n_theta rings of weight <= 1: 16 (l + n_theta) ulps.
    (13, 12, 5): n_phi = 2 L + 2, the first even n_phi that resolves l = 5 -- its Nyquist column carries nothing of the band.)"""
    lam = an.ring_lambda(n_theta, s, L, ideal=True)
    lm = wigner.LM_range(0, L)
    a = sy.dense_rows(3, (L + 1) ** 2, seed=L).astype(np.clongdouble)
    a[:, lm[:, 0] < abs(s)] = 0
    phase = an._unit_phases(np.outer(lm[:, 1], np.arange(n_phi)), n_phi, +1)  # [modes, n_phi]
    f = np.einsum("rm,jm,mk->rjk", a, lam.astype(np.clongdouble), phase)
    back = an.exact_map2salm(f, s, L, lam=lam)
    err = float(np.abs(back - a).max())
    assert err <= 16 * (L + n_theta) * LD_EPS * _scale(a), err / LD_EPS
    # the fp64-rounded harmonics of the default reference are the same function: l ulp of fp64 from the rotors' rounded half angles
    assert np.abs(an.ring_lambda(n_theta, s, L) - lam).max() < 4 * (L + 1) * EPS


# ------------------------------------------------------------------------------------------------ a wrong kernel would be caught
def _flat_bar(ref):
    """the bar of the white-noise tests of tests/test_gpu_edge_cases.py"""
    return 2e-13 * _scale(ref)


def _apply(matrix, f):
    """a kernel whose analysis matrix is `matrix` [pixels, modes], on grid rows f: the product in extended precision, rounded to fp64"""
    return (f.reshape(f.shape[0], -1).astype(np.clongdouble) @ matrix).astype(complex)


def test_a_dropped_small_term_of_the_weights_is_caught_by_every_kind_of_row():
    """The theta weights without their Nyquist term p = M / 2, whose w(p) = 2 / (1 - p^2) is 6e-4 of the leading w(0) = 2 at n_theta = 41:
    the quadrature of a kernel that drops a term whose weight is small.  The ring weights move by 1e-5 to a few per cent (most at the
    poles, where they are smallest).  The rule rejects it on band-limited, one-hot and white-noise rows."""
    n_theta, n_phi, L, s = 41, 41, 20, 0
    wrong = an.ring_weights(n_theta, nyquist=False)
    assert 1e-5 < float(np.abs(wrong / an.ring_weights(n_theta) - 1).min()) and float(np.abs(wrong - an.ring_weights(n_theta)).max()) < 2e-4
    a, f, _ = an.band_limited_rows(2, n_theta, n_phi, s, L, 0, seed=5)
    ref = an.fp64_ref(f, s, L)
    an.check("large", ref, a, ref, "the oracle itself, band-limited")
    with pytest.raises(AssertionError, match="E_got"):
        an.check("large", an.exact_map2salm(f, s, L, weights=wrong).astype(complex), a, ref, "no Nyquist term, band-limited")
    pixels = an.one_hot_pixels(n_theta, n_phi)[::7]
    ref1 = an.fp64_ref(an.one_hot_rows(pixels, n_theta, n_phi), s, L)
    with pytest.raises(AssertionError, match="E_got"):
        an.check("large_1hot", an.exact_matrix(s, L, 0, n_theta, n_phi, pixels, weights=wrong).astype(complex),
                 an.exact_matrix(s, L, 0, n_theta, n_phi, pixels), ref1, "no Nyquist term, one-hot")
    fn = an.noise_rows(3, n_theta, n_phi, seed=6)
    with pytest.raises(AssertionError, match="E_got"):
        an.check("large", an.exact_map2salm(fn, s, L, weights=wrong).astype(complex), an.exact_map2salm(fn, s, L), an.fp64_ref(fn, s, L), "no Nyquist term, noise")


def test_a_single_wrong_pixel_weight_passes_white_noise_but_not_one_hot_rows():
    """One pixel's weight off by 3e-14 of itself: the Nyquist sample k = n_phi / 2 of an even ring in the middle of the grid.  Its
    matrix entries are up to 9e-3, so they move by up to 3e-16.  On white noise the result moves by that times one sample -- inside the
    older flat bar 2e-13 by three orders AND inside the rule (the fp64 oracle itself lies 1e-15 from the exact result).  The one-hot
    rows read the entry out by itself, where the oracle is good to 9e-17 and the kernels to 1e-17, and reject it."""
    n_theta, n_phi, L, s = 25, 38, 8, -2
    pixels = an.one_hot_pixels(n_theta, n_phi)
    good = an.exact_matrix(s, L, 2, n_theta, n_phi, pixels)
    row = 12 * n_phi + n_phi // 2
    wrong = good.copy()
    wrong[row] *= 1 + np.longdouble(3e-14)
    moved = float(np.abs(wrong - good).max())
    assert 1e-16 < moved < 1e-15, moved
    f = an.noise_rows(5, n_theta, n_phi, seed=3)
    ref, exact = an.fp64_ref(f, s, L, 2), an.exact_map2salm(f, s, L, 2)
    got_noise = _apply(wrong, f)
    assert np.abs(got_noise - ref).max() < 1e-2 * _flat_bar(ref)  # the older bar lets it through
    an.check("split", got_noise, exact, ref, "one wrong pixel weight, white noise")  # and so does the rule on white noise
    ref1 = an.fp64_ref(an.one_hot_rows(pixels, n_theta, n_phi), s, L, 2)
    an.check("split_1hot", good.astype(complex), good, ref1, "the right matrix rounded to fp64, one-hot")
    with pytest.raises(AssertionError, match=f"row {row}"):
        an.check("split_1hot", wrong.astype(complex), good, ref1, "one wrong pixel weight, one-hot")


def test_a_flipped_pole_phase_is_caught_by_one_hot_and_band_limited_rows():
    """the sign of one pole ring's phase flipped (e^{+i s phi_k} for e^{-i s phi_k}: the mistake of `(spin * k) % n_phi` with a negative
    spin) -- O(1) on that ring's entries, which are the smallest of the matrix (the pole weights fall off as 1 / n_theta^2)"""
    n_theta, n_phi, L, s = 17, 17, 8, -2
    pixels = an.one_hot_pixels(n_theta, n_phi)
    good = an.exact_matrix(s, L, 2, n_theta, n_phi, pixels)
    north = pixels // n_phi == 0
    wrong = good.copy()
    wrong[north] *= an._unit_phases(2 * s * (pixels % n_phi)[north], n_phi, +1)[:, None]
    ref1 = an.fp64_ref(an.one_hot_rows(pixels, n_theta, n_phi), s, L, 2)
    with pytest.raises(AssertionError, match="E_got"):
        an.check("split_1hot", wrong.astype(complex), good, ref1, "flipped pole phase, one-hot")
    a, f, _ = an.band_limited_rows(3, n_theta, n_phi, s, L, 2, seed=8)
    ref = an.fp64_ref(f, s, L, 2)
    with pytest.raises(AssertionError, match="E_got"):
        an.check("split", _apply(wrong, f), a, ref, "flipped pole phase, band-limited")
    an.check("split", _apply(good, f), a, ref, "the right matrix, band-limited")


# the analysis_fused[_wide]_kernel<NT, KS, EPT> that exist (fused_instance_exists, kernels_analysis.hip), as (wide, NT, KS, EPT)
FUSED_BUILT = ({(w, 24, 3, 2) for w in (False, True)} | {(w, 24, 5, 2) for w in (False, True)}
               | {(w, 24, 6, e) for w in (False, True) for e in (2, 3)} | {(w, 40, 3, 2) for w in (False, True)}
               | {(w, 40, ks, e) for w in (False, True) for ks in (5, 6) for e in (2, 3, 4)}) - {(False, 40, 6, 2)}


def test_the_fused_launcher_reaches_exactly_the_instances_that_are_built():
    """every shape fused_analysis_supported accepts gets one of the 21 instances, never a refusal, and each of the 21 is reached: the
    launcher's dispatch instantiates no other, so a shape outside this set would come back as hipErrorInvalidValue"""
    assert len(FUSED_BUILT) == 21
    reached = set()
    for L in range(1, 33):
        n_outs = {an.n_out_of(L, lo) for lo in range(L + 1)}
        for n_out in n_outs:
            for n_theta in range(2, 41):
                for n_phi in range(2, 48):
                    if not an.fused_takes(n_theta, n_phi, L, n_out):
                        continue
                    inst = an.fused_instance(n_theta, n_phi, L, n_out)
                    assert inst is not None, (n_theta, n_phi, L, n_out)
                    reached.add(inst[:4])
    assert reached == FUSED_BUILT, (sorted(reached - FUSED_BUILT), sorted(FUSED_BUILT - reached))
    # and the rule the predicate states: at most ceil(NT 4 KS / 256) items per thread; no <40, 6, 2> of the one-role kernel
    assert FUSED_BUILT == {(w, nt, ks, e) for w in (False, True) for nt in (24, 40) for ks in (3, 5, 6) for e in (2, 3, 4)
                           if e <= (nt * 4 * ks + 255) // 256 and (w or (nt, ks, e) != (40, 6, 2))}
    # A_CASES runs every one of them on the GPU
    ran = {an.fused_instance(c.n_theta, c.n_phi, c.L, an.n_out_of(c.L, c.ell_min))[:4] for c in an.A_CASES
           if an.family_of(c).startswith("fused")}
    assert ran == FUSED_BUILT
