"""The yardstick of the brackets of two waveforms (tests/helpers/pair_cases.py) pinned without a GPU: against the reference's own
LVector and LLComparisonMatrix (tests/golden/g13_ref_mode_calculations.npz) and against the composition of ladder operators that the
host route of scri_amd.mode_calculations evaluates (restated here in numpy: bms_mode_map with a real coefficient per column is
out[:, j] = coef[j] data[:, src[j]])."""
import os

import numpy as np
import pytest

from tests.helpers import pair_cases as pc

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(G, "g13_ref_mode_calculations.npz"), allow_pickle=False)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_yardstick_gives_the_references_vector_and_matrix(g13, tag):
    """the reference sums the same terms in double: 1e-13 of the largest value, the bar tests/test_golden.py holds the package to"""
    f, g = g13[f"{tag}_data"], g13[f"{tag}_other"]
    lmin, lmax = (int(x) for x in g13[f"{tag}_ells"])
    y = pc.yardstick(f, g, lmin, lmax)
    lv, llc = g13[f"{tag}_LVector"], g13[f"{tag}_LLComparisonMatrix"]
    got_v, got_m = pc.xyz_vector(pc.group(y, "L")[0]), pc.xyz_matrix(pc.group(y, "LL")[0])
    assert got_v.shape == lv.shape and got_m.shape == llc.shape
    assert np.abs(got_v - lv).max() < 1e-13 * np.abs(lv).max()
    assert np.abs(got_m - llc).max() < 1e-13 * np.abs(llc).max()
    assert np.all(got_m[:, 1, 2] == 0) and np.all(llc[:, 1, 2] == 0)


def _ladder_applied(data, lmin, lmax, which):
    """scri_amd.mode_calculations._ladder_applied in numpy"""
    from scri_amd.mode_algebra import LM_range

    LM = np.asarray(LM_range(lmin, lmax))
    ell, m = LM[:, 0], LM[:, 1]
    own = np.arange(ell.size)
    if which == "z":
        src, coef = own, m.astype(float)
    elif which == "+":
        src = np.where(m - 1 >= -ell, own - 1, -1)
        coef = np.sqrt(np.maximum((ell - (m - 1)) * (ell + (m - 1) + 1.0), 0.0))
    else:
        src = np.where(m + 1 <= ell, own + 1, -1)
        coef = np.sqrt(np.maximum((ell + (m + 1)) * (ell - (m + 1) + 1.0), 0.0))
    return np.where(src >= 0, coef * data[:, np.maximum(src, 0)], 0.0)


@pytest.mark.parametrize("lmin,lmax", [(0, 0), (0, 1), (2, 2), (2, 3), (3, 5), (2, 8)])
def test_yardstick_bounds_the_composition_of_ladder_operators(lmin, lmax):
    f, g = pc.pair(lmin, lmax, 7, 3)
    y = pc.yardstick(f, g, lmin, lmax)
    braket = lambda x: np.einsum("ij, ij -> i", np.conjugate(f), x)  # noqa: E731
    sign = {"p": "+", "m": "-", "z": "z"}
    assert pc.ratio(braket(g), *y["inner"]) <= 1.0
    for a in pc.L_NAMES:
        assert pc.ratio(braket(_ladder_applied(g, lmin, lmax, sign[a])), *y[a]) <= 1.0, a
    for ab in pc.LL_NAMES:
        inner = _ladder_applied(g, lmin, lmax, sign[ab[1]])
        assert pc.ratio(braket(_ladder_applied(inner, lmin, lmax, sign[ab[0]])), *y[ab]) <= 1.0, ab


def test_every_ladder_term_of_a_single_column_is_clipped():
    T = pc.terms(0, 0)
    assert all(len(T[k][0]) == 0 for k in ("p", "m", "pp", "pm", "mp", "mm", "pz", "zp", "mz", "zm"))
    assert all(len(T[k][0]) == 1 for k in ("inner", "z", "zz"))
    # m +- 2 exists only at the ends of the l = 1 block
    T = pc.terms(0, 1)
    assert T["pp"][1].tolist() == [1] and T["pp"][0].tolist() == [3] and T["mm"][1].tolist() == [3] and T["mm"][0].tolist() == [1]
    assert np.abs(T["pp"][2] - 2).max() < 1e-18 and np.abs(T["pm"][2] - 2).max() < 1e-18 and T["pm"][1].tolist() == [2, 3]
