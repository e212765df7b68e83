"""The long-double yardstick of the Bondi-gauge violations (tests/helpers/constraint_cases.py) against the reference's own values: the
right-hand sides, the mass-aspect sides and the violation norms that scri/asymptotic_bondi_data/constraints.py recorded for both
constructions of g26 (ell_max = 4, 41 steps), with the derivative rows from scipy.interpolate.CubicSpline as the reference takes them.
No GPU.

Observed (printed by the tests): the spline reproduces the recorded left-hand sides exactly; the right-hand sides of the three Bianchi
identities lie at 0.035 - 0.086 of the bar, that of psi3 at 0.37, that of psi4 at 0 (a copy), the two mass-aspect sides at 0.011 and
0.045; the six norms at <= 0.22 of the norm bar (psi3's; the others <= 0.02), v0's norm of 2.3e-3 included, which is spline truncation
and the same in the reference and the yardstick, not noise."""
import os

import numpy as np
import pytest

from tests.helpers import constraint_cases as cc
from tests.helpers import product_cases as pc

G26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_ref_initial_values.npz")


@pytest.fixture(scope="module")
def recorded():
    from scipy.interpolate import CubicSpline

    g = np.load(G26)
    u, L = g["u"], int(g["ell_max"])
    out = {}
    for tag in ("exact", "numeric"):
        raw = g[f"{tag}_raw"]
        d = lambda x, order: CubicSpline(u, x, axis=0).derivative(order)(u)  # noqa: E731
        rows = ([d(raw[0], 1), d(raw[1], 1), d(raw[2], 1)], d(raw[5], 1), d(raw[5], 2))
        out[tag] = (g, L, raw, rows, cc.sides(raw, *rows, L), cc.yardstick(raw, *rows, L))
    return out


@pytest.mark.parametrize("tag", ["exact", "numeric"])
def test_recorded_sides_within_the_bars(recorded, tag):
    g, L, raw, rows, sides, _ = recorded[tag]
    for k in range(3):  # the left-hand sides are the spline's derivatives: the rows the yardstick is fed
        assert np.array_equal(rows[0][k], g[f"{tag}_lhs"][k]), (tag, k)
    assert np.array_equal(raw[3], g[f"{tag}_lhs"][3]) and np.array_equal(raw[4], g[f"{tag}_lhs"][4])
    shares = []
    for k in range(5):
        _, rhs, bar = sides[k]
        shares.append(pc.ratio(g[f"{tag}_rhs"][k], rhs, bar))
    lhs, rhs, bar = sides[5]
    shares += [pc.ratio(g[f"{tag}_mass_aspect_lhs"], lhs, bar), pc.ratio(g[f"{tag}_mass_aspect_rhs"], rhs, bar)]
    print(f"g26 {tag}: recorded right-hand sides 0 .. 4 and the two mass-aspect sides at {', '.join(f'{r:.3f}' for r in shares)} of the bar")
    assert max(shares) <= 1.0, (tag, shares)


@pytest.mark.parametrize("tag", ["exact", "numeric"])
def test_recorded_norms_within_the_norm_bars(recorded, tag):
    g, L, _, _, _, (_, (norms, bars)) = recorded[tag]
    ref = g[f"{tag}_violation_norms"]  # [6, n]
    assert ref.shape == norms.T.shape
    shares = [cc.norm_ratio(ref[k], norms[:, k], bars[:, k]) for k in range(6)]
    print(f"g26 {tag}: recorded norms at {', '.join(f'{r:.3f}' for r in shares)} of the norm bar; largest norms {', '.join(f'{float(x):.2e}' for x in norms.max(axis=0))}")
    assert max(shares) <= 1.0, (tag, shares)


def test_eth_factor_is_the_series_operator():
    """the factor of the yardstick is the one DeviceModesTimeSeries.eth_GHP multiplies by, to a rounding of each"""
    import math

    from scri_amd import device_series

    for s in (1, 0, -1, -2):
        f = device_series._eth_factor(0, 6, s, True).real / math.sqrt(2)
        assert np.all(np.abs(f - cc.eth_factor(6, s)) <= 2 * cc.U * np.abs(cc.eth_factor(6, s))), s
        assert np.array_equal(f == 0, cc.eth_factor(6, s) == 0)
