"""The yardstick of the cut entries (tests/helpers/superrest_cut_ref.py) against the reference's own recorded values (g19), the window
identity the entry's window rule rests on, and the host side of the new interface: exported symbols, wrappers, the shape refusal.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers import superrest_cut_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
G19 = os.path.join(HERE, "golden", "g19_ref_superrest_helpers.npz")


def test_restatement_reproduces_the_recorded_reference_values():
    g = np.load(G19)
    L = int(g["ell_max"])
    modes, _, _, _ = ref.supermomentum_on_cut(g["u"], g["PsiM"], g["alpha"], L)
    d = np.abs(modes - g["PsiM_at_alpha"]).max() / np.abs(g["PsiM_at_alpha"]).max()
    da = ref.alpha_perturbation(g["PsiM_at_alpha"], g["M_at_alpha"], g["K_at_alpha"], L)
    e = np.abs(da - g["alpha_perturbation"]).max() / np.abs(g["alpha_perturbation"]).max()
    print(f"restatement against g19: PsiM_at_alpha {d:.2e}, alpha_perturbation {e:.2e} (relative)")
    assert d <= 1e-14 and e <= 1e-14
    # M and K of the row itself are what g19 recorded for it
    assert np.abs(ref.alpha_perturbation(g["PsiM_at_alpha"], None, None, L) - g["alpha_perturbation"]).max() <= 1e-14 * np.abs(g["alpha_perturbation"]).max()


@pytest.mark.parametrize("where", ["interior", "first_rows", "last_rows"])
def test_the_window_of_64_knots_holds_the_whole_series_value(where):
    """a not-a-knot cubic spline forgets data 64 knots away like 0.268^64 = 3e-37: on the window the restatement gives the value of the
    whole series, on a non-uniform axis, inside and at both clipped ends"""
    L, n = 3, 400
    rng = np.random.default_rng(5)
    t = np.cumsum(0.1 * (1.0 + 0.4 * rng.uniform(-1, 1, n)))
    data = ref.smooth_series(t, L, 11)
    centre = {"interior": t[200], "first_rows": t[1], "last_rows": t[-2]}[where]
    alpha = ref.smooth_alpha(L, 12, centre, 0.35)
    lo, hi = ref.rows_near(t, alpha)
    assert (lo == 0) == (where == "first_rows") and (hi == n) == (where == "last_rows") and hi - lo < n
    whole = ref.supermomentum_on_cut(t, data, alpha, L)
    part = ref.supermomentum_on_cut(t, data, alpha, L, window=(lo, hi))
    for a, b in zip(whole, part):
        assert np.abs(a - b).max() <= 1e-15 * np.abs(a).max()


def test_library_exports_and_wrappers():
    import scri_amd
    from scri_amd import _lib, engine
    from scri_amd import map_to_superrest_frame as m

    path = os.path.join(os.path.dirname(os.path.abspath(scri_amd.__file__)), "libscri_amd.so")
    lib = ctypes.CDLL(path)
    for name in ("bms_supermomentum_on_cut", "bms_alpha_perturbation"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.KERNEL_TAGS[-1] == "cut"
    assert callable(engine.supermomentum_on_cut) and callable(engine.alpha_perturbation)
    for name in ("_compute_Moreschi_supermomentum_composed", "_compute_alpha_perturbation_composed", "_target_at_composed", "composed_route"):
        assert callable(getattr(m, name)), name


def test_wrapper_refuses_modes_that_do_not_end_at_ell_max():
    from scri_amd import engine

    t = np.linspace(0.0, 1.0, 8)
    with pytest.raises(ValueError, match="ell_max"):
        engine.supermomentum_on_cut(t, np.zeros((8, 16), dtype=complex), np.zeros((9, 9)), 4)
    with pytest.raises(ValueError, match="want"):
        engine.supermomentum_on_cut(t, np.zeros((8, 25), dtype=complex), np.zeros((9, 9)), 4, want=("grid",))
    with pytest.raises(ValueError, match="ell_max"):
        engine.alpha_perturbation(np.zeros(16, dtype=complex), 4)
