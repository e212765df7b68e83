"""The yardsticks of tests/test_gpu_frame_edges.py, pinned on the CPU: the long-double truths of tests/helpers/frame_cases.py are
checked by properties they do not owe to the code they restate, and every float64 reference error E_ref that a GPU bar is a multiple
of is bounded here, so that a bad reference cannot widen a GPU bar.  Where np.longdouble has eps >= 1e-18 the module skips.

MEASURED (x86-64 long double; E_ref = max|float64 reference - truth| in units of eps, bound = next power of two above twice it):
see the table in BOUNDS below; the figures beside each entry are the measured ones."""
import numpy as np
import pytest

from oracle import spline_exact
from tests import test_squad_statement as st
from tests.helpers import frame_cases as fc

pytestmark = st.pytestmark

LD, EPS = fc.LD, fc.EPS

# what is bounded -> (bound on E_ref in units of eps times the scale of the rule, the worst figure measured): the bound is the next
# power of two above twice the measurement
BOUNDS = {
    "frame": (64.0, 29.8),              # the host march, n <= 513, both axes (worst: uniform n = 257)
    "frame_long": (4096.0, 1310.0),     # the host march, n >= 65535 (worst: uniform n = 131072; 411 .. 786 at the other sizes)
    "frame_tolerances": (128.0, 63.2),  # n = 257 at tolerance 1e-20 (336 sub-steps); 8.6 at tolerance 1
    "frame_exact": (64.0, 18.4),        # the host march against the closed form, n = 5 and 257
    "frame_exact_long": (2048.0, 525.0),  # n = 65537
    "frame_capped": (1024.0, 354.0),    # the interval of 1.16e6 sub-steps
    "axis": (16.0, 6.01),               # eigh; generic 6.01, one off-diagonal element 0.79 .. 4.0, tiny 4.5, gaps 1.2 .. 1.5 / gap
    "omega": (16.0, 6.76),              # scipy's slopes; worst graded n = 1025
    "minrot": (64.0, 27.9),             # scipy's minimal rotation, n <= 257 (worst: graded n = 255, three iterations)
    "minrot_long": (1024.0, 496.0),     # n = 1025 (worst: uniform, one iteration)
    "adjust": (4.0, 1.2),
    "adjust_exp": (4.0, 1.63),
}


def _bounded(key, e_ref, scale, what):
    print(f"E_REF {key} {e_ref / (EPS * scale):.3g} eps scale (scale {scale:.3g}) | {what}")
    assert e_ref <= BOUNDS[key][0] * EPS * scale, (what, e_ref / (EPS * scale), BOUNDS[key])


# ------------------------------------------------------------------------------------------------ A
def test_case_table_matches_the_launch_geometry():
    from scri_amd import engine

    for n, blocks in fc.FRAME_SIZES.items():
        assert engine.frame_scan_blocks(n) == blocks, n
    assert engine.frame_scan_blocks(256) == 1 and engine.frame_scan_blocks(257) == 2  # a block is 256 steps
    for n in fc.SIGN_SIZES:
        assert fc.sign_anchors(n)[0] == 0 and fc.sign_anchors(n)[-1] == n - 1
    lengths = {length for n in fc.SIGN_SIZES for a in fc.sign_anchors(n) for length in (n - a, a + 1)}
    assert {1, 256, 257, 65536, 65537} <= lengths
    for want in (1, 256, 257, 65536, 65537):  # each scan on its own
        assert any(n - a == want for n in fc.SIGN_SIZES for a in fc.sign_anchors(n))
        assert any(a + 1 == want for n in fc.SIGN_SIZES for a in fc.sign_anchors(n))


def test_omega_input_does_what_the_cases_need():
    for kind in st.AXES:
        t = fc.time_axis(kind, 513)
        om, der = fc.cubic_omega(t)
        nr = np.linalg.norm(om, axis=1)
        turn = float(np.arccos(om[0] @ om[-1] / (nr[0] * nr[-1])))
        assert turn > 1.0 and 1.5 < nr.min() and nr.max() < 4.0, (turn, nr.min(), nr.max())
        # the not-a-knot spline reproduces a cubic: the long-double slopes are the analytic derivative up to the rounding of the
        # samples (eps/2 |omega| each, divided by the smallest step, times a modest norm of the inverse spline matrix)
        s = spline_exact.slopes(t, om)
        bar = 16 * EPS * nr.max() / np.diff(t).min()
        print(f"slopes vs the analytic derivative ({kind}): {float(np.abs(s - der).max()):.3e} (bar {bar:.3e})")
        assert float(np.abs(s - der).max()) <= bar
        # successive interval rotors do not commute
        E = fc.interval_rotors_longdouble(t, om, 1e-12)
        comm = fc.mul(E[1:], E[:-1]) - fc.mul(E[:-1], E[1:])
        assert float(np.abs(comm).max()) > 1e-6


@pytest.mark.parametrize("kind", st.AXES)
def test_substep_counts(kind):
    sizes = fc.FRAME_SIZES if kind == "uniform" else fc.GRADED_FRAME_SIZES
    for n in sizes:
        c = fc.frame_case(kind, n)
        assert fc.clear_of_integers(c["ratio"]) >= 1e-9, (kind, n)
        assert c["m"].max() < fc.MAX_SUBSTEPS
        if kind == "uniform":
            assert 20 <= c["m"].min() and c["m"].max() <= 50, (n, c["m"].min(), c["m"].max())
        elif n >= 63:
            assert c["m"].min() == 1 and c["m"].max() >= 10, (n, c["m"].min(), c["m"].max())
    for tol, lo, hi in ((1.0, 1, 2), (1e-20, 150, 400), (0.0, 20, 50)):
        c = fc.frame_case("uniform", 257, tol)
        assert fc.clear_of_integers(c["ratio"]) >= 1e-9 and lo <= c["m"].min() and c["m"].max() <= hi, (tol, c["m"].min(), c["m"].max())
    assert fc.amax_of(1.0) == 0.2 and fc.amax_of(1e-20) == 1e-3 and fc.amax_of(0.0) == fc.amax_of(1e-12) == 2.0 * 1e-12 ** 0.2
    assert np.array_equal(fc.frame_case("uniform", 257, 0.0)["truth"], fc.frame_case("uniform", 257, 1e-12)["truth"])


@pytest.mark.parametrize("kind", st.AXES)
def test_host_march_against_the_restated_rule(kind):
    sizes = fc.FRAME_SIZES if kind == "uniform" else fc.GRADED_FRAME_SIZES
    for n in sizes:
        c = fc.frame_case(kind, n)
        assert float(np.abs(fc.norm(c["truth"][1:]) - 1).max()) <= 4 * float(np.finfo(LD).eps)
        assert np.array_equal(c["truth"][0], fc.R0.astype(LD)) and np.array_equal(c["ref"][0], fc.R0)
        _bounded("frame" if n <= 513 else "frame_long", fc.error(c["ref"], c["truth"]), 1.0, f"host march, {kind} n={n}")
    if kind == "uniform":
        for tol in fc.TOLERANCES:
            c = fc.frame_case("uniform", 257, tol)
            _bounded("frame_tolerances", fc.error(c["ref"], c["truth"]), 1.0, f"host march, tolerance {tol:g}")


def test_restated_rule_against_the_closed_form():
    """The commuting case: the sub-step rotors commute and two Gauss points integrate a cubic exactly, so the restated rule must
    give the closed form to long-double rounding -- a check of the restatement by something it does not contain."""
    for n in fc.EXACT_SIZES:
        c = fc.commuting_case(n)
        assert fc.clear_of_integers(c["ratio"]) >= 1e-9 and c["m"].min() >= 20
        restated = fc.prefix_frame_longdouble(fc.interval_rotors_longdouble(c["t"], c["om"], 1e-12), fc.R0)
        gap = fc.error(restated, c["truth"])
        # what is left is the restated rule's own rounding: every interval rotor a few long-double eps off, n of them multiplied
        half_angle = float(np.abs(fc.spline_integral_pairs(c["t"], c["om"][:, 0] / fc.AXIS_DYADIC[0], factor=LD(7) / 16)[0]).max())
        print(f"restated rule vs closed form, n={n}: {gap / EPS:.3g} eps (half angle {half_angle:.3g})")
        assert gap <= 8 * float(np.finfo(LD).eps) * np.sqrt(n)
        _bounded("frame_exact" if n <= 257 else "frame_exact_long", fc.error(c["ref"], c["truth"]), 1.0, f"host march vs closed form, n={n}")
    c = fc.capped_case()
    assert c["ratio"][1] > fc.MAX_SUBSTEPS and c["m"][1] == fc.MAX_SUBSTEPS and c["m"][0] < 2000 and c["m"][2] < 2000
    _bounded("frame_capped", fc.error(c["ref"], c["truth"]), 1.0, "host march vs closed form, the capped interval")


# ------------------------------------------------------------------------------------------------ B
ALL_FAMILIES = fc.ACCURACY_FAMILIES + ("diag0", "diag1", "diag2", "zero", "tie_diag", "tie_rotated")


@pytest.mark.parametrize("name", ALL_FAMILIES)
def test_eigen_truth_by_its_own_residual(name):
    A = fc.axis_family(name)
    assert A.shape == (fc.N_AXIS, 3, 3) and np.array_equal(A, np.swapaxes(A, 1, 2))
    lam, V = fc.eigen_longdouble(A)
    a = A.astype(LD)
    size = np.abs(a).reshape(-1, 9).max(axis=1)
    res = np.einsum("nij,njk->nik", a, V) - V * lam[:, None, :]
    assert np.all(np.abs(res).reshape(-1, 9).max(axis=1) <= 2.0 ** -58 * size), name
    orth = np.einsum("nji,njk->nik", V, V) - np.eye(3, dtype=LD)[None]
    assert float(np.abs(orth).max()) <= 2.0 ** -58
    top, v, gap = fc.axis_truth(name)
    assert np.all(np.abs(np.einsum("nij,nj->ni", a, v) - top[:, None] * v).max(axis=1) <= 2.0 ** -58 * size), name
    # the lower triangle alone is read
    B = A.copy()
    B[:, 0, 1] = B[:, 0, 2] = B[:, 1, 2] = np.nan
    assert np.array_equal(fc.eigen_longdouble(B)[0], lam)
    assert np.array_equal(np.linalg.eigh(B)[1], np.linalg.eigh(A)[1])


@pytest.mark.parametrize("name", fc.ACCURACY_FAMILIES)
def test_eigh_against_the_eigen_truth(name):
    A = fc.axis_family(name)
    top, v, gap = fc.axis_truth(name)
    g = fc.nominal_gap(name)
    if g is None:
        assert float(gap.min()) >= 0.05, float(gap.min())
    else:
        assert 0.5 * g <= float(gap.min()) and float(gap.max()) <= 2 * g, (float(gap.min()), float(gap.max()))
    if name.startswith("plane"):
        p, q = int(name[5]), int(name[6])
        off = np.abs(A[:, [1, 2, 2], [0, 0, 1]])
        assert np.all(np.count_nonzero(off, axis=1) == 1) and np.all(A[:, q, p] != 0)
    if name == "tiny":
        off = np.abs(A[:, [1, 2, 2], [0, 0, 1]])
        assert np.all(np.count_nonzero(off, axis=1) == 1) and off.max() < 1e-19
    ref = fc.signed_like(fc.eigh_axis(A), v)
    _bounded("axis", fc.error(ref, v), 1.0 if g is None else 1.0 / g, f"eigh, {name}")


def test_exact_axis_families():
    for k in range(3):
        top, v, gap = fc.axis_truth(f"diag{k}")
        assert np.array_equal(np.abs(v), np.eye(3, dtype=LD)[np.full(fc.N_AXIS, k)]) and float(gap.min()) >= 0.2
    top, v, gap = fc.axis_truth("zero")
    assert not top.any()
    assert np.array_equal(fc.eigh_axis(fc.axis_family("zero")), np.eye(3)[np.full(fc.N_AXIS, 2)])  # what eigh returns: (0, 0, 1)
    for name in ("tie_diag", "tie_rotated"):
        lam, _ = fc.eigen_longdouble(fc.axis_family(name))
        srt = np.sort(lam, axis=1)
        assert float(((srt[:, 2] - srt[:, 1]) / srt[:, 2]).max()) <= (0.0 if name == "tie_diag" else 8 * EPS)
        assert float(((srt[:, 2] - srt[:, 0]) / srt[:, 2]).min()) >= 0.5
        top = srt[:, 2]
        e_ref = float(np.abs(fc.rayleigh_longdouble(fc.axis_family(name), fc.eigh_axis(fc.axis_family(name))) - top).max())
        _bounded("axis", e_ref, max(1.0, float(top.max())), f"Rayleigh quotient of eigh's vector, {name}")


def test_fast_sign_loop_is_the_loop():
    for n in (1, 2, 3, 257, 513, 65537):
        ll, raw = fc.sign_series(n)
        assert np.array_equal(fc.eigh_axis(ll) if n < 1000 else raw, raw)  # the raw axis is known: e_k of the largest entry
        if n > 1:
            fc.assert_neighbour_cosines_clear_of_half(raw)
            cos = np.sum(raw[1:] * raw[:-1], axis=1)
            assert set(np.unique(cos)) <= {0.0, 1.0}
        if n > 256:
            assert np.all(cos[254:n - 1:256] == 0.0) and np.all(cos[255:n - 1:256] == 0.0)  # jumps on both sides of every block edge
        for a in fc.sign_anchors(n) if n < 1000 else (0, 256, n - 1):
            for rough in (np.ones(3), -np.ones(3)):
                assert fc.same_bits(fc.continuous_loop_on_unit_vectors(raw, rough, a), fc.continuous_loop(raw, rough, a)), (n, a)
    for n in (257, 65793):  # the quiet series: one jump, so the far end carries the sign of the anchor or of the jump
        ll, raw = fc.sign_series(n, quiet=True)
        assert np.count_nonzero(np.sum(raw[1:] * raw[:-1], axis=1) == 0.0) == 1
        for a in (0, n - 1):
            for rough in (np.ones(3), -np.ones(3)):
                ref = fc.continuous_loop(raw, rough, a)
                assert fc.same_bits(fc.sign_loop(n, True)(rough, a), ref)
                near, far = (ref[0], ref[-1]) if a == 0 else (ref[-1], ref[0])
                assert near.sum() == rough[0] and far.sum() == -1.0  # the anchor's sign up to the jump, flipped beyond it
    J = fc.jumpy_series()
    vals, vecs = np.linalg.eigh(J)
    assert ((vals[:, 2] - vals[:, 1]) / vals[:, 2]).min() >= 0.05
    fc.assert_neighbour_cosines_clear_of_half(vecs[:, :, 2])


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("kind", st.AXES)
def test_scipy_statements_against_the_long_double_ones(kind):
    for n in fc.POINT_SIZES:
        c = fc.rotor_case(kind, n)
        _bounded("omega", fc.error(c["om_ref"], c["om_truth"]), max(1.0, float(np.abs(c["om_truth"]).max())), f"rotor angular velocity, {kind} n={n}")
        for it in fc.ITERATIONS:
            assert float(np.abs(fc.norm(c["min_truth"][it]) - 1).max()) <= 4 * EPS
            _bounded("minrot" if n <= 257 else "minrot_long", fc.error(c["min_ref"][it], c["min_truth"][it]), 1.0, f"minimal rotation x{it}, {kind} n={n}")
    # what the minimal rotation is for: no angular velocity of the result about its own z axis (away from the spline ends)
    c = fc.rotor_case(kind, 1025)
    Rm = c["min_truth"][3]
    z_axis = fc.mul(fc.mul(Rm, fc.Z[None, :]), fc.conj(Rm))[:, 1:]
    along = np.sum(fc.rotor_omega_longdouble(c["t"], Rm) * z_axis, axis=1)
    before = np.sum(c["om_truth"] * fc.mul(fc.mul(c["R"].astype(LD), fc.Z[None, :]), fc.conj(c["R"].astype(LD)))[:, 1:], axis=1)
    print(f"about the own axis ({kind}): {float(np.abs(along[50:-50]).max()):.3e} after, {float(np.abs(before).min()):.3e} before")
    assert float(np.abs(along[50:-50]).max()) < 1e-6 and float(np.abs(before).min()) > 0.05


def test_frame_adjust_references():
    assert fc.POW2 == 2.0 ** 39
    for n in fc.POINT_SIZES:
        frame = fc.adjust_frame(n)
        nr = np.linalg.norm(frame, axis=1)
        assert nr.min() < 0.7 and nr.max() > 1.3 if n > 5 else True
        for right in (None, fc.RIGHT):
            truth = fc.adjust_longdouble(frame, right)
            assert float(np.abs(fc.norm(truth) - 1).max()) <= 4 * float(np.finfo(LD).eps)
            _bounded("adjust", fc.error(fc.adjust_reference(frame, right), truth), 1.0, f"normalised product, n={n}, right {right is not None}")
        # the exponential of a logarithm on the 2^-39 lattice: the host statement against the long-double one
        from scri_amd import quaternions as Q

        L = np.rint(fc.qlog(truth).astype(float) * fc.POW2) / fc.POW2
        _bounded("adjust_exp", fc.error(Q.exp(L), fc.qexp(L.astype(LD))), 1.0, f"exp of the rounded logarithm, n={n}")
