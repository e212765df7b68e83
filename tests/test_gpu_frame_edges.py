"""GPU parity of the frame chain (kernels_frames.hip, engine_frames.hip) with long-double truths at every scan, sweep and step edge:
interval rotors and their prefix product, Jacobi and the sign scans, the pointwise rotor kernels.  Inputs, truths and the rule are in
tests/helpers/frame_cases.py; tests/test_oracle_frame_exact.py pins the truths and bounds every E_ref on the CPU.

The rule: E_got <= max(F * E_ref, G * eps * scale), E_got = max|GPU - truth|, E_ref = max|float64 host reference - truth| (the host
march, numpy.linalg.eigh, scri_amd.quaternions on the host), F <= 32 and G <= 256 whatever is measured.  Every case also asserts a
finite result, the same bits from a repeated call and from device memory, and masks no time step.  F and G (frame_cases.RULE) are the
next power of two above twice the worst ratio measured; G is measured where E_ref < 4 eps scale, where its term is the bar.

MEASURED on an MI355X (E in units of eps; got/ref = E_got / E_ref).  No cap was needed in any family.
  A. frame_from_angular_velocity against the restated rule; m = sub-steps per interval              family "frame": F = 2, G = 2
     axis     n        m         E_got   E_ref   got/ref  |  axis     n        m         E_got   E_ref   got/ref
     uniform  4        27..43    0.76    3.06    0.25     |  graded   4        1..5      0.61    1.08    0.57
     uniform  5        26..43    0.68    5.11    0.13     |  graded   5        1..5      0.70    0.84    0.83
     uniform  63       23..43    3.82    12.4    0.31     |  graded   63       1..33     1.19    12.9    0.09
     uniform  64       23..43    2.44    12.3    0.20     |  graded   64       1..33     1.40    7.23    0.19
     uniform  65       23..43    2.54    16.3    0.16     |  graded   65       1..33     1.73    7.72    0.22
     uniform  255      23..43    3.08    24.4    0.13     |  graded   255      1..40     2.45    9.47    0.26
     uniform  256      23..43    4.04    20.3    0.20     |  graded   256      1..40     1.94    14.5    0.13
     uniform  257      23..43    7.26    29.8    0.24     |  graded   257      1..40     2.77    7.84    0.35
     uniform  511      23..43    6.77    28.4    0.24     |  graded   511      1..41     2.39    27.2    0.09
     uniform  512      23..43    4.80    23.9    0.20     |  graded   512      1..41     3.33    16.2    0.21
     uniform  513      23..43    5.21    26.1    0.20     |  graded   513      1..41     2.49    16.5    0.15
     uniform  65535    23..43    347     411     0.84     |  graded   65537    1..42     68.1    443     0.15
     uniform  65536    23..43    423     545     0.78     |
     uniform  65537    23..43    494     761     0.65     |  uniform n = 257 by tolerance:
     uniform  65793    23..43    406     786     0.52     |  1 (amax 0.2)       1..2       4.43    8.6     0.52
     uniform  131072   23..43    518     1310    0.40     |  1e-20 (amax 1e-3)  177..336   10.2    63.2    0.16
     uniform  131073   23..43    345     721     0.48     |  0 = 1e-12: the same bits
     against the closed form (commuting sub-steps)                                             family "frame_exact": F = 1, G = 2
     uniform  5        32..33    0.65    1.94    0.33
     uniform  257      30..33    4.51    18.4    0.25
     uniform  65537    30..33    73.2    525     0.14
     n = 4, the middle interval at MAX_SUBSTEPS = 2^20 (host march: 1.16e6 steps)   125   354   0.35;  one call takes 0.6 .. 0.8 s
  B. dominant_axis, 257 matrices per family; scale = 1 / gap in the gap families          family "axis": F = 2, G = 2
     family     E_got      E_ref      got/ref   E_got / scale
     generic    4.72       6.01       0.79      4.72
     gap 1e-3   510        1.52e3     0.34      0.51
     gap 1e-6   5.45e5     1.39e6     0.39      0.55
     gap 1e-9   4.99e8     1.22e9     0.41      0.50
     plane 01   0.47       0.88       0.53      0.47
     plane 02   0.45       4.00       0.11      0.45
     plane 12   0.47       0.79       0.60      0.47
     tiny       2e-21      4.50       5e-22     2e-21     (the eigenvector is e_k to 1e-20; eigh is 4.5 eps off)
     jumpy 513  1.35       4.27       0.32      1.35      (anchors 255 and 256, both signs of rough)
     Rayleigh quotient of the result where the two top eigenvalues are equal               family "axis_rayleigh": F = 2, G = 1
     tie_diag   0          0          -         0         (the axis is exactly one of the tied places)
     tie_rotated 15.1      15.4       0.98      0.47      (scale 31.9)
     diag0..2: exactly +e_k; zero: (0, 0, 1) times the anchor's sign; generic * 2^-500 and * 2^+500, and NaN above the diagonal:
     the same bits.  Sign scans: equal to the loop at every size, anchor and sign of rough, on the series with jumps everywhere and
     on the quiet one (one jump: only there does a block total or the carry between chunks of totals reach the result).
  C. rotor_angular_velocity ("omega": F = 16, G = 32; scale = max(1, max|omega|)) and minimal_rotation x1 / x2 / x3 ("minrot": F = 4, G = 8)
     axis     n      omega E_got  E_ref  got/ref  scale |  minrot E_got           E_ref                 worst got/ref
     uniform  4      1.50   0.30   5.09     1     |  0.21 / 0.44 / 0.49     0.21 / 0.44 / 0.49    1.00
     uniform  5      1.09   0.47   2.34     1     |  0.44 / 0.37 / 0.45     0.44 / 0.37 / 0.45    1.00
     uniform  255    3.00   5.00   0.60     1.13  |  18.1 / 0.87 / 0.88     25.1 / 1.05 / 0.91    0.96
     uniform  256    3.11   3.13   1.00     1.14  |  18.1 / 0.87 / 1.05     25.1 / 1.23 / 1.26    0.83
     uniform  257    3.88   4.12   0.94     1.14  |  18.1 / 1.21 / 0.97     25.1 / 1.21 / 1.43    1.01
     uniform  1025   41.1   7.29   5.63     4.22  |  334 / 7.19 / 5.27      496 / 15.7 / 12.3     0.67
     graded   4      0.57   1.01   0.57     1     |  0.35 / 0.35 / 0.35     0.35 / 0.35 / 0.35    1.00
     graded   5      0.98   1.33   0.74     1     |  0.24 / 0.21 / 0.22     0.24 / 0.21 / 0.22    1.00
     graded   255    0.88   1.30   0.68     1     |  3.09 / 3.56 / 12.2     2.26 / 8.14 / 27.9    1.37
     graded   256    3.29   1.30   2.53     1     |  2.28 / 3.56 / 12.2     2.26 / 4.06 / 12.0    1.02
     graded   257    1.15   1.30   0.88     1     |  2.59 / 4.13 / 21.0     2.26 / 4.05 / 12.0    1.75
     graded   1025   2.32   8.66   0.27     1.28  |  23.5 / 46.6 / 137      100 / 74.2 / 281      0.63
     frame_adjust ("adjust": F = 4, G = 4), n = 4 .. 1025: E_got 0.20 .. 1.62, E_ref 0.30 .. 1.63, worst got/ref 1.33 (with `right`, n = 4);
     the rounded logarithm times 2^39 is an integer within 0.5 of the truth's (never beyond it: 0.5 - 0.25 eps 2^39 at the closest).
     Axis -z: on modes (l, +-l) alone the device's <LL> is exactly diagonal, the axis is -e_z bit for bit and the frame is (0, 1, 0, 0)
     exactly; on the reference's constant waveform the device's <LL> has off-diagonal elements of 1.4e-12 beside a diagonal of 6.9e4
     (its sums cancel in exact arithmetic only), the axis is 0.23 eps from -e_z with z = -1 exactly, and the frame is the same.

No kernel defect was found.  Two things the measurements showed about the tests themselves: with jumps everywhere every block total of
the sign scan is a constant map, which forgets what came before it, so a scan_totals_kernel without its carry passed until the quiet
series was added; and the long-double closed form of the commuting case needs its angle as a sum of two long doubles, because an
angle of 1e4 radians rounded to one long double is already 2 eps of float64 off.
"""
import time

import numpy as np
import pytest

from tests import test_squad_statement as st
from tests.helpers import frame_cases as fc

pytestmark = [pytest.mark.gpu, st.pytestmark]

LD, EPS = fc.LD, fc.EPS


def _dev(ctx, a):
    import torch

    from scri_amd import device_series

    return torch.from_numpy(np.array(a, order="C")).to(device_series.attach(ctx))


def _thrice(call, host_in, ctx, what):
    """the result of call(input) on host memory; asserts it finite, the same bits from a second call and from device memory"""
    got = call(host_in)
    assert np.isfinite(got).all(), what
    assert fc.same_bits(call(host_in), got), f"{what}: a repeated call gives other bits"
    on_dev = call(_dev(ctx, host_in))
    assert on_dev.is_cuda and fc.same_bits(on_dev.cpu().numpy(), got), f"{what}: device memory gives other bits"
    return got


def _frame(ctx, c, tolerance=1e-12):
    from scri_amd import engine

    got = _thrice(lambda om: engine.frame_from_angular_velocity(c["t"], om, R0=fc.R0, tolerance=tolerance, ctx=ctx), c["om"], ctx, "frame")
    assert fc.same_bits(got[0], fc.R0)
    drift = float(np.abs(np.linalg.norm(got, axis=1) - 1).max())
    assert drift <= 4 * EPS, drift  # one normalisation per step: four quotients by a correctly rounded norm
    return got


# ================================================================================================ A
@pytest.mark.parametrize("kind,n", [("uniform", n) for n in fc.FRAME_SIZES] + [("graded", n) for n in fc.GRADED_FRAME_SIZES])
def test_frame_against_the_restated_rule(ctx, kind, n):
    from scri_amd import engine

    assert engine.frame_scan_blocks(n) == fc.FRAME_SIZES[n]
    c = fc.frame_case(kind, n)
    assert fc.clear_of_integers(c["ratio"]) >= 1e-9
    if kind == "graded" and n >= 63:
        assert c["m"].min() == 1 and c["m"].max() >= 10
    fc.check("frame", _frame(ctx, c), c["truth"], c["ref"], f"frame {kind} n={n} (m = {c['m'].min()} .. {c['m'].max()})", scale=1.0)


def test_frame_tolerances_and_the_clamps(ctx):
    got = {}
    for tol in fc.TOLERANCES:
        c = fc.frame_case("uniform", 257, tol)
        got[tol] = _frame(ctx, c, tol)
        fc.check("frame", got[tol], c["truth"], c["ref"], f"frame uniform n=257 tolerance {tol:g} (m = {c['m'].min()} .. {c['m'].max()})", scale=1.0)
    assert fc.same_bits(got[0.0], got[1e-12])
    assert not fc.same_bits(got[1.0], got[1e-12]) and not fc.same_bits(got[1e-20], got[1e-12])


@pytest.mark.parametrize("n", fc.EXACT_SIZES)
def test_frame_against_the_closed_form(ctx, n):
    c = fc.commuting_case(n)
    assert fc.clear_of_integers(c["ratio"]) >= 1e-9
    fc.check("frame_exact", _frame(ctx, c), c["truth"], c["ref"], f"commuting frame n={n} (m = {c['m'].min()} .. {c['m'].max()})", scale=1.0)


def test_frame_at_the_cap_of_substeps(ctx):
    """One interval of 2^20 sub-steps in one thread (the host march takes 1.16e6 there: for commuting steps that changes rounding only)."""
    from scri_amd import engine

    c = fc.capped_case()
    assert c["m"][1] == fc.MAX_SUBSTEPS and c["ratio"][1] > fc.MAX_SUBSTEPS
    engine.frame_from_angular_velocity(c["t"], c["om"], R0=fc.R0, ctx=ctx)
    start = time.perf_counter()
    engine.frame_from_angular_velocity(c["t"], c["om"], R0=fc.R0, ctx=ctx)
    print(f"TIME one call with an interval at the cap: {time.perf_counter() - start:.3f} s")
    fc.check("frame_exact", _frame(ctx, c), c["truth"], c["ref"], "frame with an interval at MAX_SUBSTEPS", scale=1.0)


# ================================================================================================ B
def _axis(ctx, ll, rough=(1.0, 1.0, 1.0), anchor=0, what="axis"):
    from scri_amd import engine

    return _thrice(lambda a: engine.dominant_axis(a, rough=rough, rough_index=anchor, ctx=ctx), ll, ctx, what)


@pytest.mark.parametrize("name", fc.ACCURACY_FAMILIES)
def test_axis_against_the_eigen_truth(ctx, name):
    ll = fc.axis_family(name)
    top, v, gap = fc.axis_truth(name)
    g = fc.nominal_gap(name)
    assert (float(gap.min()) >= 0.05) if g is None else (0.5 * g <= float(gap.min()) and float(gap.max()) <= 2 * g)
    got = _axis(ctx, ll, what=name)
    assert float(np.abs(np.linalg.norm(got, axis=1) - 1).max()) <= 4 * EPS
    fc.check("axis", fc.signed_like(got, v), v, fc.signed_like(fc.eigh_axis(ll), v), f"axis {name}", scale=1.0 if g is None else 1.0 / g)


def test_axis_of_diagonal_zero_and_tied_matrices(ctx):
    n = fc.N_AXIS
    for k in range(3):
        assert np.array_equal(_axis(ctx, fc.axis_family(f"diag{k}"), what=f"diag{k}"), np.eye(3)[np.full(n, k)])  # exactly +e_k
    for side in (1.0, -1.0):
        got = _axis(ctx, fc.axis_family("zero"), rough=(0.0, 0.0, side), what="zero")
        assert np.array_equal(got, side * np.eye(3)[np.full(n, 2)])  # (0, 0, 1) up to the anchor's sign, as eigh
    for name in ("tie_diag", "tie_rotated"):
        ll = fc.axis_family(name)
        top = fc.axis_truth(name)[0]
        got = _axis(ctx, ll, what=name)
        assert float(np.abs(np.linalg.norm(got, axis=1) - 1).max()) <= 4 * EPS
        fc.check("axis_rayleigh", fc.rayleigh_longdouble(ll, got), top, fc.rayleigh_longdouble(ll, fc.eigh_axis(ll)), f"Rayleigh quotient, {name}")
        if name == "tie_diag":  # the axis is one of the two tied places, exactly
            tied = np.diagonal(ll, axis1=1, axis2=2) == np.diagonal(ll, axis1=1, axis2=2).max(axis=1)[:, None]
            assert np.array_equal(np.abs(got).sum(axis=1), np.ones(n)) and np.all(np.abs(got)[tied].reshape(n, 2).sum(axis=1) == 1.0)


def test_axis_does_not_depend_on_scale_or_on_the_upper_triangle(ctx):
    ll = fc.axis_family("generic")
    base = _axis(ctx, ll, what="generic")
    for power in (-500, 500):
        assert fc.same_bits(_axis(ctx, ll * 2.0 ** power, what=f"generic * 2^{power}"), base), power
    for name in ("generic", "gap1e-6", "plane02"):
        ll = fc.axis_family(name)
        upper = ll.copy()
        upper[:, 0, 1] = upper[:, 0, 2] = upper[:, 1, 2] = np.nan
        assert fc.same_bits(_axis(ctx, upper, what=f"{name}, NaN above the diagonal"), _axis(ctx, ll, what=name)), name


@pytest.mark.parametrize("quiet", [False, True], ids=["jumps", "quiet"])
@pytest.mark.parametrize("n", fc.SIGN_SIZES)
def test_sign_scans_against_the_loop(ctx, n, quiet):
    from scri_amd import engine

    ll, raw = fc.sign_series(n, quiet)
    if n > 1:
        fc.assert_neighbour_cosines_clear_of_half(raw)
        assert set(np.unique(np.sum(raw[1:] * raw[:-1], axis=1))) <= {0.0, 1.0}
    ll_dev = _dev(ctx, ll)
    for anchor in fc.sign_anchors(n):
        for rough in (np.ones(3), -np.ones(3)):
            ref = fc.sign_loop(n, quiet)(rough, anchor)
            got = engine.dominant_axis(ll, rough=rough, rough_index=anchor, ctx=ctx)
            assert np.array_equal(got, ref), (n, anchor, rough[0], int(np.sum(np.any(got != ref, axis=1))))
            on_dev = engine.dominant_axis(ll_dev, rough=rough, rough_index=anchor, ctx=ctx)
            assert fc.same_bits(on_dev.cpu().numpy(), got), (n, anchor, rough[0])
    assert fc.same_bits(engine.dominant_axis(ll, rough=rough, rough_index=anchor, ctx=ctx), got)  # a repeated call


def test_sign_scan_of_a_jumpy_series_across_a_block_edge(ctx):
    ll = fc.jumpy_series()
    n = ll.shape[0]
    raw = fc.eigh_axis(ll)
    fc.assert_neighbour_cosines_clear_of_half(raw)
    top, v, gap = fc.top_longdouble(ll)
    assert float(gap.min()) >= 0.05
    for anchor in (255, 256):
        for rough in (np.array([0.3, -0.2, -1.0]), np.array([-0.3, 0.2, 1.0])):
            ref = fc.continuous_loop(raw, rough, anchor)
            got = _axis(ctx, ll, rough=rough, anchor=anchor, what="jumpy")
            assert np.array_equal(np.sign(np.sum(got * ref, axis=1)), np.ones(n)), (anchor, rough[2])
            truth = fc.signed_like(v, ref.astype(LD))
            fc.check("axis", got, truth, ref, f"jumpy axis, anchor {anchor}", scale=1.0)


# ================================================================================================ C
@pytest.mark.parametrize("kind", st.AXES)
def test_rotor_angular_velocity_and_minimal_rotation(ctx, kind):
    from scri_amd import engine

    for n in fc.POINT_SIZES:
        c = fc.rotor_case(kind, n)
        t, R = c["t"], c["R"]
        om = _thrice(lambda r: engine.rotor_angular_velocity(t, r, ctx=ctx), R, ctx, "rotor omega")
        fc.check("omega", om, c["om_truth"], c["om_ref"], f"rotor angular velocity {kind} n={n}")
        for it in fc.ITERATIONS:
            Rm = _thrice(lambda r: engine.minimal_rotation(t, r, iterations=it, ctx=ctx), R, ctx, "minimal rotation")
            fc.check("minrot", Rm, c["min_truth"][it], c["min_ref"][it], f"minimal rotation x{it} {kind} n={n}", scale=1.0)


def _adjust(ctx, frame, **kw):
    """(frame, log, spinors) of engine.frame_adjust on a host copy; the same bits asserted from a second call and from device memory"""
    from scri_amd import engine

    def once(f):
        log, sp = engine.frame_adjust(f, ctx=ctx, **kw)
        return [x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in (f, log, sp) if x is not None]

    first, second, third = once(frame.copy()), once(frame.copy()), once(_dev(ctx, frame))
    assert all(np.isfinite(x).all() for x in first)
    assert all(fc.same_bits(a, b) for a, b in zip(first, second)) and all(fc.same_bits(a, b) for a, b in zip(first, third))
    return first


def test_frame_adjust(ctx):
    from scri_amd import quaternions as Q

    _, G = fc.RULE["adjust"]
    for n in fc.POINT_SIZES:
        frame = fc.adjust_frame(n)
        plain = _adjust(ctx, frame)[0]
        fc.check("adjust", plain, fc.adjust_longdouble(frame, None), fc.adjust_reference(frame, None), f"frame_adjust n={n}", scale=1.0)
        assert fc.same_bits(_adjust(ctx, frame, right=(1.0, 0.0, 0.0, 0.0))[0], plain)
        truth = fc.adjust_longdouble(frame, fc.RIGHT)
        turned, spinors = _adjust(ctx, frame, right=fc.RIGHT, want_spinors=True)
        fc.check("adjust", turned, truth, fc.adjust_reference(frame, fc.RIGHT), f"frame_adjust with right, n={n}", scale=1.0)
        assert fc.same_bits(spinors, np.ascontiguousarray(turned[:, [0, 3, 2, 1]]))
        # truncation: the rounded logarithm is on the 2^-39 lattice, within half a step (and the logarithm's rounding) of the truth's
        cut, log, spinors = _adjust(ctx, frame, right=fc.RIGHT, truncate_tolerance=fc.TRUNCATE_TOLERANCE, want_log=True, want_spinors=True)
        assert fc.same_bits(_adjust(ctx, frame, right=fc.RIGHT, truncate_tolerance=fc.TRUNCATE_TOLERANCE)[0], cut)
        steps = log * fc.POW2
        assert np.array_equal(steps, np.rint(steps))
        L = fc.qlog(truth)
        off = float(np.abs(steps.astype(LD) - L * LD(fc.POW2)).max())
        scale = max(1.0, float(np.abs(L).max()))
        print(f"RULE adjust_log n={n}: | log 2^39 - truth 2^39 | = 0.5 + {(off - 0.5) / (EPS * fc.POW2 * scale):.3g} eps 2^39 scale")
        assert off <= 0.5 + G * EPS * fc.POW2 * scale
        fc.check("adjust", cut, fc.qexp(log.astype(LD)), Q.exp(log), f"frame_adjust, exp of the rounded logarithm, n={n}", scale=1.0)
        assert fc.same_bits(spinors, np.ascontiguousarray(cut[:, [0, 3, 2, 1]]))


def _minus_z_waveform(which, n):
    """modes l = 0 .. 8 [n, 81], constant in time.  "extreme": real amplitudes in the modes (l, +-l), l = 2 .. 8, alone -- every term of
    an off-diagonal element of <LL> has a zero factor, so <LL> is exactly diagonal whatever the order of its sums (asserted on the
    device's own <LL>).  "constant": the reference's constant waveform (tests/test_gpu_frame_chain.py), whose off-diagonal sums
    cancel only in exact arithmetic."""
    LM = np.array([[l, m] for l in range(0, 9) for m in range(-l, l + 1)])
    if which == "constant":
        row = (LM[:, 1] - 1j * LM[:, 1]).astype(complex)
    else:
        row = np.where((np.abs(LM[:, 1]) == LM[:, 0]) & (LM[:, 0] >= 2), 1.0 / LM[:, 0].clip(1) + 0.125 * (LM[:, 1] > 0), 0.0).astype(complex)
    return np.repeat(row[None, :], n, axis=0)


@pytest.mark.parametrize("n", [5, 257])
def test_axis_exactly_minus_z(ctx, n):
    """<LL> exactly diagonal with the largest entry in the zz place, rough = (0, 0, -1): the axis is -e_z bit for bit, and
    axis_rotor_kernel takes its w <= 1e-150 branch, the rotor (0, 1, 0, 0).  On the reference's constant waveform the device's <LL>
    has xz and yz elements at rounding level, and the axis is -e_z within the rule only; the branch is taken all the same."""
    from scri_amd import engine

    _, G = fc.RULE["adjust"]
    t = np.linspace(1.0, 100.0, n)

    def run(rough, d):
        return engine.coprecessing_frame(t, d, 0, 8, rough=rough, rough_index=0, iterations=3, want_frame=True, want_axis=True, ctx=ctx)

    for which in ("extreme", "constant"):
        data = _minus_z_waveform(which, n)
        ll = engine.angular_velocity(t, data, 0, 8, ctx=ctx, parts=True)[1]
        diag = np.diagonal(ll, axis1=1, axis2=2)
        off = float(np.abs(ll - diag[:, :, None] * np.eye(3)[None]).max())
        print(f"RULE minus_z {which} n={n}: largest off-diagonal element of the device's <LL> = {off:.3e} (diagonal {diag[0]})")
        assert np.all(diag[:, 2] > 1.5 * diag[:, 0]) and np.all(diag[:, 2] > 1.5 * diag[:, 1])  # zz is the largest by far
        frame, axis = run((0.0, 0.0, -1.0), data)
        again, dev = run((0.0, 0.0, -1.0), data), run((0.0, 0.0, -1.0), _dev(ctx, data))
        assert all(fc.same_bits(a, b) for a, b in zip((frame, axis), again)) and all(fc.same_bits(a, b) for a, b in zip((frame, axis), dev))
        assert np.isfinite(frame).all() and np.isfinite(axis).all()
        minus_z = np.repeat([[0.0, 0.0, -1.0]], n, axis=0)
        if which == "extreme":
            assert off == 0.0
            assert np.array_equal(axis, minus_z)
        print(f"RULE minus_z {which} n={n}: | axis + e_z | = {float(np.abs(axis - minus_z).max()) / EPS:.3g} eps")
        assert float(np.abs(axis - minus_z).max()) <= G * EPS and np.all(axis[:, 2] == -1.0)
        away = max(float(np.abs(frame[:, [0, 3]]).max()), float(np.abs(np.linalg.norm(frame, axis=1) - 1).max()))
        print(f"RULE minus_z {which} n={n}: (w, z) and | |R| - 1 | within {away / EPS:.3g} eps; x, y = {frame[0, 1]:.17g}, {frame[0, 2]:.17g}")
        assert away <= G * EPS  # (0, 1, 0, 0) times a rotation about z is (0, cos, -sin, 0)
        frame, axis = run((0.0, 0.0, 1.0), data)
        assert np.array_equal(axis, -minus_z) if which == "extreme" else float(np.abs(axis + minus_z).max()) <= G * EPS
        assert float(np.abs(frame - np.array([1.0, 0.0, 0.0, 0.0])).max()) <= G * EPS
