"""GPU parity of the synthesis kernels (modes -> grid: kernels_synthesis.hip, kernels_synthesis_large.hip, kernels_synthesis_eval.hip
and the dense swsh_kernel + zgemm3m route) at the GRID level, at every template branch and edge of their launchers, against the
oracle's harmonics carried in extended precision (oracle/wigner.py).  The counterpart of tests/test_gpu_spline_edges.py.

Every input is flat-spectrum -- nothing falls off with l, so the last K-chunk, the padded ring tile, the Nyquist column and the side
columns weigh as much as anything else -- and nothing is analysed back: an error orthogonal to the band stays visible.

One rule serves groups A and B (tests/helpers/synthesis_cases.py): with E_got = max|got - exact|, E_ref = max|fp64 oracle - exact| and
scale = max(1, max|exact|),
    E_got <= max(F * E_ref, G * eps * scale),     F <= 32 and G <= 256 whatever is measured.
Dense rows: exact is the input times swsh_grid (fp64-rounded) accumulated in np.clongdouble, ref the fp64 product of
oracle/spinsfast_ref.py salm2map (oracle/waveform_grid_ref.py from_modes in group B).  One-hot rows (row r = a single 1 at mode r): the
result is the synthesis matrix itself; exact is swsh_grid, ref swsh_grid with its recurrences in fp64.  The comparison is against the
oracle and its own fp64 distance, never against another route of the library.  The one-hot rows of the two-kernel route are held to a
second, sharper reference as well (family large_rings, see MEASURED).

Group A -- engine.salm2map (bms_salm2map: ell_min = 0, no offset, no scale).  launch_synthesis_large picks
theta_synthesis_mfma_kernel<KL, NTJ> + phi_synthesis_folded_kernel<KM, NTC>; synthesis_cases.branch_of restates its arithmetic and
test_case_table_reaches_every_template_instance (no GPU) holds the table to all 12 (KL, NTJ) and all 9 (KM, NTC).  Every shape runs on
the default route AND with SCRI_AMD_NO_LARGE_SYNTHESIS=1 (swsh_kernel<3> + zgemm3m), each under the rule; the default call is
repeated (same bits) and made from device memory into a tensor of NaN (same bits again).
  A_ELL       l = 19, 20, 21, 27, 28, 29, 33 on 9 x 10: every edge of KL = 5 | 7 | 9 and KM = 5 | 7 | 9
  A_THETA     n_theta = 3 .. 104 at the ring tiles of 8 (phi stage) and 16 (theta stage), the padded sixth tile of NTJ = 7 (81 .. 96)
  A_PHI       n_phi = 1 .. 127, both parities at every edge of NTC
  A_ROWS      1 .. 257 rows on 5 x 6 (wave trips of 8 steps, rows_per_block = 256); 104 x 11 with 158 rows (the phi stage's grid stride)
  A_SPINS     s = -4 .. 4 on 33 x 34, l <= 14
  A_PAIRS     l = 12 | 24 | 30 times n_theta = 40 | 60 | 72 | 100 and times n_phi = 40 | 80 | 120
  A_CORNERS   99 x 99 / l <= 24 / s = 2 and 104 x 127 / l <= 33, dense rows plus the one-hot rows at the edges of the (l, m) triangle
  A_FALLBACK  n_theta = 105, n_phi = 128, l = 34, n_theta = 2: the dense route by itself
Group B -- WaveformGrid.from_modes under the identity transformation, SCRI_AMD_NO_SMALL_DENSE=1: the one-kernel forms and the
two-kernel route with ell_min > 0.  The not-a-knot spline interpolates its samples, so once g.t equals the input axis the exact result
is the synthesis of the input rows.  Four routes per shape (synthesis_cases.B_ROUTES): synthesis_split_kernel, synthesis_eval_kernel,
the two-kernel route, the dense product.  A route that does not take a shape (n_theta = 41, n_phi = 40; the evaluating kernel where
synthesis_eval_supported declines) hands over to the launcher's next choice, under the same family.  from_modes refuses a grid of fewer than
2 l + 1 rings or columns, as the reference does; for the edge shapes below that (n_theta = 3 .. 25 at l = 16, n_phi = 2, 3 ...)
the refusal is asserted and the same engine entry (engine.transform_modes(grid=True)) is called directly: synthesis does not alias.
  B_SWEEP     ell_max = 2 .. 16 with ell_min = 2 (psi4) and 1 .. 16 with ell_min = 1 (psi3; the identity needs no companion) on (2 l + 1)^2
  B_EDGES     l = 6 and 16: n_theta in 3, 23, 24, 25, 39, 40, 41; n_phi in 2, 3, 32, 33, 34, 35, 38, 39, 40
  B_ROWS      9, 10, 11 time steps
  h and sigma with a pure l >= 1 supertranslation (the `off` column is live) and one frame rotation: the time spline takes part, so
  these are held to oracle from_modes at the bar of test_waveform_grid_from_modes_and_to_modes, 2e-12 max|grid|.
Group C -- engine.grid_multiply reaches the split kernel with ell_min = 0 (synthesis_cases.C_CASES), against
oracle/modes_time_series_ref.py at 2e-13; one row is refused by the one-kernel form and must fall through.

MEASURED on an MI355X, every call of this module (F and G of tests/helpers/synthesis_cases.py are the next power of two above twice
the first two columns; second column only over calls with E_ref < 4 eps scale; shapes as n_theta x n_phi / l_max):
  family       worst E_got/E_ref                 worst E_got/(eps scale)           worst E_got/scale: E_got, E_ref, shape
  large        30.4  104 x 127 / 33 dense        62.6  104 x 127 / 33 dense        1.4e-14: 6.0e-13, 2.0e-14, 104 x 127 / 33 dense
  gemm         8.23  40 x 6 / 30 dense           16.2  9 x 10 / 28 dense           3.6e-15: 9.8e-14, 1.6e-14, 9 x 10 / 28 dense
  large_1hot   2.69  3 x 6 / 9                   5.94  3 x 6 / 9                   1.2e-14: 2.7e-14, 3.6e-14, 104 x 127 / 33
  gemm_1hot    0.37  3 x 6 / 9                   0.81  3 x 6 / 9                   2.1e-16: 4.4e-16, 5.4e-15, 9 x 10 / 28
  large_rings  0.70  7 x 62 / 9                  1.79  7 x 95 / 9                  4.0e-16: 4.9e-16, 1.1e-15, 7 x 95 / 9
  split        14.3  news 3 x 13 / 6             24.2  news 23 x 33 / 16           7.2e-15: 1.4e-13, 1.2e-13, psi3 31 x 31 / 15
  eval         14.0  news 3 x 13 / 6             25.9  news 23 x 33 / 16           7.1e-15: 1.3e-13, 1.2e-13, psi3 31 x 31 / 15
  large_b      14.3  news 3 x 13 / 6             24.2  news 23 x 33 / 16           7.2e-15: 1.4e-13, 1.2e-13, psi3 31 x 31 / 15
  gemm_b       5.90  news 23 x 33 / 16           12.0  news 23 x 33 / 16           3.0e-15: 6.1e-14, 1.2e-13, psi4 33 x 33 / 16
  inhomogeneous term and rotation: 2.6e-15 .. 4.1e-15 of max|grid| against the bar of 2e-12; grid_multiply 2.4e-14 .. 6.1e-14 absolute at
  max|modes| = 9 .. 22 against 2e-13 max|modes|.
No case needed a change of a kernel, and every case passes within the caps.  One family touches them: for `large` the recipe gives
F = 64, so F stays AT the cap of 32 and 104 x 127 / l <= 33 passes on the G term (62.6, G = 128).  That distance belongs to the oracle's
input, not to the kernels: swsh_grid takes e^{i m phi} from the fp64 components of the rotors R(theta_j, phi_k), whose rounding moves
sYlm by about m eps -- max|swsh_grid - harmonics at the ideal angles| is 2.7e-14 at 104 x 127 / l <= 33, the very E_got of `large_1hot`
there -- while the phi stage has k m mod n_phi exactly.  Held to the rings' harmonics times exact phases (synthesis_cases.ring_harmonics:
the `large_rings` row, every one-hot call of the two-kernel route) the synthesis matrix is within 1.8 eps at every shape, 1.5 eps at
104 x 127 / l <= 33.  The dense route takes the same rounded rotors as the oracle and stays within 0.94 eps of it.  In group B the
oracle's own result (scipy's spline at its knots) lies up to 35 eps scale from the exact one; the kernels lie up to 33.
"""
import numpy as np
import pytest

from oracle import containers, wigner
from oracle import modes_time_series_ref as mref
from oracle import spinsfast_ref
from oracle import waveform_grid_ref as grid_ref
from tests.helpers import synthesis_cases as sy

gpu = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------- the case table
def test_case_table_reaches_every_template_instance():
    """no GPU: the launcher's arithmetic on the table of group A"""
    taken = [c for c in sy.A_CASES if sy.two_kernel_takes(*c[:3])]
    branches = [sy.branch_of(*c[:3]) for c in taken]
    assert {(b[0], b[1]) for b in branches} == {(kl, ntj) for kl in (5, 7, 9) for ntj in (3, 4, 5, 7)}
    assert {(b[2], b[3]) for b in branches} == {(km, ntc) for km in (5, 7, 9) for ntc in (2, 3, 4)}
    # the edges of each rule
    assert [sy.branch_of(9, 10, L)[0] for L in (19, 20, 27, 28, 33)] == [5, 7, 7, 9, 9]
    assert [sy.branch_of(9, 10, L)[2] for L in (20, 21, 28, 29, 33)] == [5, 7, 7, 9, 9]
    assert [sy.branch_of(nt, 6, 9)[1] for nt in (3, 48, 49, 64, 65, 80, 81, 96, 97, 104)] == [3, 3, 4, 4, 5, 5, 7, 7, 7, 7]
    assert [sy.branch_of(7, nph, 9)[3] for nph in (1, 62, 63, 64, 95, 96, 126, 127)] == [2, 2, 2, 3, 3, 4, 4, 4]
    # what the table must hold
    have = lambda pos: {c[pos] for c in taken}  # noqa: E731
    assert {19, 20, 21, 27, 28, 29, 33} <= have(2)
    assert {3, 8, 9, 16, 17, 48, 49, 64, 65, 80, 81, 96, 97, 104} <= have(0)
    assert {1, 2, 3, 62, 63, 64, 95, 96, 126, 127} <= have(1)
    assert {1, 7, 8, 9, 255, 256, 257} <= {c[4] for c in taken if c[:2] == (5, 6)} and (104, 11, 8, -2, 158) in taken
    assert set(range(-4, 5)) <= have(3)
    assert (99, 99, 24, 2, 9) in taken and (104, 127, 33, -2, 9) in taken
    assert [c[:3] for c in sy.A_CASES if not sy.two_kernel_takes(*c[:3])] == [(105, 6, 6), (6, 128, 6), (9, 10, 34), (2, 5, 4)]
    assert len({sy.case_id(c) for c in sy.A_CASES}) == len(sy.A_CASES)
    # group B: the shapes either side of the one-kernel form's limits
    assert sy.one_kernel_takes(40, 39, 16, 2) and not sy.one_kernel_takes(41, 39, 16, 2) and not sy.one_kernel_takes(40, 40, 16, 2)
    assert all(sy.two_kernel_takes(*c[3:5], c[2], c[1]) for c in sy.B_CASES)
    # group C: the grids the library works on
    assert [2 * sy.grid_multiply_working_ell_max(c[1], c[3], c[4]) + 1 for c in sy.C_CASES[:3]] == [33, 41, 43]


def test_mix6_case_table_reaches_every_template_instance():
    """no GPU: the table of tests/test_gpu_separable_large.py's fused-ABD test on the launcher's arithmetic -- every case is one the fused
    kernel takes (not its fallback, the unfused phi stage), and together they reach all nine phi_synthesis_mix6_kernel<KM, NTC>"""
    branches = [sy.mix6_branch_of(nt, nph, L) for L, nt, nph, _ in sy.M6_CASES]
    assert None not in branches
    assert set(branches) == {(km, ntc) for km in (5, 7, 9) for ntc in (2, 3, 4)}
    assert branches == [(5, 2), (7, 2), (9, 2), (9, 2), (5, 3), (7, 3), (9, 3), (5, 4), (7, 4), (9, 4), (5, 2)]
    assert all(n >= 8 for *_, n in sy.M6_CASES)  # fewer steps: no B-spline form, so no elimination on the modes and no fused mixing
    # the restatement declines where abd_mix6_supported does
    assert sy.mix6_branch_of(63, 63, 32) is None and sy.mix6_branch_of(63, 63, 31) == (9, 2)  # 2 L + 1 <= n_phi
    assert sy.mix6_branch_of(105, 63, 20) is None and sy.mix6_branch_of(41, 128, 20) is None and sy.mix6_branch_of(69, 127, 34) is None


# ------------------------------------------------------------------------------------------------------------- group A
def _device_salm2map(ctx, a, spin, ell_max, n_theta, n_phi):
    """bms_salm2map on device memory: the modes in a tensor, the grid into a tensor that starts as NaN"""
    import torch

    from scri_amd import _lib, device_series

    dev = device_series.attach(ctx)
    nan = complex(float("nan"), float("nan"))
    src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to(dev)
    out = torch.full((a.shape[0], n_theta * n_phi), nan, dtype=torch.complex128, device=dev)
    torch.cuda.synchronize(dev)
    rc = _lib.load().bms_salm2map(ctx.handle, _lib.c_vp(src.data_ptr()), _lib.BMS_DEVICE, a.shape[0], int(spin), int(ell_max), int(n_theta),
                                  int(n_phi), _lib.c_vp(out.data_ptr()))
    ctx.check(rc, "bms_salm2map")
    torch.cuda.synchronize(dev)
    return out.cpu().numpy()


def _salm2map_both_routes(ctx, route, case, a, exact, ref, suffix, what):
    """the default route (repeated, and from device memory) and the dense route on the same input, each under the rule"""
    from scri_amd import engine

    n_theta, n_phi, L, s = case[:4]
    call = lambda: engine.salm2map(a, s, L, n_theta, n_phi, ctx=ctx).reshape(a.shape[0], n_theta * n_phi)  # noqa: E731
    family = ("large" if sy.two_kernel_takes(n_theta, n_phi, L) else "gemm") + suffix
    got = call()
    sy.check(family, got, exact, ref, f"{what} default route")
    assert _same_bits(got, call()), f"{what}: a repeated call gives other bits"
    got_dev = _device_salm2map(ctx, a, s, L, n_theta, n_phi)
    assert np.isfinite(got_dev).all(), f"{what}: device output keeps NaN"
    assert _same_bits(got, got_dev), f"{what}: host and device-resident input give other bits"
    if family.startswith("large"):
        route("SCRI_AMD_NO_LARGE_SYNTHESIS", "1")
        try:
            sy.check("gemm" + suffix, call(), exact, ref, f"{what} NO_LARGE_SYNTHESIS")
        finally:
            route("SCRI_AMD_NO_LARGE_SYNTHESIS", None)
    return got


def _branch(case):
    return f"branch={sy.branch_of(*case[:3])}" if sy.two_kernel_takes(*case[:3]) else "dense route only"


@gpu
@pytest.mark.parametrize("kind", ["dense", "one_hot"])  # (the two kinds of a shape follow each other: they share its harmonics)
@pytest.mark.parametrize("case", sy.A_CASES, ids=sy.case_id)
def test_a_salm2map(ctx, route, case, kind):
    """dense rows: flat spectrum over all modes.  one_hot: the synthesis matrix row by row against swsh_grid at the grid's rotors, no
    product on the reference side"""
    n_theta, n_phi, L, s, rows = case
    Y = sy.harmonics(n_theta, n_phi, s, L)
    if kind == "dense":
        if n_theta * n_phi * (L + 1) ** 2 > 4e6:
            rows = min(rows, 9 if L <= 24 else 3)  # (the extended-precision product is the cost of the test at the two corners)
        a = sy.dense_rows(rows, (L + 1) ** 2, seed=n_theta * 131 + n_phi * 17 + L)
        exact, ref = sy.exact_product(a, Y), sy.fp64_product(a, Y)
        _salm2map_both_routes(ctx, route, case, a, exact, ref, "", f"A {sy.case_id(case)} {_branch(case)} dense rows")
    else:
        modes = sy.one_hot_modes(n_theta * n_phi, s, L)
        a = sy.one_hot_rows(modes, (L + 1) ** 2)
        exact = Y[:, modes].T
        ref = sy.harmonics(n_theta, n_phi, s, L, extended=False)[:, modes].T
        assert not exact[wigner.LM_range(0, L)[modes, 0] < abs(s)].any()  # the rows l < |s| are zero: what must not leak
        what = f"A {sy.case_id(case)} {_branch(case)} {len(modes)} one-hot rows"
        got = _salm2map_both_routes(ctx, route, case, a, exact, ref, "_1hot", what)
        if sy.two_kernel_takes(n_theta, n_phi, L):
            # the separable route takes the rings' rotors and the exact k m mod n_phi: held to that as well, which is sharper
            sy.check("large_rings", got, sy.ring_harmonics(n_theta, n_phi, s, L, modes), sy.ring_harmonics(n_theta, n_phi, s, L, modes, extended=False),
                     f"{what} against rings x exact phases")


def test_fp64_product_is_the_oracles_salm2map():
    """no GPU: the yardstick of the dense rows is spinsfast_ref.salm2map bit for bit (the helper only keeps the harmonics)"""
    n_theta, n_phi, L, s = 9, 10, 7, -2
    a = sy.dense_rows(3, (L + 1) ** 2, seed=1)
    assert _same_bits(sy.fp64_product(a, sy.harmonics(n_theta, n_phi, s, L)).reshape(3, n_theta, n_phi), spinsfast_ref.salm2map(a, s, L, n_theta, n_phi))
    with sy.fp64_recurrences():
        assert not wigner.EXTENDED
    assert wigner.EXTENDED
    assert np.abs(sy.harmonics(n_theta, n_phi, s, L) - sy.harmonics(n_theta, n_phi, s, L, extended=False)).max() < 1e-14


# ------------------------------------------------------------------------------------------------------------- group B
def _waveforms(ctx, name, ell_min, ell_max, t, data):
    import scri_amd

    w_o = containers.WM(t=t, data=data, ell_min=ell_min, ell_max=ell_max, dataType=getattr(containers, name))
    w_g = scri_amd.WaveformModes(t=t, data=data, ell_min=ell_min, ell_max=ell_max, dataType=getattr(scri_amd, name), frameType=scri_amd.Inertial,
                                 r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    return w_o, w_g


def _routes(route):
    """the four settings of group B, one after the other: yields the family"""
    try:
        for family, options in sy.B_ROUTES:
            for name in sy.B_OPTIONS:
                route(name, str(options[name]) if name in options else None)
            yield family
    finally:
        for name in sy.B_OPTIONS:
            route(name, None)


@gpu
@pytest.mark.parametrize("case", sy.B_CASES, ids=lambda c: f"{c[0]}-l{c[1]}-{c[2]}-{c[3]}x{c[4]}-n{c[5]}")
def test_b_from_modes_identity(ctx, route, case):
    import scri_amd
    from scri_amd import engine

    name, ell_min, ell_max, n_theta, n_phi, n = case
    route("SCRI_AMD_NO_SMALL_DENSE", "1")
    t = np.linspace(-3.0, 9.0, n)
    data = sy.dense_rows(n, (ell_max + 1) ** 2 - ell_min**2, seed=ell_max * 1000 + n_theta * 41 + n_phi)
    w_o, w_g = _waveforms(ctx, name, ell_min, ell_max, t, data)
    s = w_o.spin_weight
    assert s == w_g.spin_weight and abs(s) == ell_min
    Y = sy.harmonics(n_theta, n_phi, s, ell_max)[:, ell_min**2 :]
    exact = sy.exact_product(data, Y)
    resolved = min(n_theta, n_phi) >= 2 * ell_max + 1
    if resolved:
        t_ref, ref, nt_ref, nph_ref = grid_ref.from_modes(w_o, n_theta=n_theta, n_phi=n_phi)
        assert (nt_ref, nph_ref) == (n_theta, n_phi) and np.array_equal(t_ref, t)
        ref = ref.reshape(n, n_theta * n_phi)
    else:  # the oracle refuses the grid as the library does: the fp64 product is the yardstick
        with pytest.raises(ValueError, match="too small"):
            grid_ref.from_modes(w_o, n_theta=n_theta, n_phi=n_phi)
        with pytest.raises(ValueError, match="too small"):
            scri_amd.WaveformGrid.from_modes(w_g, n_theta=n_theta, n_phi=n_phi)
        ref = sy.fp64_product(data, Y)
        tr = engine.make_transformation(np.zeros(4, dtype=complex), [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0], n_theta, n_phi, ell_max)
    for family in _routes(route):
        if resolved:
            g = scri_amd.WaveformGrid.from_modes(w_g, n_theta=n_theta, n_phi=n_phi)
            assert (g.n_theta, g.n_phi) == (n_theta, n_phi)
            t_got, got = g.t, g.data
        else:
            t_got, got = engine.transform_modes(t, data, ell_min, ell_max, s, w_g.conformal_weight, engine.BMS_TERM_NONE, tr, ctx=ctx, grid=True)
        assert np.array_equal(t_got, t), family  # the spline is evaluated at its own knots
        sy.check(family, got, exact, ref, f"B {name} l={ell_min}..{ell_max} {n_theta}x{n_phi} n={n} {family}")


def _real_supertranslation(ell_max, seed, size):
    """alpha_lm of a real function, l = 0 left out"""
    rng = np.random.default_rng(seed)
    a = size * (rng.normal(size=(ell_max + 1) ** 2) + 1j * rng.normal(size=(ell_max + 1) ** 2))
    for ell in range(ell_max + 1):
        for m in range(ell + 1):
            ip, im = wigner.LM_index(ell, m, 0), wigner.LM_index(ell, -m, 0)
            a[ip] = (a[ip] + (-1.0) ** m * np.conj(a[im])) / 2
            a[im] = (-1.0) ** m * np.conj(a[ip])
    a[0] = 0.0
    return a


@gpu
@pytest.mark.parametrize("name,kw", [
    ("h", dict(supertranslation=_real_supertranslation(2, 11, 0.05))),
    ("sigma", dict(supertranslation=_real_supertranslation(2, 12, 0.05))),
    ("psi4", dict(frame_rotation=np.array([0.8, -0.3, 0.4, 0.2]) / np.linalg.norm([0.8, -0.3, 0.4, 0.2]))),
], ids=["h-supertranslation", "sigma-supertranslation", "psi4-rotation"])
def test_b_inhomogeneous_term_and_rotation(ctx, route, name, kw):
    """the `off` column live (h, sigma), and modes rotated before the same kernels; against oracle from_modes, the time spline included"""
    import scri_amd

    route("SCRI_AMD_NO_SMALL_DENSE", "1")
    ell_min, ell_max, n = 2, 10, 60
    t = np.linspace(-5.0, 20.0, n)
    nm = (ell_max + 1) ** 2 - ell_min**2
    data = sy.dense_rows(1, nm, seed=len(name))[0][None, :] * np.exp(1j * np.outer(0.1 * t + 1e-3 * t**2, np.arange(nm) % 5 - 2))
    w_o, w_g = _waveforms(ctx, name, ell_min, ell_max, t, data)
    t_ref, ref, n_theta, n_phi = grid_ref.from_modes(w_o, **kw)
    ref = ref.reshape(t_ref.size, -1)
    for family in _routes(route):
        g = scri_amd.WaveformGrid.from_modes(w_g, **kw)
        assert (g.n_theta, g.n_phi) == (n_theta, n_phi) and g.data.shape == ref.shape and np.isfinite(g.data).all()
        assert np.abs(g.t - t_ref).max() < 1e-13
        err = float(np.abs(g.data - ref).max())
        print(f"B {name} {sorted(kw)} {family}: max|grid - oracle| = {err:.3e} = {err / np.abs(ref).max():.3e} max|grid|")
        assert err < 2e-12 * np.abs(ref).max(), family


# ------------------------------------------------------------------------------------------------------------- group C
@gpu
@pytest.mark.parametrize("case", sy.C_CASES, ids=lambda c: f"l{c[1]}+{c[3]}-out{c[4]}-r{c[5]}")
def test_c_grid_multiply_flat_factors(ctx, case):
    from scri_amd import engine

    sa, la, sb, lb, out, rows = case
    a = sy.dense_rows(rows, (la + 1) ** 2, seed=la + 7 * rows)
    b = sy.dense_rows(rows, (lb + 1) ** 2, seed=lb + 7 * rows + 1)
    got = engine.grid_multiply(a, sa, la, b, sb, lb, la + lb, out, ctx=ctx)
    # (the oracle on the grid the library works on: it resolves the product, and the reference's default W = l_a + l_b gives the
    # same modes to rounding at many times the cost)
    expect = mref.grid_multiply(a, sa, la, b, sb, lb, sy.grid_multiply_working_ell_max(la, lb, out), out)
    assert got.shape == expect.shape and np.isfinite(got).all()
    err = float(np.abs(got - expect).max())
    print(f"C {case}: max|got - oracle| = {err:.3e}, max|oracle| = {np.abs(expect).max():.3e}")
    assert err < 2e-13 * max(1.0, np.abs(expect).max())
    assert _same_bits(got, engine.grid_multiply(a, sa, la, b, sb, lb, la + lb, out, ctx=ctx))
