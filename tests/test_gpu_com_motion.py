"""The centre-of-mass correction on the GPU (kernels_com.hip behind bms_com_motion and bms_com_fit, scri_amd/com_motion.py,
scri_amd/pn/boosted_comcharge.py).

The fit is held to the EXACT value of the rule it implements, evaluated in rationals on the same fp64 inputs
(tests/helpers/com_motion_cases.py): |engine - exact| <= 4 eps max_component |exact| per quantity.  The bar is derived, not tuned: sums
and closed form are carried in double-double (1e-31 relative), far below eps even after the cancellation of the closed form (up to 1e13
in the windows of two to five samples at t = 5000), so what remains is the final rounding; the 4 covers the hi + lo conversions.
The reference's own fp64 evaluation (g31) is then required to lie within its OWN distance from the exact value plus that bar."""
import os
from fractions import Fraction

import numpy as np
import pytest

from tests.helpers import com_motion_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g31_ref_com_motion.npz")
BLOCK = 256  # samples one workgroup of the track kernel covers


@pytest.fixture(scope="module")
def g31():
    return np.load(GOLDEN)


def _device(x, ctx):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.device("cuda", ctx.device))


# ---------------------------------------------------------------------------------------------------------------- 1. the track


def _numpy_track(t, x_a, x_b, m_a, m_b, matter):
    m = m_a + m_b
    com = ((m_a[:, np.newaxis] * x_a) + (m_b[:, np.newaxis] * x_b)) / m[:, np.newaxis]
    if matter:
        return t / m, com / m[:, np.newaxis]
    return t, com


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17])
@pytest.mark.parametrize("matter", [False, True])
def test_track_equals_the_numpy_expression(n, matter, ctx):
    from scri_amd import engine

    rng = np.random.default_rng(n)
    t = cases.graded_axis(max(n, 2), 5000.0, n)[:n]
    x_a, x_b = rng.normal(size=(n, 3)) * 7.0, rng.normal(size=(n, 3)) * 9.0
    per_sample = (0.6 + 1e-3 * rng.normal(size=n), 0.4 + 1e-3 * rng.normal(size=n))
    for m_a, m_b in (per_sample, (np.array([1.35]), np.array([1.4])), (per_sample[0], np.array([1.4])), (np.array([5.6]), per_sample[1])):
        want_t, want = _numpy_track(t, x_a, x_b, m_a, m_b, matter)
        got_t, got = engine.com_track(t, x_a, x_b, m_a, m_b, matter=matter, ctx=ctx)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want) and np.array_equal(got_t, want_t)
        dev_t, dev = engine.com_track(_device(t, ctx), _device(x_a, ctx), _device(x_b, ctx), _device(m_a, ctx), _device(m_b, ctx), matter=matter, ctx=ctx)
        assert dev.is_cuda and dev_t.is_cuda
        assert np.array_equal(dev.cpu().numpy(), want) and np.array_equal(dev_t.cpu().numpy(), want_t)


@pytest.mark.parametrize("name", ["bbh", "nsns", "bhns_longer_horizons", "bhns_given_mass"])
def test_com_motion_against_the_reference(name, g31, ctx):
    """the reference's own (t, CoM) for its three branches, bit for bit, from host tables and from tables on the device"""
    from scri_amd.SpEC.com_motion import com_motion

    hz, mt, m_A, m_B = cases.track_inputs()[name]
    t, com = com_motion(hz, mt, m_A, m_B, ctx=ctx)
    assert np.array_equal(t, g31[f"track_{name}_t"]) and np.array_equal(com, g31[f"track_{name}_com"])
    on_device = [None if d is None else {k: _device(v, ctx) for k, v in d.items()} for d in (hz, mt)]
    t, com = com_motion(on_device[0], on_device[1], m_A, m_B, ctx=ctx)
    assert com.is_cuda and t.is_cuda
    assert np.array_equal(t.cpu().numpy(), g31[f"track_{name}_t"]) and np.array_equal(com.cpu().numpy(), g31[f"track_{name}_com"])


# ---------------------------------------------------------------------------------------------------------------- 2. the fit, exactly


def _check_against_exact(t, com, fb, fe, ctx, label):
    """both fits of one track against the exact values; returns (exact moments, window)"""
    from scri_amd import engine

    t_i, t_f, i_i, i_f = cases.window(t, fb, fe)
    moments = cases.exact_moments(t, com, i_i, i_f)
    for acc in (False, True):
        fit = engine.com_fit(t, com, fb, fe, acc, ctx=ctx)
        assert (fit["t_i"], fit["t_f"], fit["i_i"], fit["i_f"]) == (t_i, t_f, i_i, i_f), label
        exact = cases.exact_fit(moments, t_i, t_f, acc)
        for key, ex in zip(("x_i", "v_i", "a_i"), exact):
            if key == "a_i" and not acc:
                assert np.array_equal(fit[key], np.zeros(3))
                continue
            d, bar = cases.distance(fit[key], ex), cases.bar(ex)
            print(f"{label} acc={int(acc)} {key}: |engine - exact| = {float(d):.3e}, bar {float(bar):.3e}")
            assert d <= bar, (label, acc, key, float(d), float(bar))
        for k in range(3 if acc else 2):  # the moments themselves, rounded once
            assert cases.distance(fit["moments"][k], moments[k]) <= cases.bar(moments[k]), (label, acc, k)
    return moments, (t_i, t_f, i_i, i_f)


def _window_lengths():
    from scri_amd import engine

    T = engine.com_fit_tile_panels()
    return [2, 3, 4, 5] + list(range(2 * T - 1, 2 * T + 4)) + [3 * 2 * T + 4]


@pytest.mark.parametrize("start", [0.0, 5000.0])
@pytest.mark.parametrize("lead", [4, 5])
def test_fit_is_the_correctly_rounded_rule(start, lead, ctx):
    """window lengths 2 .. 5; 2T - 1 .. 2T + 3 samples for tiles of T panels (the issue's list: T - 1 .. T + 1 panels, so these straddle the
    end of the FIRST tile, with and without a last interval left over); three tiles plus 4 samples; i_i even and odd; axes from 0 and 5000"""
    for length in _window_lengths():
        n = lead + length + 6
        t = cases.dyadic_axis(n, start, 1000 + length)
        com = cases.track(t, 2000 + length + lead)
        fb, fe = cases.fractions_for_window(t, lead, lead + length - 1)
        _, (_, _, i_i, i_f) = _check_against_exact(t, com, fb, fe, ctx, f"start={start:g} lead={lead} length={length}")
        assert (i_i, i_f) == (lead, lead + length - 1)  # (the construction of the case, not the engine)


def test_fit_with_generic_steps(ctx):
    t = cases.graded_axis(587, 5000.0, 77)
    _check_against_exact(t, cases.track(t, 78), 0.013, 0.087, ctx, "generic steps")


def test_fit_beyond_one_lap_of_the_final_sum(ctx):
    """more than 64 tiles (a window above 32 768 samples): com_fit_kernel's lanes each add several partials before the tree.  Dyadic steps
    keep the exact value cheap; the same bits from device memory."""
    from scri_amd import engine

    n = 2 * engine.com_fit_tile_panels() * 78 + 41
    t = cases.dyadic_axis(n, 5000.0, 51)
    com = cases.track(t, 52)
    _, (_, _, i_i, i_f) = _check_against_exact(t, com, 0.01, 0.10, ctx, f"n={n}")
    assert i_f - i_i + 1 > 64 * 2 * engine.com_fit_tile_panels()
    for acc in (False, True):
        host, resident = engine.com_fit(t, com, 0.01, 0.10, acc, ctx=ctx), engine.com_fit(_device(t, ctx), _device(com, ctx), 0.01, 0.10, acc, ctx=ctx)
        assert all(np.array_equal(host[k], resident[k]) for k in host)


def test_window_search_beyond_its_workgroup_cap(ctx):
    """n above 1024 x 256: com_window_kernel's workgroups stride over the axis and every workgroup of com_moments_kernel reduces 1024
    partial minima.  The window must be numpy's; the moments are held to scipy's fp64 rule on an axis from 0, where 3e5 fp64 additions
    are good to n eps = 7e-11 of the sum of magnitudes at worst (bar 1e-9 of max |integrand| x span); the same bits from device memory."""
    from scipy.integrate import simpson

    from scri_amd import engine

    n = 1024 * 256 + 40_001
    rng = np.random.default_rng(61)
    t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.15, size=n - 1))])
    com = cases.track(t, 62)
    t_i, t_f, i_i, i_f = cases.window(t, 0.0137, 0.0921)
    fit = engine.com_fit(t, com, 0.0137, 0.0921, True, ctx=ctx)
    assert (fit["t_i"], fit["t_f"], fit["i_i"], fit["i_f"]) == (t_i, t_f, i_i, i_f)
    for k, y in enumerate((com, t[:, None] * com, (t * t)[:, None] * com)):
        want = simpson(y[i_i : i_f + 1], x=t[i_i : i_f + 1], axis=0)
        assert np.abs(fit["moments"][k] - want).max() <= 1e-9 * np.abs(y).max() * (t_f - t_i), k
    resident = engine.com_fit(_device(t, ctx), _device(com, ctx), 0.0137, 0.0921, True, ctx=ctx)
    assert all(np.array_equal(fit[k], resident[k]) for k in fit)


# ---------------------------------------------------------------------------------------------------------------- 3. the fit, against g31


@pytest.mark.parametrize("position_name", list(enumerate(cases.fit_cases())), ids=lambda p: p[1])
def test_fit_against_the_reference(position_name, g31, ctx):
    """|engine - reference| <= |reference - exact| + the bar of the exact test; window and indices equal to the reference's"""
    from scri_amd import engine

    position, name = position_name
    t, com = g31[f"fit_{name}_t"], g31[f"fit_{name}_com"]
    fb, fe = g31[f"fit_{name}_fractions"]
    assert np.array_equal(t, cases.fit_cases()[name][0]) and np.array_equal(com, cases.fit_case_track(position, t))
    moments, (t_i, t_f, i_i, i_f) = _check_against_exact(t, com, fb, fe, ctx, name)
    assert (t_i, t_f) == tuple(g31[f"fit_{name}_window"]) and (i_i, i_f) == tuple(g31[f"fit_{name}_indices"])
    for acc, key in ((False, "linear"), (True, "accelerated")):
        fit = engine.com_fit(t, com, fb, fe, acc, ctx=ctx)
        exact = cases.exact_fit(moments, t_i, t_f, acc)
        for q, ref in zip(("x_i", "v_i", "a_i"), g31[f"fit_{name}_{key}"]):
            ex = exact[("x_i", "v_i", "a_i").index(q)]
            d_ref = cases.distance(ref, ex)
            print(f"{name} {key} {q}: d_ref = {float(d_ref):.3e} ({float(d_ref / max(abs(e) for e in ex)):.1e} relative)")
            assert max(abs(Fraction(float(a)) - Fraction(float(b))) for a, b in zip(fit[q], ref)) <= d_ref + cases.bar(ex), (name, key, q)


def test_estimate_returns_and_prints_as_the_reference(g31, ctx, capsys):
    from scri_amd import engine
    from scri_amd.SpEC.com_motion import estimate_avg_com_motion

    name = "default_fractions_501_from_5000"
    t, com = g31[f"fit_{name}_t"], g31[f"fit_{name}_com"]
    x, v, t_i, t_f = estimate_avg_com_motion(cases.horizons_of_track(t, com), ctx=ctx)  # (the default fractions are the case's)
    fit = engine.com_fit(t, com, 0.01, 0.10, False, ctx=ctx)
    assert np.array_equal(x, fit["x_i"]) and np.array_equal(v, fit["v_i"]) and (t_i, t_f) == tuple(g31[f"fit_{name}_window"])
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["Optimal x_i: [{}, {}, {}]".format(*x), "Optimal v_i: [{}, {}, {}]".format(*v), f"t_i, t_f: {t_i}, {t_f}"]
    out = estimate_avg_com_motion((t, com), fit_acceleration=True, ctx=ctx)
    assert len(out) == 5 and len(capsys.readouterr().out.splitlines()) == 4


def test_refusals(ctx):
    import ctypes

    from scri_amd import _lib, engine

    t = np.arange(9.0)
    com = np.zeros((9, 3))
    with pytest.raises(ValueError, match="fewer than two samples"):
        engine.com_fit(t, com, 0.6, 0.6, ctx=ctx)  # i_f < i_i
    with pytest.raises(ValueError, match="t_f equals t_i"):
        engine.com_fit(t, com, 0.5, 0.5, ctx=ctx)
    with pytest.raises(ValueError, match="t_f equals t_i"):
        engine.com_fit(np.array([1.0, 1.0, 1.0]), com[:3], 0.0, 0.0, ctx=ctx)
    with pytest.raises(ValueError, match="at least 2 samples"):
        engine.com_fit(t[:1], com[:1], ctx=ctx)
    res = _lib.bms_com_fit_result()
    dp = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    lib = _lib.load()
    assert lib.bms_com_fit(ctx.handle, dp(t), dp(com), 1, _lib.BMS_HOST, 0.0, 0.0, 0, ctypes.byref(res)) < 0
    assert lib.bms_com_fit(ctx.handle, None, dp(com), 9, _lib.BMS_HOST, 0.0, 0.0, 0, ctypes.byref(res)) < 0
    assert lib.bms_com_fit(ctx.handle, dp(t), dp(com), 9, _lib.BMS_HOST, 0.0, 0.0, 0, None) < 0
    assert lib.bms_com_fit(ctx.handle, dp(t), dp(com), 9, 7, 0.0, 0.0, 0, ctypes.byref(res)) < 0
    assert lib.bms_com_fit(ctx.handle, dp(t), dp(com), 9, _lib.BMS_HOST, float("nan"), 0.0, 0, ctypes.byref(res)) < 0
    assert lib.bms_com_motion(ctx.handle, dp(t), dp(com), dp(com), dp(t), 4, dp(t), 1, 9, 0, _lib.BMS_HOST, None, dp(com)) < 0  # masses of length 4
    # a NaN in the track propagates into the fit instead of being refused
    com = cases.track(t, 3)
    com[4, 1] = np.nan
    fit = engine.com_fit(t, com, 0.0, 0.0, ctx=ctx)
    assert np.isnan(fit["x_i"][1]) and np.isnan(fit["v_i"][1]) and np.all(np.isfinite(fit["x_i"][[0, 2]]))


# ---------------------------------------------------------------------------------------------------------------- 4. determinism, residency


def test_same_bits_again_and_from_device_memory(ctx):
    from scri_amd import engine

    n = 5 * 2 * engine.com_fit_tile_panels() + 123
    t = cases.graded_axis(n, 5000.0, 5)
    com = cases.track(t, 6)
    t_dev, com_dev = _device(t, ctx), _device(com, ctx)
    ptrs = (t_dev.data_ptr(), com_dev.data_ptr())
    for acc in (False, True):
        first = engine.com_fit(t, com, 0.01, 0.10, acc, ctx=ctx)
        again = engine.com_fit(t, com, 0.01, 0.10, acc, ctx=ctx)
        resident = engine.com_fit(t_dev, com_dev, 0.01, 0.10, acc, ctx=ctx)
        for key in ("x_i", "v_i", "a_i", "t_i", "t_f", "i_i", "i_f", "moments"):
            assert np.array_equal(first[key], again[key]) and np.array_equal(first[key], resident[key]), (acc, key)
    # The engine has no upload counter, so this is the fallback the issue names: the tensors are where and what they were.  That alone
    # would also hold for a round trip through the host; that there is none rests on the code -- bms_com_fit hands device pointers
    # straight to its kernels (stage_in returns `src` itself for BMS_DEVICE) and reads back only the 24 doubles of the result.
    assert (t_dev.data_ptr(), com_dev.data_ptr()) == ptrs
    assert np.array_equal(t_dev.cpu().numpy(), t) and np.array_equal(com_dev.cpu().numpy(), com)


# ---------------------------------------------------------------------------------------------------------------- 5. remove_avg_com_motion


def _horizons_for_waveform(t_w):
    t = cases.graded_axis(400, float(t_w[0]), 91)
    t = t_w[0] + (t - t[0]) * (t_w[-1] - t_w[0]) / (t[-1] - t[0])
    return cases.horizons_of_track(t, 1e-3 * cases.track(t, 92))


def _waveform(ctx, t, ell_min, data_type, seed, resident):
    import scri_amd
    from scri_amd import synthetic

    w = scri_amd.WaveformModes(t=t, data=synthetic.chirp_modes(t, ell_min, 4, seed), ell_min=ell_min, ell_max=4, dataType=data_type,
                               frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    return w.to_device() if resident else w


def _psi2_with_companions(ctx, t, resident, resident_psi3=None, resident_psi4=None):
    import scri_amd

    return _waveform(ctx, t, 0, scri_amd.psi2, 2, resident), dict(
        psi3_modes=_waveform(ctx, t, 1, scri_amd.psi3, 3, resident if resident_psi3 is None else resident_psi3),
        psi4_modes=_waveform(ctx, t, 2, scri_amd.psi4, 4, resident if resident_psi4 is None else resident_psi4))


@pytest.mark.parametrize("resident", [False, True])
@pytest.mark.parametrize("kind", ["h", "psi2"])
def test_remove_avg_com_motion(kind, resident, ctx, capsys):
    import scri_amd
    from scri_amd.SpEC.com_motion import estimate_avg_com_motion, remove_avg_com_motion

    t = np.linspace(0.0, 190.0, 96)

    def build(on_device):
        return (_waveform(ctx, t, 2, scri_amd.h, 1, on_device), {}) if kind == "h" else _psi2_with_companions(ctx, t, on_device)

    w, companions = build(resident)
    w.version_hist = [["0123abc", "extrapolated"]]
    w.extrapolate_coord_radii = [120.0, 240.0, 480.0]
    horizons = _horizons_for_waveform(t)
    x_0, v_0, _, _ = estimate_avg_com_motion(horizons, ctx=ctx)
    assert np.abs(x_0).max() > 0 and np.abs(v_0).max() > 0
    by_hand = w.transform(space_translation=x_0, boost_velocity=v_0, **companions)
    out = remove_avg_com_motion(w, horizons, ctx=ctx, **companions)
    assert out.is_device_resident == resident and w.is_device_resident == resident
    assert all(c.is_device_resident == resident for c in companions.values())
    assert np.array_equal(out.space_translation, x_0) and np.array_equal(out.boost_velocity, v_0)
    assert out.version_hist == [["0123abc", "extrapolated"]] and out.extrapolate_coord_radii == [120.0, 240.0, 480.0]
    assert out.dataType == w.dataType and np.array_equal(out.t, by_hand.t) and np.array_equal(out.data, by_hand.data)
    assert out.n_times > 60 and np.all(np.isfinite(out.data.view(float)))
    if resident:  # the route through HBM runs the kernels of the route through host memory on the same values: the same bits
        w_host, companions_host = build(False)
        on_host = w_host.transform(space_translation=x_0, boost_velocity=v_0, **companions_host)
        assert not on_host.is_device_resident
        assert np.array_equal(out.t, on_host.t) and np.array_equal(out.data, on_host.data)


@pytest.mark.parametrize("psi3_resident, psi4_resident", [(True, False), (False, True)])
def test_resident_waveform_with_a_host_companion(psi3_resident, psi4_resident, ctx):
    """a device-resident psi2 with one companion in HBM and one in host memory: the result stays in HBM and equals the all-host result;
    each companion stays where it was"""
    import scri_amd

    t = np.linspace(0.0, 190.0, 96)
    kw = dict(space_translation=[3e-3, -1e-3, 2e-3], boost_velocity=[1e-4, 2e-4, -3e-4])
    w, companions = _psi2_with_companions(ctx, t, True, psi3_resident, psi4_resident)
    out = w.transform(**kw, **companions)
    assert out.is_device_resident and w.is_device_resident
    assert companions["psi3_modes"].is_device_resident == psi3_resident and companions["psi4_modes"].is_device_resident == psi4_resident
    w_host, companions_host = _psi2_with_companions(ctx, t, False)
    on_host = w_host.transform(**kw, **companions_host)
    assert np.array_equal(out.t, on_host.t) and np.array_equal(out.data, on_host.data)
    # the companions matter (a swapped or dropped one would show): without the boost's mixing the result is another
    swapped = w_host.transform(**kw, psi3_modes=companions_host["psi3_modes"], psi4_modes=_waveform(ctx, t, 2, scri_amd.psi4, 5, False))
    assert np.abs(swapped.data - on_host.data).max() > 1e-8 * np.abs(on_host.data).max()


# ---------------------------------------------------------------------------------------------------------------- 6. PN_charges


def test_pn_charges_on_a_small_abd(g31, ctx):
    """the four callables on an AsymptoticBondiData object of 64 steps, l <= 4, against the PN series evaluated here, from the engine's own
    angular velocity, by Horner's rule from tables of rational coefficients (8 ulp of each result: a short polynomial after x).  The
    tables are first held to g31 on its stored angular velocity: two evaluations of a cubic in fp64, each a few roundings from the
    exact value, so 6 ulp."""
    from fractions import Fraction as F

    import scri_amd
    from scri_amd import synthetic
    from scri_amd.pn.boosted_comcharge import PN_charges

    # bracket of the energy / angular momentum: sum_k x^k sum_j table[k][j] nu^j (Blanchet 2014, Eqs. 337, 338)
    two_pn = [F(-27, 8), F(19, 8), F(-1, 24)]
    energy_table = [[F(1)], [F(-3, 4), F(-1, 12)], two_pn]
    momentum_table = [[F(1)], [F(3, 2), F(1, 6)], two_pn, [F(135, 16), F(-6889, 144), F(31, 24), F(7, 1296)]]
    pi_squared_term = 41 / 24 * np.pi**2  # the one irrational coefficient: of nu x^3 in the angular momentum

    def bracket(table, ν, x, extra=0.0):
        coefficients = [float(sum(c * F(ν) ** j for j, c in enumerate(row))) for row in table]
        if len(coefficients) == 4:
            coefficients[3] += extra * ν
        total = np.full_like(x, coefficients[-1])
        for c in coefficients[-2::-1]:
            total = total * x + c
        return total

    def expected(m, ν, ω, h_21):
        x = np.power(m * np.sqrt((ω * ω).sum(axis=1)), 2 / 3)
        energy = m - m * ν / 2 * x * bracket(energy_table, ν, x)
        momentum = m * m * ν / np.sqrt(x) * bracket(momentum_table, ν, x, pi_squared_term)
        charge = -1142 / 105 * (m * ν) ** 2 * np.sqrt(1 - 4 * ν) * np.power(x, 2.5)
        return energy, momentum, charge, np.unwrap(np.pi / 2 - np.angle(-h_21))

    m, ν = float(g31["pn_m"]), float(g31["pn_nu"])
    for mine, ref in zip(expected(m, ν, g31["pn_omega"], g31["pn_modes"][:, 3]), g31["pn_charges"]):
        assert np.all(np.abs(mine - ref) <= 6 * np.spacing(np.abs(ref)))
    n = 64
    u = np.linspace(-200.0, -60.0, n)
    abd = scri_amd.AsymptoticBondiData(u, 4, ctx=ctx)
    sigma = np.zeros((n, 25), dtype=complex)
    sigma[:, 4:] = 0.5 * np.conj(synthetic.chirp_modes(u, 2, 4, 9))
    abd.sigma = sigma
    h = abd.h
    ω = h.angular_velocity()
    assert ω.shape == (n, 3) and np.linalg.norm(ω, axis=1).min() > 0
    want = expected(m, ν, ω, h.data[:, h.index(2, 1)])
    for f, expect in zip(PN_charges(m, ν), want):
        got = f(abd)
        assert got.shape == (n,) and np.all(np.abs(got - expect) <= 8 * np.spacing(np.abs(expect))), f.__name__
