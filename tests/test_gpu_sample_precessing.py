"""`fake_precessing_waveform` and `fake_finite_radius_waveforms` on the GPU (bms_precessing_waveform, bms_radius_terms;
scri_amd/csrc/kernels_sample.hip) against the reference's own outputs (g30, tests/golden/make_golden_sample_precessing.py), against
themselves (host / device, corotating / inertial, strided output, repeated calls), through the fluxes, and through the extrapolation
of the finite-radius family back to the waveform it was built on.

Bars.  Data: 1e-12 max|data| absolute, the project's bar for composite paths; frame: 1e-12 per component, same sign.
Measured on an MI355X: see DESIGN section 2 (the maxima are printed by the test).  Fluxes: 1e-13 of the largest value, the bar of the g14
flux test.  Extrapolation: the bar of tests/test_gpu_extrapolation.py, C kappa eps max|y| per time step."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden.make_golden_sample_precessing import CASES
from tests.test_gpu_extrapolation import _bar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G30 = os.path.join(ROOT, "tests", "golden", "g30_ref_fake_precessing.npz")
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def g30():
    return np.load(G30)


@pytest.fixture(scope="module")
def generated(ctx):
    """every case in both frames, generated once (host data) and left unchanged"""
    from scri_amd.sample_waveforms import fake_precessing_waveform

    return {(name, inertial): fake_precessing_waveform(inertial=inertial, ctx=ctx, **kw) for name, kw in CASES.items() for inertial in (True, False)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_reference(generated, g30, name):
    import scri_amd

    for inertial in (False, True):
        tag = f"{name}_{'inertial' if inertial else 'corotating'}"
        W, ref, ref_frame = generated[name, inertial], g30[f"{tag}_data"], g30[f"{tag}_frame"]
        np.testing.assert_array_equal(W.t, g30[f"{tag}_t"])
        assert W.data.shape == ref.shape and W.frame.shape == ref_frame.shape
        assert (W.ell_min, W.dataType, W.r_is_scaled_out, W.m_is_scaled_out) == (2, scri_amd.h, True, True)
        assert W.frameType == (scri_amd.Inertial if inertial else scri_amd.Corotating)
        assert not W.is_device_resident and "fake_precessing_waveform(" in W.history[-2 if inertial else -1]
        d_err, f_err = np.abs(W.data - ref).max(), np.abs(W.frame - ref_frame).max()
        print(f"{tag}: max |data - reference| = {d_err:.3e} ({d_err / np.abs(ref).max():.3e} of max|data|), max |frame - reference| = {f_err:.3e}")
        assert d_err <= 1e-12 * np.abs(ref).max()
        assert f_err <= 1e-12
        assert np.all(np.isfinite(W.data.view(float)))
    if name == "B":  # equal masses: the (l + m)-parity / sigma(l) combinations that vanish, and m = 0
        zero = np.all(g30["B_corotating_data"] == 0, axis=0)
        assert zero.sum() == 8
        assert np.all(generated["B", False].data[:, zero] == 0)
        zero = np.all(g30["B_inertial_data"] == 0, axis=0)
        assert np.all(generated["B", True].data[:, zero] == 0)


def test_device_and_host_output_are_the_same_bits(ctx, generated):
    from scri_amd.sample_waveforms import fake_precessing_waveform

    for inertial in (False, True):
        W = fake_precessing_waveform(inertial=inertial, device=True, ctx=ctx, **CASES["A"])
        assert W.is_device_resident and W._data_shape() == (841, 21)
        frame = W.frame.copy()
        assert W.is_device_resident  # (reading the frame moves nothing)
        np.testing.assert_array_equal(W.data, generated["A", inertial].data)
        np.testing.assert_array_equal(frame, generated["A", inertial].frame)


def test_inertial_is_the_corotating_waveform_taken_to_the_inertial_frame(ctx, generated):
    from scri_amd.sample_waveforms import fake_precessing_waveform

    for name in sorted(CASES):
        back = generated[name, False].copy().to_inertial_frame()
        np.testing.assert_array_equal(back.data, generated[name, True].data)
        np.testing.assert_array_equal(back.frame, generated[name, True].frame)
        assert back.frameType == generated[name, True].frameType
    W = fake_precessing_waveform(inertial=False, device=True, ctx=ctx, **CASES["C"]).to_inertial_frame()
    assert W.is_device_resident
    np.testing.assert_array_equal(W.data, generated["C", True].data)


def test_a_second_call_on_the_same_context_gives_the_same_bits(ctx, generated):
    from scri_amd.sample_waveforms import fake_precessing_waveform

    fake_precessing_waveform(ctx=ctx, **CASES["C"])  # (another shape in between: the work space is reused)
    for inertial in (False, True):
        again = fake_precessing_waveform(inertial=inertial, ctx=ctx, **CASES["A"])
        np.testing.assert_array_equal(again.data, generated["A", inertial].data)
        np.testing.assert_array_equal(again.frame, generated["A", inertial].frame)


def test_a_wider_row_stride_leaves_the_padding_alone(ctx, generated):
    import torch

    from scri_amd import device_series, engine
    from scri_amd.sample_waveforms import _pn_amplitude_tables

    kw = CASES["A"]
    t = np.arange(-20.0, kw["t_1"] + 0.99 * kw["dt"], kw["dt"])
    coef, power = _pn_amplitude_tables(kw["ell_max"], 2.0)
    dev = device_series.attach(ctx)
    for inertial in (False, True):
        wide = torch.full((t.size + 2, 21 + 7), SENTINEL, dtype=torch.complex128, device=dev)
        data, frame = engine.precessing_waveform(t, kw["ell_max"], kw["t_1"] - 100.0, 2.0, np.pi / 6.0, None, 0.1, None, coef, power,
                                                 inertial=inertial, out=wide[1:-1], ctx=ctx)
        got = wide.cpu().numpy()
        assert np.all(got[0] == SENTINEL) and np.all(got[-1] == SENTINEL) and np.all(got[:, 21:] == SENTINEL)
        np.testing.assert_array_equal(got[1:-1, :21], generated["A", inertial].data)
        np.testing.assert_array_equal(frame, generated["A", False].frame)  # (the corotating frame whatever `inertial` is)


def test_fluxes_of_case_a(generated, g30):
    W = generated["A", True]
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()  # noqa: E731
    figures = {name: rel(getattr(W, name)(), g30[f"A_{name}"]) for name in ("energy_flux", "momentum_flux", "angular_momentum_flux")}
    print("fluxes of case A against the reference's, relative to the largest value:", {k: f"{v:.3e}" for k, v in figures.items()})
    for name, value in figures.items():
        assert value < 1e-13, (name, value)


@pytest.mark.parametrize("kw", [dict(), dict(mass_ratio=2, precession_opening_angle=np.pi / 6)], ids=["defaults", "precessing"])
def test_extrapolation_recovers_the_asymptotic_waveform(ctx, kw):
    from scri_amd import _Extrapolate
    from scri_amd.sample_waveforms import fake_finite_radius_waveforms

    Ws, Radii, h0 = fake_finite_radius_waveforms(t_1=400, dt=0.5, ell_max=4, n_radii=8, ctx=ctx, **kw)
    assert len(Ws) == len(Radii) == 8 and h0.data.shape == (801, 21) and not h0.is_device_resident
    radii = np.array(Radii)
    expected = (1 / np.linspace(1 / 100.0, 1 / 600.0, 8)).astype(int) + 1.0
    np.testing.assert_array_equal(radii, np.repeat(expected[:, None], 801, axis=1))
    data = np.array([W.data for W in Ws])
    # the family itself: the docstring's model on the one h0
    phase = np.exp(1j * np.arange(1, 4)[:, None] * 50 * np.pi / 801 * h0.t[None, :])
    model = h0.data[None] + np.einsum("rk,kt,tm->rtm", expected[:, None] ** -np.arange(1.0, 4.0)[None, :], phase, np.abs(h0.data))
    assert np.abs(data - model).max() <= 8 * np.finfo(float).eps * np.abs(h0.data).max()
    orders = [2, 3, 4, 5]
    out = _Extrapolate(Ws, Radii, orders)
    rows = np.arange(801)
    for N, W in zip(orders, out):
        err = np.abs(W.data - h0.data).max(axis=1)
        print(f"order {N}: max |extrapolated - h0| = {err.max():.3e} (scale {np.abs(h0.data).max():.3f})")
        if N == 2:  # the 1 / r^3 term is there
            assert 1e-9 < err.max() < 1e-6
        else:
            assert np.all(err <= _bar(radii, data, rows, N)), (N, err.max())
    # device=True leaves everything in HBM, with the same values
    Wd, _, hd = fake_finite_radius_waveforms(t_1=400, dt=0.5, ell_max=4, n_radii=8, device=True, ctx=ctx, **kw)
    assert hd.is_device_resident and all(W.is_device_resident for W in Wd)
    np.testing.assert_array_equal(Wd[3].data, Ws[3].data)


def test_the_tutorial_s_first_waveform(ctx):
    """docs/tutorial_waveformmodes.rst:134-138 of the reference"""
    import scri_amd as scri

    h = scri.sample_waveforms.fake_precessing_waveform(t_0=0.0, t_1=300.0, ctx=ctx)
    assert h.dataType == scri.h and h.frameType == scri.Inertial and (h.ell_min, h.ell_max) == (2, 8)
    assert h.data.shape == (3001, 77) and np.all(np.isfinite(h.data.view(float)))
    assert scri.WaveformModes(h).to_corotating_frame().frameType == scri.Corotating
    assert scri.WaveformModes(h).to_coprecessing_frame().frameType == scri.Coprecessing


_BOUNDARY = r"""
import ctypes, sys
sys.path.insert(0, %r)
import numpy as np
from scri_amd import _lib, engine
from scri_amd.sample_waveforms import _pn_amplitude_tables
lib, ctx = _lib.load(), _lib.Context(0)
t = np.arange(-20.0, 400.0 + 0.99 * 0.5, 0.5)
coef, power = _pn_amplitude_tables(4, 2.0)
def good():
    return engine.precessing_waveform(t, 4, 300.0, 2.0, 0.5, None, 0.1, None, coef, power, inertial=True, ctx=ctx)
first = good()
def params(**kw):
    f = dict(mass_ratio=2.0, t_merger=300.0, opening_angle=0.5, opening_angle_dot=0.0, relative_rate=0.1, nutation_angle=0.0,
             derive_opening_angle_dot=1, derive_nutation_angle=1, coef=coef.ctypes.data, power=_lib.dptr(power))
    f.update(kw)
    return _lib.bms_precessing_params(**f)
out, frame = np.zeros((t.size, 21), dtype=complex), np.zeros((t.size, 4))
def call(tp=_lib.dptr(t), n=t.size, ell_max=4, p=None, data=_lib.vptr(out), ld=21, null_params=False):
    p = params() if p is None else p
    return lib.bms_precessing_waveform(ctx.handle, tp, n, ell_max, None if null_params else ctypes.byref(p), 1, data, ld, _lib.BMS_HOST, _lib.dptr(frame))
status = dict(null_t=call(tp=None), null_params=call(null_params=True), null_data=call(data=None), n_zero=call(n=0), ell_1=call(ell_max=1),
              ell_beyond=call(ell_max=8193), nan=call(p=params(opening_angle=float("nan"))), negative_ld=call(ld=-21),
              null_table=call(p=params(coef=None)))
messages = bool(lib.bms_last_error(ctx.handle))
second = good()
print(status)
print("OK" if all(s < 0 for s in status.values()) and messages and not out.any() and np.array_equal(first[0], second[0])
      and np.array_equal(first[1], second[1]) else "FAILED")
"""


def test_bad_arguments_come_back_as_statuses_and_leave_the_context_usable():
    out = subprocess.run([sys.executable, "-c", _BOUNDARY % ROOT], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    print(out.stdout)
    assert out.stdout.strip().splitlines()[-1] == "OK", out.stdout
