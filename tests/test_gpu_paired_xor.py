"""The corotating paired-XOR storage form on the GPU (scri_amd/corotating_paired_xor.py; bms_pack_paired_xor, bms_unpack_paired_xor,
kernels_bits.hip) against the oracle's existing pieces composed in tests/helpers/paired_xor_cases.py: packed words and checksums bit for
bit, the way back value for value, the round trip within the bound the truncation implies, the Inertial path, the C ABI (row stride,
pieces, overlap, rows that cannot be packed) and the errors.

Round-trip bound (derived, not measured): the quantum 2^-e lies in [a, 2a) with a = tol |w| / sqrt(n_modes); each of the 2 n_modes real
parts of the paired row moves by at most half a quantum, i.e. the row by at most sqrt(2 n_modes) a = sqrt2 tol |w|; the pairing is
unitary.  (1 + 1e-6) covers the rounding of the pairing itself, ~1e-16 |w| each way."""
import ctypes

import numpy as np
import pytest

from tests.helpers import paired_xor_cases as px

pytestmark = pytest.mark.gpu


def _tile():
    from scri_amd import corotating_paired_xor

    return corotating_paired_xor.TILE_ROWS


def _shapes():
    T = _tile()
    return px.FIXED_SHAPES + [(2, 3, T - 1), (2, 3, T), (2, 3, T + 1), (2, 3, 2 * T + 1)]


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        metafunc.parametrize("shape", _shapes(), ids=lambda s: "l%d-%d_n%d" % s)
    if "tol" in metafunc.fixturenames:
        metafunc.parametrize("tol", px.TOLERANCES)
    if "device" in metafunc.fixturenames:
        metafunc.parametrize("device", [False, True], ids=["host", "device"])


_cache = {}


def _log_frame(n):
    t = np.linspace(0.0, 1.0, n) if n > 1 else np.zeros(1)
    lf = np.stack([0.3 * np.sin(2.0 * t), -0.2 * t, 0.5 + 0.25 * t * t], axis=1)
    lf[0, 1] = -0.0  # (a negative zero for the + 0.0 to remove)
    return lf


def _case(shape, tol):
    """inputs and the oracle's packed arrays of one (shape, tolerance), computed once and left unchanged"""
    key = (shape, tol)
    if key not in _cache:
        ell_min, ell_max, n = shape
        t, data = px.smooth_modes(ell_min, ell_max, n)
        lf = _log_frame(n)
        words = px.oracle_pack(data, ell_min, ell_max, tol)
        for a in (lf, words):
            a.setflags(write=False)
        _cache[key] = dict(t=t, data=data, log_frame=lf, words=words, time_words=px.oracle_xor_real(t), lf_words=px.oracle_xor_real(lf))
    return _cache[key]


def _waveform(case, shape, ctx, device, frame=None):
    import scri_amd

    w = scri_amd.WaveformModes(t=case["t"].copy(), data=case["data"].copy(), ell_min=shape[0], ell_max=shape[1], frameType=scri_amd.Corotating,
                               dataType=scri_amd.h, r_is_scaled_out=True, m_is_scaled_out=True, frame=frame, ctx=ctx)
    return w.to_device() if device else w


def _exp_pure(v):
    """exp of the pure quaternions (0, v): (cos |v|, sin |v| v / |v|)"""
    a = np.linalg.norm(v, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(a > 0, np.sin(a) / np.where(a > 0, a, 1.0), 1.0)
    return np.concatenate([np.cos(a)[:, None], s[:, None] * v], axis=1)


# ------------------------------------------------------------------------------------------------ 1. pack bits
def test_pack_bits_and_checksums(ctx, shape, tol, device):
    from scri_amd import corotating_paired_xor as cpx

    case = _case(shape, tol)
    margin = px.exponent_margin(case["data"], shape[0], shape[1], tol)
    assert margin >= px.MARGIN, f"bad input: a row's exponent hinges on the last bits of its norm (margin {margin:.3e})"
    w = _waveform(case, shape, ctx, device)
    packed = cpx.pack(w, L2norm_fractional_tolerance=tol, log_frame=case["log_frame"])
    assert packed.is_device_resident == device
    fl = packed.json_data["validation"]["fletcher32"]  # (taken where the modes live, before they are read)
    assert packed.is_device_resident == device
    modes = packed.modes
    assert modes.dtype == np.uint64 and modes.shape == case["words"].shape
    differing = np.nonzero(np.any(modes != case["words"], axis=1))[0]
    print(f"{shape} tol={tol} device={device}: {differing.size} of {shape[2]} rows differ, exponent margin {margin:.3e}")
    assert np.array_equal(modes, case["words"])
    assert packed.time.dtype == np.uint64 and np.array_equal(packed.time, case["time_words"])
    assert packed.log_frame.dtype == np.uint64 and np.array_equal(packed.log_frame, case["lf_words"])
    from oracle import utilities_ref

    assert fl == {"time": utilities_ref.fletcher32(case["time_words"]), "modes": utilities_ref.fletcher32(case["words"]),
                  "log_frame": utilities_ref.fletcher32(case["lf_words"])}
    assert packed.json_data["validation"]["n_times"] == shape[2] and packed.json_data["transformations"]["truncation"] == tol
    assert (packed.ell_min, packed.ell_max) == shape[:2]
    # the input is a copy's business: the waveform is as it was
    assert w.is_device_resident == device and np.array_equal(w.data, case["data"])
    assert "corotating_paired_xor.pack(" in packed.history[-1]


def test_log_frame_of_a_corotating_waveform_is_rounded_as_the_reference_rounds_it(ctx):
    from scri_amd import corotating_paired_xor as cpx, quaternions

    shape, tol = (2, 3, 257), 1e-3
    case = _case(shape, tol)
    frame = _exp_pure(case["log_frame"])
    packed = cpx.pack(_waveform(case, shape, ctx, False, frame=frame), L2norm_fractional_tolerance=tol)
    power_of_2 = 2 ** (-np.floor(np.log2(tol / 10))).astype("int")  # corotating_paired_xor.py:79-80
    expected = np.round(quaternions.log(frame)[:, 1:] * power_of_2) / power_of_2
    assert np.array_equal(packed.log_frame, px.oracle_xor_real(expected))
    assert np.array_equal(packed.modes, case["words"])


@pytest.mark.parametrize("wide", [(0, 45, 5), (0, 66, 3)], ids=lambda s: "l%d-%d_n%d" % s)
def test_rows_beyond_64_kb_of_lds(ctx, wide, device):
    """2116 and 4489 modes: the staged row, the previous packed row and the partner table take 76 KB and 162 KB of LDS, beyond what a
    kernel gets without asking; lanes stride over 34 and 71 columns each"""
    from scri_amd import corotating_paired_xor as cpx

    tol = 1e-10
    case = _case(wide, tol)
    assert px.exponent_margin(case["data"], wide[0], wide[1], tol) >= px.MARGIN
    packed = cpx.pack(_waveform(case, wide, ctx, device), L2norm_fractional_tolerance=tol, log_frame=case["log_frame"])
    assert packed.is_device_resident == device
    back = cpx.unpack(packed)
    assert np.array_equal(packed.modes, case["words"])
    assert np.array_equal(back.data, px.oracle_unpack(case["words"], wide[0], wide[1]))


# ------------------------------------------------------------------------------------------------ 2. unpack
def test_unpack_of_the_oracles_words(ctx, shape, tol, device):
    import scri_amd
    from scri_amd import corotating_paired_xor as cpx

    case = _case(shape, tol)
    expected = px.oracle_unpack(case["words"], shape[0], shape[1])
    words = case["words"].copy()
    if device:
        import torch

        words = torch.from_numpy(words.view(np.int64)).to(f"cuda:{ctx.device}")
    packed = cpx.PackedWaveform(case["time_words"].copy(), words, case["lf_words"].copy(), shape[0], shape[1], scri_amd.h, {"sxs_format": "corotating_paired_xor"}, ctx=ctx)
    w = cpx.unpack(packed)
    assert w.is_device_resident == device
    assert w.frameType == scri_amd.Corotating and w.dataType == scri_amd.h and w.m_is_scaled_out and w.r_is_scaled_out
    assert (w.ell_min, w.ell_max) == shape[:2] and w.json_data is packed.json_data
    assert np.array_equal(w.t, case["t"] + 0.0)
    assert np.array_equal(w.log_frame, case["log_frame"] + 0.0)
    frame_err = np.abs(w.frame - _exp_pure(case["log_frame"])).max()
    data = w.data
    print(f"{shape} tol={tol} device={device}: max |frame - exp(log_frame)| = {frame_err:.3e}, {np.count_nonzero(data != expected)} values differ")
    assert frame_err <= 1e-15
    assert data.shape == expected.shape and np.array_equal(data, expected)
    assert "corotating_paired_xor.unpack(" in w.history[-1]


# ------------------------------------------------------------------------------------------------ 3. round trip
def test_round_trip_within_the_truncation_bound(ctx, shape, tol, device):
    from scri_amd import corotating_paired_xor as cpx

    case = _case(shape, tol)
    w = _waveform(case, shape, ctx, device)
    back = cpx.unpack(cpx.pack(w, L2norm_fractional_tolerance=tol, log_frame=case["log_frame"]))
    assert back.is_device_resident == device
    err = np.linalg.norm(back.data - case["data"], axis=1)
    norm = np.linalg.norm(case["data"], axis=1)
    print(f"{shape} tol={tol} device={device}: max row error / (tol |w|) = {np.max(err / (tol * norm)):.4f} (bound sqrt2)")
    assert np.all(err <= np.sqrt(2.0) * tol * norm * (1.0 + 1e-6))


# ------------------------------------------------------------------------------------------------ 4. Inertial path
def test_inertial_waveform_goes_through_its_corotating_frame(ctx, tol):
    import scri_amd
    from scri_amd import corotating_paired_xor as cpx
    from scri_amd.sample_waveforms import fake_precessing_waveform

    w = fake_precessing_waveform(t_1=200.0, dt=0.5, ell_max=4, ctx=ctx)
    assert w.frameType == scri_amd.Inertial
    packed = cpx.pack(w, L2norm_fractional_tolerance=tol)
    assert w.frameType == scri_amd.Inertial  # (a copy was packed)
    wc, log_frame = w.copy().to_corotating_frame(tolerance=1e-10, z_alignment_region=(0.1, 0.95), truncate_log_frame=True)
    by_hand = cpx.pack(wc, L2norm_fractional_tolerance=tol, log_frame=log_frame[:, 1:])
    assert np.array_equal(packed.modes, by_hand.modes)
    assert np.array_equal(packed.time, by_hand.time) and np.array_equal(packed.log_frame, by_hand.log_frame)
    assert packed.json_data == by_hand.json_data
    back = cpx.unpack(packed).to_inertial_frame()
    assert back.frameType == scri_amd.Inertial
    err = np.linalg.norm(back.data - w.data, axis=1)
    norm = np.linalg.norm(w.data, axis=1)
    rotation = 1e-10 * np.abs(w.data).max()  # the bar of the frame round trip (tests/test_gpu_tutorials.py, corotating -> inertial)
    print(f"tol={tol}: max (row error / (tol |w|)) = {np.max(err / (tol * norm)):.4f}")
    assert np.all(err <= np.sqrt(2.0) * tol * norm * (1.0 + 1e-6) + rotation)


# ------------------------------------------------------------------------------------------------ 5. ABI level
def _abi_pack(ctx, data, ld, n, ell_min, ell_max, mem, tol, out):
    from scri_amd import _lib

    bad = ctypes.c_int64(-7)
    rc = _lib.load().bms_pack_paired_xor(ctx.handle, data, ld, n, ell_min, ell_max, mem, tol, out, ctypes.byref(bad))
    return rc, bad.value


def test_abi_row_stride_pieces_and_memory_kinds_give_the_same_bits(ctx):
    import torch
    from scri_amd import _lib

    shape, tol = (2, 8, 700), 1e-10
    ell_min, ell_max, n = shape
    case = _case(shape, tol)
    nm = px.n_modes(ell_min, ell_max)
    ld = nm + 3
    padded = np.full((n, ld), 12345.0 + 6789.0j)
    padded[:, :nm] = case["data"]
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    # host, one piece, ld > n_modes
    one = np.zeros((n, 2 * nm), dtype=np.uint64)
    assert _abi_pack(ctx, vp(padded), ld, n, ell_min, ell_max, _lib.BMS_HOST, tol, vp(one)) == (0, -1)
    assert np.array_equal(one, case["words"])
    # host, forced through pieces of 37 rows (19 pieces, none aligned with the kernel's tiles)
    small = _lib.Context(ctx.device, workspace_limit=37 * 32 * nm)
    try:
        pieces = np.zeros((n, 2 * nm), dtype=np.uint64)
        assert _abi_pack(small, vp(padded), ld, n, ell_min, ell_max, _lib.BMS_HOST, tol, vp(pieces)) == (0, -1)
        assert np.array_equal(pieces, case["words"])
        back = np.full((n, ld), 5.0 + 5.0j)
        rc = _lib.load().bms_unpack_paired_xor(small.handle, vp(pieces), n, ell_min, ell_max, _lib.BMS_HOST, vp(back), ld)
        assert rc == 0
        assert np.array_equal(back[:, :nm], px.oracle_unpack(case["words"], ell_min, ell_max)) and np.all(back[:, nm:] == 5.0 + 5.0j)
    finally:
        small.close()
    # device memory, in place, ld > n_modes both ways
    d_in = torch.from_numpy(padded).to(f"cuda:{ctx.device}")
    d_out = torch.zeros((n, 2 * nm), dtype=torch.int64, device=d_in.device)
    assert _abi_pack(ctx, ctypes.c_void_p(d_in.data_ptr()), ld, n, ell_min, ell_max, _lib.BMS_DEVICE, tol, ctypes.c_void_p(d_out.data_ptr())) == (0, -1)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), case["words"])
    d_back = torch.full((n, ld), 5.0 + 5.0j, dtype=torch.complex128, device=d_in.device)
    rc = _lib.load().bms_unpack_paired_xor(ctx.handle, ctypes.c_void_p(d_out.data_ptr()), n, ell_min, ell_max, _lib.BMS_DEVICE, ctypes.c_void_p(d_back.data_ptr()), ld)
    assert rc == 0
    assert np.array_equal(d_back.cpu().numpy(), back)


def test_abi_refuses_overlap_bad_tolerance_and_short_stride(ctx):
    from scri_amd import _lib

    ell_min, ell_max, n = 2, 3, 40
    nm = px.n_modes(ell_min, ell_max)
    _, data = px.smooth_modes(ell_min, ell_max, n)
    buf = np.zeros((2 * n, nm), dtype=complex)
    buf[:n] = data
    vp = lambda a, off=0: ctypes.c_void_p(a.ctypes.data + off)
    lib = _lib.load()
    rc, bad = _abi_pack(ctx, vp(buf), nm, n, ell_min, ell_max, _lib.BMS_HOST, 1e-10, vp(buf, 16 * nm * (n - 1)))  # last input row = first output row
    assert rc == _lib.BMS_ERR_INVALID and bad == -1 and b"overlap" in lib.bms_last_error(ctx.handle)
    assert np.array_equal(buf[:n], data)  # nothing was written
    out = np.zeros((n, 2 * nm), dtype=np.uint64)
    for tol in (0.0, -1e-10, float("nan"), float("inf")):
        assert _abi_pack(ctx, vp(buf), nm, n, ell_min, ell_max, _lib.BMS_HOST, tol, vp(out))[0] == _lib.BMS_ERR_INVALID
    assert _abi_pack(ctx, vp(buf), nm - 1, n, ell_min, ell_max, _lib.BMS_HOST, 1e-10, vp(out))[0] == _lib.BMS_ERR_INVALID
    assert _abi_pack(ctx, vp(buf), nm, n, 3, 2, _lib.BMS_HOST, 1e-10, vp(out))[0] == _lib.BMS_ERR_INVALID
    assert _abi_pack(ctx, vp(buf), nm, n, ell_min, ell_max, 7, 1e-10, vp(out))[0] == _lib.BMS_ERR_INVALID
    assert lib.bms_unpack_paired_xor(ctx.handle, vp(out), n, ell_min, ell_max, _lib.BMS_HOST, vp(out, 64), nm) == _lib.BMS_ERR_INVALID
    assert lib.bms_unpack_paired_xor(ctx.handle, vp(out), n, ell_min, ell_max, _lib.BMS_HOST, vp(buf), nm - 1) == _lib.BMS_ERR_INVALID
    assert not np.any(out)


@pytest.mark.parametrize("what", ["zero", "inf", "nan"])
def test_abi_names_the_first_row_it_cannot_pack(ctx, what):
    """input checks: the kernel reports the row through its first-bad-row word, nothing is packed silently and nothing faults"""
    from scri_amd import _lib

    T = _tile()
    ell_min, ell_max, n = 2, 3, 2 * T + 9
    nm = px.n_modes(ell_min, ell_max)
    data = np.array(px.smooth_modes(ell_min, ell_max, n)[1])
    planted, later = T + 3, 2 * T + 1  # in the second tile; another one behind it, which must not win
    for row in (planted, later):
        if what == "zero":
            data[row] = 0.0
        else:
            data[row, 5] = complex(1.0, float(what))
    out = np.zeros((n, 2 * nm), dtype=np.uint64)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc, bad = _abi_pack(ctx, vp(data), nm, n, ell_min, ell_max, _lib.BMS_HOST, 1e-10, vp(out))
    assert rc == _lib.BMS_ERR_INVALID and bad == planted
    assert f"row {planted} ".encode() in _lib.load().bms_last_error(ctx.handle)
    # the first row of a tile and row 0
    for row in (T, 0):
        data = np.array(px.smooth_modes(ell_min, ell_max, n)[1])
        data[row] = 0.0 if what == "zero" else complex(float(what), 0.0)
        assert _abi_pack(ctx, vp(data), nm, n, ell_min, ell_max, _lib.BMS_HOST, 1e-10, vp(out)) == (_lib.BMS_ERR_INVALID, row)


# ------------------------------------------------------------------------------------------------ 6. errors
def test_errors(ctx):
    import scri_amd
    from scri_amd import corotating_paired_xor as cpx

    shape = (2, 3, 40)
    case = _case(shape, 1e-10)
    w = _waveform(case, shape, ctx, False)
    with pytest.raises(ValueError, match="tolerance"):
        cpx.pack(w, L2norm_fractional_tolerance=0.0, log_frame=case["log_frame"])
    w.frameType = scri_amd.Coprecessing
    with pytest.raises(ValueError, match="Frame type of input waveform must be 'Corotating' or 'Inertial'; it is Coprecessing"):
        cpx.pack(w, log_frame=case["log_frame"])
    for device in (False, True):
        w = _waveform(case, shape, ctx, False)
        w.data[17] = 0.0
        if device:
            w.to_device()
        with pytest.raises(ValueError, match="time step 17 "):
            cpx.pack(w, log_frame=case["log_frame"])
