"""The in-memory core of the SXS catalogue's compressed waveform format (scri/SpEC/file_io/corotating_paired_xor.py): `pack` is what
`save` does to a waveform before it writes the files (:44-90) -- corotating frame, conjugate pairs, precision truncation, -0.0 -> +0.0,
XOR of successive time steps -- and `unpack` what `load` does after it has read them (:239-255).  Writing and reading the HDF5 / JSON
files stays with the caller.

The modes go through one fused kernel each way (bms_pack_paired_xor, bms_unpack_paired_xor: kernels_bits.hip); for a device-resident
waveform they never leave HBM.  Time and log frame (n and 3n doubles) take the existing `xor_timeseries`.

Two deliberate differences from the reference: a tolerance of 0 is refused (the reference's `save` skips pairing and XOR
there while its `load` always undoes them), and a time step of zero norm or with a non-finite value raises instead of storing NaN."""
import ctypes

import numpy as np

from . import _lib, engine, quaternions, utilities
from . import Inertial, Corotating

sxs_formats = ["corotating_paired_xor"]

TILE_ROWS = engine.paired_xor_tile_rows()  # rows one tile of the pack kernel owns: series lengths around it cross a tile edge


class PackedWaveform:
    """What `save` would write: `time` uint64 [n], `modes` uint64 [n, 2 n_modes], `log_frame` uint64 [n, 3], the l range, the data type
    and `json_data`.  The modes of a device-resident waveform stay in HBM (`modes_device`, a torch int64 tensor) until `.modes` is read."""

    def __init__(self, time, modes, log_frame, ell_min, ell_max, dataType, json_data, history=(), ctx=None):
        self.time, self.log_frame = time, log_frame
        self._modes_host, self._modes_dev = (None, modes) if hasattr(modes, "data_ptr") else (modes, None)
        self.ell_min, self.ell_max, self.dataType = int(ell_min), int(ell_max), int(dataType)
        self.json_data = json_data
        self.history = list(history)
        self._ctx = ctx

    @property
    def is_device_resident(self):
        return self._modes_dev is not None

    @property
    def modes_device(self):
        return self._modes_dev

    @property
    def modes(self):
        if self._modes_host is None:
            self._modes_host, self._modes_dev = self._modes_dev.cpu().numpy().view(np.uint64), None
        return self._modes_host

    @property
    def n_times(self):
        return int(self.time.shape[0])


def _fletcher32(array, ctx):
    """bms_fletcher32 of a host array, or of a device tensor where it lives"""
    if hasattr(array, "data_ptr"):
        out = ctypes.c_uint32(0)
        rc = _lib.load().bms_fletcher32(ctx.handle, ctypes.c_void_p(array.data_ptr()), _lib.BMS_DEVICE, array.numel() * array.element_size(), ctypes.byref(out))
        ctx.check(rc, "bms_fletcher32")
        return int(out.value)
    return int(utilities.fletcher32(array, ctx=ctx))


def _xor_words(x, ctx):
    """+ 0.0 (-0.0 -> 0.0), then xor_timeseries: the uint64 words of a real series"""
    x = np.ascontiguousarray(x, dtype=float) + 0.0
    if x.size:
        utilities.xor_timeseries(x, ctx=ctx)
    return x.view(np.uint64)


def pack(w, L2norm_fractional_tolerance=1e-10, log_frame=None, z_alignment_region=None):
    """The storage form of `w` (corotating_paired_xor.py:44-90, statement by statement, without the files): a `PackedWaveform`.
    An Inertial waveform is taken to its corotating frame first (tolerance 1e-10, z_alignment_region (0.1, 0.95) unless given, log frame
    truncated); a Corotating one is packed as it is, with `log_frame` [n, 3] as given or the logarithm of its frame rounded to multiples
    of 2^floor(log2(tolerance / 10))."""
    tol = float(L2norm_fractional_tolerance)
    if tol == 0.0:
        raise ValueError("L2norm_fractional_tolerance = 0 is not supported: the reference's `save` stores unpaired, un-XORed modes there, "
                         "which its own `load` cannot read back")
    if not tol > 0.0:
        raise ValueError(f"L2norm_fractional_tolerance must be positive, got {L2norm_fractional_tolerance}")
    source = str(w)
    w = w.copy()
    if log_frame is not None:
        log_frame = np.array(log_frame, dtype=float, copy=True)
    if w.frameType == Inertial:
        region = (0.1, 0.95) if z_alignment_region is None else z_alignment_region
        w, log_frame = w.to_corotating_frame(tolerance=1e-10, z_alignment_region=region, truncate_log_frame=True)
        log_frame = log_frame[:, 1:]
    if w.frameType != Corotating:
        raise ValueError("Frame type of input waveform must be 'Corotating' or 'Inertial'; " f"it is {w.frame_type_string}")
    if log_frame is None:
        if w.frame.shape[0] != w.n_times:
            raise ValueError(f"a Corotating waveform needs one frame rotor per time step ({w.n_times}), or `log_frame`; it has {w.frame.shape[0]}")
    elif log_frame.shape != (w.n_times, 3):
        raise ValueError(f"log_frame must have shape ({w.n_times}, 3), not {log_frame.shape}")
    ctx = w._ctx if w._ctx is not None else _lib.default_context()

    # conjugate pairs, truncation, -0.0 -> 0.0 and the XOR of the modes: one kernel, where the modes live
    words = engine.pack_paired_xor(w._dev if w.is_device_resident else w.data, w.ell_min, w.ell_max, tol, ctx=ctx)

    if log_frame is None:
        log_frame = quaternions.log(w.frame)[:, 1:]
        power_of_2 = 2.0 ** int(-np.floor(np.log2(tol / 10)))
        log_frame = np.round(log_frame * power_of_2) / power_of_2
    time_words = _xor_words(w.t, ctx)
    log_frame_words = _xor_words(log_frame, ctx)

    json_data = {
        "sxs_format": "corotating_paired_xor",
        "data_info": {
            "data_type": w.data_type_string,
            "spin_weight": int(w.spin_weight),
            "ell_min": int(w.ell_min),
            "ell_max": int(w.ell_max),
        },
        "transformations": {"truncation": L2norm_fractional_tolerance},
        "validation": {
            "n_times": int(w.n_times),
            "fletcher32": {
                "time": _fletcher32(time_words, ctx),
                "modes": _fletcher32(words, ctx),
                "log_frame": _fletcher32(log_frame_words, ctx),
            },
        },
    }
    if hasattr(w, "boost_velocity"):
        json_data["transformations"]["boost_velocity"] = np.asarray(w.boost_velocity).tolist()
    if hasattr(w, "space_translation"):
        json_data["transformations"]["space_translation"] = np.asarray(w.space_translation).tolist()
    packed = PackedWaveform(time_words, words, log_frame_words, w.ell_min, w.ell_max, w.dataType, json_data, history=w.history, ctx=ctx)
    packed.history.append(f"packed = corotating_paired_xor.pack({source}, L2norm_fractional_tolerance={L2norm_fractional_tolerance})")
    return packed


def unpack(packed):
    """The waveform a `PackedWaveform` stores (corotating_paired_xor.py:239-255): Corotating, its frame exp of the stored log frame, its
    modes device-resident if the packed ones are; `json_data` and `log_frame` are attached."""
    from . import WaveformModes

    ctx = packed._ctx if packed._ctx is not None else _lib.default_context()
    time = np.array(packed.time, dtype=np.uint64, copy=True)
    log_frame = np.array(packed.log_frame, dtype=np.uint64, copy=True)
    if time.size:
        utilities.xor_timeseries_reverse(time, ctx=ctx)
    if log_frame.size:
        utilities.xor_timeseries_reverse(log_frame, ctx=ctx)
    time, log_frame = time.view(np.float64), log_frame.view(np.float64)
    frame = quaternions.exp(np.insert(log_frame, 0, 0.0, axis=1))
    data = engine.unpack_paired_xor(packed.modes_device if packed.is_device_resident else packed.modes, packed.ell_min, packed.ell_max, ctx=ctx)
    resident = hasattr(data, "data_ptr")
    w = WaveformModes(
        t=time, frame=frame, data=np.empty((0, data.shape[1]), dtype=complex) if resident else data, frameType=Corotating,
        dataType=packed.dataType, m_is_scaled_out=True, r_is_scaled_out=True, ell_min=packed.ell_min, ell_max=packed.ell_max,
        history=list(packed.history), ctx=ctx,
    )
    if resident:
        w._host, w._dev = None, data
    w.json_data = packed.json_data
    w.log_frame = log_frame
    w._append_history(f"{w} = corotating_paired_xor.unpack(packed)")
    return w
