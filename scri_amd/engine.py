"""numpy-level wrappers of the C ABI (one function per exported entry point).

These take and return plain numpy arrays (host memory) or, with `device=True`, raw device
pointers (ints, e.g. ``torch.Tensor.data_ptr()``) for callers that keep data resident in HBM.
The scri-compatible classes in ``scri_amd.waveform_modes`` etc. are built on top of these.
"""
import collections
import ctypes
import math
import os
import sys
import threading

import numpy as np

from . import _lib
from ._lib import (
    BMS_HOST,
    BMS_DEVICE,
    BMS_TERM_NONE,
    BMS_TERM_H,
    BMS_TERM_SIGMA,
    BMS_TERM_PSI,
    bms_wm_input,
    bms_transformation,
    bms_shard,
    c_i64,
    c_vp,
    dptr,
    vptr,
)


def _ctx(ctx):
    return ctx if ctx is not None else _lib.default_context()


def LM_total_size(ell_min, ell_max):
    return (ell_max + 1) ** 2 - ell_min**2


def LM_index(ell, m, ell_min):
    return ell * (ell + 1) - ell_min**2 + m


def total_size_D_matrices(ell_min, ell_max):
    f = lambda l: (4 * l**3 - l) // 3
    return f(ell_max + 1) - f(ell_min)


# ---------------------------------------------------------------------------------- rotation


def _rotate_dealt(data, devices, ctx, call):
    """call(ctx, row0, row1) on one host thread per device: each context uploads, rotates and downloads its own block of rows"""
    errors = _run_dealt(contexts_for(devices, first=ctx), data.shape[0], call)
    for e in errors:
        if e is not None:
            raise e
    return data


def rotate_const(data, ell_min, ell_max, quaternion, ctx=None, devices=None):
    """In place: data[t, l, m] <- sum_m' data[t, l, m'] D^l_{m',m}(q)   (scri/rotations.py:346-367).
    `data`: C-contiguous complex128 [N, >= n_modes] numpy array.  devices: the GPUs of this process the rows are dealt over
    (one context and one host thread each; default SCRI_AMD_DEVICES, else the one context)."""
    assert data.dtype == np.complex128 and data.ndim == 2 and data.strides[1] == 16
    q = np.ascontiguousarray(quaternion, dtype=float)
    devices = devices if devices is not None else (default_devices() if data.nbytes >= PIPELINE_MIN_BYTES else None)

    def call(cx, r0, r1):
        block = data[r0:r1]
        rc = _lib.load().bms_rotate_const(cx.handle, vptr(block), BMS_HOST, block.shape[0], data.strides[0] // 16, ell_min, ell_max, dptr(q))
        cx.check(rc, "bms_rotate_const")

    if devices and len(devices) > 1 and data.shape[0] >= 2 * len(devices):
        return _rotate_dealt(data, devices, ctx, call)
    _lib.register_if_reused(data)  # (seen a second time, a long series is page-locked in place: its blocks then go up and come back side by side)
    call(_ctx(ctx), 0, data.shape[0])
    return data


def rotate_const_D(data, ell_min, ell_max, D, ctx=None):
    """In place with the packed Wigner matrices handed over, the signature of the reference's numba kernel
    (scri/rotations.py:346-367; D block l row-major (m', m) at sf._linear_matrix_offset(l, ell_min))."""
    ctx = _ctx(ctx)
    assert data.dtype == np.complex128 and data.ndim == 2 and data.strides[1] == 16
    D = np.ascontiguousarray(D, dtype=np.complex128)
    if D.shape != (total_size_D_matrices(ell_min, ell_max),):
        raise ValueError(f"D must hold {total_size_D_matrices(ell_min, ell_max)} elements, got shape {D.shape}")
    _lib.register_if_reused(data)
    rc = _lib.load().bms_rotate_const_D(
        ctx.handle, vptr(data), BMS_HOST, data.shape[0], data.strides[0] // 16, ell_min, ell_max, vptr(D)
    )
    ctx.check(rc, "bms_rotate_const_D")
    return data


def rotate_series(data, ell_min, ell_max, spinors, ctx=None, devices=None):
    """In place, one rotor per time step; spinors complex128 [N, 2] = (w + i z, y + i x)
    (scri/rotations.py:370-392).  devices: as rotate_const -- contiguous blocks of time steps per GPU, no exchange."""
    assert data.dtype == np.complex128 and data.ndim == 2 and data.strides[1] == 16
    sp = np.ascontiguousarray(spinors, dtype=np.complex128)
    if sp.shape != (data.shape[0], 2):
        raise ValueError(f"spinors must have shape ({data.shape[0]}, 2), got {sp.shape}")
    devices = devices if devices is not None else (default_devices() if data.nbytes >= PIPELINE_MIN_BYTES else None)

    def call(cx, r0, r1):
        block = data[r0:r1]
        rc = _lib.load().bms_rotate_series(cx.handle, vptr(block), BMS_HOST, block.shape[0], data.strides[0] // 16, ell_min, ell_max, vptr(sp[r0:r1]))
        cx.check(rc, "bms_rotate_series")

    if devices and len(devices) > 1 and data.shape[0] >= 2 * len(devices):
        return _rotate_dealt(data, devices, ctx, call)
    _lib.register_if_reused(data)
    call(_ctx(ctx), 0, data.shape[0])
    return data


def rotate_device(data_ptr, n_times, ld, ell_min, ell_max, spinors_ptr=None, quaternion=None, ctx=None):
    """Device-resident variant: data_ptr / spinors_ptr are device addresses."""
    ctx = _ctx(ctx)
    lib = _lib.load()
    if spinors_ptr is not None:
        rc = lib.bms_rotate_series(ctx.handle, c_vp(data_ptr), BMS_DEVICE, n_times, ld, ell_min, ell_max, c_vp(spinors_ptr))
        ctx.check(rc, "bms_rotate_series")
    else:
        q = np.ascontiguousarray(quaternion, dtype=float)
        rc = lib.bms_rotate_const(ctx.handle, c_vp(data_ptr), BMS_DEVICE, n_times, ld, ell_min, ell_max, dptr(q))
        ctx.check(rc, "bms_rotate_const")


def wigner_D(quaternion, ell_min, ell_max, ctx=None):
    """Packed D^l_{m',m}(q), layout of sf.Wigner_D_matrices."""
    ctx = _ctx(ctx)
    q = np.ascontiguousarray(quaternion, dtype=float)
    D = np.zeros(total_size_D_matrices(ell_min, ell_max), dtype=np.complex128)
    ctx.check(_lib.load().bms_wigner_D(ctx.handle, dptr(q), ell_min, ell_max, vptr(D)), "bms_wigner_D")
    return D


# ---------------------------------------------------------------------------------- transform


def make_transformation(supertranslation, frame_rotation, boost_velocity, n_theta, n_phi, ell_max_out):
    st = np.ascontiguousarray(supertranslation, dtype=np.complex128)
    lst = int(round(np.sqrt(st.size))) - 1
    if (lst + 1) ** 2 != st.size or lst < 1:
        raise ValueError("supertranslation must hold (L+1)^2 modes with L >= 1")
    tr = bms_transformation()
    tr.supertranslation = st.ctypes.data
    tr.ell_max_supertranslation = lst
    tr.frame_rotation[:] = [float(x) for x in frame_rotation]
    tr.boost_velocity[:] = [float(x) for x in boost_velocity]
    tr.n_theta, tr.n_phi, tr.ell_max_out = int(n_theta), int(n_phi), int(ell_max_out)
    tr._keep = st  # keep the array alive
    return tr


# Host arrays in and out: below this size one call moves the data and computes; above it the time axis is pipelined
PIPELINE_MIN_BYTES = 64 << 20
PIPELINE_PIECES = int(os.environ.get("SCRI_AMD_PIPELINE_PIECES", "10"))  # cfg3, round 2: 15.5 ms at 4 pieces, 15.0 at 6, 13.9 at 8, 13.6 at 10 (26.9 as one call)
_PIECES_FORCED = "SCRI_AMD_PIPELINE_PIECES" in os.environ


def auto_pieces(n_rows, ell_max, nbytes):
    """Time shards of a host-memory WaveformModes call on ONE context, from the series' shape (profiles/r06_r_host_path_by_size.txt:
    l <= 4, 8, 16, 24, 2.5e3 .. 4e5 rows, 1 .. 20 shards each).  More shards overlap more of the transfers with the kernels -- until a
    shard falls below about 70 000 / l_max rows, where upload, kernels and download stop running side by side (the call is 50 % slower
    from one shard count to the next, and bimodal at the edge).  So: shards of at least 100 000 / l_max rows, at most 20 of them; a
    series too short for two such shards is still cut in two from 16 MB on (1.77 against 2.34 ms at 43 MB, l <= 16).  1: one call.
    Against the fixed ten shards from 64 MB on that this replaces: 87 MB 3.79 -> 2.94 ms, 130 MB 5.28 -> 4.00, 44 MB 2.34 -> 1.77,
    435 MB 11.0 -> 10.7 (l <= 16); 117 MB 4.74 -> 3.31 (l <= 8)."""
    if _PIECES_FORCED:
        return PIPELINE_PIECES if nbytes >= PIPELINE_MIN_BYTES else 1
    rows_per_piece = -(-100000 // max(int(ell_max), 4))
    pieces = min(int(n_rows) // rows_per_piece, 20)
    if pieces < 2:
        pieces = 2 if nbytes >= min(16 << 20, PIPELINE_MIN_BYTES) else 1  # (PIPELINE_MIN_BYTES: the threshold of the six-field call; tests lower it)
    return pieces


def auto_pieces_abd(nbytes):
    """The same choice for the six-field call (profiles/r06_r_host_path_by_size.txt, second half): a shard of six fields costs about a
    millisecond of set-up of its own (six synthesis matrices), so shards of at least 75 MB, at most ten, one call below 64 MB.  Against the
    fixed ten shards this replaces: 77 MB 14.1 -> 6.3 ms, 155 MB 17.0 -> 10.4, 309 MB 23.0 -> 17.8 (l <= 12); 90 MB 10.2 -> 5.1 (l <= 6);
    unchanged from 600 MB on."""
    if _PIECES_FORCED:
        return PIPELINE_PIECES if nbytes >= PIPELINE_MIN_BYTES else 1
    if nbytes < PIPELINE_MIN_BYTES:
        return 1
    return max(2, min(int(nbytes // (75 << 20)), 10))


_device_contexts = {}  # (device, slot) -> Context of the one-process multi-device calls (slot: the k-th context on that device)
_device_contexts_lock = threading.Lock()


def default_devices():
    """SCRI_AMD_DEVICES = "0,1,2,3" (or "all"): the devices host-memory transformations of long series are dealt over when the caller
    names none -- existing callers of w.transform(**kw) / abd.transform(**kw) then use every GPU of the node unchanged.  Unset: one."""
    env = os.environ.get("SCRI_AMD_DEVICES", "").strip()
    if not env:
        return None
    if env == "all":
        import torch  # (device_count() does not initialise the GPU)

        return list(range(max(torch.cuda.device_count(), 1)))
    return [int(x) for x in env.split(",") if x.strip() != ""]


def contexts_for(devices, first=None):
    """One context per entry of `devices` (a device named k times gets k contexts: on a one-GPU box `[0, 0, 0, 0]` runs the
    four-way code path).  Kept for the life of the process -- their work space is what makes the second call fast.  `first`: a
    context the caller already has; it serves the first entry that names its device."""
    out, counts = [], {}
    with _device_contexts_lock:
        for d in devices:
            d = int(d)
            slot = counts.get(d, 0)
            counts[d] = slot + 1
            if first is not None and first.device == d and slot == 0:
                out.append(first)
                continue
            ctx = _device_contexts.get((d, slot))
            if ctx is None or not ctx.handle:
                ctx = _device_contexts[(d, slot)] = _lib.Context(d)
            out.append(ctx)
    return out


def pieces_for(devices, n_rows=None, ell_max=None, nbytes=None, abd=False):
    """How many time shards a multi-device call cuts the output window into.  Every context runs the one-context pipeline on its share
    of the series (its own link, its own three streams), so its share is cut by the one-context rule for a series of that size
    (auto_pieces / auto_pieces_abd on n_rows / n, nbytes / n), at least two shards per context where the share allows it: upload,
    kernels and download of neighbouring shards overlap inside each context.  Without the shape: three per context and at least
    PIPELINE_PIECES in all (round 6's first rule -- which at cfg3 on eight devices cuts shards of 4 166 rows, on the edge
    profiles/r06_r_host_path_by_size.txt shows)."""
    n = len(devices)
    if n_rows is None or nbytes is None or (ell_max is None and not abd) or _PIECES_FORCED:
        return n * max(3, -(-PIPELINE_PIECES // n))
    share_rows, share_bytes = int(n_rows) // n, int(nbytes) // n
    per = auto_pieces_abd(share_bytes) if abd else auto_pieces(share_rows, ell_max, share_bytes)
    if per < 2 and share_rows >= 64:
        per = 2
    return n * per


def _run_dealt(ctxs, pieces, call):
    """call(ctx, item0, item1) for contiguous runs of `pieces` items on one host thread per context (ctypes releases the GIL inside
    the library; a context is used by one thread at a time: the threading contract of include/scri_amd.h).  Returns the exceptions,
    per context.  The rotations deal their rows with it; the transformations' time shards are dealt inside the library by the
    same rule (bms_transform_modes_multi / bms_transform_abd_multi)."""
    n = len(ctxs)
    errors = [None] * n

    def run(k):
        try:
            p0, p1 = (pieces * k) // n, (pieces * (k + 1)) // n
            if p1 > p0:
                call(ctxs[k], p0, p1)
        except BaseException as e:  # noqa: BLE001 -- re-raised by the caller's thread
            errors[k] = e

    threads = [threading.Thread(target=run, args=(k,)) for k in range(1, n)]
    for th in threads:
        th.start()
    run(0)
    for th in threads:
        th.join()
    return errors


def _context_array(ctxs):
    arr = (c_vp * len(ctxs))(*[c.handle for c in ctxs])
    return arr


def _wm_input(t, data, ld, mem, ell_min, ell_max, spin_weight, conformal_weight, type_term, aux=()):
    """bms_wm_input of the time axis `t` (float64, contiguous), the data's address, row stride and memory kind, and per psi companion
    (address, row stride, ell_min, ell_max, spin, coeff, power)."""
    inp = bms_wm_input()
    inp.n_times, inp.t = t.shape[0], dptr(t)
    inp.data, inp.ld, inp.mem = int(data), int(ld), mem
    inp.ell_min, inp.ell_max = int(ell_min), int(ell_max)
    inp.spin_weight, inp.conformal_weight, inp.type_term = int(spin_weight), int(conformal_weight), int(type_term)
    inp.n_aux = len(aux)
    for i, (adata, ald, amin, amax, aspin, acoeff, apower) in enumerate(aux):
        inp.aux_data[i], inp.aux_ld[i] = int(adata), int(ald)
        inp.aux_ell_min[i], inp.aux_ell_max[i], inp.aux_spin[i] = int(amin), int(amax), int(aspin)
        inp.aux_coeff[i], inp.aux_power[i] = float(acoeff), int(apower)
    return inp


def _run_pipelined(ctxs, single, multi, *args):
    """The pipelined call on one context (entry `single`) or its time shards dealt in contiguous runs over several, one host thread each
    inside the library (entry `multi`); every context ships its own rows + halo at upload time, no GPU-to-GPU traffic.  `args` follow
    the context argument(s).  False: a series the engine does not shard (graded time steps), which the one-call path takes."""
    lib = _lib.load()
    if len(ctxs) == 1:
        name, rc = single, getattr(lib, single)(ctxs[0].handle, *args)
    else:
        name, rc = multi, getattr(lib, multi)(_context_array(ctxs), len(ctxs), *args)
    try:
        ctxs[0].check(rc, name)
    except NotImplementedError:
        return False
    return True


def _transform_modes_pipelined(t, data, inp, transformation, n_out, ctxs, pieces):
    """Host-memory callers of a long series wait for PCIe, not for the kernels (cfg3: 456 MB each way against 6 ms of
    kernels), and one call does upload -> kernels -> download one after the other.  bms_transform_modes_pipelined cuts the
    output range into `pieces` time shards (bms_shard_plan names the input rows each one needs, exactly as for the
    multi-GPU split) and runs upload, kernels and download of neighbouring shards side by side on three streams;
    bms_transform_modes_multi deals the shards over the contexts `ctxs`.  Results are those of the sharded path (equal to the
    one-call path to rounding; tests/test_gpu_sharding.py) and depend on `pieces` only.  Returns None when the series cannot
    be sharded (graded time steps).  (`data`, the array `inp` points to, is not read: it keeps the argument order of the two
    helpers this one merges.)"""
    if not np.all(np.diff(t) > 0):
        return None  # the one-call path raises the ValueError the reference's callers expect
    n = t.shape[0]
    if n < 8 * pieces + 16:
        return None
    # (sized for the whole series: the window of valid outputs is at most that, and asking for it first would cost a round trip to
    # the device before anything is dealt; the result is the leading rows, a view)
    out = _lib.pinned_empty((n, n_out), np.complex128)
    t_out = np.empty(n, dtype=float)
    got = c_i64(0)
    if not _run_pipelined(ctxs, "bms_transform_modes_pipelined", "bms_transform_modes_multi", ctypes.byref(inp), ctypes.byref(transformation),
                          int(pieces), dptr(t_out), vptr(out), ctypes.byref(got)):
        return None
    return t_out[: got.value], out[: got.value]


_transform_modes_multi = _transform_modes_pipelined  # (the dealt call site's name: `devices=` calls are observed under it on their own)


def transform_modes(
    t,
    data,
    ell_min,
    ell_max,
    spin_weight,
    conformal_weight,
    type_term,
    transformation,
    aux=(),
    ctx=None,
    device=False,
    ld=None,
    out_ptr=None,
    shard=None,
    grid=False,
    devices=None,
    pieces=None,
):
    """bms_transform_modes.  Host mode: data complex128 [N, n_modes] -> (t_out[N'], data_out[N', n_out]).
    grid=True (host mode, no shard): bms_modes_to_grid instead -- the field on the distorted grid at the new time slices,
    (t_out[N'], grid[N', n_theta * n_phi]), i.e. WaveformGrid.from_modes without the analysis back to modes.
    Device mode (device=True): `data` and each aux data are device addresses, `ld` the row stride,
    `out_ptr` a device buffer of N * n_out complex; returns (t_out[N'], N').
    aux: sequence of (data, ell_min, ell_max, spin, coeff, power[, ld]).
    shard: optional (data_row0, data_rows, out_i0, out_i1) -- `t` stays the GLOBAL time array, `data` holds only
    rows [data_row0, data_row0 + data_rows); outputs are those with global input index in [out_i0, out_i1);
    the returned tuple then has the first global index appended.  Two more entries (col_part, col_parts) select a
    part of the grid columns (include/scri_amd.h, bms_shard): the output is then that part's contribution, to be
    summed over the parts.
    devices (host mode, no shard): the GPUs of this process the time shards of the pipelined call are dealt over, one
    context and one host thread per entry, e.g. [0, 1, ..., 7] (default: SCRI_AMD_DEVICES, else the one context `ctx`); every
    device receives its own rows + halo at upload time, psi companions' rows included.  pieces: the number of time shards (default
    PIPELINE_PIECES on one context, pieces_for(devices) on several); the result depends on `pieces` only (to rounding), not on how
    they are dealt.  A call with psi companions takes the pipelined or dealt path only when it names `devices` or `pieces`:
    neither SCRI_AMD_DEVICES nor auto_pieces applies to it."""
    if devices is None and not device and shard is None and not grid and not aux and np.asarray(data).nbytes >= PIPELINE_MIN_BYTES:
        devices = default_devices()  # (the environment's default is for LONG series: a short one is not worth k threads and k set-ups)
    if devices is not None and (device or shard is not None or grid):
        raise ValueError("`devices` deals a whole host-memory series over several GPUs: no shard, no device pointers, no grid output")
    ctx = _ctx(ctx) if not devices else contexts_for(devices[:1], first=ctx)[0]
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    n_rows = n if shard is None else int(shard[1])
    if not device:
        data = _lib.as_c16(data)
        if data.shape != (n_rows, LM_total_size(ell_min, ell_max)):
            raise ValueError(f"data shape {data.shape} inconsistent with rows={n_rows}, ell range [{ell_min}, {ell_max}]")
    aux_host = []  # (the host companions, kept alive through the call)
    aux_in = []
    for a in aux:
        adata, amin, amax, aspin, acoeff, apower = a[:6]
        if device:
            aux_in.append((adata, a[6], amin, amax, aspin, acoeff, apower))
            continue
        adata = _lib.as_c16(adata)
        if adata.shape != (n_rows, LM_total_size(amin, amax)):
            raise ValueError("auxiliary data shape mismatch")
        aux_host.append(adata)
        aux_in.append((adata.ctypes.data, adata.shape[1], amin, amax, aspin, acoeff, apower))
    if device:
        inp = _wm_input(t, data, ld, BMS_DEVICE, ell_min, ell_max, spin_weight, conformal_weight, type_term, aux_in)
    else:
        inp = _wm_input(t, data.ctypes.data, data.shape[1], BMS_HOST, ell_min, ell_max, spin_weight, conformal_weight, type_term, aux_in)
    s = abs(int(spin_weight))
    n_out = LM_total_size(s, transformation.ell_max_out)
    n_new = c_i64(0)
    first = c_i64(0)
    sh = None
    n_alloc = n
    if shard is not None:
        sh = bms_shard(*[int(x) for x in shard])
        n_alloc = max(0, min(n, int(shard[3])) - max(0, int(shard[2])))
    t_out = np.empty(max(n_alloc, 1), dtype=float)
    shp = ctypes.byref(sh) if sh is not None else None
    if device:
        rc = _lib.load().bms_transform_modes_shard(
            ctx.handle, ctypes.byref(inp), ctypes.byref(transformation), shp, dptr(t_out), c_vp(int(out_ptr)),
            ctypes.byref(n_new), ctypes.byref(first),
        )
        ctx.check(rc, "bms_transform_modes")
        res = (t_out[: n_new.value], n_new.value)
        return res + (first.value,) if shard is not None else res
    if grid:
        if shard is not None:
            raise ValueError("the grid output does not combine with a shard")
        out = _lib.pinned_empty((max(n, 1), transformation.n_theta * transformation.n_phi), np.complex128)
        rc = _lib.load().bms_modes_to_grid(ctx.handle, ctypes.byref(inp), ctypes.byref(transformation), dptr(t_out), vptr(out), ctypes.byref(n_new))
        ctx.check(rc, "bms_modes_to_grid")
        return t_out[: n_new.value], out[: n_new.value]
    if not device:
        _lib.register_if_reused(data)  # an input array seen for the second time is page-locked in place: uploads at PCIe rate
        if devices or pieces is not None:
            for adata in aux_host:  # (the companions travel with every shard's rows: the same rate for them)
                _lib.register_if_reused(adata)
    if devices:
        res = _transform_modes_multi(t, data, inp, transformation, n_out, contexts_for(devices, first=ctx),
                                     int(pieces or pieces_for(devices, n, ell_max, data.nbytes)))
        if res is not None:
            return res
    elif shard is None and (not aux or pieces is not None) and not os.environ.get("SCRI_AMD_NO_PIPELINE"):
        chosen = int(pieces) if pieces is not None else auto_pieces(n, ell_max, data.nbytes)
        if pieces is not None or chosen >= 2:
            res = _transform_modes_pipelined(t, data, inp, transformation, n_out, [ctx], chosen)
            if res is not None:
                return res
    out = _lib.pinned_empty((max(n_alloc, 1), n_out), np.complex128)
    rc = _lib.load().bms_transform_modes_shard(
        ctx.handle, ctypes.byref(inp), ctypes.byref(transformation), shp, dptr(t_out), vptr(out), ctypes.byref(n_new),
        ctypes.byref(first),
    )
    ctx.check(rc, "bms_transform_modes")
    res = (t_out[: n_new.value], out[: n_new.value])  # leading rows: contiguous views, no trimming copy
    return res + (first.value,) if shard is not None else res


def transform_modes_series(t, data, ell_min, ell_max, spin_weight, conformal_weight, type_term, transformation, aux=(), ctx=None, grid=False,
                           device=False, n_series=None, out_ptr=None):
    """bms_transform_modes_series: data complex [N, n_modes, F] -- F independent series under one transformation, the reference's
    extra trailing data dimensions flattened (scri/waveform_grid.py:299-308, 574-594) -- -> (t_out[N'], out[N', n_out, F]) in ONE
    engine call.  The arrays cross PCIe as they are (the trailing index fastest: no strided copy on the host; the permutation to one
    block of columns per series runs on the device) and the set-up (time axis, spline tables, per-direction tables, window) is shared.
    aux: (data [N, aux_modes, F], ell_min, ell_max, spin, coeff, power) per psi companion.  grid=True: the field on the grid instead
    (WaveformGrid.from_modes), out[N', n_theta n_phi, F].
    device=True: `data` (and each aux data) is a device address of c16[N][n_modes * n_series] in that same layout, `out_ptr` a device
    buffer of N * n_out * n_series complex; nothing crosses PCIe; returns (t_out, N')."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    if device:
        aux_in = [(a[0], LM_total_size(a[1], a[2]) * int(n_series)) + tuple(a[1:6]) for a in aux]
        inp = _wm_input(t, data, LM_total_size(ell_min, ell_max) * int(n_series), BMS_DEVICE, ell_min, ell_max, spin_weight, conformal_weight,
                        type_term, aux_in)
        t_out = np.empty(max(n, 1), dtype=float)
        n_new = c_i64(0)
        rc = _lib.load().bms_transform_modes_series(ctx.handle, ctypes.byref(inp), int(n_series), ctypes.byref(transformation), dptr(t_out),
                                                    None if grid else c_vp(int(out_ptr)), c_vp(int(out_ptr)) if grid else None, ctypes.byref(n_new))
        ctx.check(rc, "bms_transform_modes_series")
        return t_out[: n_new.value], n_new.value
    data = _lib.as_c16(data)
    if data.ndim != 3 or data.shape[:2] != (n, LM_total_size(ell_min, ell_max)):
        raise ValueError(f"data shape {data.shape} inconsistent with {n} time steps, ell range [{ell_min}, {ell_max}] and one trailing axis")
    n_series = data.shape[2]
    aux_host = []  # (kept alive through the call)
    for a in aux:
        adata = _lib.as_c16(a[0])
        if adata.shape != (n, LM_total_size(a[1], a[2]), n_series):
            raise ValueError("auxiliary data shape mismatch")
        aux_host.append(adata)
    aux_in = [(h.ctypes.data, h.shape[1] * n_series) + tuple(a[1:6]) for h, a in zip(aux_host, aux)]
    inp = _wm_input(t, data.ctypes.data, data.shape[1] * n_series, BMS_HOST, ell_min, ell_max, spin_weight, conformal_weight, type_term, aux_in)
    n_out = transformation.n_theta * transformation.n_phi if grid else LM_total_size(abs(int(spin_weight)), transformation.ell_max_out)
    out = _lib.pinned_empty((max(n, 1), n_out, n_series), np.complex128)
    t_out = np.empty(max(n, 1), dtype=float)
    n_new = c_i64(0)
    rc = _lib.load().bms_transform_modes_series(ctx.handle, ctypes.byref(inp), n_series, ctypes.byref(transformation), dptr(t_out),
                                                None if grid else vptr(out), vptr(out) if grid else None, ctypes.byref(n_new))
    ctx.check(rc, "bms_transform_modes_series")
    return t_out[: n_new.value], out[: n_new.value]


def output_window(t, transformation, abd=False, ctx=None):
    """bms_output_window -> (i_lo, i_hi): output sample r of the transformation has input index i_lo + r."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    win = (c_i64 * 2)()
    rc = _lib.load().bms_output_window(ctx.handle, dptr(t), t.shape[0], ctypes.byref(transformation), int(bool(abd)), win)
    ctx.check(rc, "bms_output_window")
    return int(win[0]), int(win[1])


def shard_plan(t, transformation, out_i0, out_i1, ctx=None):
    """bms_shard_plan -> ((need_row0, need_row1), (i_lo, i_hi)): input rows a rank must hold to produce the
    outputs with global input index in [out_i0, out_i1), and the global valid output window."""
    t = np.ascontiguousarray(t, dtype=float)
    need = (c_i64 * 2)()
    win = (c_i64 * 2)()
    # host-only planning: works without a GPU context
    rc = _lib.load().bms_shard_plan(None, dptr(t), t.shape[0], ctypes.byref(transformation), int(out_i0), int(out_i1), need, win)
    if rc != 0:
        _lib._raise(rc, None, "bms_shard_plan")
    return (need[0], need[1]), (win[0], win[1])


def transform_abd(u, raw, ell_max, transformation, ctx=None, shard=None, device=False, out_ptr=None, devices=None, pieces=None):
    """bms_transform_abd[_shard]: raw complex128 [6, N, (ell_max+1)^2] -> (u_out[N'], raw_out[6, N', n_out]).

    shard = (data_row0, data_rows, out_i0, out_i1): `u` stays the GLOBAL time axis, `raw` holds rows
    [data_row0, data_row0 + data_rows) of every field, and the result carries a third element, the global input
    index of output row 0.  device=True: `raw` and `out_ptr` are device pointers (c16[6][data_rows][n_modes] and
    c16[6][out_i1 - out_i0][n_out]); returns (u_out, n_new[, first]).
    devices / pieces (host arrays, no shard): as transform_modes -- the time shards of the pipelined call dealt over one context
    per device of this process."""
    if devices is None and not device and shard is None and np.asarray(raw).nbytes >= PIPELINE_MIN_BYTES:
        devices = default_devices()
    if devices is not None and (device or shard is not None):
        raise ValueError("`devices` deals a whole host-memory series over several GPUs: no shard, no device pointers")
    ctx = _ctx(ctx) if not devices else contexts_for(devices[:1], first=ctx)[0]
    u = np.ascontiguousarray(u, dtype=float)
    n = u.shape[0]
    n_rows = n if shard is None else int(shard[1])
    n_out = (transformation.ell_max_out + 1) ** 2
    sh = None
    fs_out = n
    if shard is not None:
        sh = bms_shard(*[int(x) for x in shard])
        fs_out = int(shard[3]) - int(shard[2])
    shp = ctypes.byref(sh) if sh is not None else None
    u_out = np.empty(max(fs_out, 1), dtype=float)
    n_new = c_i64(0)
    first = c_i64(0)
    if device:
        rc = _lib.load().bms_transform_abd_shard(
            ctx.handle, dptr(u), c_vp(int(raw)), BMS_DEVICE, n, int(ell_max), ctypes.byref(transformation), shp, dptr(u_out),
            c_vp(int(out_ptr)), ctypes.byref(n_new), ctypes.byref(first),
        )
        ctx.check(rc, "bms_transform_abd")
        res = (u_out[: n_new.value], n_new.value)
        return res + (first.value,) if shard is not None else res
    raw = _lib.as_c16(raw)
    if raw.shape != (6, n_rows, (ell_max + 1) ** 2):
        raise ValueError(f"raw shape {raw.shape} inconsistent")
    _lib.register_if_reused(raw)
    if shard is None:
        # size the result exactly (the window is known before the data move): no trimming copy of hundreds of MB afterwards
        i_lo, i_hi = output_window(u, transformation, abd=True, ctx=ctx)
        sh = bms_shard(0, n, i_lo, i_hi)
        shp = ctypes.byref(sh)
        fs_out = i_hi - i_lo
        u_out = np.empty(max(fs_out, 1), dtype=float)
    out = _lib.pinned_empty((6, max(fs_out, 1), n_out), np.complex128)
    n_pieces = int(pieces or (pieces_for(devices, n, None, raw.nbytes, abd=True) if devices else auto_pieces_abd(raw.nbytes)))
    ctxs = None
    if devices:
        # one process, several GPUs: the time shards dealt over one context per device, rows + halo shipped at upload time
        if fs_out >= 8 * n_pieces and np.all(np.diff(u) > 0):
            ctxs = contexts_for(devices, first=ctx)
    elif (shard is None and (pieces is not None or n_pieces >= 2) and fs_out >= 8 * n_pieces
          and not os.environ.get("SCRI_AMD_NO_PIPELINE")):
        ctxs = [ctx]  # a long series in host memory: uploads, kernels and downloads of consecutive time shards side by side
    # (graded time steps are not sharded: the one-call path below takes them)
    if ctxs and _run_pipelined(ctxs, "bms_transform_abd_pipelined", "bms_transform_abd_multi", dptr(u), vptr(raw), n, int(ell_max),
                               ctypes.byref(transformation), n_pieces, dptr(u_out), vptr(out), ctypes.byref(n_new)):
        if n_new.value != out.shape[1]:
            raise RuntimeError(f"the pipelined ABD transform produced {n_new.value} rows, expected {out.shape[1]}")
        return u_out, out
    rc = _lib.load().bms_transform_abd_shard(
        ctx.handle, dptr(u), vptr(raw), BMS_HOST, n, int(ell_max), ctypes.byref(transformation), shp, dptr(u_out), vptr(out),
        ctypes.byref(n_new), ctypes.byref(first),
    )
    ctx.check(rc, "bms_transform_abd")
    if n_new.value == out.shape[1]:
        res = (u_out, out)
    else:
        res = (u_out[: n_new.value].copy(), out[:, : n_new.value].copy())
    return res + (first.value,) if shard is not None else res


# ---------------------------------------------------------------------------------- building blocks


def rotor_grid(frame_rotation, boost_velocity, n_theta, n_phi, ctx=None, device=False):
    """boosted_grid / R_j_k.  Default: host-only evaluation (works without a GPU); device=True runs the GPU kernel the
    transforms use (same code, pixel_math.h) on `ctx`."""
    fr = np.ascontiguousarray(frame_rotation, dtype=float)
    v = np.ascontiguousarray(boost_velocity, dtype=float)
    out = np.empty((n_theta, n_phi, 4))
    h = _ctx(ctx).handle if device else None
    rc = _lib.load().bms_rotor_grid(h, dptr(fr), dptr(v), n_theta, n_phi, dptr(out))
    if rc != 0:
        _lib._raise(rc, h, "bms_rotor_grid")
    return out


def ring_colatitudes(frame_rotation, boost_velocity, n_theta, n_phi):
    """The colatitudes Theta_j of the rotor grid's rings if it is frame_rotation * R(Theta_j, phi'_k) -- no boost, or one along the
    polar axis of the rotated grid -- else None.  Host only: the test that sends a transformation to the separable synthesis."""
    fr = np.ascontiguousarray(frame_rotation, dtype=float)
    v = np.ascontiguousarray(boost_velocity, dtype=float)
    out = np.empty(n_theta)
    rc = _lib.load().bms_ring_colatitudes(dptr(fr), dptr(v), n_theta, n_phi, dptr(out))
    if rc < 0:
        _lib._raise(rc, None, "bms_ring_colatitudes")
    return out if rc == 1 else None


def conformal_factors(boost_velocity, rotors):
    """bms_conformal_factors: (k, eth k / k, 1/k, 1/k^3) on rotors [..., 4], each shaped like rotors[..., 0]."""
    v = np.ascontiguousarray(boost_velocity, dtype=float)
    R = np.ascontiguousarray(rotors, dtype=float)
    shape = R.shape[:-1]
    n = int(np.prod(shape))
    k, ik, ik3 = np.empty(n), np.empty(n), np.empty(n)
    e = np.empty(n, dtype=np.complex128)
    rc = _lib.load().bms_conformal_factors(None, dptr(v), dptr(R), n, dptr(k), vptr(e), dptr(ik), dptr(ik3))
    if rc != 0:
        _lib._raise(rc, None, "bms_conformal_factors")
    return k.reshape(shape), e.reshape(shape), ik.reshape(shape), ik3.reshape(shape)


def swsh_grid(rotors, spin, ell_min, ell_max, ctx=None, host=False):
    """sf.SWSH_grid(R, s, ell_max)[..., ell_min^2:].  host=True: the set-up header evaluated on the host (no GPU)."""
    R = np.ascontiguousarray(rotors, dtype=float)
    shape = R.shape[:-1]
    R2 = R.reshape(-1, 4)
    out = np.zeros((R2.shape[0], LM_total_size(ell_min, ell_max)), dtype=np.complex128)
    if host:
        rc = _lib.load().bms_swsh_grid(None, dptr(R2), R2.shape[0], spin, ell_min, ell_max, vptr(out))
        if rc != 0:
            _lib._raise(rc, None, "bms_swsh_grid")
    else:
        ctx = _ctx(ctx)
        ctx.check(_lib.load().bms_swsh_grid(ctx.handle, dptr(R2), R2.shape[0], spin, ell_min, ell_max, vptr(out)), "bms_swsh_grid")
    return out.reshape(shape + (out.shape[1],))


def evaluate_modes(modes, spin, ell_min, ell_max, rotors, ctx=None):
    """sf.Modes(modes, spin_weight=s, ell_min, ell_max).evaluate(R): modes[..., n_modes] at rotors[..., 4] -> [..., *rotors.shape[:-1]]
    (the harmonics at the rotors and one product on the matrix cores: bms_evaluate_modes)."""
    ctx = _ctx(ctx)
    a = _lib.as_c16(modes)
    nm = LM_total_size(ell_min, ell_max)
    if a.shape[-1] != nm:
        raise ValueError(f"modes must hold l = {ell_min}..{ell_max} ({nm} columns), got {a.shape[-1]}")
    R = np.ascontiguousarray(rotors, dtype=float)
    if R.shape[-1] != 4:
        raise ValueError("rotors must be float quaternions [..., 4]")
    R2 = R.reshape(-1, 4)
    a2 = a.reshape(-1, nm)
    out = np.empty((a2.shape[0], R2.shape[0]), dtype=np.complex128)
    rc = _lib.load().bms_evaluate_modes(ctx.handle, vptr(a2), BMS_HOST, a2.shape[0], nm, int(spin), int(ell_min), int(ell_max), dptr(R2),
                                        R2.shape[0], vptr(out))
    ctx.check(rc, "bms_evaluate_modes")
    return out.reshape(a.shape[:-1] + R.shape[:-1])


def map2salm(grid, spin, ell_max, ell_min=0, ctx=None):
    """spinsfast.map2salm(grid[..., n_theta, n_phi], s, ell_max)[..., ell_min^2:]."""
    ctx = _ctx(ctx)
    g = _lib.as_c16(grid)
    n_theta, n_phi = g.shape[-2:]
    lead = g.shape[:-2]
    g2 = g.reshape(-1, n_theta * n_phi)
    out = np.empty((g2.shape[0], LM_total_size(ell_min, ell_max)), dtype=np.complex128)
    rc = _lib.load().bms_map2salm(ctx.handle, vptr(g2), BMS_HOST, g2.shape[0], n_theta, n_phi, spin, ell_min, ell_max, vptr(out))
    ctx.check(rc, "bms_map2salm")
    return out.reshape(lead + (out.shape[1],))


# ---- one description of a caller's array for the entries that take `int mem`: a numpy array (host) or a torch tensor (device)

# ptr: the address (c_vp); ld: row stride in elements; rows, cols; mem: BMS_HOST / BMS_DEVICE; tail: the trailing shape of a host array
# that was flattened to [rows, cols]; keep: the object that owns the memory (alive through the call); device: the torch device or None
_Arg = collections.namedtuple("_Arg", "ptr ld rows cols mem tail keep device")
_TORCH_DTYPE = {np.complex128: "complex128", float: "float64", np.uint64: "int64"}  # (the packed words travel as int64 in torch)
_torch_dtypes = {}  # the torch dtype objects of those names, looked up once (torch is imported only by a call that passes a tensor)


def _torch_dtype(dtype):
    t = _torch_dtypes.get(dtype)
    if t is None:
        import torch

        t = _torch_dtypes[dtype] = getattr(torch, _TORCH_DTYPE[dtype])
    return t


def _is_device_array(x):
    """a torch tensor: device memory to the wrappers, which refuse one that is not on the context's device (_on_device_of)"""
    return hasattr(x, "data_ptr")


def _on_device_of(ctx, *arrays):
    for x in arrays:
        if _is_device_array(x) and x.device.index != ctx.device:
            raise ValueError(f"a device array on {x.device} was passed to a context on device {ctx.device}")


def _address(a):
    """the address of a C-contiguous numpy array as c_vp: through the buffer protocol, several times quicker than `a.ctypes`, which
    only read-only and empty arrays still go through"""
    try:
        return c_vp(ctypes.addressof(ctypes.c_char.from_buffer(a)))
    except (TypeError, ValueError):
        return vptr(a)


def _shape_is(shape, actual):
    """`actual` is 2-d and has the rows and the columns `shape` names (None: any)"""
    return len(actual) == 2 and (shape is None or ((shape[0] is None or shape[0] == actual[0]) and (shape[1] is None or shape[1] == actual[1])))


def _row_stride(x, rows, cols):
    """THE row-stride rule: the row stride in elements of a device tensor [rows, cols] with unit column stride (the stride of one row
    is anything, e.g. 1 for a transposed column: the entries take the columns)"""
    return x.stride(0) if rows > 1 else max(cols, 1)


def _stage(ctx, x, dtype, what, shape=None, flatten=False, contiguous=False, check_dtype=True, attach=True):
    """The _Arg of `x`, [rows, cols] elements of `dtype` (np.complex128, float, or np.uint64 words).  shape: the (rows, cols) it must
    have, None for any.  A device tensor is 2-d with unit column stride unless it has one column (any row stride: THE row-stride rule
    is _row_stride), or with contiguous=True any shape of rows * cols elements in one block; it must live on the context's device.  A host
    array is converted to a C-contiguous one; flatten: it may be [rows, ...], whose trailing axes become the columns.
    check_dtype=False / attach=False: the wrappers that never checked a device tensor's dtype / never ordered the context's work
    with torch's stream (device_series.attach) keep that.  (On the path of every small call: no numpy reductions, no generators.)"""
    if hasattr(x, "data_ptr"):  # (_is_device_array, without the call)
        if attach:
            from . import device_series

            device_series.attach(ctx)
        if x.device.index != ctx.device:
            _on_device_of(ctx, x)  # (raises)
        sh = x.shape
        if contiguous:
            rows, cols = shape if shape is not None else ((sh[0] if sh else 1), math.prod(sh[1:]))
            ok = x.is_contiguous() and x.numel() == rows * cols
        else:
            ok = (len(sh) == 2 if shape is None else _shape_is(shape, sh)) and (sh[1] <= 1 or x.stride(1) == 1)
            rows, cols = (sh[0], sh[1]) if ok else (0, 0)
        if not ok or (check_dtype and x.dtype != _torch_dtype(dtype)):
            raise ValueError(f"{what}: expected a {'contiguous ' if contiguous else ''}{_TORCH_DTYPE[dtype]} device array{_shape_text(shape)}"
                             f"{'' if contiguous else ' with unit column stride'}, got {x.dtype} of shape {tuple(x.shape)} on {x.device}")
        ld = cols if contiguous else _row_stride(x, rows, cols)
        return _Arg(c_vp(x.data_ptr()), ld, rows, cols, BMS_DEVICE, (cols,), x, x.device)
    a = np.ascontiguousarray(x, dtype=dtype)
    sh = a.shape
    tail = sh[1:]
    if flatten and len(sh) != 2:
        a = a.reshape(sh[0], math.prod(tail))
        sh = a.shape
    if shape is not None and not _shape_is(shape, sh):
        raise ValueError(f"{what} must have shape{_shape_text(shape)}; it has shape {sh}")
    cols = sh[1] if len(sh) == 2 else math.prod(tail)
    return _Arg(_address(a), cols or 1, (sh[0] if sh else 1), cols, BMS_HOST, tail, a, None)


def _shape_text(shape):
    return "" if shape is None else " (" + ", ".join("n" if s is None else str(s) for s in shape) + ")"


def _beside(x):
    """what out_like reads of an _Arg -- the memory kind and the torch device -- for an array that is not staged"""
    return _Arg(None, None, None, None, BMS_DEVICE if _is_device_array(x) else BMS_HOST, None, x, x.device if _is_device_array(x) else None)


def out_like(arg, shape, dtype, out=None):
    """(address, array): a new array of `shape` and `dtype` beside `arg` -- a torch tensor on its device, or a numpy array.  out: the
    contiguous device tensor of that many elements the caller wants written instead (device arguments only)."""
    if arg.mem == BMS_DEVICE:
        tdtype = _torch_dtype(dtype)
        if out is None:
            out = sys.modules["torch"].empty(*shape, dtype=tdtype, device=arg.device)  # (sizes one by one: quicker than a tuple)
        elif out.dtype != tdtype or out.device != arg.device or not out.is_contiguous() or out.numel() != math.prod(shape):
            raise ValueError(f"out: expected a contiguous {_TORCH_DTYPE[dtype]} array of {' x '.join(str(s) for s in shape)} values on {arg.device}")
        return c_vp(out.data_ptr()), out
    if out is not None:
        raise ValueError("out= names a device array; with a host input the result is a new host array")
    out = np.empty(shape, dtype=dtype)
    return _address(out), out


def _spline_call(entry, x, y, x_new, ctx, *order):
    ctx = _ctx(ctx)
    x = np.ascontiguousarray(x, dtype=float)
    xn = np.ascontiguousarray(x_new, dtype=float)
    a = _stage(ctx, y, np.complex128, "a series", flatten=True)
    # (a device series has the knots' rows, as it always had to; of a longer host series the first rows are used, as they always
    # were; a shorter one the entry would read past)
    wrong_rows = (a.rows != x.shape[0]) if a.mem == BMS_DEVICE else (a.rows < x.shape[0])
    if wrong_rows:
        raise ValueError(f"a series of {a.rows} rows on {x.shape[0]} knots")
    out_ptr, out = out_like(a, (xn.shape[0], a.cols), np.complex128)
    rc = getattr(_lib.load(), entry)(ctx.handle, dptr(x), x.shape[0], a.ptr, a.ld, a.cols, a.mem, dptr(xn), xn.shape[0], *order, out_ptr)
    ctx.check(rc, entry)
    return out if a.mem == BMS_DEVICE else out.reshape((xn.shape[0],) + a.tail)


def cubic_spline(x, y, x_new, ctx=None):
    """scipy.interpolate.CubicSpline(x, y)(x_new) for complex y[N, ...] (axis 0 = time).  y may be a device tensor [N, n_cols]
    (complex128, unit column stride): the same launches read it where it is and the result is a new device tensor."""
    return _spline_call("bms_cubic_spline", x, y, x_new, ctx)


def extrapolate(series, radii, orders, ctx=None, device=False, out=None, blocks=0):
    """Constant term of the polynomial fit in 1/r of every mode at every time step, for each order (scri/extrapolation.py:1434:
    numpy.polynomial.polynomial.polyfit(1 / radii[:, t], y[:, t, :], N)[0, :]), on the GPU (bms_extrapolate).

    Host data: `series` holds n_radii arrays c16[n_times, n_modes] (row strides may differ), `radii` is f8[n_radii, n_times].
    device=True: `series` holds n_radii device addresses of contiguous c16[n_times, n_modes], `radii` is (device address of
    f8[n_radii][n_times], n_times, n_modes) and `out` the device address of c16[n_orders][n_times][n_modes].
    orders: 0 <= N < n_radii.  blocks: pipelined blocks of time steps for host data (0: chosen by size).
    Returns (out c16[n_orders, n_times, n_modes], or None with device=True; the number of rank-deficient steps per order, whose
    rows are NaN)."""
    ctx = _ctx(ctx)
    orders_c = np.ascontiguousarray(orders, dtype=np.int32)
    n_r = len(series)
    counts = np.zeros(len(orders_c), dtype=np.int64)
    ptrs = (ctypes.c_void_p * max(n_r, 1))()
    lds = np.zeros(max(n_r, 1), dtype=np.int64)
    if device:
        r_ptr, n_times, n_modes = radii
        for i, p in enumerate(series):
            ptrs[i], lds[i] = int(p), n_modes
        mem, out_ptr, r_arg, keep = BMS_DEVICE, c_vp(int(out)), c_vp(int(r_ptr)), None
    else:
        keep = [np.asarray(s) for s in series]
        for i, s in enumerate(keep):
            if s.dtype != np.complex128 or s.ndim != 2 or s.strides[1] != 16 or s.strides[0] % 16 or s.strides[0] < 16 * s.shape[1]:
                keep[i] = s = np.ascontiguousarray(s, dtype=np.complex128)  # (a row view of stride ld >= n_modes is passed as it is)
            ptrs[i], lds[i] = s.ctypes.data, s.strides[0] // 16
        n_times, n_modes = keep[0].shape if n_r else (0, 0)
        for s in keep:
            if s.shape != (n_times, n_modes):
                raise ValueError(f"every series must have shape ({n_times}, {n_modes}), got {s.shape}")
        r_host = np.ascontiguousarray(radii, dtype=float)
        if r_host.shape != (n_r, n_times):
            raise ValueError(f"radii must have shape ({n_r}, {n_times}), got {r_host.shape}")
        out = np.empty((len(orders_c), n_times, n_modes), dtype=np.complex128)
        mem, out_ptr, r_arg = BMS_HOST, vptr(out), dptr(r_host)
    rc = _lib.load().bms_extrapolate(
        ctx.handle, n_r, ptrs, lds.ctypes.data_as(ctypes.POINTER(c_i64)), mem, int(n_times), int(n_modes), r_arg, len(orders_c),
        orders_c.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), out_ptr, int(blocks), counts.ctypes.data_as(ctypes.POINTER(c_i64)),
    )
    ctx.check(rc, "bms_extrapolate")
    return (None if device else out), counts


def precessing_waveform(t, ell_max, t_merger, mass_ratio, opening_angle, opening_angle_dot, relative_rate, nutation_angle, coef, power,
                        inertial=False, out=None, ctx=None):
    """The modes and the frame of scri's `fake_precessing_waveform` on the time axis t (bms_precessing_waveform): data[N, n_modes],
    l = 2 .. ell_max, in the corotating frame or (inertial) rotated back from it, and the corotating frame [N, 4] (host).
    opening_angle_dot / nutation_angle None: the reference's defaults.  coef, power: the amplitude tables of the modes.  `out`: a device
    tensor [N, >= n_modes] (complex128, unit column stride) that receives the modes, or None for a new host array.  Returns (data, frame)."""
    ctx = _ctx(ctx)
    _on_device_of(ctx, out)
    t = np.ascontiguousarray(t, dtype=float)
    n, n_modes = t.shape[0], LM_total_size(2, ell_max)
    coef = np.ascontiguousarray(coef, dtype=np.complex128)
    power = np.ascontiguousarray(power, dtype=float)
    if coef.shape != (n_modes,) or power.shape != (n_modes,):
        raise ValueError(f"the amplitude tables must hold {n_modes} modes, got {coef.shape} and {power.shape}")
    p = _lib.bms_precessing_params(
        mass_ratio=float(mass_ratio), t_merger=float(t_merger), opening_angle=float(opening_angle),
        opening_angle_dot=0.0 if opening_angle_dot is None else float(opening_angle_dot), relative_rate=float(relative_rate),
        nutation_angle=0.0 if nutation_angle is None else float(nutation_angle), derive_opening_angle_dot=int(opening_angle_dot is None),
        derive_nutation_angle=int(nutation_angle is None), coef=coef.ctypes.data, power=dptr(power))
    if out is None:
        data = np.empty((n, n_modes), dtype=np.complex128)
        ptr, ld, mem = vptr(data), n_modes, BMS_HOST
    else:
        data = out
        if out.shape[0] != n or out.shape[1] < n_modes or (out.shape[1] > 1 and out.stride(1) != 1):
            raise ValueError(f"out of shape {tuple(out.shape)} cannot take {n} rows of {n_modes} modes")
        ptr, ld, mem = c_vp(out.data_ptr()), (out.stride(0) if n > 1 else out.shape[1]), BMS_DEVICE
    frame = np.empty((n, 4))
    rc = _lib.load().bms_precessing_waveform(ctx.handle, dptr(t), n, int(ell_max), ctypes.byref(p), int(bool(inertial)), ptr, ld, mem, dptr(frame))
    ctx.check(rc, "bms_precessing_waveform")
    return data, frame


def radius_terms(t, h0, n_terms, amp, radius, out, ctx=None):
    """out = h0 + |h0| sum_{k=1..n_terms} amp radius^-k exp(i k (50 pi / N) t) (bms_radius_terms): one member of the finite-radius
    family of scri's sample waveforms.  h0 and out: device tensors [N, n_cols] (complex128, unit column stride), or numpy arrays."""
    ctx = _ctx(ctx)
    _on_device_of(ctx, h0, out)
    t = np.ascontiguousarray(t, dtype=float)
    n, n_cols = t.shape[0], int(h0.shape[1])
    if tuple(h0.shape) != (n, n_cols) or tuple(out.shape) != (n, n_cols):
        raise ValueError(f"h0 {tuple(h0.shape)} and out {tuple(out.shape)} must both be ({n}, {n_cols})")
    if _is_device_array(h0) != _is_device_array(out):
        raise ValueError("h0 and out must live in the same memory")
    if _is_device_array(h0):
        args = (c_vp(h0.data_ptr()), h0.stride(0) if n > 1 else n_cols, n_cols, int(n_terms), float(amp), float(radius), c_vp(out.data_ptr()),
                out.stride(0) if n > 1 else n_cols, BMS_DEVICE)
    else:
        h0 = _lib.as_c16(h0)
        if out.dtype != np.complex128 or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous complex128 array")
        args = (vptr(h0), n_cols, n_cols, int(n_terms), float(amp), float(radius), vptr(out), n_cols, BMS_HOST)
    rc = _lib.load().bms_radius_terms(ctx.handle, dptr(t), n, *args)
    ctx.check(rc, "bms_radius_terms")
    return out


def spline_derivative(x, y, x_new, order=0, ctx=None):
    """scipy CubicSpline(x, y, axis=0) differentiated (`order` 1..3) or integrated (`order` -1 .. -16; zero at x[0]) and
    evaluated at x_new, for complex y[N, ...].  y may be a device tensor [N, n_cols] (complex128, unit column stride): the same
    launches read it where it is and the result is a new device tensor."""
    return _spline_call("bms_spline_derivative", x, y, x_new, ctx, int(order))


def grid_multiply(a, spin_a, ell_max_a, b, spin_b, ell_max_b, working_ell_max, output_ell_max, ctx=None):
    """Modes (l_min = 0) of the product of two spin-weighted functions given by their modes a[N, (la+1)^2], b[N, (lb+1)^2]:
    synthesis on the (2W+1)^2 grid, pointwise product, analysis up to output_ell_max."""
    ctx = _ctx(ctx)
    a = _lib.as_c16(a)
    b = _lib.as_c16(b)
    if a.ndim != 2 or b.ndim != 2 or a.shape[0] != b.shape[0]:
        raise ValueError("mode arrays must be [n_times, n_modes] with equal n_times")
    if a.shape[1] != (ell_max_a + 1) ** 2 or b.shape[1] != (ell_max_b + 1) ** 2:
        raise ValueError("mode arrays must start at l = 0 and end at their ell_max")
    out = np.empty((a.shape[0], (output_ell_max + 1) ** 2), dtype=np.complex128)
    rc = _lib.load().bms_grid_multiply(
        ctx.handle, vptr(a), int(spin_a), int(ell_max_a), vptr(b), int(spin_b), int(ell_max_b), BMS_HOST, a.shape[0],
        int(working_ell_max), int(output_ell_max), vptr(out),
    )
    ctx.check(rc, "bms_grid_multiply")
    return out


def mode_map(a, idx_a, coef_a, conj_a=False, b=None, idx_b=None, coef_b=None, conj_b=False, row_scale=None, ctx=None):
    """bms_mode_map on host arrays: out[t, j] = r_t (coef_a[j] op_a(a[t, idx_a[j]]) + coef_b[j] op_b(b[t, idx_b[j]])), op = identity or
    complex conjugation, idx = -1 for a zero term.  a, b complex128 [N, *]; returns complex128 [N, len(idx_a)]."""
    ctx = _ctx(ctx)
    a = _lib.as_c16(a)
    idx_a = np.ascontiguousarray(idx_a, dtype=np.int32)
    coef_a = np.ascontiguousarray(coef_a, dtype=np.complex128)
    n_cols = idx_a.shape[0]
    if coef_a.shape != (n_cols,) or a.ndim != 2:
        raise ValueError("mode_map takes a [N, n] array and tables of one length")
    out = np.empty((a.shape[0], n_cols), dtype=np.complex128)
    i32 = ctypes.POINTER(ctypes.c_int32)
    args_b = (None, 0, None, None, 0)
    if b is not None:
        b = _lib.as_c16(b)
        idx_b = np.ascontiguousarray(idx_b, dtype=np.int32)
        coef_b = np.ascontiguousarray(coef_b, dtype=np.complex128)
        if b.ndim != 2 or b.shape[0] != a.shape[0] or idx_b.shape != (n_cols,) or coef_b.shape != (n_cols,):
            raise ValueError("mode_map: the second operand needs the rows of the first and tables of the same length")
        args_b = (vptr(b), b.shape[1], idx_b.ctypes.data_as(i32), vptr(coef_b), int(bool(conj_b)))
    rs = None
    if row_scale is not None:
        rs = np.ascontiguousarray(row_scale, dtype=float)
        if rs.shape != (a.shape[0],):
            raise ValueError("mode_map: one row factor per row")
    if out.size:
        rc = _lib.load().bms_mode_map(
            ctx.handle, vptr(out), n_cols, a.shape[0], n_cols, vptr(a), a.shape[1], idx_a.ctypes.data_as(i32), vptr(coef_a), int(bool(conj_a)),
            *args_b, vptr(rs) if rs is not None else None, BMS_HOST,
        )
        ctx.check(rc, "bms_mode_map")
    return out


def row_norm(data, take_sqrt=False, ctx=None, device_tensor=None):
    """bms_row_norm: sum over the columns of |data|^2 (its square root with take_sqrt) per row, accumulated in the reference's
    order (scri/waveform_base.py:19-35).  `data` complex128 [N, n] on the host, or `device_tensor` (torch, [N, n], unit column
    stride) for data resident on the GPU; returns a host float array [N]."""
    ctx = _ctx(ctx)
    if device_tensor is not None:
        # (as it always was: the tensor is taken as it is -- its dtype, device and column stride are the caller's business -- and
        # without a record: this call is all wrapper, and those checks cost a microsecond of its 32)
        import torch

        n_rows, n_cols = device_tensor.shape
        out = torch.empty(n_rows, dtype=torch.float64, device=device_tensor.device)
        if n_rows:
            rc = _lib.load().bms_row_norm(ctx.handle, c_vp(device_tensor.data_ptr()), _row_stride(device_tensor, n_rows, n_cols), n_rows, n_cols, BMS_DEVICE,
                                          int(bool(take_sqrt)), c_vp(out.data_ptr()))
            ctx.check(rc, "bms_row_norm")
        return out.cpu().numpy()
    a = _stage(ctx, data, np.complex128, "row_norm takes a [N, n] array: data", shape=(None, None))
    out_ptr, out = out_like(a, (a.rows,), float)
    if a.rows:
        rc = _lib.load().bms_row_norm(ctx.handle, a.ptr, a.ld, a.rows, a.cols, a.mem, int(bool(take_sqrt)), out_ptr)
        ctx.check(rc, "bms_row_norm")
    return out


def polar_tile_rows():
    """rows per tile of the wrap-count scan behind abs_arg(unwrap=True) (bms_polar_tile_rows)"""
    return int(_lib.load().bms_polar_tile_rows())


POLAR_TILE_ROWS = polar_tile_rows()  # the kernel's constant: series lengths around its multiples cross a tile edge

def abs_arg(data, unwrap=False, want=("abs", "arg"), ctx=None):
    """bms_polar: |data| and the angle atan2(im, re) of a complex series data[N, ...] (axis 0 = time), the statements numpy.abs and
    numpy.angle; with unwrap=True the angle is unwrapped along the time axis, the statement numpy.unwrap(numpy.angle(data), axis=0).
    A numpy array in gives numpy arrays out; a device tensor in ([N, n_cols] complex128, unit column stride, any row stride) gives
    float64 device tensors out, so amplitude and phase stay in HBM.  want: the results to compute, in the order they are returned
    (a tuple); one name as a string returns that array alone."""
    ctx = _ctx(ctx)
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= {"abs", "arg"}:
        raise ValueError(f"want names 'abs' and / or 'arg', got {want!r}")
    a = _stage(ctx, data, np.complex128, "a series", flatten=True)
    out = {k: out_like(a, (a.rows, a.cols), float) for k in names}
    if a.rows and a.cols:
        rc = _lib.load().bms_polar(ctx.handle, a.ptr, a.ld, a.rows, a.cols, a.mem, int(bool(unwrap)), out["abs"][0] if "abs" in out else None,
                                   out["arg"][0] if "arg" in out else None, a.cols)
        ctx.check(rc, "bms_polar")
    res = tuple(out[k][1] if a.mem == BMS_DEVICE else out[k][1].reshape((a.rows,) + tuple(a.tail)) for k in names)
    return res[0] if isinstance(want, str) else res


def count_nonfinite(data, ctx=None):
    """bms_count_nonfinite: (the number of elements of the complex series data[N, ...] with a non-finite real or imaginary part, the
    first row that holds one or -1).  data: a numpy array, or a device tensor as abs_arg takes it (it stays where it is)."""
    ctx = _ctx(ctx)
    a = _stage(ctx, data, np.complex128, "a series", flatten=True)
    count, first = c_i64(0), c_i64(-1)
    if a.rows and a.cols:
        rc = _lib.load().bms_count_nonfinite(ctx.handle, a.ptr, a.ld, a.rows, a.cols, a.mem, ctypes.byref(count), ctypes.byref(first))
        ctx.check(rc, "bms_count_nonfinite")
    return int(count.value), int(first.value)


FLUX_NAMES = ("energy", "momentum", "angular", "boost")


def flux_launch_shape(n_modes):
    """(time steps per pass of one workgroup, workgroups at most, whether the coefficient tables sit in LDS) of the fused flux kernel
    for n_modes columns on the current device (bms_flux_launch_shape); None if the range is not supported"""
    shape = (c_i64 * 3)()
    if not _lib.load().bms_flux_launch_shape(int(n_modes), shape):
        return None
    return int(shape[0]), int(shape[1]), bool(shape[2])


def flux_coefficients(ell_min, ell_max):
    """the coefficient tables of the fused flux kernel, f8[30, n_modes] (bms_flux_coefficients: a host routine, no device needed)"""
    out = np.empty((30, LM_total_size(ell_min, ell_max)))
    rc = _lib.load().bms_flux_coefficients(int(ell_min), int(ell_max), dptr(out))
    if rc != 0:
        raise ValueError(f"bms_flux_coefficients: bad ell range [{ell_min}, {ell_max}] (status {rc})")
    return out


def poincare_fluxes(t, h, hdot, ell_min, ell_max, want=FLUX_NAMES, ctx=None):
    """bms_poincare_fluxes: the fluxes named in `want` -- "energy" [N], "momentum", "angular", "boost" [N, 3] -- of the strain h[N, n_modes]
    and its time derivative hdot, l = ell_min .. ell_max, ell_min >= 2, in one launch.  h and hdot are numpy arrays (numpy arrays out) or
    device tensors (complex128, unit column stride, any row stride: float64 device tensors out); h may be None when neither "angular" nor
    "boost" is wanted.  Returns the results in the order of `want` (a tuple); one name as a string returns that array alone."""
    ctx = _ctx(ctx)
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= set(FLUX_NAMES):
        raise ValueError(f"want names {', '.join(repr(k) for k in FLUX_NAMES)}, got {want!r}")
    n_modes = LM_total_size(ell_min, ell_max)
    N = _stage(ctx, hdot, np.complex128, "hdot", shape=(None, n_modes))
    with_h = "angular" in names or "boost" in names
    if with_h and h is None:
        raise ValueError("the angular-momentum and boost fluxes need h")
    H = _stage(ctx, h, np.complex128, "h", shape=(N.rows, n_modes)) if with_h else None
    if H is not None and H.mem != N.mem:
        raise ValueError("h and hdot must live in the same memory")
    t = np.ascontiguousarray(t, dtype=float) if "boost" in names else None
    if t is not None and t.shape != (N.rows,):
        raise ValueError(f"{N.rows} time steps of modes on {t.shape} times")
    out = {k: out_like(N, (N.rows,) if k == "energy" else (N.rows, 3), float) for k in names}
    if N.rows:
        ptr = lambda k: out[k][0] if k in out else None  # noqa: E731
        rc = _lib.load().bms_poincare_fluxes(ctx.handle, dptr(t) if t is not None else None, H.ptr if H is not None else None,
                                             H.ld if H is not None else 0, N.ptr, N.ld, N.rows, int(ell_min), int(ell_max), N.mem,
                                             ptr("energy"), ptr("momentum"), ptr("angular"), ptr("boost"))
        ctx.check(rc, "bms_poincare_fluxes")
    res = tuple(out[k][1] for k in names)
    return res[0] if isinstance(want, str) else res


def expectation_values(a, rows, cols, values, b, conj_a=False, ctx=None):
    """bms_expectation_values: out[t] = sum_e op(a[t, rows[e]]) values[e] b[t, cols[e]], op = conjugation with conj_a, for any triplets
    (the reference's sparse_expectation_value).  a, b: numpy arrays [N, n] (a numpy array out) or device tensors (complex128, unit column
    stride: a device tensor out); rows, cols, values: host arrays of one length."""
    ctx = _ctx(ctx)
    A = _stage(ctx, a, np.complex128, "a", shape=(None, None))
    B = _stage(ctx, b, np.complex128, "b", shape=(A.rows, A.cols))
    if A.mem != B.mem:
        raise ValueError("a and b must live in the same memory")
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    values = np.ascontiguousarray(values, dtype=np.complex128)
    if rows.ndim != 1 or cols.shape != rows.shape or values.shape != rows.shape:
        raise ValueError("rows, cols and values must be one-dimensional and of one length")
    out_ptr, out = out_like(A, (A.rows,), np.complex128)
    if A.rows:
        i32 = ctypes.POINTER(ctypes.c_int32)
        rc = _lib.load().bms_expectation_values(ctx.handle, A.ptr, A.ld, int(bool(conj_a)), B.ptr, B.ld, A.rows, A.cols, rows.ctypes.data_as(i32),
                                                cols.ctypes.data_as(i32), vptr(values), rows.shape[0], A.mem, out_ptr)
        ctx.check(rc, "bms_expectation_values")
    return out


PAIR_NAMES = ("inner", "L", "LL")
_PAIR_WIDTH = {"inner": None, "L": 3, "LL": 9}


def pair_launch_shape(n_modes):
    """(time steps per pass of one workgroup, workgroups at most) of the bracket kernel for n_modes columns on the current device
    (bms_pair_launch_shape); None if a row does not fit in LDS"""
    shape = (c_i64 * 3)()
    if not _lib.load().bms_pair_launch_shape(int(n_modes), shape):
        return None
    return int(shape[0]), int(shape[1])


def pair_brackets(a, b, ell_min, ell_max, ell_min_a=None, ell_min_b=None, want=PAIR_NAMES, ctx=None):
    """bms_pair_brackets: the brackets named in `want` of the modes a and b on the common range l = ell_min .. ell_max, per time step and
    in the (+, -, z) basis, in one launch -- "inner" [N]: sum conj(a) b; "L" [N, 3]: <a|L_a|b>, a = +, -, z; "LL" [N, 9]: <a|L_a L_b|b>,
    ab = pp, pm, mp, mm, pz, zp, mz, zm, zz.  a and b are numpy arrays (numpy arrays out) or device tensors (complex128, unit column
    stride, any row stride: device tensors out), both in the same memory; their rows start at l = ell_min_a and ell_min_b (default:
    ell_min) and may go on beyond ell_max: the common range is read where it lies.  Returns the results in the order of `want` (a
    tuple); one name as a string returns that array alone."""
    ctx = _ctx(ctx)
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= set(PAIR_NAMES):
        raise ValueError(f"want names {', '.join(repr(k) for k in PAIR_NAMES)}, got {want!r}")
    ell_min_a = ell_min if ell_min_a is None else ell_min_a
    ell_min_b = ell_min if ell_min_b is None else ell_min_b
    A = _stage(ctx, a, np.complex128, "a", shape=(None, None))
    B = _stage(ctx, b, np.complex128, "b", shape=(A.rows, None))
    if A.mem != B.mem:
        raise ValueError("a and b must live in the same memory")
    if 0 <= ell_min_a <= ell_min <= ell_max and 0 <= ell_min_b <= ell_min:  # (any other range: the entry refuses it)
        for x, first, name in ((A, ell_min_a, "a"), (B, ell_min_b, "b")):
            if x.cols < (ell_max + 1) ** 2 - first**2:
                raise ValueError(f"{name} has {x.cols} columns: rows from l = {first} to {ell_max} hold {(ell_max + 1) ** 2 - first**2}")
    out = {k: out_like(A, (A.rows,) if _PAIR_WIDTH[k] is None else (A.rows, _PAIR_WIDTH[k]), np.complex128) for k in names}
    if A.rows:
        ptr = lambda k: out[k][0] if k in out else None  # noqa: E731
        rc = _lib.load().bms_pair_brackets(ctx.handle, A.ptr, A.ld, int(ell_min_a), B.ptr, B.ld, int(ell_min_b), A.rows, int(ell_min), int(ell_max),
                                           A.mem, ptr("inner"), ptr("L"), ptr("LL"))
        ctx.check(rc, "bms_pair_brackets")
    res = tuple(out[k][1] for k in names)
    return res[0] if isinstance(want, str) else res


CHARGE_NAMES = ("four_momentum", "angular", "boost", "com")


def charge_launch_shape(n_modes):
    """(time steps per pass of one workgroup, workgroups at most, whether the coefficient tables sit in LDS) of the Bondi-charge kernel for
    n_modes = (ell_max + 1)^2 columns on the current device (bms_charge_launch_shape); None if the rows do not fit in LDS"""
    shape = (c_i64 * 3)()
    if not _lib.load().bms_charge_launch_shape(int(n_modes), shape):
        return None
    return int(shape[0]), int(shape[1]), bool(shape[2])


def charge_coefficients(ell_max):
    """the coefficient tables of the Bondi-charge kernel, f8[20, (ell_max + 1)^2] (bms_charge_coefficients: a host routine, no device needed)"""
    if ell_max < 2:
        raise ValueError(f"bms_charge_coefficients: ell_max = {ell_max} is below 2")
    out = np.empty((20, (int(ell_max) + 1) ** 2))
    rc = _lib.load().bms_charge_coefficients(int(ell_max), dptr(out))
    if rc != 0:
        raise ValueError(f"bms_charge_coefficients: bad ell_max = {ell_max} (status {rc})")
    return out


def bondi_charges(t, psi1, psi2, sigma, sigma_dot, ell_max, want=CHARGE_NAMES, ctx=None):
    """bms_bondi_charges: the charges named in `want` -- "four_momentum" [N, 4], "angular", "boost", "com" [N, 3] -- of the fields psi1,
    psi2, sigma and sigma_dot = d sigma / dt, each [N, (ell_max + 1)^2] from l = 0 as AsymptoticBondiData stores them, in one launch.  The
    fields are numpy arrays (numpy arrays out) or device tensors (complex128, unit column stride, any row stride: float64 device tensors
    out), all in one memory.  sigma_dot and psi2 may be None when neither "four_momentum" nor "boost" is wanted, psi1 when "four_momentum"
    alone is, t when "boost" is not.  Returns the results in the order of `want` (a tuple); one name as a string returns that array alone."""
    ctx = _ctx(ctx)
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= set(CHARGE_NAMES):
        raise ValueError(f"want names {', '.join(repr(k) for k in CHARGE_NAMES)}, got {want!r}")
    n_modes = (int(ell_max) + 1) ** 2
    S = _stage(ctx, sigma, np.complex128, "sigma", shape=(None, n_modes))
    with_dot = "four_momentum" in names or "boost" in names
    with_psi1 = names != ("four_momentum",)
    needed = (("sigma_dot", sigma_dot, with_dot), ("psi2", psi2, with_dot), ("psi1", psi1, with_psi1))
    for name, x, need in needed:
        if need and x is None:
            raise ValueError(f"the charges asked for ({', '.join(names)}) need {name}")
    staged = {name: _stage(ctx, x, np.complex128, name, shape=(S.rows, n_modes)) if need else None for name, x, need in needed}
    if any(x is not None and x.mem != S.mem for x in staged.values()):
        raise ValueError("psi1, psi2, sigma and sigma_dot must live in the same memory")
    t = np.ascontiguousarray(t, dtype=float) if "boost" in names else None
    if t is not None and t.shape != (S.rows,):
        raise ValueError(f"{S.rows} time steps of modes on {t.shape} times")
    out = {k: out_like(S, (S.rows, 4 if k == "four_momentum" else 3), float) for k in names}
    if S.rows:
        ptr = lambda k: out[k][0] if k in out else None  # noqa: E731
        arg = lambda x: (x.ptr, x.ld) if x is not None else (None, 0)  # noqa: E731
        rc = _lib.load().bms_bondi_charges(ctx.handle, dptr(t) if t is not None else None, *arg(staged["psi1"]), *arg(staged["psi2"]), S.ptr, S.ld,
                                           *arg(staged["sigma_dot"]), S.rows, int(ell_max), S.mem, ptr("four_momentum"), ptr("angular"),
                                           ptr("boost"), ptr("com"))
        ctx.check(rc, "bms_bondi_charges")
    res = tuple(out[k][1] for k in names)
    return res[0] if isinstance(want, str) else res


SUPERMOMENTA_NAMES = ("bondi_sachs", "moreschi", "geroch", "geroch_winicour", "mass_aspect")


def product_nodes(ell_max_a, ell_max_b, ell_max_out):
    """the Gauss-Legendre rows on which the product truncated at ell_max_out is exact: floor((l_a + l_b + l_out) / 2) + 1"""
    return (int(ell_max_a) + int(ell_max_b) + int(ell_max_out)) // 2 + 1


def product_launch_shape(ell_max_a, ell_max_b, ell_max_out):
    """(time steps per pass of one workgroup, workgroups at most, whether the tables sit in LDS) of the product kernel on the current
    device (bms_product_launch_shape); None if the rows and panels of one time step do not fit in LDS"""
    shape = (c_i64 * 3)()
    if not _lib.load().bms_product_launch_shape(int(ell_max_a), int(ell_max_b), int(ell_max_out), shape):
        return None
    return int(shape[0]), int(shape[1]), bool(shape[2])


def product_tables(spin, ell_max, n_nodes):
    """(cos_theta f8[n], weights f8[n], table f8[n, (ell_max + 1)^2]): the Gauss-Legendre rule of n_nodes points and sYlm(theta_j, 0) of
    `spin` as the product kernel reads it (bms_product_tables: a host routine, no device needed)"""
    x, w, table = np.empty(int(n_nodes)), np.empty(int(n_nodes)), np.empty((int(n_nodes), (int(ell_max) + 1) ** 2))
    rc = _lib.load().bms_product_tables(int(spin), int(ell_max), int(n_nodes), dptr(x), dptr(w), dptr(table))
    if rc != 0:
        raise ValueError(f"bms_product_tables: bad spin = {spin}, ell_max = {ell_max} or n_nodes = {n_nodes} (status {rc})")
    return x, w, table


def mode_product(a, spin_a, ell_max_a, b, spin_b, ell_max_b, ell_max_out, conj_a=False, conj_b=False, ctx=None):
    """bms_mode_product: the modes l = 0 .. ell_max_out of op(a) op(b) for a [N, (ell_max_a + 1)^2] and b [N, (ell_max_b + 1)^2] from l = 0,
    spin_* the spin of the stored rows, op = bar where conj_* is set (an operand of spin -spin_*): exact for ell_max_out <= ell_max_a +
    ell_max_b, on Gauss-Legendre rows, with no grid.  numpy arrays (a numpy array out) or device tensors (complex128, unit column stride,
    any row stride: a device tensor out), both in one memory; a and b may be the same array."""
    ctx = _ctx(ctx)
    A = _stage(ctx, a, np.complex128, "a", shape=(None, (int(ell_max_a) + 1) ** 2))
    B = _stage(ctx, b, np.complex128, "b", shape=(A.rows, (int(ell_max_b) + 1) ** 2))
    if A.mem != B.mem:
        raise ValueError("a and b must live in the same memory")
    if ell_max_out < 0:
        raise ValueError(f"ell_max_out = {ell_max_out} is negative")
    n_out = (int(ell_max_out) + 1) ** 2
    ptr, out = out_like(A, (A.rows, n_out), np.complex128)
    if A.rows:
        rc = _lib.load().bms_mode_product(ctx.handle, A.ptr, A.ld, int(spin_a), int(ell_max_a), int(bool(conj_a)), B.ptr, B.ld, int(spin_b), int(ell_max_b),
                                          int(bool(conj_b)), A.rows, int(ell_max_out), A.mem, ptr, n_out)
        ctx.check(rc, "bms_mode_product")
    return out


def supermomenta(psi2, sigma, sigma_dot, ell_max, ell_max_out=None, want=SUPERMOMENTA_NAMES, integrated=False, ctx=None):
    """bms_supermomenta: the fields named in `want` -- "bondi_sachs", "moreschi", "geroch", "geroch_winicour" (written as -bar / (2 sqrt(pi))
    with integrated=True) and "mass_aspect" (never altered) -- each [N, (ell_max_out + 1)^2] from l = 0, of psi2, sigma and sigma_dot =
    d sigma / dt, each [N, (ell_max + 1)^2] from l = 0 as AsymptoticBondiData stores them, in one launch; ell_max_out <= ell_max (default:
    ell_max).  The fields are numpy arrays (numpy arrays out) or device tensors (complex128, unit column stride, any row stride: device
    tensors out), all in one memory.  Returns the results in the order of `want` (a tuple); one name as a string returns that array alone."""
    ctx = _ctx(ctx)
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= set(SUPERMOMENTA_NAMES):
        raise ValueError(f"want names {', '.join(repr(k) for k in SUPERMOMENTA_NAMES)}, got {want!r}")
    ell_max = int(ell_max)
    ell_max_out = ell_max if ell_max_out is None else int(ell_max_out)
    if not 0 <= ell_max_out <= ell_max:
        raise ValueError(f"ell_max_out = {ell_max_out} is outside 0 .. ell_max = {ell_max}")
    n_modes, n_out = (ell_max + 1) ** 2, (ell_max_out + 1) ** 2
    S = _stage(ctx, sigma, np.complex128, "sigma", shape=(None, n_modes))
    D = _stage(ctx, sigma_dot, np.complex128, "sigma_dot", shape=(S.rows, n_modes))
    P = _stage(ctx, psi2, np.complex128, "psi2", shape=(S.rows, None))
    if P.cols < n_out:
        raise ValueError(f"psi2 has {P.cols} columns, fewer than the (ell_max_out + 1)^2 = {n_out} read")
    if D.mem != S.mem or P.mem != S.mem:
        raise ValueError("psi2, sigma and sigma_dot must live in the same memory")
    out = {k: out_like(S, (S.rows, n_out), np.complex128) for k in names}
    if S.rows:
        ptr = lambda k: out[k][0] if k in out else None  # noqa: E731
        rc = _lib.load().bms_supermomenta(ctx.handle, P.ptr, P.ld, S.ptr, S.ld, D.ptr, D.ld, S.rows, ell_max, ell_max_out, S.mem, int(bool(integrated)),
                                          *(ptr(k) for k in SUPERMOMENTA_NAMES), n_out)
        ctx.check(rc, "bms_supermomenta")
    res = tuple(out[k][1] for k in names)
    return res[0] if isinstance(want, str) else res


# the inputs each violation of bms_bondi_constraints reads, as indices into (psi0 .. psi4, sigma, psi0_dot, psi1_dot, psi2_dot, sigma_dot, sigma_ddot)
_CONSTRAINT_READS = ((1, 2, 5, 6), (2, 3, 5, 7), (3, 4, 5, 8), (3, 9), (4, 10), (2, 5, 9))
_CONSTRAINT_INPUTS = ("psi0", "psi1", "psi2", "psi3", "psi4", "sigma", "psi0_dot", "psi1_dot", "psi2_dot", "sigma_dot", "sigma_ddot")


def bondi_constraints(fields, psi_dot, sigma_dot, sigma_ddot, ell_max, want=(0, 1, 2, 3, 4, 5), norms=True, ctx=None):
    """bms_bondi_constraints: the violations of the six Bondi-gauge relations named in `want` (0 .. 5: the three Bianchi identities, psi3,
    psi4 and the imaginary part of the mass aspect; scri/asymptotic_bondi_data/constraints.py) and, with norms=True, the L2 norms of all
    six, in one launch.  fields: psi0 .. psi4, sigma (six arrays or one [6, N, (ell_max + 1)^2]); psi_dot: d/du of psi0, psi1, psi2;
    sigma_dot, sigma_ddot: the first and second derivative of sigma; each [N, (ell_max + 1)^2] from l = 0, numpy arrays or device
    tensors (complex128, unit column stride, any row stride), all in one memory.  An input that nothing asked for reads may be None
    (psi0 never is read).  Returns (violations, norms): a tuple in the order of `want` -- numpy arrays, or device tensors for device
    inputs -- and a host array [N, 6] (None with norms=False)."""
    ctx = _ctx(ctx)
    want = tuple(int(k) for k in want)
    if len(set(want)) != len(want) or not set(want) <= set(range(6)):
        raise ValueError(f"want names violations 0 .. 5, each once; got {want!r}")
    if not want and not norms:
        raise ValueError("neither a violation nor the norms are asked for")
    ell_max = int(ell_max)
    n_modes = (ell_max + 1) ** 2
    given = list(fields) + list(psi_dot) + [sigma_dot, sigma_ddot]
    if len(given) != 11:
        raise ValueError("fields holds psi0 .. psi4 and sigma, psi_dot the derivatives of psi0, psi1, psi2")
    read = set(range(1, 11)) if norms else {i for k in want for i in _CONSTRAINT_READS[k]}
    staged, first = [None] * 11, None
    for i in sorted(read):
        if given[i] is None:
            raise ValueError(f"the outputs asked for need {_CONSTRAINT_INPUTS[i]}")
        staged[i] = _stage(ctx, given[i], np.complex128, _CONSTRAINT_INPUTS[i], shape=(None if first is None else first.rows, n_modes))
        first = first if first is not None else staged[i]
        if staged[i].mem != first.mem:
            raise ValueError("the fields and their derivatives must live in the same memory")
    out = {k: out_like(first, (first.rows, n_modes), np.complex128) for k in want}
    norm_ptr, norm_out = out_like(first, (first.rows, 6), float) if norms else (None, None)
    if first.rows:
        ptrs = lambda idx: (c_vp * len(idx))(*(staged[i].ptr if staged[i] is not None else None for i in idx))  # noqa: E731
        lds = lambda idx: (c_i64 * len(idx))(*(staged[i].ld if staged[i] is not None else 0 for i in idx))  # noqa: E731
        dot = lambda i: (staged[i].ptr, staged[i].ld) if staged[i] is not None else (None, 0)  # noqa: E731
        homes = (c_vp * 6)(*(out[k][0] if k in out else None for k in range(6)))
        rc = _lib.load().bms_bondi_constraints(ctx.handle, ptrs(range(6)), lds(range(6)), ptrs(range(6, 9)), lds(range(6, 9)), *dot(9), *dot(10),
                                               first.rows, ell_max, first.mem, homes, n_modes, norm_ptr)
        ctx.check(rc, "bms_bondi_constraints")
    if norms and first.mem == BMS_DEVICE:
        norm_out = norm_out.cpu().numpy()
    return tuple(out[k][1] for k in want), norm_out


def _rows_out(arg, out, n_modes, what):
    """(address, row stride) of the device tensor `out` [arg.rows, n_modes] (complex128, unit column stride, any row stride) that a
    device call writes in place"""
    if arg.mem != BMS_DEVICE:
        raise ValueError("out= names device arrays; with host inputs the results are new host arrays")
    if (not _is_device_array(out) or out.dtype != _torch_dtype(np.complex128) or out.device != arg.device or tuple(out.shape) != (arg.rows, n_modes)
            or (n_modes > 1 and out.stride(1) != 1)):
        raise ValueError(f"{what}: expected a complex128 device array ({arg.rows}, {n_modes}) with unit column stride on {arg.device}")
    return c_vp(out.data_ptr()), _row_stride(out, arg.rows, n_modes)


def bianchi_rhs(k, sigma, a, b, ell_max, ctx=None, out=None):
    """bms_bianchi_rhs: one stage of the Bianchi identities run forwards, rhs = eth a + (3 - k) sigma b with the GHP eth and the product
    truncated at ell_max, every array [N, (ell_max + 1)^2] from l = 0.  k = 1: a = psi2, b = psi3; k = 0: a = psi1, b = psi2; k = 2 (the
    head): a = sigma_dot, b = sigma_ddot as stored, and psi4 = -bar(b), psi3 = -eth bar(a), rhs = eth psi3 + sigma psi4.  numpy arrays
    (numpy arrays out) or device tensors (complex128, unit column stride, any row stride: device tensors out), all in one memory.
    out: the device tensor the result is written into, (rhs, psi3, psi4) of them at k = 2 -- row views of wider tensors are written through
    their row stride.  Returns rhs, or (rhs, psi3, psi4) at k = 2."""
    ctx = _ctx(ctx)
    k, ell_max = int(k), int(ell_max)
    n_modes = (ell_max + 1) ** 2
    S = _stage(ctx, sigma, np.complex128, "sigma", shape=(None, n_modes))
    A = _stage(ctx, a, np.complex128, "a", shape=(S.rows, n_modes))
    B = _stage(ctx, b, np.complex128, "b", shape=(S.rows, n_modes))
    if A.mem != S.mem or B.mem != S.mem:
        raise ValueError("sigma, a and b must live in the same memory")
    n_out = 3 if k == 2 else 1
    if out is None:
        made = [out_like(S, (S.rows, n_modes), np.complex128) for _ in range(n_out)]
        ptrs, lds, res = [p for p, _ in made], [n_modes] * n_out, [o for _, o in made]
    else:
        res = list(out) if isinstance(out, (tuple, list)) else [out]
        if len(res) != n_out:
            raise ValueError(f"out names {len(res)} arrays; stage k = {k} writes {n_out}")
        homes = [_rows_out(S, o, n_modes, name) for o, name in zip(res, ("rhs", "psi3", "psi4"))]
        ptrs, lds = [p for p, _ in homes], [ld for _, ld in homes]
        if n_out == 3 and lds[1] != lds[2]:
            raise ValueError("psi3 and psi4 share one row stride")
    if S.rows:
        psi = (ptrs[1], ptrs[2], lds[1]) if n_out == 3 else (None, None, 0)
        rc = _lib.load().bms_bianchi_rhs(ctx.handle, k, S.ptr, S.ld, A.ptr, A.ld, B.ptr, B.ld, S.rows, ell_max, S.mem, ptrs[0], lds[0], *psi)
        ctx.check(rc, "bms_bianchi_rhs")
    return tuple(res) if n_out == 3 else res[0]


CUT_NAMES = ("modes", "psi", "k")


def supermomentum_on_cut(t, psi, alpha, ell_max, want=("modes",), ctx=None):
    """bms_supermomentum_on_cut: the series psi [N, (ell_max + 1)^2] of spin-0 modes from l = 0 on the times t, evaluated on the cut
    u = alpha, a real [2 ell_max + 1, 2 ell_max + 1] function on the equiangular grid.  want names "psi" (the real part of the series at
    every pixel's own time, by not-a-knot cubic splines through the rows within 64 knots of alpha's range), "k" (the conformal factor of the
    series' four-momentum there) and "modes" (the Moreschi supermomentum of the cut, map_to_superrest_frame.py:155-197).  psi is a numpy
    array or a device tensor (complex128, unit column stride, any row stride: read where it is); the results are host arrays, in the
    order of `want` (a tuple); one name as a string returns that array alone.  NotImplementedError: ell_max outside 2 .. 24, fewer than 4
    rows, or a window too long for the kernel's LDS."""
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names or len(set(names)) != len(names) or not set(names) <= set(CUT_NAMES):
        raise ValueError(f"want names {', '.join(repr(k) for k in CUT_NAMES)}, got {want!r}")
    ell_max = int(ell_max)
    n_modes, n = (ell_max + 1) ** 2, 2 * ell_max + 1
    t = np.ascontiguousarray(t, dtype=float)
    if len(psi.shape) != 2 or psi.shape[1] != n_modes:
        raise ValueError(f"psi must hold the (ell_max + 1)^2 = {n_modes} modes from l = 0 to ell_max = {ell_max} in every row; it has shape {tuple(psi.shape)}")
    if t.shape != (psi.shape[0],):
        raise ValueError(f"{psi.shape[0]} rows of modes on {t.shape} times")
    alpha = np.ascontiguousarray(alpha, dtype=float)
    if alpha.shape != (n, n):
        raise ValueError(f"alpha must have shape ({n}, {n}); it has shape {alpha.shape}")
    ctx = _ctx(ctx)
    a = _stage(ctx, psi, np.complex128, "psi", shape=(t.shape[0], n_modes))
    out = {"modes": np.empty(n_modes, dtype=np.complex128), "psi": np.empty((n, n)), "k": np.empty((n, n))}
    ptr = lambda k, f: f(out[k]) if k in names else None  # noqa: E731
    rc = _lib.load().bms_supermomentum_on_cut(ctx.handle, dptr(t), t.shape[0], a.ptr, a.ld, a.mem, ell_max, dptr(alpha), ptr("modes", vptr),
                                              ptr("psi", dptr), ptr("k", dptr))
    ctx.check(rc, "bms_supermomentum_on_cut")
    res = tuple(out[k] for k in names)
    return res[0] if isinstance(want, str) else res


def alpha_perturbation(psi_modes, ell_max, m_grid=None, k_grid=None, ctx=None):
    """bms_alpha_perturbation: Re salm2map(D^-1 map2salm(salm2map(psi_modes) + M K^3)) on the [2 ell_max + 1, 2 ell_max + 1] grid for one row
    psi_modes [(ell_max + 1)^2] from l = 0 (map_to_superrest_frame.py:200-224).  m_grid, k_grid: real grids, or None: the rest mass / the
    conformal factor of psi_modes' own four-momentum.  NotImplementedError: ell_max outside 2 .. 24."""
    ell_max = int(ell_max)
    n_modes, n = (ell_max + 1) ** 2, 2 * ell_max + 1
    psi_modes = np.ascontiguousarray(psi_modes, dtype=np.complex128)
    if psi_modes.shape != (n_modes,):
        raise ValueError(f"psi_modes must hold the (ell_max + 1)^2 = {n_modes} modes from l = 0 to ell_max = {ell_max}; it has shape {psi_modes.shape}")
    grids = []
    for name, g in (("m_grid", m_grid), ("k_grid", k_grid)):
        g = None if g is None else np.ascontiguousarray(g, dtype=float)
        if g is not None and g.shape != (n, n):
            raise ValueError(f"{name} must have shape ({n}, {n}); it has shape {g.shape}")
        grids.append(g)
    ctx = _ctx(ctx)
    out = np.empty((n, n))
    rc = _lib.load().bms_alpha_perturbation(ctx.handle, vptr(psi_modes), ell_max, *(dptr(g) if g is not None else None for g in grids), dptr(out))
    ctx.check(rc, "bms_alpha_perturbation")
    return out


PRODUCT_COMPLEX, PRODUCT_REAL, PRODUCT_COMPLEX_4M = 0, 1, 2


def dense_product(form, a_ptr, lda, b_ptr, ldb, c_ptr, ldc, M, N, K, col_off_ptr=None, col_scale_ptr=None, ctx=None):
    """bms_dense_product: C[M x N] = (A[M x K] . B[K x N] - col_off) * col_scale on the matrix-core kernels.  Every operand is a device
    ADDRESS (int) of the caller's, pitches in doubles; include/scri_amd.h says what is read, written and refused.  Stream-ordered on
    the context's stream: ctx.synchronize() is the host-side wait."""
    ctx = _ctx(ctx)
    rc = _lib.load().bms_dense_product(ctx.handle, int(form), c_vp(a_ptr), int(lda), c_vp(b_ptr), int(ldb), c_vp(c_ptr), int(ldc), int(M),
                                       int(N), int(K), c_vp(col_off_ptr), c_vp(col_scale_ptr))
    ctx.check(rc, "bms_dense_product")


def _modes_arg(ctx, data, n, ell_min, ell_max):
    """the _Arg of modes [n, n_modes]: a numpy array on the host, or a torch tensor (unit column stride) for modes resident on the GPU
    (as it always was: neither a tensor's dtype is checked nor the context moved to torch's stream)"""
    return _stage(ctx, data, np.complex128, f"modes of {n} time steps and ell range [{ell_min}, {ell_max}]", shape=(n, LM_total_size(ell_min, ell_max)),
                  check_dtype=False, attach=False)


def angular_velocity(t, data, ell_min, ell_max, ctx=None, parts=False):
    """omega[N, 3] = -<LL>^-1 <Ldt> of modes data[N, n_modes] (numpy, or a device tensor: the modes then stay where they are);
    parts=True returns (<Ldt>[N, 3], <LL>[N, 3, 3], omega).  The results are host arrays."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    a = _modes_arg(ctx, data, n, ell_min, ell_max)
    ldt = np.empty((n, 3))
    ll = np.empty((n, 3, 3))
    om = np.empty((n, 3))
    rc = _lib.load().bms_angular_velocity(ctx.handle, dptr(t), n, a.ptr, a.ld, int(ell_min), int(ell_max), a.mem, dptr(ldt), dptr(ll), dptr(om))
    ctx.check(rc, "bms_angular_velocity")
    return (ldt, ll, om) if parts else om


# ---- the frame chain on the device (bms_frame_from_angular_velocity ... bms_coprecessing_frame).  Per-step arrays are numpy arrays on
# the host or torch tensors (float64, contiguous) on the device; a result lives where its input does.


def _step_arg(ctx, x, n, width, what):
    """the _Arg of a per-step array f8[n][width]: a numpy array, or a contiguous float64 device tensor of n * width values (as it
    always was, the context is not moved to torch's stream)"""
    return _stage(ctx, x, float, what, shape=(n, width), contiguous=True, attach=False)


def frame_from_angular_velocity(t, omega, R0=(1.0, 0.0, 0.0, 0.0), tolerance=1e-12, ctx=None, out=None):
    """R[N, 4] with R[0] = R0 and dR/dt = (1/2) Omega R for the cubic spline Omega through omega[N, 3], on the GPU: interval rotors
    and their prefix product.  `out` (device input only): the device tensor [N, 4] the frame is written to."""
    ctx = _ctx(ctx)
    _on_device_of(ctx, out)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    om = _step_arg(ctx, omega, n, 3, "omega")
    R0 = np.ascontiguousarray(R0, dtype=float).reshape(4)
    out_ptr, out = out_like(om, (n, 4), float, out)
    rc = _lib.load().bms_frame_from_angular_velocity(ctx.handle, dptr(t), n, om.ptr, om.mem, dptr(R0), float(tolerance), out_ptr)
    ctx.check(rc, "bms_frame_from_angular_velocity")
    return out


def dominant_axis(ll, rough=(0.0, 0.0, 1.0), rough_index=0, ctx=None):
    """Continuous unit principal axis [N, 3] of the symmetric matrices ll[N, 3, 3] (bms_dominant_axis)."""
    ctx = _ctx(ctx)
    n = int(ll.shape[0])
    a = _step_arg(ctx, ll.reshape(n, 9), n, 9, "ll")
    rough = np.ascontiguousarray(rough, dtype=float).reshape(3)
    out_ptr, out = out_like(a, (n, 3), float)
    rc = _lib.load().bms_dominant_axis(ctx.handle, a.ptr, n, a.mem, dptr(rough), int(rough_index), out_ptr)
    ctx.check(rc, "bms_dominant_axis")
    return out


def _rotor_series_call(entry, t, R, width, ctx, *args):
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    a = _step_arg(ctx, R, n, 4, "R")
    out_ptr, out = out_like(a, (n, width), float)
    rc = getattr(_lib.load(), entry)(ctx.handle, dptr(t), n, a.ptr, a.mem, *args, out_ptr)
    ctx.check(rc, entry)
    return out


def minimal_rotation(t, R, iterations=2, ctx=None):
    """numpy-quaternion's minimal_rotation of the rotor series R[N, 4] (bms_minimal_rotation); a new array beside R."""
    return _rotor_series_call("bms_minimal_rotation", t, R, 4, ctx, int(iterations))


def rotor_angular_velocity(t, R, ctx=None):
    """omega[N, 3] = vector part of 2 Rdot R^-1 of the rotor series R[N, 4] (bms_rotor_angular_velocity)."""
    return _rotor_series_call("bms_rotor_angular_velocity", t, R, 3, ctx)


def squad(R_in, t_in, t_out, ctx=None, out=None):
    """quaternion.squad of the rotors R_in[n, 4] at the times t_in[n] evaluated at t_out[m] (any order), on the GPU (bms_squad):
    `scri_amd.quaternions.squad` is the statement.  R_in: a numpy array, or a device tensor (float64, contiguous); the result [m, 4]
    lives where R_in does (`out`, device input only: the device tensor it is written to).  No rotors, no arguments or one rotor
    answer as the statement does, without a launch."""
    ctx = _ctx(ctx)
    _on_device_of(ctx, R_in, out)
    t_in = np.ascontiguousarray(t_in, dtype=float)
    t_out = np.ascontiguousarray(t_out, dtype=float).reshape(-1)
    on_device = _is_device_array(R_in)
    if not on_device:
        R_in = np.asarray(R_in, dtype=float)
    size = R_in.numel() if on_device else R_in.size
    n, m = (int(R_in.shape[0]) if size else 0), t_out.shape[0]
    if n < 2 or m == 0:  # the statement's answers: nothing from nothing, one rotor repeated
        rows = 0 if n == 0 or m == 0 else m
        _, res = out_like(_beside(R_in), (rows, 4), float, out)
        if rows:
            res.reshape(rows, 4)[:] = R_in.reshape(-1, 4)[:1]
        return res
    if t_in.shape != (n,):
        raise ValueError(f"t_in must have shape ({n},); it has shape {t_in.shape}")
    a = _step_arg(ctx, R_in, n, 4, "R_in")
    out_ptr, out = out_like(a, (m, 4), float, out)
    rc = _lib.load().bms_squad(ctx.handle, dptr(t_in), n, a.ptr, a.mem, dptr(t_out), m, out_ptr)
    ctx.check(rc, "bms_squad")
    return out


def frame_scan_blocks(n):
    """blocks the scans of the frame chain cut a series of n steps into (bms_frame_scan_blocks)"""
    return int(_lib.load().bms_frame_scan_blocks(int(n)))


def frame_adjust(frame, right=None, truncate_tolerance=0.0, want_log=False, want_spinors=False, ctx=None):
    """In place on frame[N, 4] (bms_frame_adjust): times the constant rotor `right`, normalised, optionally exp of its logarithm rounded
    to the bits above truncate_tolerance.  Returns (rounded log-frame or None, spinors [N, 4 doubles] = (w + i z, y + i x) or None),
    beside the frame."""
    ctx = _ctx(ctx)
    n = int(frame.shape[0])
    if not _is_device_array(frame) and not (isinstance(frame, np.ndarray) and frame.dtype == float and frame.flags.c_contiguous):
        raise ValueError("frame_adjust works in place: a contiguous float array or a device tensor")
    a = _step_arg(ctx, frame, n, 4, "frame")
    log_ptr, log = out_like(a, (n, 4), float) if want_log else (None, None)
    sp_ptr, sp = out_like(a, (n, 4), float) if want_spinors else (None, None)
    rt = None if right is None else np.ascontiguousarray(right, dtype=float).reshape(4)
    rc = _lib.load().bms_frame_adjust(ctx.handle, a.ptr, n, a.mem, None if rt is None else dptr(rt), float(truncate_tolerance), log_ptr, sp_ptr)
    ctx.check(rc, "bms_frame_adjust")
    return log, sp


def corotating_frame(t, data, ell_min, ell_max, frame_dev, R0=(1.0, 0.0, 0.0, 0.0), tolerance=1e-12, want_frame=False, want_omega=False, ctx=None):
    """bms_corotating_frame: the corotating frame of modes data[N, n_modes] (numpy or device tensor) into the device tensor frame_dev
    [N, 4]; returns (host copy of the frame or None, host omega [N, 3] or None)."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    a = _modes_arg(ctx, data, n, ell_min, ell_max)
    f = _step_arg(ctx, frame_dev, n, 4, "frame_dev")
    R0 = np.ascontiguousarray(R0, dtype=float).reshape(4)
    frame = np.empty((n, 4)) if want_frame else None
    om = np.empty((n, 3)) if want_omega else None
    rc = _lib.load().bms_corotating_frame(ctx.handle, dptr(t), n, a.ptr, a.ld, int(ell_min), int(ell_max), a.mem, dptr(R0), float(tolerance), f.ptr,
                                          None if frame is None else dptr(frame), None if om is None else dptr(om))
    ctx.check(rc, "bms_corotating_frame")
    return frame, om


def coprecessing_frame(t, data, ell_min, ell_max, rough=(0.0, 0.0, 1.0), rough_index=0, iterations=3, frame_dev=None, want_frame=False,
                       want_axis=False, ctx=None):
    """bms_coprecessing_frame: dominant axis of <LL> of modes data[N, n_modes] (numpy or device tensor), and with frame_dev (device
    tensor [N, 4]) or want_frame the minimally rotating frame that takes z to it; returns (host frame or None, host axis [N, 3] or None)."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    a = _modes_arg(ctx, data, n, ell_min, ell_max)
    f_ptr = None if frame_dev is None else _step_arg(ctx, frame_dev, n, 4, "frame_dev").ptr
    rough = np.ascontiguousarray(rough, dtype=float).reshape(3)
    frame = np.empty((n, 4)) if want_frame else None
    axis = np.empty((n, 3)) if want_axis else None
    rc = _lib.load().bms_coprecessing_frame(ctx.handle, dptr(t), n, a.ptr, a.ld, int(ell_min), int(ell_max), a.mem, dptr(rough), int(rough_index),
                                            int(iterations), f_ptr, None if frame is None else dptr(frame), None if axis is None else dptr(axis))
    ctx.check(rc, "bms_coprecessing_frame")
    return frame, axis


# ---- time-and-phase alignment from correlation moments (bms_align_moments, bms_align_residual; scri_amd/alignment.py)


def _align_bulk(ctx, x, what):
    """(address, row stride, the tensor) of a bulk array c16[n][ld]: a device tensor goes through untouched, a host array goes up once"""
    from . import device_series

    if not _is_device_array(x):
        x = device_series.to_device(ctx, x)
    a = _stage(ctx, x, np.complex128, what)
    return a.ptr, a.ld, x


def _align_series(ctx, ta, ya, sa, col_a, tw, w, b, col_b):
    """the arguments the two alignment entries share, and what has to stay alive while they run"""
    ta = np.ascontiguousarray(ta, dtype=float)
    tw = np.ascontiguousarray(tw, dtype=float)
    w = np.ascontiguousarray(w, dtype=float)
    col_a = np.ascontiguousarray(col_a, dtype=np.int32)
    col_b = np.ascontiguousarray(col_b, dtype=np.int32)
    if ta.ndim != 1 or tw.ndim != 1 or w.shape != tw.shape or col_a.ndim != 1 or col_a.shape != col_b.shape:
        raise ValueError("alignment takes 1-d time axes, one weight per window row and column tables of one length")
    ya_ptr, ld_a, ya = _align_bulk(ctx, ya, "values of the moving waveform")
    sa_ptr, ld_s, sa = _align_bulk(ctx, sa, "slopes of the moving waveform")
    b_ptr, ld_b, b = _align_bulk(ctx, b, "window rows of the fixed waveform")
    if tuple(ya.shape) != tuple(sa.shape) or ld_s != ld_a or ya.shape[0] != ta.shape[0]:
        raise ValueError("values and slopes of the moving waveform must have one shape and row stride, one row per time step")
    if b.shape[0] != tw.shape[0]:
        raise ValueError("the fixed waveform needs one row per window time")
    if col_a.size and (col_a.min() < 0 or col_a.max() >= ya.shape[1] or col_b.min() < 0 or col_b.max() >= b.shape[1]):
        raise ValueError("a column table names a column outside its array")
    i32 = ctypes.POINTER(ctypes.c_int32)
    args = (dptr(ta), ta.shape[0], ya_ptr, sa_ptr, ld_a, col_a.ctypes.data_as(i32), dptr(tw), dptr(w), tw.shape[0], b_ptr, ld_b,
            col_b.ctypes.data_as(i32), col_a.shape[0])
    return args, (ta, tw, w, col_a, col_b, ya, sa, b)


def align_moments(ta, ya, sa, col_a, tw, w, b, col_b, m_slot, n_slots, dts, order=0, ctx=None):
    """Correlation moments of the alignment cost at the time offsets `dts` (ascending) with their dt-derivatives up to `order` (0..2):
    out[o, k, 0] = (d/ddt)^o sum_i w_i sum_c |A_c(tw_i + dts_k)|^2,  out[o, k, 1 + 2 s] + i out[o, k, 2 + 2 s] =
    (d/ddt)^o sum_i w_i sum_{c: m_slot[c] = s} A_c(tw_i + dts_k) conj(b[i, col_b[c]]),  A_c = the cubic spline through (ta, ya[:, col_a[c]])
    whose knot slopes are sa.  ya, sa [na, *] and b [nw, *] are device tensors (complex128) or host arrays, which are uploaded once.
    Returns a host array [order + 1, len(dts), 1 + 2 n_slots]."""
    ctx = _ctx(ctx)
    args, _keep = _align_series(ctx, ta, ya, sa, col_a, tw, w, b, col_b)
    m_slot = np.ascontiguousarray(m_slot, dtype=np.int32)
    dts = np.ascontiguousarray(dts, dtype=float)
    if m_slot.shape != (args[-1],) or dts.ndim != 1:
        raise ValueError("align_moments takes one slot per common column and a 1-d array of offsets")
    out = np.empty((int(order) + 1, dts.shape[0], 1 + 2 * int(n_slots)))
    rc = _lib.load().bms_align_moments(ctx.handle, *args, m_slot.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(n_slots), BMS_DEVICE,
                                       dptr(dts), dts.shape[0], int(order), dptr(out))
    ctx.check(rc, "bms_align_moments")
    return out


def align_residual(ta, ya, sa, col_a, tw, w, b, col_b, m_of, dt, dphi, ctx=None):
    """(sum_i w_i sum_c |A_c(tw_i + dt) e^{i m_of[c] dphi} - b[i, col_b[c]]|^2,  sum_i w_i sum_c |b[i, col_b[c]]|^2), both summed
    directly on the GPU; arguments as align_moments."""
    ctx = _ctx(ctx)
    args, _keep = _align_series(ctx, ta, ya, sa, col_a, tw, w, b, col_b)
    m_of = np.ascontiguousarray(m_of, dtype=np.int32)
    if m_of.shape != (args[-1],):
        raise ValueError("align_residual takes one azimuthal number per common column")
    out = np.empty(2)
    rc = _lib.load().bms_align_residual(ctx.handle, *args, m_of.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), BMS_DEVICE, float(dt), float(dphi),
                                        dptr(out))
    ctx.check(rc, "bms_align_residual")
    return float(out[0]), float(out[1])


def knot_slopes(t, y, ctx=None):
    """Slopes at the knots of the not-a-knot cubic spline through (t, y) for a device tensor y [n, n_cols] (complex128, unit column
    stride): bms_spline_derivative(order = 1) evaluated at the knots themselves, device to device.  A new tensor of y's shape."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    a = _stage(ctx, y, np.complex128, "a device series", check_dtype=False)  # (as it always was: the dtype is the caller's business)
    n = a.rows
    out_ptr, out = out_like(a, (n, a.cols), np.complex128)
    rc = _lib.load().bms_spline_derivative(ctx.handle, dptr(t), n, a.ptr, a.ld, a.cols, BMS_DEVICE, dptr(t), n, 1, out_ptr)
    ctx.check(rc, "bms_spline_derivative")
    return out


def integrate_angular_velocity(t, omega, R0=(1.0, 0.0, 0.0, 0.0), tolerance=1e-12):
    """R[N, 4] with R[0] = R0 and dR/dt = (1/2) Omega R for the cubic spline Omega through omega[N, 3] (host routine)."""
    t = np.ascontiguousarray(t, dtype=float)
    omega = np.ascontiguousarray(omega, dtype=float)
    if omega.shape != (t.shape[0], 3):
        raise ValueError(f"omega must have shape ({t.shape[0]}, 3); it has shape {omega.shape}")
    R0 = np.ascontiguousarray(R0, dtype=float)
    out = np.empty((t.shape[0], 4))
    rc = _lib.load().bms_integrate_angular_velocity(None, dptr(t), t.shape[0], dptr(omega), dptr(R0), float(tolerance), dptr(out))
    if rc != 0:
        _lib._raise(rc, None, "bms_integrate_angular_velocity")
    return out


def salm2map(modes, spin, ell_max, n_theta, n_phi, ctx=None):
    """spinsfast.salm2map(modes[..., (ell_max+1)^2], s, ell_max, n_theta, n_phi) -> grid[..., n_theta, n_phi]."""
    ctx = _ctx(ctx)
    a = _lib.as_c16(modes)
    if a.shape[-1] != (ell_max + 1) ** 2:
        raise ValueError("modes must start at l = 0 and end at ell_max")
    lead = a.shape[:-1]
    a2 = a.reshape(-1, a.shape[-1])
    out = np.empty((a2.shape[0], n_theta * n_phi), dtype=np.complex128)
    rc = _lib.load().bms_salm2map(ctx.handle, vptr(a2), BMS_HOST, a2.shape[0], int(spin), int(ell_max), int(n_theta), int(n_phi), vptr(out))
    ctx.check(rc, "bms_salm2map")
    return out.reshape(lead + (n_theta, n_phi))


# ---------------------------------------------------------------------------------- corotating paired-XOR storage form


def paired_xor_tile_rows():
    """rows one tile of the pack kernel owns (bms_paired_xor_tile_rows)"""
    return int(_lib.load().bms_paired_xor_tile_rows())


def pack_paired_xor(data, ell_min, ell_max, tolerance, ctx=None):
    """bms_pack_paired_xor: modes [n, n_modes] of a corotating-frame waveform -> packed words [n, 2 n_modes] (conjugate pairs,
    truncation at `tolerance`, -0.0 -> +0.0, XOR of successive time steps).  A numpy array gives a numpy uint64 array; a device tensor
    (torch complex128, unit column stride) gives a torch int64 tensor that stays in HBM.  ValueError names the first time step that
    cannot be packed (a non-finite value, zero norm)."""
    ctx = _ctx(ctx)
    n = int(data.shape[0])
    a = _modes_arg(ctx, data, n, ell_min, ell_max)
    out_ptr, words = out_like(a, (n, 2 * a.cols), np.uint64)
    bad = c_i64(-1)
    rc = _lib.load().bms_pack_paired_xor(ctx.handle, a.ptr, a.ld, n, int(ell_min), int(ell_max), a.mem, float(tolerance), out_ptr, ctypes.byref(bad))
    if rc == _lib.BMS_ERR_INVALID and bad.value >= 0:
        raise ValueError(f"time step {bad.value} cannot be packed: it holds a non-finite value, has zero norm, or its truncation scale is "
                         "beyond the range of the doubles")
    ctx.check(rc, "bms_pack_paired_xor")
    return words


def unpack_paired_xor(words, ell_min, ell_max, ctx=None):
    """bms_unpack_paired_xor: packed words [n, 2 n_modes] (numpy uint64, or a torch int64 tensor on the device) -> modes [n, n_modes]
    (numpy complex128, or a torch complex128 tensor that stays in HBM)."""
    ctx = _ctx(ctx)
    n_modes = LM_total_size(ell_min, ell_max)
    n = int(words.shape[0])
    if tuple(words.shape) != (n, 2 * n_modes):
        raise ValueError(f"words of shape {tuple(words.shape)} inconsistent with {n} time steps and ell range [{ell_min}, {ell_max}]")
    if _is_device_array(words):
        words = words.contiguous()
    # (as it always was: a tensor's dtype is not checked, and the context is not moved to torch's stream)
    a = _stage(ctx, words, np.uint64, "words", contiguous=True, check_dtype=False, attach=False)
    out_ptr, out = out_like(a, (n, n_modes), np.complex128)
    rc = _lib.load().bms_unpack_paired_xor(ctx.handle, a.ptr, n, int(ell_min), int(ell_max), a.mem, out_ptr, n_modes)
    ctx.check(rc, "bms_unpack_paired_xor")
    return out


# ---------------------------------------------------------------------------------- centre-of-mass track and drift fit


def com_fit_tile_panels():
    """panels (two intervals each) behind one partial sum of the moments (bms_com_fit_tile_panels)"""
    return int(_lib.load().bms_com_fit_tile_panels())


def _com_arrays(ctx, arrays):
    """float64 contiguous copies of `arrays` side by side, staged: device tensors if any of them is one, numpy arrays otherwise"""
    on_gpu = [_is_device_array(x) and x.is_cuda for x in arrays]  # (a CPU tensor counts as a host array here, as it always did)
    if any(on_gpu):
        import torch

        from . import device_series

        _on_device_of(ctx, *[x for x, g in zip(arrays, on_gpu) if g])
        dev = device_series.attach(ctx)  # (torch's copies and the engine's kernels on one stream)
        arrays = [x.to(torch.float64).contiguous() if g else torch.as_tensor(np.asarray(x, dtype=float), device=dev).contiguous()
                  for x, g in zip(arrays, on_gpu)]
    else:
        arrays = [x.numpy() if _is_device_array(x) else x for x in arrays]
    staged = [_stage(ctx, x, float, "a centre-of-mass array", contiguous=True) for x in arrays]
    return [a.keep for a in staged], staged


def com_track(t, x_a, x_b, m_a, m_b, matter=False, ctx=None):
    """bms_com_motion: (t, CoM[n, 3]) with CoM = (m_A x_A + m_B x_B) / (m_A + m_B) of trajectories x_A, x_B [n, 3] and masses of length
    n or 1, bit for bit the numpy expression; matter=True also divides t and CoM by m_A + m_B.  numpy arrays give numpy arrays; if any
    trajectory is a device tensor everything stays (or is put) on the device and the results are device tensors."""
    ctx = _ctx(ctx)
    (t, x_a, x_b, m_a, m_b), args = _com_arrays(ctx, [t, x_a, x_b, m_a, m_b])
    n = int(x_a.shape[0])
    if tuple(x_a.shape) != (n, 3) or tuple(x_b.shape) != (n, 3) or tuple(t.shape) != (n,) or m_a.ndim != 1 or m_b.ndim != 1:
        raise ValueError(f"trajectories of shapes {tuple(x_a.shape)}, {tuple(x_b.shape)} and times of shape {tuple(t.shape)} do not describe "
                         f"{n} samples of two positions")
    com_ptr, com = out_like(args[1], (n, 3), float)
    t_ptr, t_out = out_like(args[1], (n,), float) if matter else (None, t)
    rc = _lib.load().bms_com_motion(ctx.handle, args[0].ptr, args[1].ptr, args[2].ptr, args[3].ptr, int(m_a.shape[0]), args[4].ptr, int(m_b.shape[0]), n,
                                    int(bool(matter)), args[1].mem, t_ptr, com_ptr)
    ctx.check(rc, "bms_com_motion")
    return t_out, com


def com_fit(t, com, skip_beginning_fraction=0.01, skip_ending_fraction=0.10, fit_acceleration=False, ctx=None):
    """bms_com_fit on t [n], com [n, 3] (numpy arrays, or device tensors that stay where they are): a dict with x_i, v_i, a_i [3], t_i,
    t_f, i_i, i_f and moments [3, 3] -- the window of the skip fractions, the Simpson moments of the track over it and the position,
    velocity (and acceleration) that bring the track closest to the origin, correctly rounded."""
    ctx = _ctx(ctx)
    (t, com), args = _com_arrays(ctx, [t, com])
    n = int(t.shape[0])
    if t.ndim != 1 or tuple(com.shape) != (n, 3):
        raise ValueError(f"times of shape {tuple(t.shape)} and a track of shape {tuple(com.shape)}: expected ({n},) and ({n}, 3)")
    res = _lib.bms_com_fit_result()
    rc = _lib.load().bms_com_fit(ctx.handle, args[0].ptr, args[1].ptr, n, args[0].mem, float(skip_beginning_fraction), float(skip_ending_fraction),
                                 int(bool(fit_acceleration)), ctypes.byref(res))
    ctx.check(rc, "bms_com_fit")
    return dict(x_i=np.array(res.x_i), v_i=np.array(res.v_i), a_i=np.array(res.a_i), t_i=np.float64(res.t_i), t_f=np.float64(res.t_f),
                i_i=int(res.i_i), i_f=int(res.i_f), moments=np.array([list(row) for row in res.moments]))


# ---------------------------------------------------------------------------------- raw finite-radius series -> tortoise time


def retard_tile():
    """samples per tile of the scans behind finite_radius_retard (bms_retard_tile)"""
    return int(_lib.load().bms_retard_tile())


def _rows_arg(ctx, x, dtype, what, n, cols=None):
    """(_Arg, array kept alive) of [n, cols] rows of `dtype` with unit column stride and any row stride >= cols: a device tensor, or a
    numpy array, whose row view is passed as it is (anything else is copied to a contiguous array)"""
    if _is_device_array(x):
        return _stage(ctx, x, dtype, what, shape=(n, cols))
    a = np.asarray(x)
    item = np.dtype(dtype).itemsize
    if a.dtype != np.dtype(dtype) or a.ndim != 2 or (a.shape[1] > 1 and a.strides[1] != item) or a.strides[0] % item or a.strides[0] < item * a.shape[1]:
        a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2 or a.shape[0] != n or (cols is not None and a.shape[1] != cols):
        raise ValueError(f"{what} must have shape ({n}, {'n' if cols is None else cols}); it has shape {a.shape}")
    ld = a.strides[0] // item if n > 1 else max(a.shape[1], 1)
    return _Arg(c_vp(a.ctypes.data), ld, n, a.shape[1], BMS_HOST, (a.shape[1],), a, None)


def finite_radius_retard(t, areal_radius, average_lapse, data, coord_radius, initial_adm_energy, ch_mass, unit_scale, radius_exponent,
                         frame=None, min_time_step=1.0e-3, out=None, ctx=None):
    """One raw finite-radius series retarded to tortoise time (bms_finite_radius_retard; scri/extrapolation.py:27-45, :356-402).

    t, areal_radius, average_lapse: the raw series f8[n_raw]; data [n_raw, n_cols] complex128 and frame [n_raw, 4] float64 (or None):
    numpy arrays (row views with a stride are read as they are) or device tensors with unit column stride, all in one kind of memory.
    out: an array [n_raw, >= n_cols] of that kind that receives the rows, or None for a new one.
    Returns (t_out[K], radii_out[K], data_out[K, n_cols], frame_out[K, 4] or None) for the K kept samples: the times and radii are
    numpy arrays, the rows and the frame views of arrays of n_raw rows in the memory of `data`."""
    ctx = _ctx(ctx)
    t = np.ascontiguousarray(t, dtype=float)
    n = t.shape[0]
    r = np.ascontiguousarray(areal_radius, dtype=float)
    lapse = np.ascontiguousarray(average_lapse, dtype=float)
    if t.ndim != 1 or r.shape != (n,) or lapse.shape != (n,):
        raise ValueError(f"times of shape {t.shape}, areal radii of shape {r.shape} and lapses of shape {lapse.shape}: expected three series of one length")
    if n < 1:
        raise ValueError("bms_finite_radius_retard: n_raw = 0: at least one sample")
    a = _rows_arg(ctx, data, np.complex128, "data", n)
    n_cols = a.cols
    if out is None:
        out_ptr, out = out_like(a, (n, n_cols), np.complex128)
        ld_out = n_cols
    else:
        if _is_device_array(out) != (a.mem == BMS_DEVICE):
            raise ValueError("data and out must live in the same memory")
        if a.mem == BMS_HOST and (not isinstance(out, np.ndarray) or out.dtype != np.complex128 or not out.flags.writeable):
            raise ValueError("out must be a writeable complex128 array")
        o = _rows_arg(ctx, out[:, :n_cols] if out.shape[1] >= n_cols else out, np.complex128, "out", n, n_cols)
        if a.mem == BMS_HOST and not np.shares_memory(o.keep, out):
            raise ValueError("out must have unit column stride and a row stride that is a multiple of 16 bytes")
        out_ptr, ld_out = o.ptr, o.ld
    f = fo = fo_ptr = None
    if frame is not None:
        if _is_device_array(frame) != (a.mem == BMS_DEVICE):
            raise ValueError("data and frame must live in the same memory")
        f = _stage(ctx, frame, float, "frame", shape=(n, 4), contiguous=_is_device_array(frame))
        fo_ptr, fo = out_like(f, (n, 4), float)
    kept = c_i64(0)
    t_out, r_out = np.empty(n), np.empty(n)
    rc = _lib.load().bms_finite_radius_retard(
        ctx.handle, dptr(t), dptr(r), dptr(lapse), n, a.ptr, a.ld, n_cols, a.mem, f.ptr if f else None, float(coord_radius),
        float(initial_adm_energy), float(ch_mass), float(unit_scale), int(radius_exponent), float(min_time_step), ctypes.byref(kept),
        dptr(t_out), dptr(r_out), out_ptr, ld_out, fo_ptr)
    ctx.check(rc, "bms_finite_radius_retard")
    k = int(kept.value)
    return t_out[:k], r_out[:k], out[:k, :n_cols], (fo[:k] if fo is not None else None)
