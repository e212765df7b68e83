"""The host / device parity table of the engine wrappers (tests/test_gpu_host_device_parity.py, tools/abi_ab_bits.py): every
wrapper of scri_amd/engine.py that takes a numpy array or a device tensor, called on the same values in each memory kind.

A case is (id, layouts, run): run(ctx, layout) returns the outputs as host arrays, layout being "host" (numpy arrays), "device"
(contiguous device tensors) or "wide" (device tensors that are column slices of wider ones, so that the row stride exceeds the
columns; with one row, where the stride rule switches, the slice for one column and for three a view with the strides of a
transposed column, (1, 1), whose row stride is no pitch at all).  The shapes are the smallest at which the staging of the arguments can
go wrong, not workload sizes: rows in {1, 2, 4, 5} cut to what an entry admits, columns in {1, 3}, modes (0, 0) and (2, 3)."""
import collections
import zlib

import numpy as np

from scri_amd import engine

Case = collections.namedtuple("Case", "id layouts run")

ROWS = (1, 2, 4, 5)
SPLINE_ROWS = (4, 5)  # the not-a-knot splines, and what check_time_axis asks of the frame entries
COLS = (1, 3)
ELL_RANGES = ((0, 0), (2, 3))
ALL = ("host", "device", "wide")
FLAT = ("host", "device")  # per-step arrays of the frame chain and the centre-of-mass entries are contiguous by contract


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _complex(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _axis(n, t0=0.0):
    """a strictly increasing, slightly uneven time axis"""
    return t0 + 0.1 * np.arange(n) + 0.01 * np.sin(np.arange(n))


def _rotors(rng, n):
    R = rng.normal(size=(n, 4))
    return R / np.linalg.norm(R, axis=1)[:, None]


def place(ctx, a, layout):
    """`a` where `layout` says: itself, a contiguous device tensor, or columns [1, 1 + n_cols) of a device tensor two columns wider"""
    if layout == "host":
        return a
    import torch

    dev = torch.device("cuda", ctx.device)
    if layout == "device" or a.ndim != 2:
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if a.shape[0] == 1 and a.shape[1] > 1:  # one row with the strides of a transposed column: its row stride (1) is no pitch of the array
        row = torch.from_numpy(a.reshape(-1).copy()).to(dev).as_strided((1, a.shape[1]), (1, 1))
        assert row.stride(0) < row.shape[1]
        return row
    wide = np.full((a.shape[0], a.shape[1] + 2), -7.0, dtype=a.dtype)
    wide[:, 1:-1] = a
    return torch.from_numpy(wide).to(dev)[:, 1:-1]


def host(x):
    """an output as a contiguous host array (None stays None)"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x)


def _outputs(*xs):
    return [host(x) for x in xs if x is not None]


def _n_modes(ell_min, ell_max):
    return engine.LM_total_size(ell_min, ell_max)


def _cases():
    out = []

    def add(case_id, layouts, run):
        out.append(Case(case_id, layouts, run))

    # ---- splines of a series
    for n in SPLINE_ROWS:
        for cols in COLS:
            for m in (1, 6):
                def run(ctx, layout, n=n, cols=cols, m=m):
                    y = _complex(_rng("cs", n, cols), (n, cols))
                    x = _axis(n)
                    return _outputs(engine.cubic_spline(x, place(ctx, y, layout), np.linspace(x[0], x[-1], m + 1)[1:], ctx=ctx))
                add(f"cubic_spline-n{n}-c{cols}-m{m}", ALL, run)
            for order in (-3, -1, 0, 1):
                def run(ctx, layout, n=n, cols=cols, order=order):
                    y = _complex(_rng("sd", n, cols), (n, cols))
                    x = _axis(n)
                    return _outputs(engine.spline_derivative(x, place(ctx, y, layout), np.linspace(x[0], x[-1], 7), order=order, ctx=ctx))
                add(f"spline_derivative-n{n}-c{cols}-order{order}", ALL, run)

    # ---- series operators
    for n in ROWS:
        for cols in COLS:
            for take_sqrt in (False, True):
                def run(ctx, layout, n=n, cols=cols, take_sqrt=take_sqrt):
                    d = _complex(_rng("rn", n, cols), (n, cols))
                    if layout == "host":
                        return _outputs(engine.row_norm(d, take_sqrt=take_sqrt, ctx=ctx))
                    return _outputs(engine.row_norm(None, take_sqrt=take_sqrt, ctx=ctx, device_tensor=place(ctx, d, layout)))
                add(f"row_norm-n{n}-c{cols}-sqrt{int(take_sqrt)}", ALL, run)
            for want in ("abs", "arg", ("abs", "arg"), ("arg", "abs")):
                for unwrap in (False, True):
                    def run(ctx, layout, n=n, cols=cols, want=want, unwrap=unwrap):
                        d = 3.0 * _complex(_rng("pa", n, cols), (n, cols))
                        res = engine.abs_arg(place(ctx, d, layout), unwrap=unwrap, want=want, ctx=ctx)
                        return _outputs(*((res,) if isinstance(want, str) else res))
                    tag = want if isinstance(want, str) else "+".join(want)
                    add(f"abs_arg-n{n}-c{cols}-{tag}-unwrap{int(unwrap)}", ALL, run)
            for bad in (False, True):
                def run(ctx, layout, n=n, cols=cols, bad=bad):
                    d = _complex(_rng("nf", n, cols), (n, cols))
                    if bad:
                        d[n - 1, cols - 1] = complex(np.nan, 1.0)
                        d[n // 2, 0] = complex(0.0, np.inf)
                    return [np.array(engine.count_nonfinite(place(ctx, d, layout), ctx=ctx), dtype=np.int64)]
                add(f"count_nonfinite-n{n}-c{cols}-bad{int(bad)}", ALL, run)
            def run(ctx, layout, n=n, cols=cols):
                rng = _rng("rt", n, cols)
                h0 = _complex(rng, (n, cols))
                res = place(ctx, np.zeros((n, cols), dtype=complex), layout)
                engine.radius_terms(_axis(n), place(ctx, h0, layout), 3, 0.25, 100.0, res, ctx=ctx)
                return _outputs(res)
            add(f"radius_terms-n{n}-c{cols}", ALL, run)

    # ---- modes in, per-step quantities out
    for n in SPLINE_ROWS:
        for ell_min, ell_max in ELL_RANGES:
            nm = _n_modes(ell_min, ell_max)

            def run(ctx, layout, n=n, ell_min=ell_min, ell_max=ell_max, nm=nm):
                d = _complex(_rng("av", n, nm), (n, nm))
                return _outputs(*engine.angular_velocity(_axis(n), place(ctx, d, layout), ell_min, ell_max, ctx=ctx, parts=True))
            add(f"angular_velocity-n{n}-l{ell_min}_{ell_max}", ALL, run)

            def run(ctx, layout, n=n, ell_min=ell_min, ell_max=ell_max, nm=nm):
                from scri_amd import device_series

                d = _complex(_rng("co", n, nm), (n, nm))
                frame_dev = device_series.empty_real(ctx, (n, 4))
                frame, om = engine.corotating_frame(_axis(n), place(ctx, d, layout), ell_min, ell_max, frame_dev, want_frame=True, want_omega=True,
                                                    ctx=ctx)
                return _outputs(frame, om, frame_dev)
            add(f"corotating_frame-n{n}-l{ell_min}_{ell_max}", ALL, run)

            for given in (False, True):
                def run(ctx, layout, n=n, ell_min=ell_min, ell_max=ell_max, nm=nm, given=given):
                    from scri_amd import device_series

                    d = _complex(_rng("cp", n, nm), (n, nm))
                    frame_dev = device_series.empty_real(ctx, (n, 4)) if given else None
                    frame, axis = engine.coprecessing_frame(_axis(n), place(ctx, d, layout), ell_min, ell_max, rough_index=n - 1, frame_dev=frame_dev,
                                                            want_frame=True, want_axis=True, ctx=ctx)
                    return _outputs(frame, axis, frame_dev)
                add(f"coprecessing_frame-n{n}-l{ell_min}_{ell_max}-dev{int(given)}", ALL, run)

    # ---- the frame chain: contiguous per-step arrays, a caller-supplied out= on the device
    def given_out(ctx, layout, given, shape):
        if not (given and layout != "host"):
            return None
        from scri_amd import device_series

        return device_series.empty_real(ctx, shape)

    for n in SPLINE_ROWS:
        for given in (False, True):
            def run(ctx, layout, n=n, given=given):
                om = 0.3 * _rng("fo", n).normal(size=(n, 3))
                o = given_out(ctx, layout, given, (n, 4))
                res = engine.frame_from_angular_velocity(_axis(n), place(ctx, om, layout), R0=(0.6, 0.0, 0.8, 0.0), ctx=ctx, out=o)
                assert o is None or res is o
                return _outputs(res)
            add(f"frame_from_angular_velocity-n{n}-out{int(given)}", FLAT, run)

        def run(ctx, layout, n=n):
            return _outputs(engine.minimal_rotation(_axis(n), place(ctx, _rotors(_rng("mr", n), n), layout), iterations=2, ctx=ctx))
        add(f"minimal_rotation-n{n}", FLAT, run)

        def run(ctx, layout, n=n):
            return _outputs(engine.rotor_angular_velocity(_axis(n), place(ctx, _rotors(_rng("ro", n), n), layout), ctx=ctx))
        add(f"rotor_angular_velocity-n{n}", FLAT, run)

    for n in ROWS:
        def run(ctx, layout, n=n):
            a = _rng("da", n).normal(size=(n, 3, 3))
            ll = a + a.transpose(0, 2, 1)
            return _outputs(engine.dominant_axis(place(ctx, ll, layout), rough=(0.1, 0.2, 1.0), rough_index=n // 2, ctx=ctx))
        add(f"dominant_axis-n{n}", FLAT, run)

        for log, spinors, right in ((False, False, False), (True, True, True), (True, False, False), (False, True, True)):
            def run(ctx, layout, n=n, log=log, spinors=spinors, right=right):
                frame = place(ctx, 1.5 * _rotors(_rng("fa", n), n), layout)
                lg, sp = engine.frame_adjust(frame, right=(0.0, 0.6, 0.0, 0.8) if right else None, truncate_tolerance=1e-6 if log else 0.0,
                                             want_log=log, want_spinors=spinors, ctx=ctx)
                return _outputs(frame, lg, sp)
            add(f"frame_adjust-n{n}-log{int(log)}-sp{int(spinors)}-right{int(right)}", FLAT, run)

    for n in (2, 4, 5):
        for m in (1, 3):
            for given in (False, True):
                def run(ctx, layout, n=n, m=m, given=given):
                    t_in = _axis(n)
                    t_out = np.linspace(t_in[-1], t_in[0], m + 2)[1:-1]
                    o = given_out(ctx, layout, given, (m, 4))
                    res = engine.squad(place(ctx, _rotors(_rng("sq", n), n), layout), t_in, t_out, ctx=ctx, out=o)
                    assert o is None or res is o
                    return _outputs(res)
                add(f"squad-n{n}-m{m}-out{int(given)}", FLAT, run)

    # ---- alignment: the bulk arrays host or device (host arrays go up once inside the wrapper)
    for na in SPLINE_ROWS:
        for cols in COLS:
            def inputs(ctx, layout, na=na, cols=cols):
                rng = _rng("al", na, cols)
                ta = _axis(na)
                tw = np.array([ta[1] + 0.01, ta[-2] + 0.02])
                col = np.arange(cols, dtype=np.int32)
                return (ta, place(ctx, _complex(rng, (na, cols)), layout), place(ctx, _complex(rng, (na, cols)), layout), col, tw, np.array([0.4, 0.6]),
                        place(ctx, _complex(rng, (2, cols)), layout), col[::-1].copy())

            def run(ctx, layout, inputs=inputs, cols=cols):
                return _outputs(engine.align_moments(*inputs(ctx, layout), np.arange(cols, dtype=np.int32) % 2, 2, np.array([-0.01, 0.0, 0.015]), order=2,
                                                     ctx=ctx))
            add(f"align_moments-n{na}-c{cols}", ALL, run)

            def run(ctx, layout, inputs=inputs, cols=cols):
                return [np.array(engine.align_residual(*inputs(ctx, layout), np.arange(cols, dtype=np.int32) - 1, 0.01, 0.3, ctx=ctx))]
            add(f"align_residual-n{na}-c{cols}", ALL, run)

    # ---- corotating paired-XOR storage
    for n in ROWS:
        for ell_min, ell_max in ELL_RANGES:
            nm = _n_modes(ell_min, ell_max)

            def run(ctx, layout, n=n, ell_min=ell_min, ell_max=ell_max, nm=nm):
                d = _complex(_rng("px", n, nm), (n, nm))
                words = engine.pack_paired_xor(place(ctx, d, layout), ell_min, ell_max, 1e-10, ctx=ctx)
                back = engine.unpack_paired_xor(words, ell_min, ell_max, ctx=ctx)  # (numpy uint64 on the host, torch int64 on the device)
                return [host(words).view(np.uint64), host(back)]
            add(f"paired_xor-n{n}-l{ell_min}_{ell_max}", ALL, run)

    # ---- centre of mass: device if any trajectory is a device tensor
    for n in ROWS:
        for matter in (False, True):
            for one_mass in (False, True):
                def run(ctx, layout, n=n, matter=matter, one_mass=one_mass):
                    rng = _rng("ct", n)
                    t = _axis(n, 10.0)
                    x_a, x_b = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
                    m_a = np.array([0.6]) if one_mass else 0.6 + 0.01 * rng.normal(size=n)
                    m_b = 0.4 + 0.01 * rng.normal(size=n)
                    return _outputs(*engine.com_track(t, place(ctx, x_a, layout), x_b, m_a, place(ctx, m_b, layout), matter=matter, ctx=ctx))
                add(f"com_track-n{n}-matter{int(matter)}-onemass{int(one_mass)}", FLAT, run)
    for n in (2, 4, 5):
        for acc in (False, True):
            def run(ctx, layout, n=n, acc=acc):
                rng = _rng("cf", n)
                t = _axis(n, 10.0)
                com = 0.01 * rng.normal(size=(n, 3)) + 0.001 * t[:, None]
                r = engine.com_fit(place(ctx, t, layout), place(ctx, com, layout), skip_beginning_fraction=0.0, skip_ending_fraction=0.0,
                                   fit_acceleration=acc, ctx=ctx)
                return [np.asarray(r[k], dtype=float) for k in ("x_i", "v_i", "a_i", "t_i", "t_f", "i_i", "i_f", "moments")]
            add(f"com_fit-n{n}-acc{int(acc)}", FLAT, run)
    return out


CASES = _cases()
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)
