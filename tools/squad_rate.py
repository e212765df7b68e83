"""Rate of the rotor interpolation on the GPU (bms_squad; DESIGN section 4, "Rotor interpolation") and what it buys a device-resident
`WaveformModes.interpolate`.

  squad        n = m = 1e5 and 1e6 (rotors on a mildly non-uniform axis, arguments at the midpoints, shuffled):
                 kernels_ms   the two launches alone, HIP events of the context (the "pointwise" class), per call
                 device_ms    engine.squad, rotors and result in device memory (the times go up, nothing comes back)
                 host_ms      engine.squad, rotors and result in host memory (upload, launches, download)
                 numpy_ms     scri_amd.quaternions.squad, the numpy statement, on the same host
  interpolate  a device-resident series of 1e5 steps, l = 2 .. 16 (285 modes), with a frame per step, onto the midpoints:
                 resident_ms  W.interpolate(T): spline where the weights live, frame through bms_squad, result resident
                 bounce_ms    the route of the commit before this one for the same object (the old extrapolation._interpolated): weights
                              to the host, numpy squad, spline from host memory, result uploaded again -- composed here from calls
                              that exist in both commits

One warm-up of every shape, then `reps` timed calls each, alternating the routes; a host clock around work that ends in a synchronise.
Medians and the spread (max - min) are reported.  Usage: python tools/squad_rate.py [reps]        (prints one JSON line)"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _axis(n, rng):
    import numpy as np

    return np.cumsum(0.1 * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, n)))


def _rotors(t):
    import numpy as np

    from scri_amd import quaternions

    a, b = 0.3 * t + 1e-6 * t * t, 0.4 + 0.1 * np.sin(0.05 * t)
    z = np.stack([np.cos(a / 2), 0 * t, 0 * t, np.sin(a / 2)], axis=1)
    y = np.stack([np.cos(b / 2), 0 * t, np.sin(b / 2), 0 * t], axis=1)
    R = quaternions.multiply(z, y)
    return R / np.linalg.norm(R, axis=1)[:, None]


def _timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _summary(samples):
    return {"median_ms": round(statistics.median(samples), 3), "spread_ms": round(max(samples) - min(samples), 3)}


def squad_rates(ctx, n, reps):
    import numpy as np
    import torch

    from scri_amd import device_series, engine, quaternions

    rng = np.random.default_rng(n)
    t = _axis(n, rng)
    R = _rotors(t)
    u = rng.permutation(np.concatenate([0.5 * (t[:-1] + t[1:]), t[-1:]]))
    dev = device_series.attach(ctx)
    R_dev = torch.from_numpy(R).to(dev)
    out_dev = torch.empty((u.size, 4), dtype=torch.float64, device=dev)
    routes = {
        "device": lambda: engine.squad(R_dev, t, u, ctx=ctx, out=out_dev),
        "host": lambda: engine.squad(R, t, u, ctx=ctx),
        "numpy": lambda: quaternions.squad(R, t, u),
    }
    for call in routes.values():  # warm-up: code objects, work-space buffers
        call()
    runs = {k: [] for k in routes}
    for _ in range(reps):
        for k, call in routes.items():
            runs[k].append(_timed(ctx, call))
    ctx.enable_timing(True)
    ctx.get_timing(reset=True)
    for _ in range(reps):
        routes["device"]()
    kernels_ms, launches = ctx.get_timing(reset=True)["pointwise"]
    ctx.enable_timing(False)
    worst = float(np.abs(out_dev.cpu().numpy() - quaternions.squad(R, t, u)).max())
    out = {"n": n, "m": int(u.size), "kernels_ms": round(kernels_ms / reps, 4), "launches_per_call": launches // reps,
           "max_abs_difference_from_numpy": worst}
    out.update({f"{k}_{key}": v for k, s in runs.items() for key, v in _summary(s).items()})
    return out


def interpolate_rates(ctx, reps, n=100000, ell_min=2, ell_max=16):
    import numpy as np

    import scri_amd

    rng = np.random.default_rng(5)
    n_modes = (ell_max + 1) ** 2 - ell_min**2
    t = _axis(n, rng)
    a = rng.normal(size=(2, n_modes)) + 1j * rng.normal(size=(2, n_modes))
    data = a[0] * np.exp(1j * np.outer(t, rng.uniform(0.01, 0.3, size=n_modes))) + a[1]
    W = scri_amd.WaveformModes(t=t, data=data, frame=_rotors(t), ell_min=ell_min, ell_max=ell_max, frameType=scri_amd.Corotating,
                               dataType=scri_amd.h, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx).to_device()
    T = 0.5 * (t[:-1] + t[1:])

    def bounce():
        host = scri_amd.WaveformModes(t=W.t, data=W._dev.cpu().numpy(), frame=W.frame, ell_min=ell_min, ell_max=ell_max, frameType=W.frameType,
                                      dataType=W.dataType, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
        return host.interpolate(T).to_device()

    routes = {"resident": lambda: W.interpolate(T), "bounce": bounce}
    results = {k: call() for k, call in routes.items()}  # warm-up, and the two results
    assert all(r.is_device_resident for r in results.values()) and W.is_device_resident
    same_data = bool(np.array_equal(results["resident"]._dev.cpu().numpy(), results["bounce"]._dev.cpu().numpy()))
    frame_difference = float(np.abs(results["resident"].frame - results["bounce"].frame).max())
    del results
    runs = {k: [] for k in routes}
    for _ in range(reps):
        for k, call in routes.items():
            runs[k].append(_timed(ctx, call))
    out = {"n_times": n, "n_modes": n_modes, "n_new": int(T.size), "same_data_bits": same_data, "max_abs_frame_difference": frame_difference}
    out.update({f"{k}_{key}": v for k, s in runs.items() for key, v in _summary(s).items()})
    return out


def main():
    import scri_amd

    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    ctx = scri_amd.Context(0)
    out = {"reps": reps, "squad": [squad_rates(ctx, n, reps) for n in (100000, 1000000)], "interpolate": interpolate_rates(ctx, reps)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
