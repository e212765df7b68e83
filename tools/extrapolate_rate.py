"""Rate of the extrapolation fit (bms_extrapolate) at 24 radii, l = 2..8 (77 modes), orders [2, 3, 4]:
milliseconds per call, the algorithmic bytes (every input value and radius read once, every output written once) per second, and
that rate as a fraction of 8 TB/s of HBM -- with the series resident in HBM, and from / to host memory (pageable and page-locked).
Usage: python tools/extrapolate_rate.py [n_times] [reps]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import scri_amd
from scri_amd import _lib, device_series, engine

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
n_r, n_m, orders = 24, 77, [2, 3, 4]
ctx = scri_amd.Context(0)
rng = np.random.default_rng(1)
t = np.arange(n, dtype=float)
radii = np.geomspace(100.0, 1000.0, n_r)[:, None] * (1.0 + 0.01 * np.sin(1e-4 * t[None, :] + np.arange(n_r)[:, None]))
data = rng.normal(size=(n_r, n, n_m)) + 1j * rng.normal(size=(n_r, n, n_m))
nbytes = data.nbytes + radii.nbytes + len(orders) * n * n_m * 16


def timed(go):
    go()
    ctx.synchronize()
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        go()  # (every call ends with the deficient-step counts on the host: the call is complete when it returns)
        walls.append(time.perf_counter() - t0)
    return float(np.median(walls))


dev = device_series.attach(ctx)
srcs = [torch.from_numpy(d).to(dev) for d in data]
r_dev = torch.from_numpy(np.ascontiguousarray(radii)).to(dev)
out = device_series.empty(ctx, (len(orders), n, n_m))
ptrs = [s.data_ptr() for s in srcs]
ctx.enable_timing(True)
w_dev = timed(lambda: engine.extrapolate(ptrs, (r_dev.data_ptr(), n, n_m), orders, ctx=ctx, device=True, out=out.data_ptr()))
kernel_ms = ctx.get_timing(reset=True)["pointwise"][0] / (reps + 1)
ctx.enable_timing(False)
host_in = list(data)
w_host = timed(lambda: engine.extrapolate(host_in, radii, orders, ctx=ctx))
locked = [np.array(d) for d in data]  # (arrays of their own: page-locked in place on the second sighting)
for d in locked:
    _lib.register_if_reused(d)
    assert _lib.register_if_reused(d)
w_locked = timed(lambda: engine.extrapolate(locked, radii, orders, ctx=ctx))
rate = lambda s: nbytes / s / 1e9
print(json.dumps({
    "n_times": n, "n_radii": n_r, "n_modes": n_m, "orders": orders, "bytes": nbytes,
    "device_kernel_ms": round(kernel_ms, 4), "device_kernel_GBps": round(rate(kernel_ms / 1e3), 1),
    "device_kernel_hbm_fraction": round(rate(kernel_ms / 1e3) / 8000.0, 3),
    "device_call_ms": round(w_dev * 1e3, 4), "device_call_GBps": round(rate(w_dev), 1),
    "host_pageable_ms": round(w_host * 1e3, 3), "host_pageable_GBps": round(rate(w_host), 1),
    "host_registered_ms": round(w_locked * 1e3, 3), "host_registered_GBps": round(rate(w_locked), 1),
}))
