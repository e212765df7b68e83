"""Wall time of scri_amd.alignment.align2d on its two routes: the device route (bms_align_moments / bms_align_residual) split into the
slopes solve, the brute-force scan, the Newton steps and the residual, and -- at the sizes where it ends within minutes -- the host
route (numpy/scipy, one CubicSpline evaluation of the whole window per offset).  l = 2..8 (77 modes) on both sides, window rows N in
{1001, 2001, 5001, 20001} at steps of 0.1, about 1.1 N offsets, uniform and jittered (steps x [0.5, 1.5]) time axis of the moving
waveform; one JSON line per (N, axis).
Usage: python tools/align_rate.py [N ...] [--host-up-to N]     (default sizes: all four; host route up to 2001 rows)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401  (the device route allocates through torch: its import is not part of the alignment's time)

import scri_amd
from scri_amd import alignment, engine

host_up_to = 2001
args = sys.argv[1:]
if "--host-up-to" in args:
    k = args.index("--host-up-to")
    host_up_to = int(args[k + 1])
    del args[k : k + 2]
sizes = [int(a) for a in args] or [1001, 2001, 5001, 20001]
ctx = scri_amd.Context(0)
LM = [(l, m) for l in range(2, 9) for m in range(-l, l + 1)]


def chirp(t, seed=1):
    rng = np.random.default_rng(seed)
    amp = rng.normal(size=len(LM)) + 1j * rng.normal(size=len(LM))
    phase = 0.07 * t + 2e-5 * t**2
    return np.stack([a * np.exp(-1j * m * phase) * (1 + 0.001 * t) for a, (l, m) in zip(amp, LM)], axis=1)


def waveform(t, data):
    return scri_amd.WaveformModes(t=t, data=data, ell_min=2, ell_max=8, dataType=scri_amd.h, frameType=scri_amd.Inertial, r_is_scaled_out=True,
                                  m_is_scaled_out=True, ctx=ctx)


clock = {}


def timed(name, fn):
    def wrapper(*a, **kw):
        key = name if name != "moments" else ("scan" if a[11] == 0 else "newton")
        t0 = time.perf_counter()
        out = fn(*a, **kw)
        clock[key] = clock.get(key, 0.0) + time.perf_counter() - t0
        clock[key + "_calls"] = clock.get(key + "_calls", 0) + 1
        return out

    return wrapper


engine.knot_slopes = timed("slopes", engine.knot_slopes)
engine.align_moments = timed("moments", engine.align_moments)
engine.align_residual = timed("residual", engine.align_residual)

for N in sizes:
    W = 0.05 * (N - 1)  # half width of the window
    tb = np.linspace(-1.5 * W, 1.5 * W, 3 * (N - 1) + 1)
    n_a = int(round(1.1 * N))
    for axis in ("uniform", "jittered"):
        ta = np.linspace(-1.1 * W, 1.1 * W, n_a)
        if axis == "jittered":
            steps = np.random.default_rng(5).uniform(0.5, 1.5, n_a - 1)
            ta = ta[0] + (ta[-1] - ta[0]) * np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum()
        dt, dphi = 0.0371 * W, 1.234
        m = np.array([m for _, m in LM])
        wa, wb = waveform(ta, chirp(ta - dt) * np.exp(-1j * m * dphi)), waveform(tb, chirp(tb))
        wa.to_device(), wb.to_device()
        line = {"rows": N, "axis": axis, "modes": len(LM)}
        for run in ("first", "again"):  # the first call of a size grows the context's work space
            clock.clear()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            err, _, res = alignment.align2d(wa, wb, -W, W)
            torch.cuda.synchronize()
            line[f"device_s_{run}"] = round(time.perf_counter() - t0, 5)
        line.update(offsets=int(max(n_a, N)), x=[float(res.x[0]), float(res.x[1])], expected=[dt, dphi], cost=float(err), nfev=int(res.nfev),
                    split_s={k: (round(v, 5) if isinstance(v, float) else v) for k, v in sorted(clock.items())})
        if N <= host_up_to:
            ha, hb = waveform(ta, wa.copy().data), waveform(tb, wb.copy().data)
            t0 = time.perf_counter()
            err_h, _, res_h = alignment.align2d(ha, hb, -W, W)
            line.update(host_s=round(time.perf_counter() - t0, 3), host_x=[float(res_h.x[0]), float(res_h.x[1])], host_cost=float(err_h))
            line["speedup"] = round(line["host_s"] / line["device_s_again"], 1)
        print(json.dumps(line), flush=True)
