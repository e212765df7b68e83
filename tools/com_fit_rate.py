"""One record (not a bar) for DESIGN section 9: `bms_com_fit` on a device-resident track of 1e6 samples -- the median of seven calls,
each a host clock around a call that ends in a device synchronise, after one warm-up -- beside scipy's time for the same rule on the same
track on that host (two `simpson` calls and the two `argmin`, as the reference spends them), and beside the track kernel.  The traffic is
32 MB, so the call is bound by its launches and the one read-back, not by HBM.

Usage: python tools/com_fit_rate.py [n_samples] [reps]        (prints one JSON line)"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(n, reps):
    import torch
    from scipy.integrate import simpson

    import scri_amd
    from scri_amd import engine

    rng = np.random.default_rng(1)
    t = 5000.0 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 0.15, size=n - 1))])
    s = t - t[0]
    com = 1e-2 * rng.normal(size=3) + 1e-7 * s[:, None] * rng.normal(size=3) + 1e-3 * np.stack([np.cos(0.3 * s), np.sin(0.3 * s), 0 * s], axis=1)
    ctx = scri_amd.Context(0)
    dev = torch.device("cuda", ctx.device)
    t_dev, com_dev = torch.from_numpy(t).to(dev), torch.from_numpy(com).to(dev)
    out = {"n_samples": n, "reps": reps, "bytes": 32 * n}
    for acc in (False, True):
        engine.com_fit(t_dev, com_dev, 0.01, 0.10, acc, ctx=ctx)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fit = engine.com_fit(t_dev, com_dev, 0.01, 0.10, acc, ctx=ctx)  # (ends in a stream synchronise and the read-back of the result)
            times.append((time.perf_counter() - t0) * 1e3)
        key = "fit_accelerated" if acc else "fit"
        if not acc:
            linear = fit
        out[key + "_ms_median"], out[key + "_ms_min"], out[key + "_ms_max"] = statistics.median(times), min(times), max(times)
    host = []
    for _ in range(reps):
        t0 = time.perf_counter()
        t_i, t_f = t[0] + (t[-1] - t[0]) * 0.01, t[-1] - (t[-1] - t[0]) * 0.10
        i_i, i_f = np.argmin(np.abs(t - t_i)), np.argmin(np.abs(t - t_f))
        c0 = simpson(com[i_i : i_f + 1], x=t[i_i : i_f + 1], axis=0)
        c1 = simpson((t[:, np.newaxis] * com)[i_i : i_f + 1], x=t[i_i : i_f + 1], axis=0)
        host.append((time.perf_counter() - t0) * 1e3)
    out["scipy_ms_median"], out["scipy_ms_min"], out["scipy_ms_max"] = statistics.median(host), min(host), max(host)
    v_host = 6 * (c0 * (-t_f - t_i) + 2 * c1) / (t_f - t_i) ** 3
    out["v_i_relative_distance_scipy_to_engine"] = float(np.abs(v_host - linear["v_i"]).max() / np.abs(v_host).max())
    x = torch.from_numpy(rng.normal(size=(n, 3))).to(dev)
    m = torch.from_numpy(1.0 + 1e-3 * rng.normal(size=n)).to(dev)
    engine.com_track(t_dev, x, com_dev, m, m, matter=True, ctx=ctx)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        engine.com_track(t_dev, x, com_dev, m, m, matter=True, ctx=ctx)
        times.append((time.perf_counter() - t0) * 1e3)
    out["track_ms_median"] = statistics.median(times)
    print(json.dumps(out))


if __name__ == "__main__":
    main(int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000, int(sys.argv[2]) if len(sys.argv) > 2 else 7)
