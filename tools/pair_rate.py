"""Time of the two-waveform operations on a pair of device-resident chirps of 1e5 time steps, l = 2..16 (285 modes) (DESIGN section 4,
"Brackets"):

  inner, lvector, llmatrix                        `a.inner_product(b)`, `LVector(a, b)`, `LLComparisonMatrix(a, b)` of the resident pair: one
                                                  bms_pair_brackets launch (and, for the inner product, the spline quadrature in HBM)
  parent_inner, parent_lvector, parent_llmatrix   the route the same calls took before the kernel existed, which two host-resident waveforms
                                                  still take: both waveforms read back to the host (reading `data` evicted them -- part of
                                                  the call, so part of the time), then the numpy sum / a bms_mode_map launch per ladder
                                                  operator and a host contraction per bracket
  kernel                                          the bracket kernel alone by HIP events (the context's timing of its one launch), all thirteen
                                                  brackets, device tensors in and out; beside it the launch that forms the inner product alone

Every timed run is a process of its own with a time limit, one at a time, the kinds alternating, `reps` runs of each; a run that fails
or exceeds its limit ends the measurement there.  The kernel's share of the HBM rate is over its own bytes, 2 N n_modes 16 + 16 13 N.
A record, not a bar.
Usage: python tools/pair_rate.py [n_times] [reps] [ell_max]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELL_MIN = 2
STEP_LIMIT_S = 400
CALLS = ("inner", "lvector", "llmatrix")
KINDS = CALLS + tuple("parent_" + k for k in CALLS) + ("kernel",)
HBM_BYTES_PER_S = 8e12  # the peak DESIGN section 4 quotes its fractions against


def _waveforms(n, ell_max):
    import numpy as np

    import scri_amd
    from scri_amd import synthetic

    t = np.linspace(0.0, 1000.0, n) + 0.003 * np.cos(np.arange(n))
    ctx = scri_amd.Context(0)
    kw = dict(t=t, ell_min=ELL_MIN, ell_max=ell_max, dataType=scri_amd.h, frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    a = scri_amd.WaveformModes(data=synthetic.chirp_modes(t, ELL_MIN, ell_max, 3) * (1 + 0.001 * t[:, None]), **kw).to_device()
    b = scri_amd.WaveformModes(data=synthetic.chirp_modes(t, ELL_MIN, ell_max, 4) * (1 - 0.0002 * t[:, None]), **kw).to_device()
    return ctx, a, b


def _call(name, a, b):
    import numpy as np

    from scri_amd import mode_calculations

    if name == "inner":
        return np.array([a.inner_product(b)])
    return mode_calculations.LVector(a, b) if name == "lvector" else mode_calculations.LLComparisonMatrix(a, b)


def _step(kind, n, ell_max):
    import numpy as np

    from scri_amd import engine

    ctx, a, b = _waveforms(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": a.n_modes}
    if kind == "kernel":
        engine.pair_brackets(a._dev, b._dev, ELL_MIN, ell_max, ctx=ctx)  # warm-up: the first launch
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        res = engine.pair_brackets(a._dev, b._dev, ELL_MIN, ell_max, ctx=ctx)
        ms, launches = ctx.get_timing(reset=True)["pointwise"]
        assert launches == 1
        out.update(ms=ms, checksum=float(res[2][-1].abs().sum().item()), launch_shape=list(engine.pair_launch_shape(a.n_modes)))
        engine.pair_brackets(a._dev, b._dev, ELL_MIN, ell_max, want="inner", ctx=ctx)
        out.update(inner_only_ms=ctx.get_timing(reset=True)["pointwise"][0])
    elif kind.startswith("parent_"):
        _call(kind[7:], a[:1000].to_host(), b[:1000].to_host())  # warm-up of the kernels, the copy path and numpy on a short piece
        ctx.synchronize()
        t0 = time.perf_counter()
        res = _call(kind[7:], a.to_host(), b.to_host())
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(np.abs(res[-1]).sum()), resident=bool(a.is_device_resident or b.is_device_resident))
    else:
        _call(kind, a, b)  # warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        res = _call(kind, a, b)
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(np.abs(res[-1]).sum()), resident=bool(a.is_device_resident and b.is_device_resident))
    ctx.close()
    print(json.dumps(out))


def main():
    import statistics

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    ell_max = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    runs = {k: [] for k in KINDS}
    for kind in list(KINDS) * reps:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n), str(ell_max)], capture_output=True, text=True,
                              timeout=STEP_LIMIT_S)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(line), file=sys.stderr, flush=True)
        runs[kind].append(line)
    n_modes = runs["kernel"][0]["n_modes"]
    summary = {"n_times": n, "ell_max": ell_max, "n_modes": n_modes, "reps": reps, "launch_shape": runs["kernel"][0]["launch_shape"]}
    for kind in KINDS:
        ms = [r["ms"] for r in runs[kind]]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 4), f"{kind}_spread_ms": round(max(ms) - min(ms), 4),
                        f"{kind}_ms": [round(v, 4) for v in ms]})
    summary["kernel_inner_only_median_ms"] = round(statistics.median(r["inner_only_ms"] for r in runs["kernel"]), 4)
    kernel_bytes = 2 * n * n_modes * 16 + 16 * 13 * n
    rate = kernel_bytes / (summary["kernel_median_ms"] * 1e-3)
    summary.update(kernel_bytes=kernel_bytes, kernel_TB_per_s=round(rate / 1e12, 3), kernel_share_of_hbm=round(rate / HBM_BYTES_PER_S, 3))
    for k in CALLS:
        summary[f"parent_over_new_{k}"] = round(summary[f"parent_{k}_median_ms"] / summary[f"{k}_median_ms"], 1)
        summary[f"{k}_spreads_separated"] = bool(max(r["ms"] for r in runs[k]) < min(r["ms"] for r in runs["parent_" + k]))
    summary["checksums"] = {kind: runs[kind][0]["checksum"] for kind in KINDS}
    summary["new_route_stays_resident"] = all(r["resident"] for k in CALLS for r in runs[k])
    summary["parent_route_evicts"] = not any(r["resident"] for k in CALLS for r in runs["parent_" + k])
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "--step":
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
