"""Time of the four Poincare fluxes of a device-resident chirp of 1e5 time steps, l = 2..16 (285 modes) ("Fluxes"):

  fused          `poincare_fluxes(w)` of the resident waveform: one spline derivative in HBM, one launch, 10 doubles per step read back
  fused_given    the same with a device-resident hdot given: the launch and the read-back
  kernel         the fused kernel alone by HIP events (the context's timing of its one launch), device tensors in and out; beside it the
                 launch that reads hdot alone (energy and momentum)
  parent         the route the same call took before the kernel existed (`flux.host_poincare_fluxes`, which host-resident waveforms
                 still take): the weights read back to the host, eleven grid products and four mode maps, numpy in and out
  parent_given   the same with hdot given

Every timed run is a process of its own with a time limit, one at a time, the kinds alternating, one warm-up and `reps` runs of each; a
run that fails or exceeds its limit ends the measurement there.  The kernel's share of the HBM rate is over its own bytes,
2 N n_modes 16 + 80 N.  A record, not a bar.
Usage: python tools/flux_rate.py [n_times] [reps] [ell_max]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELL_MIN = 2
STEP_LIMIT_S = 400
KINDS = ("fused", "fused_given", "kernel", "parent", "parent_given")
HBM_BYTES_PER_S = 8e12  # the peak DESIGN section 4 quotes its fractions against


def _waveforms(n, ell_max):
    import numpy as np

    import scri_amd
    from scri_amd import synthetic

    t = np.linspace(0.0, 1000.0, n) + 0.003 * np.cos(np.arange(n))
    ctx = scri_amd.Context(0)
    kw = dict(t=t, ell_min=ELL_MIN, ell_max=ell_max, frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)
    w = scri_amd.WaveformModes(data=synthetic.chirp_modes(t, ELL_MIN, ell_max, 3) * (1 + 0.001 * t[:, None]), dataType=scri_amd.h, **kw).to_device()
    wd = scri_amd.WaveformModes(data=synthetic.chirp_modes(t, ELL_MIN, ell_max, 4) * 0.05, dataType=scri_amd.hdot, **kw).to_device()
    return ctx, w, wd


def _step(kind, n, ell_max):
    from scri_amd import engine, flux

    ctx, w, wd = _waveforms(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": w.n_modes}
    given = kind.endswith("given")
    if kind == "kernel":
        engine.poincare_fluxes(w.t, w._dev, wd._dev, ELL_MIN, ell_max, ctx=ctx)  # warm-up: the tables, the first launch
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        res = engine.poincare_fluxes(w.t, w._dev, wd._dev, ELL_MIN, ell_max, ctx=ctx)
        ms, launches = ctx.get_timing(reset=True)["pointwise"]
        assert launches == 1
        out.update(ms=ms, checksum=float(res[3][-1].sum().item()), launch_shape=list(engine.flux_launch_shape(w.n_modes)))
        # the launch that reads hdot alone (energy and momentum: one row and one coefficient set instead of two and three)
        engine.poincare_fluxes(None, None, wd._dev, ELL_MIN, ell_max, want=("energy", "momentum"), ctx=ctx)
        out.update(hdot_only_ms=ctx.get_timing(reset=True)["pointwise"][0])
    elif kind.startswith("fused"):
        flux.poincare_fluxes(w, wd if given else None)  # warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        res = flux.poincare_fluxes(w, wd if given else None)
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(res[3][-1].sum()), resident=bool(w.is_device_resident and wd.is_device_resident))
    else:
        small, small_d = w[:1000], wd[:1000]
        flux.host_poincare_fluxes(small, small_d if given else None)  # warm-up of the kernels, the copy path and numpy on a short piece
        ctx.synchronize()
        t0 = time.perf_counter()
        res = flux.host_poincare_fluxes(w, wd if given else None)
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(res[3][-1].sum()), resident=bool(w.is_device_resident))
    ctx.close()
    print(json.dumps(out))


def main():
    import statistics

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
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
    summary["kernel_hdot_only_median_ms"] = round(statistics.median(r["hdot_only_ms"] for r in runs["kernel"]), 4)
    kernel_bytes = 2 * n * n_modes * 16 + 80 * n
    rate = kernel_bytes / (summary["kernel_median_ms"] * 1e-3)
    summary.update(kernel_bytes=kernel_bytes, kernel_TB_per_s=round(rate / 1e12, 3), kernel_share_of_hbm=round(rate / HBM_BYTES_PER_S, 3),
                   parent_over_fused=round(summary["parent_median_ms"] / summary["fused_median_ms"], 1),
                   parent_given_over_fused_given=round(summary["parent_given_median_ms"] / summary["fused_given_median_ms"], 1))
    summary["checksums"] = {kind: runs[kind][0]["checksum"] for kind in KINDS}
    summary["fused_stays_resident"] = all(r["resident"] for r in runs["fused"] + runs["fused_given"])
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "--step":
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
