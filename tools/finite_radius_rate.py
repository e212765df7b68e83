"""Time of the retardation of raw finite-radius series ("Retardation"): 24 radii of 1e5 steps and 77 modes (l = 2..8),
device resident, each on a time axis with three restarts.

  engine   24 calls of `engine.finite_radius_retard` on device tensors, the rows left in HBM (each call ends in its one wait)
  numpy    the statements of tests/helpers/finite_radius_ref.py (numpy's cumsum) on ONE radius in host memory, on that host
  trace    one `rocprofv3 --kernel-trace --stats` run of the engine step of its own: the lines of its kernel statistics that name the
           kernels of kernels_retard.hip, as the tool prints them

Every timed run is a process of its own with a time limit, one at a time, after a warm-up call inside it; a run that fails or exceeds
its limit ends the measurement there.  A record, not a bar: the parent has no such call and no share of the HBM rate is promised.
Usage: python tools/finite_radius_rate.py [n_times] [reps] [--trace DIR]        (prints one JSON line)"""
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_RADII, N_MODES = 24, 77
STEP_LIMIT_S = 240


def _series(n, i):
    import numpy as np

    rng = np.random.default_rng(3340 + i)
    t = np.cumsum(rng.uniform(0.05, 0.15, n))
    for k in (n // 5, n // 2, (4 * n) // 5):  # three restarts of about 200 samples each
        t[k:] -= t[k] - t[max(k - 200, 0)]
    R = (100.0 + 20.0 * i) * (1.0 + 1e-3 * np.sin(0.01 * t))
    lapse = 0.99 * (1.0 + 1e-3 * np.cos(0.013 * t))
    return t, R, lapse, 100.0 + 20.0 * i - 1.0


def _step(kind, n):
    import numpy as np

    out = {"step": kind, "n_times": n, "n_modes": N_MODES, "n_radii": N_RADII}
    rng = np.random.default_rng(3339)
    data = rng.normal(size=(n, N_MODES)) + 1j * rng.normal(size=(n, N_MODES))
    if kind == "engine":
        import torch

        import scri_amd
        from scri_amd import device_series, engine

        ctx = scri_amd.Context(0)
        dev = device_series.attach(ctx)
        series = [_series(n, i) for i in range(N_RADII)]
        sources = [torch.from_numpy(data).to(dev) * (1.0 + i) for i in range(N_RADII)]
        outs = [torch.empty_like(s) for s in sources]
        call = lambda i: engine.finite_radius_retard(*series[i][:3], sources[i], series[i][3], 0.99, 0.98, 1.0 / 0.98, 1, out=outs[i], ctx=ctx)  # noqa: E731
        call(0)  # warm-up: allocations, first launches
        ctx.synchronize()
        t0 = time.perf_counter()
        kept = [call(i)[0].size for i in range(N_RADII)]
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        moved = sum(2 * 16 * k * N_MODES for k in kept)
        out.update(ms=ms, kept=kept[0], gather_bytes=moved, checksum=float(outs[-1][: kept[-1]].real.sum().item()))
        ctx.close()
    else:
        from tests.helpers import finite_radius_ref as ref

        t, R, lapse, coord = _series(n, 0)
        ref.retard(t[:1000], R[:1000], lapse[:1000], data[:1000], coord, 0.99, 0.98, "h", exact=False)
        t0 = time.perf_counter()
        y = ref.retard(t, R, lapse, data, coord, 0.99, 0.98, "h", exact=False)
        out.update(ms=(time.perf_counter() - t0) * 1e3, kept=int(y["idx"].size), checksum=float(y["data"].real.sum()))
    print(json.dumps(out))


def _run(kind, n, prefix=()):
    done = subprocess.run([*prefix, sys.executable, os.path.abspath(__file__), "--step", kind, str(n)], capture_output=True, text=True,
                          timeout=STEP_LIMIT_S)
    if done.returncode != 0:
        sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
        raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
    return json.loads([l for l in done.stdout.strip().splitlines() if l.startswith("{")][-1])


def main():
    import statistics

    args = [a for a in sys.argv[1:]]
    trace_dir = None
    if "--trace" in args:
        trace_dir = args[args.index("--trace") + 1]
        del args[args.index("--trace"): args.index("--trace") + 2]
    n = int(args[0]) if args else 100000
    reps = int(args[1]) if len(args) > 1 else 7
    summary = {"n_times": n, "n_modes": N_MODES, "n_radii": N_RADII, "reps": reps}
    for kind in ("engine", "numpy"):
        runs = []
        for _ in range(reps):
            runs.append(_run(kind, n))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        ms = [r["ms"] for r in runs]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 3), f"{kind}_spread_ms": round(max(ms) - min(ms), 3),
                        f"{kind}_ms": [round(v, 3) for v in ms], f"{kind}_kept": runs[0]["kept"]})
        if kind == "engine":
            summary["gather_bytes"] = runs[0]["gather_bytes"]
    summary["numpy_is_one_radius"] = True
    if trace_dir:
        _run("engine", n, prefix=("rocprofv3", "--kernel-trace", "--stats", "-d", trace_dir, "--output-format", "csv", "--"))
        lines = []
        for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True)):
            with open(path) as f:
                rows = f.read().splitlines()
            lines += rows[:1] + [r for r in rows[1:] if "retard_" in r]
        summary["kernel_stats"] = lines
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        _step(sys.argv[2], int(sys.argv[3]))
    else:
        main()
