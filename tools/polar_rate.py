"""Time of amplitude and unwrapped phase of a device-resident series of 1e5 time steps, l = 2..16 (285 modes) (DESIGN section 9,
"Polar form"):

  engine    `engine.abs_arg(w._dev, unwrap=True)`: both results computed and left in HBM
  property  `w.arg_unwrapped` of the resident waveform: the kernels plus reading the float64 result back to the host
  parent    the route the same call took before the kernels existed: `w.data` read back to the host, then
            `np.unwrap(np.angle(data), axis=0)` there (the waveform ends up host-resident)

Every timed run is a process of its own with a time limit, one at a time, the three alternating, `reps` of each; a run that fails or
exceeds its limit ends the measurement there.  A record, not a bar: no share of the HBM rate is claimed.
Usage: python tools/polar_rate.py [n_times] [reps]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELL_MIN, ELL_MAX = 2, 16
STEP_LIMIT_S = 240
KINDS = ("engine", "property", "parent")


def _waveform(n):
    import numpy as np

    import scri_amd

    n_modes = (ELL_MAX + 1) ** 2 - ELL_MIN**2
    rng = np.random.default_rng(3)
    t = np.linspace(0.0, 1000.0, n)
    a = rng.normal(size=n_modes) + 1j * rng.normal(size=n_modes)
    omega = rng.uniform(-2.0, 2.0, size=n_modes) / (t[1] - t[0])  # steps of up to 2 rad: every column wraps, hundreds of times
    data = a * np.exp(1j * np.outer(t, omega)) * (1.0 + 0.2 * np.sin(0.01 * t))[:, None]
    ctx = scri_amd.Context(0)
    w = scri_amd.WaveformModes(t=t, data=data, ell_min=ELL_MIN, ell_max=ELL_MAX, frameType=scri_amd.Inertial, dataType=scri_amd.h,
                               r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx).to_device()
    return ctx, w


def _step(kind, n):
    import numpy as np

    from scri_amd import engine

    ctx, w = _waveform(n)
    out = {"step": kind, "n_times": n, "n_modes": w.n_modes}
    if kind == "engine":
        engine.abs_arg(w._dev, unwrap=True, ctx=ctx)  # warm-up: allocations, first launch
        ctx.synchronize()
        t0 = time.perf_counter()
        a, p = engine.abs_arg(w._dev, unwrap=True, ctx=ctx)
        ctx.synchronize()
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(p[-1].sum().item()))
    elif kind == "property":
        w.arg_unwrapped
        t0 = time.perf_counter()
        p = w.arg_unwrapped
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(p[-1].sum()), resident=bool(w.is_device_resident))
    else:
        dev = w._dev
        np.unwrap(np.angle(dev[:1000].cpu().numpy()), axis=0)  # warm-up of the copy path and of numpy
        t0 = time.perf_counter()
        p = np.unwrap(np.angle(dev.cpu().numpy()), axis=0)
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(p[-1].sum()))
    ctx.close()
    print(json.dumps(out))


def main():
    import statistics

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    runs = {k: [] for k in KINDS}
    for kind in list(KINDS) * reps:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(line), file=sys.stderr, flush=True)
        runs[kind].append(line)
    summary = {"n_times": n, "n_modes": runs["engine"][0]["n_modes"], "reps": reps}
    for kind in KINDS:
        ms = [r["ms"] for r in runs[kind]]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 3), f"{kind}_spread_ms": round(max(ms) - min(ms), 3),
                        f"{kind}_ms": [round(v, 3) for v in ms]})
    summary["checksums"] = {kind: runs[kind][0]["checksum"] for kind in KINDS}
    summary["property_stays_resident"] = all(r["resident"] for r in runs["property"])
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        _step(sys.argv[2], int(sys.argv[3]))
    else:
        main()
