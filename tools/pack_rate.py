"""Rate of the corotating paired-XOR storage form (scri_amd/corotating_paired_xor.py) at 1e5 time steps, l = 2..16 (285 modes), on a
device-resident Corotating waveform ("Storage form"):

  fused   `pack(w, log_frame=...)`: one kernel over the modes where they live (the packed modes stay in HBM; `fused_to_host_ms` adds
          reading them to the host, which is where the chain's result ends up)
  chain   the same words composed from the public calls that exist without it: copy, convert_to_conjugate_pairs, truncate, + 0.0,
          xor_timeseries on the modes, the time and the log frame (no checksums: `pack` computes three, the chain is spared them)
  kernels the pack and unpack kernels alone (HIP events of the context), as algorithmic bytes -- 2 x 16 n n_modes, plus one halo row per
          tile of the pack kernel -- per second and as a fraction of 8 TB/s of HBM

Every timed run is a process of its own with a time limit, one at a time, fused and chain alternating, `reps` of each; a run that fails or
exceeds its limit ends the measurement there.  Usage: python tools/pack_rate.py [n_times] [reps]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ELL_MIN, ELL_MAX, TOL = 2, 16, 1e-10
STEP_LIMIT_S = 240


def _waveform(n):
    import numpy as np

    import scri_amd

    n_modes = (ELL_MAX + 1) ** 2 - ELL_MIN**2
    rng = np.random.default_rng(3)
    t = np.linspace(0.0, 1000.0, n)
    a = rng.normal(size=(2, n_modes)) + 1j * rng.normal(size=(2, n_modes))
    omega = rng.uniform(0.01, 0.3, size=n_modes)
    data = a[0] * np.exp(1j * np.outer(t, omega)) + a[1]
    log_frame = np.stack([0.3 * np.sin(0.01 * t), -0.002 * t, 0.05 * t], axis=1)
    ctx = scri_amd.Context(0)
    w = scri_amd.WaveformModes(t=t, data=data, ell_min=ELL_MIN, ell_max=ELL_MAX, frameType=scri_amd.Corotating, dataType=scri_amd.h,
                               r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx).to_device()
    return ctx, w, log_frame


def _chain(w, log_frame):
    from scri_amd import utilities

    c = w.copy()
    c.convert_to_conjugate_pairs()
    c.truncate(tol=TOL)
    t, lf = c.t + 0.0, log_frame + 0.0
    c.data += 0.0
    utilities.xor_timeseries(t, ctx=c._ctx)
    utilities.xor_timeseries(c.data, ctx=c._ctx)
    utilities.xor_timeseries(lf, ctx=c._ctx)
    return t, c.data, lf


def _step(kind, n):
    import numpy as np

    from scri_amd import corotating_paired_xor as cpx

    ctx, w, log_frame = _waveform(n)
    out = {"step": kind, "n_times": n, "n_modes": w.n_modes}
    if kind == "fused":
        cpx.pack(w, L2norm_fractional_tolerance=TOL, log_frame=log_frame).modes  # warm-up: allocations, first launch
        ctx.synchronize()
        t0 = time.perf_counter()
        packed = cpx.pack(w, L2norm_fractional_tolerance=TOL, log_frame=log_frame)
        ctx.synchronize()
        t1 = time.perf_counter()
        words = packed.modes
        t2 = time.perf_counter()
        out.update(fused_ms=(t1 - t0) * 1e3, fused_to_host_ms=(t2 - t0) * 1e3, modes_fletcher32=packed.json_data["validation"]["fletcher32"]["modes"])
        del words
    elif kind == "chain":
        _chain(w, log_frame)
        ctx.synchronize()
        t0 = time.perf_counter()
        _, data, _ = _chain(w, log_frame)
        ctx.synchronize()
        out.update(chain_ms=(time.perf_counter() - t0) * 1e3)
        del data
    else:  # the two kernels alone
        reps = 10
        packed = cpx.pack(w, L2norm_fractional_tolerance=TOL, log_frame=log_frame)
        cpx.unpack(packed)
        ctx.synchronize()
        from scri_amd import engine

        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        for _ in range(reps):
            engine.pack_paired_xor(w._dev, ELL_MIN, ELL_MAX, TOL, ctx=ctx)
        pack_ms = ctx.get_timing(reset=True)["pointwise"][0] / reps
        for _ in range(reps):
            engine.unpack_paired_xor(packed.modes_device, ELL_MIN, ELL_MAX, ctx=ctx)
        unpack_ms = ctx.get_timing(reset=True)["pointwise"][0] / reps
        ctx.enable_timing(False)
        tiles = -(-n // cpx.TILE_ROWS)
        pack_bytes = 2 * 16 * n * w.n_modes + 16 * w.n_modes * (tiles - 1)
        unpack_bytes = 3 * 16 * n * w.n_modes  # the words are read twice (tile totals, then the running XOR), the modes written once
        out.update(pack_kernel_ms=pack_ms, pack_bytes=pack_bytes, pack_GBps=pack_bytes / pack_ms / 1e6, pack_hbm_fraction=pack_bytes / pack_ms / 1e6 / 8000.0,
                   unpack_kernels_ms=unpack_ms, unpack_bytes=unpack_bytes, unpack_GBps=unpack_bytes / unpack_ms / 1e6,
                   unpack_hbm_fraction=unpack_bytes / unpack_ms / 1e6 / 8000.0)
        back = cpx.unpack(packed)
        err = np.linalg.norm(back.data - w.data, axis=1) / np.linalg.norm(w.data, axis=1)
        out.update(round_trip_max_over_tol=float(err.max() / TOL))
    ctx.close()
    print(json.dumps(out))


def main():
    import statistics

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    runs = {"fused": [], "chain": [], "kernels": []}
    for kind in ["kernels"] + ["fused", "chain"] * reps:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n)], capture_output=True, text=True, timeout=STEP_LIMIT_S)
        if done.returncode != 0:
            sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
            raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
        line = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(line), file=sys.stderr, flush=True)
        runs[kind].append(line)
    fused = [r["fused_ms"] for r in runs["fused"]]
    fused_host = [r["fused_to_host_ms"] for r in runs["fused"]]
    chain = [r["chain_ms"] for r in runs["chain"]]
    spread = max(chain) - min(chain)
    summary = {
        "n_times": n, "n_modes": runs["kernels"][0]["n_modes"], "reps": reps,
        "fused_median_ms": round(statistics.median(fused), 3), "fused_to_host_median_ms": round(statistics.median(fused_host), 3),
        "chain_median_ms": round(statistics.median(chain), 3), "chain_spread_ms": round(spread, 3),
        "fused_ms": [round(v, 3) for v in fused], "fused_to_host_ms": [round(v, 3) for v in fused_host], "chain_ms": [round(v, 3) for v in chain],
        "gain_over_four_spreads": bool(statistics.median(chain) - statistics.median(fused_host) > 4 * spread),
    }
    summary.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in runs["kernels"][0].items() if k not in ("step", "n_times", "n_modes")})
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--step":
        _step(sys.argv[2], int(sys.argv[3]))
    else:
        main()
