"""Time of AsymptoticBondiData.from_initial_values on a shear series of 1e5 time steps at l_max = 16 (289 modes) (DESIGN section 4,
"Initial values"):

  resident    a shear resident in HBM in, a device-resident object out: two spline derivatives, the head launch of bms_bianchi_rhs, then
              twice a stage launch, with a spline integral after each of the three; one row comes to the host
  host        the host route on the same shear as a numpy array -- the statements of the parent commit, which this build keeps bit for
              bit for such an input -- and the `.to_device()` a caller who goes on in HBM then needs: three bms_grid_multiply calls on the
              (4 l_max + 1)^2 grid, host in and host out, numpy's eth and bar, five spline calls, one upload of [6, N, n_modes].
              `--parent DIR` takes the package of a checkout of the parent commit, with its own library built, for these runs
  sample      not timed: the six fields of both routes on every `n_times / 100`-th step; the largest difference relative to the scale

Every timed run is a process of its own with a time limit, one at a time, the two kinds alternating, one warm-up inside each process and
`reps` runs of each kind; a run that fails or exceeds its limit ends the measurement there.
Usage: python tools/ivp_rate.py [n_times] [reps] [ell_max] [--parent DIR]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 400
KINDS = ("resident", "host")
SAMPLES = 100


def _shear(n, ell_max):
    import numpy as np

    import scri_amd
    from scri_amd import synthetic

    t = np.linspace(0.0, 1000.0, n) + 0.003 * np.cos(np.arange(n))
    ctx = scri_amd.Context(0)
    sigma = 0.01 * synthetic.chirp_modes(t, 0, ell_max, 120) * (1 + 0.0004 * t[:, None])
    sigma[:, :4] = 0
    rng = np.random.default_rng(7)
    nm = (ell_max + 1) ** 2
    rows = [0.1 * (rng.normal(size=nm) + 1j * rng.normal(size=nm)) for _ in range(3)]
    return ctx, t, np.ascontiguousarray(sigma), rows


def _build(kind, ctx, t, sigma, rows, ell_max):
    import scri_amd

    psi2, psi1, psi0 = rows
    abd = scri_amd.AsymptoticBondiData.from_initial_values(t, ell_max, sigma0=sigma, psi2=psi2, psi1=psi1, psi0=psi0, ctx=ctx)
    return abd if kind == "resident" else abd.to_device()


def _step(kind, n, ell_max, scratch):
    import numpy as np

    from scri_amd import device_series

    ctx, t, sigma, rows = _shear(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": (ell_max + 1) ** 2}
    name = kind[7:] if kind.startswith("sample_") else kind
    given = device_series.to_device(ctx, sigma) if name == "resident" else sigma
    short = min(n, 1000)
    _build(name, ctx, t[:short], given[:short], rows, ell_max)  # warm-up of the kernels and the copy paths on a short piece
    if kind.startswith("sample_"):
        abd = _build(name, ctx, t, given, rows, ell_max)
        np.save(os.path.join(scratch, name + ".npy"), device_series.to_host(abd._raw_dev[:, :: max(n // SAMPLES, 1)]))
        out.update(ms=0.0)
    else:
        _build(name, ctx, t, given, rows, ell_max)  # ... and of the buffers of the full size
        ctx.synchronize()
        t0 = time.perf_counter()
        abd = _build(name, ctx, t, given, rows, ell_max)
        ctx.synchronize()
        out.update(ms=(time.perf_counter() - t0) * 1e3, resident=bool(abd.is_device_resident),
                   checksum=float(device_series.to_host(abd._raw_dev[0, n - 1:]).sum().real))
    ctx.close()
    print(json.dumps(out))


def _compare(scratch):
    import numpy as np

    new, old = np.load(os.path.join(scratch, "resident.npy")), np.load(os.path.join(scratch, "host.npy"))
    return {"largest_difference": [float(np.abs(new[f] - old[f]).max() / max(1.0, np.abs(old[f]).max())) for f in range(6)]}


def main():
    import statistics

    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        parent = os.path.abspath(args[args.index("--parent") + 1])
        del args[args.index("--parent"):args.index("--parent") + 2]
    n = int(args[0]) if len(args) > 0 else 100000
    reps = int(args[1]) if len(args) > 1 else 7
    ell_max = int(args[2]) if len(args) > 2 else 16
    order = list(KINDS) * reps + ["sample_resident", "sample_host"]
    runs = {k: [] for k in order}
    with tempfile.TemporaryDirectory() as scratch:
        for kind in order:
            root = parent if parent and kind.endswith("host") else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n), str(ell_max), root, scratch], capture_output=True,
                                  text=True, timeout=STEP_LIMIT_S, cwd=root)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
            line = json.loads(done.stdout.strip().splitlines()[-1])
            print(json.dumps(line), file=sys.stderr, flush=True)
            runs[kind].append(line)
        outputs = _compare(scratch)
    summary = {"n_times": n, "ell_max": ell_max, "n_modes": (ell_max + 1) ** 2, "reps": reps, "host_route_of": parent or "this build"}
    for kind in KINDS:
        ms = [r["ms"] for r in runs[kind]]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 3), f"{kind}_spread_ms": round(max(ms) - min(ms), 3),
                        f"{kind}_ms": [round(v, 3) for v in ms]})
    summary["stays_resident"] = all(r["resident"] for k in KINDS for r in runs[k])
    summary["host_over_resident"] = round(summary["host_median_ms"] / summary["resident_median_ms"], 1)
    summary["separated"] = bool(max(summary["resident_ms"]) < min(summary["host_ms"]))
    summary["outputs"] = outputs
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 7 and sys.argv[1] == "--step":
        sys.path.insert(0, sys.argv[5])  # the checkout whose package this run measures
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[6])
    else:
        main()
