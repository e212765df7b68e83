"""Time of the Bondi-gauge violations and their norms of a device-resident AsymptoticBondiData of 1e5 time steps at l_max = 16 (289 modes)
or 24 (625) ("Constraints"):

  norms, violations                  `abd.bondi_gauge_check(violations=False)` and `(norms=False)` of the resident object: five spline
                                     derivatives in HBM and one bms_bondi_constraints launch; the norms alone come to the host (what the two
                                     properties of this build call for such an object)
  parent_norms, parent_violations    `abd.bondi_violation_norms` and `abd.bondi_violations` in a checkout of the parent commit with its own
                                     library built (`--parent DIR`): spline derivatives, mode maps, four bms_grid_multiply calls and, for
                                     the norms, numpy's norm of six arrays brought to the host
  kernel                             the constraint kernel alone by HIP events (the context's timing of its one launch): all six
                                     violations and the norms, device tensors in and out; beside it the norms-only launch
  sample, parent_sample              not timed: the six norms of both builds on every `n_times / 100`-th step; the largest difference
                                     relative to the scale is reported

Every timed run is a process of its own with a time limit, one at a time, the kinds alternating (so the two builds alternate), one
warm-up and `reps` runs of each; a run that fails or exceeds its limit ends the measurement there.  The kernel's share of the HBM rate
is over its own bytes, (10 inputs + 6 outputs) 16 N n_modes.  The condition for the two properties to take the new route: the runs of the two
builds are SEPARATED, the slowest new run quicker than the quickest parent run, for both properties.
Usage: python tools/constraint_rate.py [n_times] [reps] [ell_max] [--parent DIR]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 400
CALLS = ("norms", "violations")
HBM_BYTES_PER_S = 8e12  # the peak DESIGN section 4 quotes its fractions against
SAMPLES = 100


def _abd(n, ell_max):
    import numpy as np

    import scri_amd
    from scri_amd import synthetic

    t = np.linspace(0.0, 1000.0, n) + 0.003 * np.cos(np.arange(n))
    ctx = scri_amd.Context(0)
    abd = scri_amd.AsymptoticBondiData(t, ell_max, multiplication_truncator=max, ctx=ctx)
    base = 0.3 * synthetic.chirp_modes(t, 0, ell_max, 120) * (1 + 0.0004 * t[:, None])
    for f, s in enumerate(synthetic.ABD_SPINS):  # one chirp, another weight and phase for each field: the time does not depend on the values
        abd._raw_data[f] = base * ((0.5 + 0.1 * f) * np.exp(0.7j * f))
        abd._raw_data[f, :, : s * s] = 0
    return ctx, abd.to_device()


def _call(name, abd):
    if hasattr(abd, "bondi_gauge_check"):  # this build: the one-launch route
        return abd.bondi_gauge_check(violations=False)[1] if name == "norms" else abd.bondi_gauge_check(norms=False)[0]
    return abd.bondi_violation_norms if name == "norms" else abd.bondi_violations


def _step(kind, n, ell_max, scratch):
    import numpy as np

    ctx, abd = _abd(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": abd.n_modes}
    name = kind[7:] if kind.startswith("parent_") else kind
    if kind == "kernel":
        from scri_amd import engine

        raw, t = abd._raw_dev, abd.t
        d = lambda x, order: engine.spline_derivative(t, x, t, order, ctx=ctx)  # noqa: E731
        rows = (raw, [d(raw[0], 1), d(raw[1], 1), d(raw[2], 1)], d(raw[5], 1), d(raw[5], 2))
        engine.bondi_constraints(*rows, ell_max, ctx=ctx)  # warm-up: the tables, the first launch
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        res, norms = engine.bondi_constraints(*rows, ell_max, ctx=ctx)
        ms, launches = ctx.get_timing(reset=True)["constraints"]
        assert launches == 1
        out.update(ms=ms, checksum=float(norms[-1].sum()), launch_shape=list(engine.product_launch_shape(ell_max, ell_max, ell_max)),
                   n_nodes=engine.product_nodes(ell_max, ell_max, ell_max))
        del res
        engine.bondi_constraints(*rows, ell_max, want=(), ctx=ctx)
        out.update(norms_only_ms=ctx.get_timing(reset=True)["constraints"][0])
    elif name == "sample":
        rows = np.arange(0, n, max(n // SAMPLES, 1))
        np.savez(os.path.join(scratch, kind + ".npz"), norms=np.array(_call("norms", abd))[:, rows])
        out.update(ms=0.0, checksum=0.0)
    else:
        _call(name, abd[:1000])  # warm-up of the kernels and the copy paths on a short piece
        _call(name, abd)         # ... and of the buffers of the full size
        ctx.synchronize()
        t0 = time.perf_counter()
        res = _call(name, abd)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        last = res[-1]
        out.update(ms=ms, checksum=float(last[-1]) if name == "norms" else float(last.rows(n - 1, n).sum().real), resident=bool(abd.is_device_resident))
    ctx.close()
    print(json.dumps(out))


def _compare(scratch):
    import numpy as np

    new, old = np.load(os.path.join(scratch, "sample.npz"))["norms"], np.load(os.path.join(scratch, "parent_sample.npz"))["norms"]
    return {"largest_difference_of_the_norms": [float(v) for v in np.abs(new - old).max(axis=1)], "scale": [float(v) for v in np.abs(old).max(axis=1)]}


def main():
    import statistics

    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        parent = os.path.abspath(args[args.index("--parent") + 1])
        del args[args.index("--parent"):args.index("--parent") + 2]
    n = int(args[0]) if len(args) > 0 else 100000
    reps = int(args[1]) if len(args) > 1 else 3
    ell_max = int(args[2]) if len(args) > 2 else 16
    new_kinds = CALLS + ("kernel",)
    parent_kinds = tuple("parent_" + k for k in CALLS) if parent else ()
    order = []
    for k in CALLS:  # new and parent runs of one call side by side
        order += [k] + (["parent_" + k] if parent else [])
    order = (order + ["kernel"]) * reps + (["sample", "parent_sample"] if parent else [])
    runs = {k: [] for k in new_kinds + parent_kinds + ("sample", "parent_sample")}
    with tempfile.TemporaryDirectory() as scratch:
        for kind in order:
            root = parent if kind.startswith("parent_") else HERE
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, str(n), str(ell_max), root, scratch], capture_output=True,
                                  text=True, timeout=STEP_LIMIT_S, cwd=root)
            if done.returncode != 0:
                sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                raise SystemExit(f"step {kind} ended with status {done.returncode}: nothing further is started")
            line = json.loads(done.stdout.strip().splitlines()[-1])
            print(json.dumps(line), file=sys.stderr, flush=True)
            runs[kind].append(line)
        outputs = _compare(scratch) if parent else None
    k0 = runs["kernel"][0]
    n_modes = k0["n_modes"]
    summary = {"n_times": n, "ell_max": ell_max, "n_modes": n_modes, "n_nodes": k0["n_nodes"], "reps": reps, "launch_shape": k0["launch_shape"]}
    for kind in new_kinds + parent_kinds:
        ms = [r["ms"] for r in runs[kind]]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 4), f"{kind}_spread_ms": round(max(ms) - min(ms), 4),
                        f"{kind}_ms": [round(v, 4) for v in ms]})
    summary["kernel_norms_only_median_ms"] = round(statistics.median(r["norms_only_ms"] for r in runs["kernel"]), 4)
    for key, outputs_written in (("kernel", 6), ("kernel_norms_only", 0)):
        nbytes = (10 + outputs_written) * 16 * n * n_modes
        rate = nbytes / (summary[f"{key}_median_ms"] * 1e-3)
        summary.update({f"{key}_bytes": nbytes, f"{key}_TB_per_s": round(rate / 1e12, 3), f"{key}_share_of_hbm": round(rate / HBM_BYTES_PER_S, 3)})
    summary["stays_resident"] = all(r["resident"] for k in CALLS for r in runs[k])
    if parent:
        for k in CALLS:
            summary[f"parent_over_new_{k}"] = round(summary[f"parent_{k}_median_ms"] / summary[f"{k}_median_ms"], 1)
            summary[f"{k}_separated"] = bool(max(summary[f"{k}_ms"]) < min(summary[f"parent_{k}_ms"]))
        summary["outputs"] = outputs
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 7 and sys.argv[1] == "--step":
        sys.path.insert(0, sys.argv[5])  # the checkout whose package this run measures
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[6])
    else:
        main()
