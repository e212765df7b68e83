"""Time of the mass aspect and the supermomenta of a device-resident AsymptoticBondiData of 1e5 time steps at l_max = 16 (289 modes) or
24 (625) ("Products on Gauss-Legendre rows"):

  moreschi, mass_aspect, supermomenta    `abd.supermomentum("Moreschi")`, `abd.mass_aspect()` and `abd.supermomenta()` of the resident
                                         object: one spline derivative of sigma in HBM and one bms_supermomenta launch
  parent_moreschi, parent_mass_aspect,   the same calls in a checkout of the parent commit with its own library built (`--parent DIR`),
  parent_supermomenta                    where they go through bms_grid_multiply (`supermomenta` there: the four supermomentum calls)
  kernel                                 the product kernel alone by HIP events (the context's timing of its one launch), all five outputs,
                                         device tensors in and out; beside it the launch for the Moreschi supermomentum alone
  sample, parent_sample                  not timed: the Moreschi supermomentum and the mass aspect of both builds on every
                                         `n_times / 100`-th step; the largest difference relative to the scale is reported

Every timed run is a process of its own with a time limit, one at a time, the kinds alternating (so the two builds alternate), one
warm-up and `reps` runs of each; a run that fails or exceeds its limit ends the measurement there.  The kernel's share of the HBM rate
is over its own bytes, (3 inputs + outputs) 16 N n_modes.  The condition is DESIGN section 9's: a gain counts if the parent's median
exceeds the new median by more than four of the parent's spreads (max - min).
Usage: python tools/product_rate.py [n_times] [reps] [ell_max] [--parent DIR]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 400
CALLS = ("moreschi", "mass_aspect", "supermomenta")
HBM_BYTES_PER_S = 8e12  # the peak DESIGN section 4 quotes its fractions against
SAMPLES = 100


def _abd(n, ell_max):
    import numpy as np

    import scri_amd
    from scri_amd import synthetic

    t = np.linspace(0.0, 1000.0, n) + 0.003 * np.cos(np.arange(n))
    ctx = scri_amd.Context(0)
    abd = scri_amd.AsymptoticBondiData(t, ell_max, ctx=ctx)
    for f, s in enumerate(synthetic.ABD_SPINS):
        if f in (2, 5):  # psi2, sigma: what the mass aspect and the supermomenta read
            abd._raw_data[f] = 0.3 * synthetic.chirp_modes(t, 0, ell_max, 120 + f) * (1 + 0.0004 * t[:, None])
            abd._raw_data[f, :, : s * s] = 0
    return ctx, abd.to_device()


def _call(name, abd):
    if name == "moreschi":
        return abd.supermomentum("Moreschi")
    if name == "mass_aspect":
        return abd.mass_aspect()
    if hasattr(abd, "supermomenta"):
        return abd.supermomenta()
    return tuple(abd.supermomentum(k) for k in ("Bondi-Sachs", "Moreschi", "Geroch", "Geroch-Winicour"))


def _step(kind, n, ell_max, scratch):
    import numpy as np

    ctx, abd = _abd(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": abd.n_modes}
    name = kind[7:] if kind.startswith("parent_") else kind
    if kind == "kernel":
        from scri_amd import engine

        raw = abd._raw_dev
        sigma_dot = engine.spline_derivative(abd.t, raw[5], abd.t, 1, ctx=ctx)
        engine.supermomenta(raw[2], raw[5], sigma_dot, ell_max, ctx=ctx)  # warm-up: the tables, the first launch
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        res = engine.supermomenta(raw[2], raw[5], sigma_dot, ell_max, ctx=ctx)
        ms, launches = ctx.get_timing(reset=True)["pointwise"]
        assert launches == 1
        out.update(ms=ms, checksum=float(res[1][-1].sum().real.item()), launch_shape=list(engine.product_launch_shape(ell_max, ell_max, ell_max)),
                   n_nodes=engine.product_nodes(ell_max, ell_max, ell_max))
        del res
        engine.supermomenta(raw[2], raw[5], sigma_dot, ell_max, want="moreschi", ctx=ctx)
        out.update(one_output_ms=ctx.get_timing(reset=True)["pointwise"][0])
    elif name == "sample":
        rows = np.arange(0, n, max(n // SAMPLES, 1))
        psi_m, mass = _call("moreschi", abd), _call("mass_aspect", abd)
        np.savez(os.path.join(scratch, kind + ".npz"), moreschi=psi_m.rows(0, n)[rows], mass_aspect=mass.rows(0, n)[rows])
        out.update(ms=0.0, checksum=0.0)
    else:
        _call(name, abd[:1000])  # warm-up of the kernels and the copy paths on a short piece
        _call(name, abd)         # ... and of the buffers of the full size
        ctx.synchronize()
        t0 = time.perf_counter()
        res = _call(name, abd)
        ctx.synchronize()
        last = res[1] if isinstance(res, tuple) else res
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(last.rows(n - 1, n).sum().real), resident=bool(abd.is_device_resident))
    ctx.close()
    print(json.dumps(out))


def _compare(scratch):
    import numpy as np

    new, old = np.load(os.path.join(scratch, "sample.npz")), np.load(os.path.join(scratch, "parent_sample.npz"))
    return {k: {"largest_difference": float(np.abs(new[k] - old[k]).max()), "scale": float(np.abs(old[k]).max())} for k in ("moreschi", "mass_aspect")}


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
    summary["kernel_one_output_median_ms"] = round(statistics.median(r["one_output_ms"] for r in runs["kernel"]), 4)
    for key, outputs_written in (("kernel", 5), ("kernel_one_output", 1)):
        nbytes = (3 + outputs_written) * 16 * n * n_modes
        rate = nbytes / (summary[f"{key}_median_ms"] * 1e-3)
        summary.update({f"{key}_bytes": nbytes, f"{key}_TB_per_s": round(rate / 1e12, 3), f"{key}_share_of_hbm": round(rate / HBM_BYTES_PER_S, 3)})
    summary["stays_resident"] = all(r["resident"] for k in CALLS for r in runs[k])
    if parent:
        for k in CALLS:
            gain = summary[f"parent_{k}_median_ms"] - summary[f"{k}_median_ms"]
            summary[f"parent_over_new_{k}"] = round(summary[f"parent_{k}_median_ms"] / summary[f"{k}_median_ms"], 1)
            summary[f"{k}_gain_over_four_parent_spreads"] = bool(gain > 4 * summary[f"parent_{k}_spread_ms"])
        summary["outputs"] = outputs
    print(json.dumps(summary))


if __name__ == "__main__":
    if len(sys.argv) >= 7 and sys.argv[1] == "--step":
        sys.path.insert(0, sys.argv[5])  # the checkout whose package this run measures
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[6])
    else:
        main()
