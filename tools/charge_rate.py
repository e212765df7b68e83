"""Time of the Bondi charges of a device-resident AsymptoticBondiData of 1e5 time steps at l_max = 16 (289 modes) or 24 (625)
("Charges"):

  spin, com, charges                     `abd.bondi_dimensionless_spin()`, `abd.bondi_CoM_charge()` and `abd.bondi_charges()` of the resident
                                         object: at most one spline derivative of sigma in HBM and one bms_bondi_charges launch
  parent_spin, parent_com, parent_charges   the same calls in a checkout of the parent commit with its own library built (`--parent DIR`),
                                         where they go through bms_grid_multiply (`charges` there: the four single methods)
  kernel                                 the charge kernel alone by HIP events (the context's timing of its one launch), all four charges,
                                         device tensors in and out; beside it the launch for J and G alone (one row, no sigma_dot)
  sample, parent_sample                  not timed: the four charges of both builds on every `n_times / 100`-th step, held against the
                                         long-double yardstick of tests/helpers/charge_cases.py there:
                                         |new - parent| <= bar + the parent's own distance from the yardstick

Every timed run is a process of its own with a time limit, one at a time, the kinds alternating (so the two builds alternate), one
warm-up and `reps` runs of each; a run that fails or exceeds its limit ends the measurement there.  The kernel's share of the HBM rate
is over its own bytes, 2 N n_modes 16 + 104 N.  The condition is separation: the slowest new run of a call against the quickest parent run.
Usage: python tools/charge_rate.py [n_times] [reps] [ell_max] [--parent DIR]        (prints one JSON line)"""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 400
CALLS = ("spin", "com", "charges")
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
        if f in (1, 2, 5):  # psi1, psi2, sigma: what the charges read
            abd._raw_data[f] = 0.3 * synthetic.chirp_modes(t, 0, ell_max, 120 + f) * (1 + 0.0004 * t[:, None])
            abd._raw_data[f, :, : s * s] = 0
    abd._raw_data[2, :, 0] -= 5.0 * np.sqrt(4 * np.pi)  # a dominant mass monopole keeps the four-momentum timelike
    return ctx, abd.to_device()


def _call(name, abd):
    if name == "spin":
        return abd.bondi_dimensionless_spin()
    if name == "com":
        return abd.bondi_CoM_charge()
    if hasattr(abd, "bondi_charges"):
        return abd.bondi_charges()
    return abd.bondi_four_momentum(), abd.bondi_angular_momentum(), abd.bondi_boost_charge(), abd.bondi_CoM_charge()


def _step(kind, n, ell_max, scratch):
    import numpy as np

    ctx, abd = _abd(n, ell_max)
    out = {"step": kind, "n_times": n, "n_modes": abd.n_modes}
    name = kind[7:] if kind.startswith("parent_") else kind
    if kind == "kernel":
        from scri_amd import engine

        raw = abd._raw_dev
        sigma_dot = engine.spline_derivative(abd.t, raw[5], abd.t, 1, ctx=ctx)
        engine.bondi_charges(abd.t, raw[1], raw[2], raw[5], sigma_dot, ell_max, ctx=ctx)  # warm-up: the tables, the first launch
        ctx.synchronize()
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        res = engine.bondi_charges(abd.t, raw[1], raw[2], raw[5], sigma_dot, ell_max, ctx=ctx)
        ms, launches = ctx.get_timing(reset=True)["pointwise"]
        assert launches == 1
        out.update(ms=ms, checksum=float(res[2][-1].sum().item()), launch_shape=list(engine.charge_launch_shape(abd.n_modes)))
        engine.bondi_charges(None, raw[1], None, raw[5], None, ell_max, want=("angular", "com"), ctx=ctx)
        out.update(no_dot_ms=ctx.get_timing(reset=True)["pointwise"][0])
    elif name == "sample":
        rows = np.arange(0, n, max(n // SAMPLES, 1))
        P, J, N, G = _call("charges", abd)
        keep = dict(P=P[rows], J=J[rows], N=N[rows], G=G[rows])
        if kind == "sample":
            from scri_amd import engine

            raw = abd._raw_dev
            sigma_dot = engine.spline_derivative(abd.t, raw[5], abd.t, 1, ctx=ctx)
            keep.update(t=abd.t[rows], psi1=raw[1].cpu().numpy()[rows], psi2=raw[2].cpu().numpy()[rows], sigma=raw[5].cpu().numpy()[rows],
                        sigma_dot=sigma_dot.cpu().numpy()[rows])
        np.savez(os.path.join(scratch, kind + ".npz"), **keep)
        out.update(ms=0.0, checksum=float(N[-1].sum()))
    else:
        _call(name, abd[:1000])  # warm-up of the kernels and the copy paths on a short piece
        _call(name, abd)         # ... and of the buffers of the full size
        ctx.synchronize()
        t0 = time.perf_counter()
        res = _call(name, abd)
        last = res[2] if isinstance(res, tuple) else res
        out.update(ms=(time.perf_counter() - t0) * 1e3, checksum=float(last[-1].sum()), resident=bool(abd.is_device_resident))
    ctx.close()
    print(json.dumps(out))


def _compare(scratch, ell_max):
    """the two builds' charges on the sampled steps against the yardstick on the new build's derivative of sigma"""
    import numpy as np

    sys.path.insert(0, HERE)
    from tests.helpers import charge_cases as cc

    new, old = np.load(os.path.join(scratch, "sample.npz")), np.load(os.path.join(scratch, "parent_sample.npz"))
    y = cc.yardstick(new["t"], new["psi1"], new["psi2"], new["sigma"], new["sigma_dot"], ell_max)
    report, ok = {}, True
    for name, key in zip(cc.CHARGES, "PJNG"):
        value, bar = y[name]
        parent_distance = np.abs(old[key].astype(cc.LD) - value)
        within = bool(np.all(np.abs(new[key].astype(cc.LD) - old[key].astype(cc.LD)) <= bar + parent_distance))
        ok = ok and within
        report[name] = {"new_share_of_bar": round(cc.ratio(new[key], value, bar), 3), "parent_bars_from_yardstick": round(float((parent_distance / bar).max()), 2),
                        "largest_difference": float(np.abs(new[key] - old[key]).max()), "scale": float(np.abs(old[key]).max()), "within": within}
    return report, ok


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
        outputs = _compare(scratch, ell_max) if parent else None
    n_modes = runs["kernel"][0]["n_modes"]
    summary = {"n_times": n, "ell_max": ell_max, "n_modes": n_modes, "reps": reps, "launch_shape": runs["kernel"][0]["launch_shape"]}
    for kind in new_kinds + parent_kinds:
        ms = [r["ms"] for r in runs[kind]]
        summary.update({f"{kind}_median_ms": round(statistics.median(ms), 4), f"{kind}_spread_ms": round(max(ms) - min(ms), 4),
                        f"{kind}_ms": [round(v, 4) for v in ms]})
    summary["kernel_no_dot_median_ms"] = round(statistics.median(r["no_dot_ms"] for r in runs["kernel"]), 4)
    kernel_bytes = 2 * n * n_modes * 16 + 104 * n
    rate = kernel_bytes / (summary["kernel_median_ms"] * 1e-3)
    summary.update(kernel_bytes=kernel_bytes, kernel_TB_per_s=round(rate / 1e12, 3), kernel_share_of_hbm=round(rate / HBM_BYTES_PER_S, 3))
    summary["stays_resident"] = all(r["resident"] for k in CALLS for r in runs[k])
    if parent:
        for k in CALLS:
            summary[f"parent_over_new_{k}"] = round(summary[f"parent_{k}_median_ms"] / summary[f"{k}_median_ms"], 1)
            summary[f"{k}_spreads_separated"] = bool(max(r["ms"] for r in runs[k]) < min(r["ms"] for r in runs["parent_" + k]))
        summary["outputs"], summary["outputs_within_the_bars"] = outputs
    print(json.dumps(summary))
    if parent and not (summary["outputs_within_the_bars"] and all(summary[f"{k}_spreads_separated"] for k in CALLS)):
        raise SystemExit("the new runs are not separated from the parent's, or the outputs differ by more than the bars")


if __name__ == "__main__":
    if len(sys.argv) >= 7 and sys.argv[1] == "--step":
        sys.path.insert(0, sys.argv[5])  # the checkout whose package this run measures
        _step(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[6])
    else:
        main()
