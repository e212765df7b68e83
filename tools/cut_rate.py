"""Time of the supertranslation solve's pieces on the cut entries against the composed bodies they replace ("Cuts"),
both arms in this checkout (scri_amd.map_to_superrest_frame.composed_route switches the three helpers back):

  call    `compute_Moreschi_supermomentum(PsiM, alpha, ell_max)` on a device-resident window of `n_window` rows at dt = 0.1 (9001: +-450),
          |alpha| of a few time units
  solve   one full `supertranslation_to_map_to_superrest_frame` on that window
  frame   `map_to_superrest_frame` of a device-resident object of n_frame = 1e5 steps, padding 250 (the shape of tools/superrest_timing.py)

Every timed run is a process of its own with a time limit, one at a time, the two arms alternating, one warm-up and a host clock around a
call that ends in a read-back; `reps` runs of each.  Reported: medians and max - min per arm; a difference counts as a gain only if it
exceeds four of the composed arm's spreads.  A run that fails or exceeds its limit ends the measurement there.
Usage: python tools/cut_rate.py [kinds, e.g. call,solve,frame] [ell_max, e.g. 12,16] [reps] [n_window] [n_frame]     (prints one JSON line per kind and ell_max)"""
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 300
ARMS = ("cut", "composed")


def _moved_abd(n, ell_max, half_span):
    import numpy as np

    import scri_amd
    from tests.test_oracle_charges import kerr_schild_abd

    ctx = scri_amd.Context(0)
    u = np.linspace(-half_span, half_span, num=n)
    a = scri_amd.AsymptoticBondiData(u, ell_max, ctx=ctx)
    a._raw_data[:] = kerr_schild_abd(2.0, 0.456, ell_max, u)
    st = np.array([0.0, 3e-2 - 1j * 5e-3, 1e-3, -3e-2 - 1j * 5e-3, 2e-4 + 1j * 1e-4, 1j * 3e-3, 1e-2, 1j * 3e-3, 2e-4 - 1j * 1e-4])
    moved = a.transform(supertranslation=st, frame_rotation=np.array([1.0, 2, 3, 4]) / np.sqrt(30), boost_velocity=np.array([2e-4, -3e-5, 2e-4]))
    return ctx, moved.to_device()


def _step(kind, arm, ell_max, n_window, n_frame):
    import contextlib

    import numpy as np
    import torch  # (its import is not part of any timed call)

    from scri_amd import map_to_superrest_frame as m

    route = m.composed_route if arm == "composed" else contextlib.nullcontext
    out = {"kind": kind, "arm": arm, "ell_max": ell_max}
    with route():
        if kind == "frame":
            ctx, abd = _moved_abd(n_frame, ell_max, 1000.0)
            run = lambda: abd.map_to_superrest_frame(t_0=0, padding_time=250.0)[2]  # noqa: E731
        else:
            ctx, abd = _moved_abd(n_window, ell_max, 0.05 * (n_window - 1))
            n = 2 * ell_max + 1
            theta, phi = np.meshgrid(np.pi * np.arange(n) / (n - 1), 2 * np.pi * np.arange(n) / n, indexing="ij")
            alpha = 3.0 * np.sin(theta) * np.cos(phi) + 1.5 * np.cos(theta) ** 2 - 0.7 * np.sin(theta) ** 2 * np.sin(2 * phi)
            PsiM = abd.supermomentum("Moreschi")
            if kind == "call":
                run = lambda: m.compute_Moreschi_supermomentum(PsiM, alpha, ell_max, ctx)  # noqa: E731
            else:
                run = lambda: m.supertranslation_to_map_to_superrest_frame(abd, ell_max=ell_max)[1]  # noqa: E731
        run()  # warm-up: tables, buffers, the first launches
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run()
        out["ms"] = (time.perf_counter() - t0) * 1e3
    out["checksum"] = float(np.sum(np.abs(np.asarray(res, dtype=complex)[np.isfinite(np.asarray(res, dtype=complex))])))
    ctx.close()
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    kinds = args[0].split(",") if len(args) > 0 else ["call", "solve", "frame"]
    ells = [int(x) for x in args[1].split(",")] if len(args) > 1 else [12, 16]
    reps = int(args[2]) if len(args) > 2 else 7
    n_window = int(args[3]) if len(args) > 3 else 9001
    n_frame = int(args[4]) if len(args) > 4 else 100000
    for kind in kinds:
        for ell_max in ells if kind != "frame" else ells[:1]:
            runs = {arm: [] for arm in ARMS}
            for arm in ARMS * reps:
                done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", kind, arm, str(ell_max), str(n_window), str(n_frame)],
                                      capture_output=True, text=True, timeout=STEP_LIMIT_S, cwd=HERE)
                if done.returncode != 0:
                    sys.stderr.write(done.stdout[-2000:] + done.stderr[-4000:])
                    raise SystemExit(f"step {kind} / {arm} ended with status {done.returncode}: nothing further is started")
                line = json.loads(done.stdout.strip().splitlines()[-1])
                print(json.dumps(line), file=sys.stderr, flush=True)
                runs[arm].append(line)
            summary = {"kind": kind, "ell_max": ell_max, "reps": reps, "rows": n_frame if kind == "frame" else n_window}
            for arm in ARMS:
                ms = [r["ms"] for r in runs[arm]]
                summary.update({f"{arm}_median_ms": round(statistics.median(ms), 3), f"{arm}_spread_ms": round(max(ms) - min(ms), 3),
                                f"{arm}_ms": [round(v, 3) for v in ms], f"{arm}_checksum": runs[arm][0]["checksum"]})
            gain = summary["composed_median_ms"] - summary["cut_median_ms"]
            summary.update(composed_over_cut=round(summary["composed_median_ms"] / summary["cut_median_ms"], 2),
                           gain_counts=bool(gain > 4 * summary["composed_spread_ms"]))
            print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 7 and sys.argv[1] == "--step":
        sys.path.insert(0, HERE)
        _step(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]))
    else:
        main()
