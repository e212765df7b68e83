"""Time to_corotating_frame() and to_coprecessing_frame() on a device-resident l = 2..8 series (N = 1e5 and 1e6 by default).

    python tools/frame_chain_timing.py --out profiles/<name>.json [--root <checkout>] [--n 100000 1000000] [--runs 12]

One process, one context.  Per size: a waveform that is simple in a precessing, spinning frame is built on the GPU, and each call is
timed on a fresh device copy of it, synchronised before and after; the figure is the median of `--runs` (>= 10) calls after two
warm-up calls.  Every size runs under an alarm of its own (--limit seconds): a step that hangs ends the process instead of holding
the GPU.  --root names the checkout whose package is imported and whose kernel sources are hashed (default: the one this file is
in), so that the same script times another commit's tree; the comparison the result is for is always between two commits."""
import argparse
import glob
import hashlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np


def csrc_hash(root):
    """as bench.csrc_hash: the kernel sources and the ABI header of the tree that was timed"""
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(root, "scri_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "scri_amd", "csrc", "*.h"))
                   + [os.path.join(root, "scri_amd", "csrc", "Makefile"), os.path.join(root, "include", "scri_amd.h")])
    for f in files:
        h.update(os.path.basename(f).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def about(axis, angle):
    axis = np.asarray(axis, dtype=float) / np.linalg.norm(axis)
    return np.concatenate([np.cos(angle / 2)[:, None], np.sin(angle / 2)[:, None] * axis[None, :]], axis=-1)


def build(scri_amd, ctx, n):
    from scri_amd import quaternions as Q

    t = np.linspace(0.0, 0.02 * n, n)
    LM = np.array([[l, m] for l in range(2, 9) for m in range(-l, l + 1)])
    rng = np.random.default_rng(1)
    amp = 0.01 * (rng.normal(size=LM.shape[0]) + 1j * rng.normal(size=LM.shape[0]))
    amp[(LM[:, 0] == 2) & (np.abs(LM[:, 1]) == 2)] += 1.0
    data = amp[None, :] * np.exp(-1j * LM[None, :, 1] * (0.05 * t)[:, None])
    w = scri_amd.WaveformModes(t=t, data=data, ell_min=2, ell_max=8, dataType=scri_amd.h, frameType=scri_amd.Inertial,
                               r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx).to_device()
    R = Q.multiply(Q.multiply(about([0, 0, 1], 0.002 * t), about([0, 1, 0], 0.3 + 0.0 * t)), about([0, 0, 1], 0.015 * t))
    w.rotate_physical_system(R)
    w.frame = np.zeros((0, 4))
    w.frameType = scri_amd.Inertial
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=240, help="seconds one size may take before the process ends")
    args = ap.parse_args()
    if args.runs < 10:
        ap.error("--runs must be at least 10")
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    import torch

    import scri_amd

    assert os.path.abspath(os.path.dirname(os.path.dirname(scri_amd.__file__))) == root, scri_amd.__file__
    ctx = scri_amd.Context(0)
    result = {"_meta": {"csrc_hash": csrc_hash(root), "device": torch.cuda.get_device_name(0), "runs": args.runs, "warmup": 2,
                        "what": "median seconds per call on a device-resident l = 2..8 series, synchronised around each call"}}
    for n in args.n:
        signal.alarm(args.limit)
        base = build(scri_amd, ctx, n)
        row = {}
        for name, call in (("to_corotating_frame", lambda w: w.to_corotating_frame()), ("to_coprecessing_frame", lambda w: w.to_coprecessing_frame())):
            times, resident = [], True
            for k in range(args.runs + 2):
                w = base.copy()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call(w)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                resident = resident and w.is_device_resident
            times = times[2:]
            row[name] = {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "steps_per_s": n / statistics.median(times),
                         "still_device_resident": resident}
            print(f"N = {n:8d}  {name:24s} median {1e3 * statistics.median(times):9.3f} ms  (min {1e3 * min(times):.3f}, max {1e3 * max(times):.3f})"
                  f"  resident afterwards: {resident}", flush=True)
        result[str(n)] = row
        signal.alarm(0)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
