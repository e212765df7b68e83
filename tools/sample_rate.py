"""Time `scri_amd.sample_waveforms.fake_precessing_waveform`: the reference's default call (200 201 steps x 77 modes) with the result
left on the device and with host output, and a device-resident call of 10^6 steps.

    python tools/sample_rate.py [--runs 12] [--limit 240]

One process, one context.  Each figure is the median of `--runs` (>= 10) calls after two warm-up calls, the device synchronised before
and after every call.  After the timed calls one more call of each kind runs with the context's per-kernel timing on, and the time of
its kernels is printed by class (the waveform's own kernels are "pointwise", the inertial rotation "rotate", the spline solves the
rest).  Every kind runs under an alarm of its own (--limit seconds): a call that hangs ends the process instead of holding the GPU."""
import argparse
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--limit", type=int, default=240, help="seconds one kind of call may take before the process ends")
    args = ap.parse_args()
    if args.runs < 10:
        ap.error("--runs must be at least 10")
    sys.path.insert(0, ROOT)
    import torch

    import scri_amd
    from scri_amd.sample_waveforms import fake_precessing_waveform

    ctx = scri_amd.Context(0)
    kinds = (
        ("default call, device resident", dict(device=True)),
        ("default call, host output", dict(device=False)),
        ("default call, corotating, device resident", dict(device=True, inertial=False)),
        ("10^6 steps, device resident", dict(device=True, t_1=100_000.0 - 20.0 - 0.1)),
    )
    for name, kw in kinds:
        signal.alarm(args.limit)
        times, shape = [], None
        for _ in range(args.runs + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = fake_precessing_waveform(ctx=ctx, **kw)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            assert w.is_device_resident == kw["device"]
            shape = w._data_shape()
            del w
        times = times[2:]
        med = statistics.median(times)
        print(f"{name:44s} {shape[0]:8d} x {shape[1]}  median {1e3 * med:9.3f} ms  (min {1e3 * min(times):.3f}, max {1e3 * max(times):.3f})"
              f"  {16 * shape[0] * shape[1] / med / 1e9:8.1f} GB/s of modes", flush=True)
        ctx.enable_timing(True)
        ctx.get_timing(reset=True)
        w = fake_precessing_waveform(ctx=ctx, **kw)
        by_class = {k: v for k, v in ctx.get_timing(reset=True).items() if v[1]}
        ctx.enable_timing(False)
        del w
        print("    kernels of one call: " + ", ".join(f"{k} {ms:.3f} ms in {calls} launches" for k, (ms, calls) in by_class.items()), flush=True)
        signal.alarm(0)
    ctx.close()


if __name__ == "__main__":
    main()
