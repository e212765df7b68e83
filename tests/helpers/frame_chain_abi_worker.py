"""Child process of tests/test_gpu_frame_chain.py: the exports of the device frame chain under callers that get one argument wrong
(a NULL pointer, too few time steps, a time axis that does not increase, a memory kind that does not exist, an anchor outside the
series, no iterations).  One line per call: `<label> <want0|wantneg> <status>`, flushed BEFORE the call is made complete, then
`done <count>`.  Nothing here is meant to fault: every call is refused by the argument checks or is well formed."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from scri_amd import _lib  # noqa: E402


def main():
    lib = _lib.load()
    ctx = _lib.Context(0)
    h = ctx.handle
    dp = ctypes.POINTER(ctypes.c_double)
    vp = ctypes.c_void_p
    n, nm = 64, 21
    t = np.linspace(0.0, 6.3, n)
    t_bad = t.copy()
    t_bad[10] = t_bad[9]
    om = np.stack([0.1 * np.sin(t), 0.2 * np.cos(t), 0.3 + 0 * t], axis=1).copy()
    R = np.stack([np.cos(0.1 * t), 0 * t, np.sin(0.1 * t) * 0.6, np.sin(0.1 * t) * 0.8], axis=1).copy()
    ll = np.repeat(np.diag([1.0, 2.0, 4.0]).reshape(1, 9), n, axis=0).copy()
    rng = np.random.default_rng(0)
    data = (rng.normal(size=(n, nm)) + 1j * rng.normal(size=(n, nm))).copy()
    out = np.zeros((n, 4))
    out3 = np.zeros((n, 3))
    q = np.array([1.0, 0.0, 0.0, 0.0])
    z = np.array([0.0, 0.0, 1.0])
    import torch

    fdev = torch.empty((n, 4), dtype=torch.float64, device="cuda:0")
    H, D, BAD = _lib.BMS_HOST, _lib.BMS_DEVICE, 7
    P = lambda a: None if a is None else a.ctypes.data_as(dp)  # noqa: E731
    V = lambda a: None if a is None else vp(a.ctypes.data)  # noqa: E731
    F = vp(fdev.data_ptr())
    count = 0

    def call(label, want, fn, *args):
        nonlocal count
        print(label, want, end=" ", flush=True)
        print(fn(*args), flush=True)
        count += 1

    f = lib.bms_frame_from_angular_velocity
    call("frame_from_angular_velocity ok", "want0", f, h, P(t), n, V(om), H, P(q), 1e-12, V(out))
    call("frame_from_angular_velocity tolerance<=0", "want0", f, h, P(t), n, V(om), H, P(q), 0.0, V(out))
    for label, args in (("t=NULL", (h, None, n, V(om), H, P(q), 1e-12, V(out))), ("omega=NULL", (h, P(t), n, None, H, P(q), 1e-12, V(out))),
                        ("R0=NULL", (h, P(t), n, V(om), H, None, 1e-12, V(out))), ("out=NULL", (h, P(t), n, V(om), H, P(q), 1e-12, None)),
                        ("n=3", (h, P(t), 3, V(om), H, P(q), 1e-12, V(out))), ("n=0", (h, P(t), 0, V(om), H, P(q), 1e-12, V(out))),
                        ("n=-5", (h, P(t), -5, V(om), H, P(q), 1e-12, V(out))), ("t-not-increasing", (h, P(t_bad), n, V(om), H, P(q), 1e-12, V(out))),
                        ("bad-mem", (h, P(t), n, V(om), BAD, P(q), 1e-12, V(out)))):
        call("frame_from_angular_velocity " + label, "wantneg", f, *args)

    f = lib.bms_dominant_axis
    call("dominant_axis ok", "want0", f, h, V(ll), n, H, P(z), 5, V(out3))
    call("dominant_axis one-step", "want0", f, h, V(ll), 1, H, P(z), 0, V(out3))
    for label, args in (("ll=NULL", (h, None, n, H, P(z), 0, V(out3))), ("rough=NULL", (h, V(ll), n, H, None, 0, V(out3))),
                        ("out=NULL", (h, V(ll), n, H, P(z), 0, None)), ("n=0", (h, V(ll), 0, H, P(z), 0, V(out3))),
                        ("n=-1", (h, V(ll), -1, H, P(z), 0, V(out3))), ("bad-mem", (h, V(ll), n, BAD, P(z), 0, V(out3))),
                        ("rough_index=n", (h, V(ll), n, H, P(z), n, V(out3))), ("rough_index=-1", (h, V(ll), n, H, P(z), -1, V(out3)))):
        call("dominant_axis " + label, "wantneg", f, *args)

    f = lib.bms_minimal_rotation
    call("minimal_rotation ok", "want0", f, h, P(t), n, V(R), H, 3, V(out))
    for label, args in (("t=NULL", (h, None, n, V(R), H, 3, V(out))), ("R=NULL", (h, P(t), n, None, H, 3, V(out))),
                        ("out=NULL", (h, P(t), n, V(R), H, 3, None)), ("n=3", (h, P(t), 3, V(R), H, 3, V(out))),
                        ("t-not-increasing", (h, P(t_bad), n, V(R), H, 3, V(out))), ("bad-mem", (h, P(t), n, V(R), BAD, 3, V(out))),
                        ("iterations=0", (h, P(t), n, V(R), H, 0, V(out))), ("iterations=-2", (h, P(t), n, V(R), H, -2, V(out)))):
        call("minimal_rotation " + label, "wantneg", f, *args)

    f = lib.bms_rotor_angular_velocity
    call("rotor_angular_velocity ok", "want0", f, h, P(t), n, V(R), H, V(out3))
    for label, args in (("t=NULL", (h, None, n, V(R), H, V(out3))), ("R=NULL", (h, P(t), n, None, H, V(out3))),
                        ("out=NULL", (h, P(t), n, V(R), H, None)), ("n=2", (h, P(t), 2, V(R), H, V(out3))),
                        ("t-not-increasing", (h, P(t_bad), n, V(R), H, V(out3))), ("bad-mem", (h, P(t), n, V(R), -1, V(out3)))):
        call("rotor_angular_velocity " + label, "wantneg", f, *args)

    f = lib.bms_frame_adjust
    frame = R.copy()  # (adjusted in place)
    call("frame_adjust ok", "want0", f, h, V(frame), n, H, P(q), 1e-12, V(out), None)
    call("frame_adjust nothing-to-do", "want0", f, h, V(frame), 0, H, None, 0.0, None, None)
    for label, args in (("frame=NULL", (h, None, n, H, None, 0.0, None, None)), ("n=-1", (h, V(R), -1, H, None, 0.0, None, None)),
                        ("bad-mem", (h, V(R), n, BAD, None, 0.0, None, None)), ("tolerance=inf", (h, V(R), n, H, None, float("inf"), None, None))):
        call("frame_adjust " + label, "wantneg", f, *args)

    f = lib.bms_corotating_frame
    ok = (h, P(t), n, V(data), nm, 2, 4, H, P(q), 1e-12, F, P(out), P(out3))
    call("corotating_frame ok", "want0", f, *ok)

    def but(args, i, v):
        a = list(args)
        a[i] = v
        return a

    for label, i, v in (("t=NULL", 1, None), ("n=3", 2, 3), ("data=NULL", 3, None), ("ld<n_modes", 4, nm - 1), ("ell_min<0", 5, -1),
                        ("ell_max<ell_min", 6, 1), ("ell_max>MAX_ELL", 6, 100000), ("bad-mem", 7, BAD), ("R0=NULL", 8, None),
                        ("frame_dev=NULL", 10, None), ("t-not-increasing", 1, P(t_bad))):
        call("corotating_frame " + label, "wantneg", f, *but(ok, i, v))

    f = lib.bms_coprecessing_frame
    ok = (h, P(t), n, V(data), nm, 2, 4, H, P(z), 8, 3, F, P(out), P(out3))
    call("coprecessing_frame ok", "want0", f, *ok)
    call("coprecessing_frame axis-only", "want0", f, h, None, 1, V(data), nm, 2, 4, H, P(z), 0, 0, None, None, P(out3))
    for label, i, v in (("t=NULL", 1, None), ("n=3", 2, 3), ("data=NULL", 3, None), ("ld<n_modes", 4, nm - 1), ("ell_max>MAX_ELL", 6, 100000),
                        ("bad-mem", 7, BAD), ("rough=NULL", 8, None), ("rough_index=n", 9, n), ("rough_index=-1", 9, -1),
                        ("iterations=0", 10, 0), ("iterations=-1", 10, -1), ("t-not-increasing", 1, P(t_bad))):
        call("coprecessing_frame " + label, "wantneg", f, *but(ok, i, v))
    call("coprecessing_frame axis-only n=0", "wantneg", f, h, None, 0, V(data), nm, 2, 4, H, P(z), 0, 0, None, None, P(out3))
    # the context still works
    call("frame_from_angular_velocity ok-again", "want0", lib.bms_frame_from_angular_velocity, h, P(t), n, V(om), H, P(q), 1e-12, V(out))
    ctx.close()
    print("done", count)


if __name__ == "__main__":
    main()
