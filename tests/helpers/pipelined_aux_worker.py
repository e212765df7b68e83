"""Child process of tests/test_gpu_pipelined_companions.py: bms_transform_modes_pipelined with psi companions, well-formed and with one
companion field made wrong at a time.  Prints `<label> <status> [<same bits as the first call>]`; the last line is `done <n calls>`."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402

from scri_amd import _lib, engine  # noqa: E402


def main():
    lib = _lib.load()
    ctx = _lib.Context(0)
    n, lmax = 600, 4
    rng = np.random.default_rng(17)
    t = np.arange(n) * 0.1
    # psi2 (s = 0, l >= 0) with psi3 (s = -1, l >= 1) and psi4 (s = -2, l >= 2)
    nm = [(lmax + 1) ** 2 - lmin**2 for lmin in (0, 1, 2)]
    fields = [np.ascontiguousarray((rng.normal(size=(n, k)) + 1j * rng.normal(size=(n, k))) * np.exp(0.05j * t[:, None])) for k in nm]
    st = np.zeros(9, dtype=complex)
    st[0], st[2] = 0.3, 0.05
    tr = engine.make_transformation(st, [0.9, 0.1, -0.3, 0.2], [2e-3, -1e-3, 3e-3], 2 * (lmax + 2) + 1, 2 * (lmax + 2) + 1, lmax)
    t_out = np.zeros(n)
    out = np.zeros((n, (lmax + 1) ** 2), dtype=complex)
    got = ctypes.c_int64(0)

    def wm():
        w = _lib.bms_wm_input()
        w.n_times, w.t, w.data, w.ld, w.mem = n, _lib.dptr(t), fields[0].ctypes.data, nm[0], _lib.BMS_HOST
        w.ell_min, w.ell_max, w.spin_weight, w.conformal_weight, w.type_term, w.n_aux = 0, lmax, 0, -3, _lib.BMS_TERM_PSI, 2
        for i, (lmin, s, coeff) in enumerate(((1, -1, 2.0), (2, -2, 1.0))):
            w.aux_data[i], w.aux_ld[i] = fields[1 + i].ctypes.data, nm[1 + i]
            w.aux_ell_min[i], w.aux_ell_max[i], w.aux_spin[i], w.aux_coeff[i], w.aux_power[i] = lmin, lmax, s, coeff, i + 1
        return w

    def call(w):
        out[:] = 0
        return lib.bms_transform_modes_pipelined(ctx.handle, ctypes.byref(w), ctypes.byref(tr), 4, _lib.dptr(t_out), _lib.vptr(out), ctypes.byref(got))

    count = 0
    rc = call(wm())
    first = out[: got.value].copy()
    print("well-formed", rc, flush=True)

    def wrong(label, edit):
        nonlocal count
        w = wm()
        edit(w)
        print(label, end=" ", flush=True)
        print(call(w), flush=True)
        count += 1

    wrong("aux_ld-too-small", lambda w: w.aux_ld.__setitem__(0, nm[1] - 1))
    wrong("aux-ell-range-inverted", lambda w: (w.aux_ell_min.__setitem__(1, 3), w.aux_ell_max.__setitem__(1, 2)))
    wrong("aux_data1-NULL", lambda w: w.aux_data.__setitem__(1, None))
    wrong("n_aux-5", lambda w: setattr(w, "n_aux", 5))
    wrong("n_aux-negative", lambda w: setattr(w, "n_aux", -1))
    rc = call(wm())
    print("well-formed-again", rc, int(np.array_equal(out[: got.value], first)), flush=True)
    print("done", count + 2, flush=True)


if __name__ == "__main__":
    main()
