"""psi companions on the pipelined and dealt host paths (bms_transform_modes_pipelined_part): a psi2 series with its psi3 and psi4
companions dealt over four contexts of the one GPU equals the one-context pipelined call with the same shard count bit for bit, and
the one-call path to rounding; a companion described wrongly is refused before anything moves."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "pipelined_aux_worker.py")


def _psi2_case(n_times=4000, ell_max=16):
    """cfg3's shape and transformation: psi2 (l >= 0) with psi3 (l >= 1) and psi4 (l >= 2), host arrays"""
    import scri_amd
    from scri_amd import synthetic

    rng = np.random.default_rng(23)
    spec = synthetic.CONFIGS["cfg3"]
    t = synthetic.time_axis(n_times, spec["dt"])
    ph = 0.05 * t + 2e-5 * t**2
    waves = {}
    for name, lmin in (("psi2", 0), ("psi3", 1), ("psi4", 2)):
        m = np.concatenate([np.arange(-l, l + 1) for l in range(lmin, ell_max + 1)])
        a = rng.normal(size=m.size) + 1j * rng.normal(size=m.size)
        waves[name] = scri_amd.WaveformModes(t=t, data=np.ascontiguousarray(a[None, :] * np.exp(1j * m[None, :] * ph[:, None])), ell_min=lmin,
                                             ell_max=ell_max, dataType=getattr(scri_amd, name), frameType=scri_amd.Inertial, r_is_scaled_out=True,
                                             m_is_scaled_out=True)
    return t, waves, dict(spec["kwargs"]), ell_max


def test_dealt_companions_equal_one_context_pieces(ctx, monkeypatch):
    from scri_amd import engine

    t, waves, kw, L = _psi2_case()
    w = waves["psi2"]
    n_theta = 2 * (L + 2) + 1
    tr = engine.make_transformation(kw["supertranslation"], kw["frame_rotation"], kw["boost_velocity"], n_theta, n_theta, L)
    aux = [(waves["psi3"].data, 1, L, -1, 2.0, 1), (waves["psi4"].data, 2, L, -2, 1.0, 2)]  # (coeff: comb(5 - 3, 5 - n), power: n - 3)
    args = (t, w.data, 0, L, 0, w.conformal_weight, engine.BMS_TERM_PSI, tr)
    devices = [0, 0, 0, 0]
    pieces = engine.pieces_for(devices, t.size, L, w.data.nbytes)
    assert pieces >= 4
    t_one, d_one = engine.transform_modes(*args, aux=aux, ctx=ctx)  # the default route: one call
    t_pc, d_pc = engine.transform_modes(*args, aux=aux, ctx=ctx, pieces=pieces)
    t_dev, d_dev = engine.transform_modes(*args, aux=aux, ctx=ctx, devices=devices, pieces=pieces)
    scale = np.abs(d_one).max()
    assert np.array_equal(t_dev, t_pc) and np.array_equal(d_dev, d_pc)  # a piece's arithmetic depends on its cut only
    assert np.array_equal(t_pc, t_one) and np.abs(d_pc - d_one).max() < 1e-12 * scale
    # the public call honours `devices` with companions (the dealt path with pieces_for's shard count: the one-context call with that
    # count, bit for bit); without `devices` it stays on the one-call path
    calls = []
    real = engine.transform_modes

    def spy(*a, **k):
        calls.append((a, k))
        return real(*a, **k)

    monkeypatch.setattr(engine, "transform_modes", spy)
    got = w.transform(devices=devices, psi3_modes=waves["psi3"], psi4_modes=waves["psi4"], **kw)
    plain = w.transform(psi3_modes=waves["psi3"], psi4_modes=waves["psi4"], **kw)
    monkeypatch.undo()
    (a_dev, k_dev), (a_plain, k_plain) = calls
    assert list(k_dev["devices"]) == devices and len(k_dev["aux"]) == 2 and k_plain.get("devices") is None and k_plain.get("pieces") is None
    _, d_pieces = engine.transform_modes(*a_dev, **dict(k_dev, devices=None, pieces=pieces))
    assert np.array_equal(got.data, d_pieces)
    _, d_call = engine.transform_modes(*a_plain, **k_plain)
    assert np.array_equal(plain.data, d_call) and np.abs(plain.data - d_one).max() < 1e-12 * scale  # (its rotor is normalised anew: ulps)


def test_pipelined_entry_refuses_wrong_companions():
    out = subprocess.run([sys.executable, WORKER], capture_output=True, text=True, timeout=600)
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert out.returncode == 0 and lines and lines[-1].startswith("done"), (
        f"the child died (exit {out.returncode}) in: {lines[-1] if lines else '(nothing printed)'}\n{out.stderr[-1500:]}")
    for l in lines[:-1]:
        parts = l.split()
        if parts[0] == "well-formed":
            assert int(parts[1]) == 0, l
        elif parts[0] == "well-formed-again":
            assert int(parts[1]) == 0 and int(parts[2]) == 1, l  # the context still gives the first answer, bit for bit
        else:
            assert int(parts[1]) < 0, l
