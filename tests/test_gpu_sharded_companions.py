"""Three ranks of a gloo group sharing the one GPU: a psi1 series with its psi2..psi4 companions under WaveformModes.transform(group=...)
(time shards, time shards with the interior under the exchange, grid columns) and a strongly boosted AsymptoticBondiData series under
AsymptoticBondiData.transform(group=..., partition="auto" | "columns"), host and device-resident, against the one-context call on the
whole series.  Worker: tests/helpers/sharded_companions_worker.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(900)
def test_three_ranks_companions_and_abd_columns_equal_single_gpu(ctx, tmp_path):
    import scri_amd
    from tests.helpers.sharded_companions_worker import abd_kw, psi_case, waveform
    from tests.test_gpu_sharding import _abd_case

    world = 3
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "helpers", "sharded_companions_worker.py"), str(tmp_path)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=800)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    parts = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]

    ell_max = 8
    t, fields, kw = psi_case(ell_max=ell_max)
    whole = (0, t.size)
    comp = {f"{k}_modes": waveform(t, fields, k, ell_max, whole, ctx=ctx) for k in ("psi2", "psi3", "psi4")}
    ref = waveform(t, fields, "psi1", ell_max, whole, ctx=ctx).transform(**comp, **kw)
    scale = np.abs(ref.data).max()
    errs = {}
    for tag in ("host", "device", "overlap", "columns", "columns_device"):
        t_sh = np.concatenate([p[f"wm_{tag}_t"] for p in parts])
        d_sh = np.concatenate([p[f"wm_{tag}_d"] for p in parts])
        assert np.array_equal(t_sh, ref.t), tag
        errs[tag] = np.abs(d_sh - ref.data).max() / scale
    for tag, e in errs.items():
        assert e < (2e-14 if tag.startswith("columns") else 1e-14), errs

    u, raw, _, L = _abd_case(n=3000, ell_max=4)
    abd = scri_amd.AsymptoticBondiData(u, L, ctx=ctx)
    abd._raw_data[:] = raw
    ref = abd.transform(**abd_kw(L))
    scale = max(1.0, np.abs(ref._raw_data).max())
    errs = {}
    for tag in ("auto", "columns", "auto_device", "columns_device"):
        u_sh = np.concatenate([p[f"abd_{tag}_u"] for p in parts])
        r_sh = np.concatenate([p[f"abd_{tag}_raw"] for p in parts], axis=1)
        assert np.array_equal(u_sh, ref.t), tag
        assert r_sh.shape == ref._raw_data.shape, tag
        errs[tag] = np.abs(r_sh - ref._raw_data).max() / scale
    assert max(errs.values()) < 2e-14, errs
    for p in parts:  # "auto" chose the columns: the same calls
        assert np.array_equal(p["abd_auto_raw"], p["abd_columns_raw"])
