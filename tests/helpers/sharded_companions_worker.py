"""One rank of tests/test_gpu_sharded_companions.py: a rank-local psi1 series with its psi2..psi4 companions through
WaveformModes.transform(group=...), and a strongly boosted AsymptoticBondiData series through AsymptoticBondiData.transform(group=...,
partition=...), on the GPU (gloo group, the ranks share device 0).
Usage: RANK=r WORLD_SIZE=w MASTER_PORT=p python sharded_companions_worker.py <out_dir>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V_DIR = np.array([0.6, -0.5, 0.6]) / np.linalg.norm([0.6, -0.5, 0.6])


def psi_case(n_times=6000, ell_max=8):
    """psi1 (l >= 1) and its companions psi2 (l >= 0), psi3 (l >= 1), psi4 (l >= 2); cfg3's transformation with a visible boost"""
    from scri_amd import synthetic

    rng = np.random.default_rng(13)
    t = np.arange(n_times) * 0.1
    ph = 0.05 * t + 2e-5 * t**2
    fields = {}
    for name, lmin in (("psi1", 1), ("psi2", 0), ("psi3", 1), ("psi4", 2)):
        m = np.concatenate([np.arange(-l, l + 1) for l in range(lmin, ell_max + 1)])
        a = rng.normal(size=m.size) + 1j * rng.normal(size=m.size)
        fields[name] = (lmin, np.ascontiguousarray(a[None, :] * np.exp(1j * m[None, :] * ph[:, None])))
    kw = dict(supertranslation=np.array(synthetic.S9, dtype=complex), frame_rotation=np.array([1.0, 2, 3, 4]) / np.sqrt(30),
              boost_velocity=np.array([1.0, 2.0, 3.0]) * 1e-3)
    return t, fields, kw


def abd_kw(L, beta=0.2):
    st = np.zeros(9, dtype=complex)
    st[0], st[2], st[6] = 0.3, 0.05, 0.02
    return dict(supertranslation=st, frame_rotation=[0.9, 0.1, -0.3, 0.2], boost_velocity=beta * V_DIR, working_ell_max=2 * L + 2)


def waveform(t, fields, name, ell_max, rows, ctx=None):
    import scri_amd

    i0, i1 = rows
    lmin, data = fields[name]
    return scri_amd.WaveformModes(t=t[i0:i1], data=np.ascontiguousarray(data[i0:i1]), ell_min=lmin, ell_max=ell_max, dataType=getattr(scri_amd, name),
                                  frameType=scri_amd.Inertial, r_is_scaled_out=True, m_is_scaled_out=True, ctx=ctx)


def main(out_dir):
    import torch
    import torch.distributed as dist

    import scri_amd
    from scri_amd import engine, sharding
    from test_gpu_sharding import _abd_case

    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    try:
        g = dist.group.WORLD
        # psi1 + three companions, deliberately uneven blocks
        ell_max = 8
        t, fields, kw = psi_case(ell_max=ell_max)
        n = t.size
        cuts = [0] + [int(n * (0.2 + 0.6 * (r + 1) / world)) if r + 1 < world else n for r in range(world)]
        rows = (cuts[rank], cuts[rank + 1])
        for tag, extra, resident in (("host", {}, False), ("device", {}, True), ("overlap", dict(overlap_halo=True), True),
                                     ("columns", dict(partition="columns"), False), ("columns_device", dict(partition="columns"), True)):
            w = waveform(t, fields, "psi1", ell_max, rows)
            comp = {f"{k}_modes": waveform(t, fields, k, ell_max, rows) for k in ("psi2", "psi3", "psi4")}
            if resident:
                w.to_device()
                for c in comp.values():
                    c.to_device()
            got = w.transform(group=g, **comp, **kw, **extra)
            assert got.is_device_resident == resident, tag
            res[f"wm_{tag}_t"], res[f"wm_{tag}_d"] = got.t, np.array(got.data)
        # AsymptoticBondiData under a strong boost: plan B
        u, raw, _, L = _abd_case(n=3000, ell_max=4)
        kw_abd = abd_kw(L)
        j0, j1 = sharding.shard_bounds(u.size, world, rank)
        tr = engine.make_transformation(kw_abd["supertranslation"], kw_abd["frame_rotation"], kw_abd["boost_velocity"], 2 * (2 * L + 2) + 1,
                                        2 * (2 * L + 2) + 1, L)
        assert sharding.ShardedTransform("abd", u, tr, ell_max=L, group=g, partition="auto").partition == "columns"
        for tag, partition, resident in (("auto", "auto", False), ("columns", "columns", False), ("auto_device", "auto", True),
                                         ("columns_device", "columns", True)):
            abd = scri_amd.AsymptoticBondiData(u[j0:j1], L)
            abd._raw_data[:] = raw[:, j0:j1]
            if resident:
                abd = abd.to_device()
            got = abd.transform(group=g, partition=partition, **kw_abd)
            assert got.is_device_resident == resident, tag
            res[f"abd_{tag}_u"], res[f"abd_{tag}_raw"] = got.t, np.array(got._raw_data)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **res)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
