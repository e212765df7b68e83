"""usage: SCRI_AMD_LIB_PATH=LIB python tools/analysis_ab_speed.py LABEL -- per-tag kernel times (the context's timers, ms per call, five
calls after a warm one) of four analysis shapes as one JSON line; run a process per build, alternating, and compare medians"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from scri_amd import _lib, engine

ctx = _lib.Context(0)
SHAPES = [  # name, n_theta, n_phi, ell_min, L, spin, rows, route option, tag
    ("one_role 33x33 l2..16", 33, 33, 2, 16, -2, 20000, "SCRI_AMD_NO_SPLIT_ANALYSIS", "analysis_fused"),
    ("wide 40x39 l3..19", 40, 39, 3, 19, -2, 20000, None, "analysis_fused"),
    ("two_kernel 99x99 l0..24", 99, 99, 0, 24, -2, 2000, None, "analysis_large"),
    ("older_pair 67x67 l0..33", 67, 67, 0, 33, -2, 2000, None, "theta_quadrature"),
]
res = {"label": sys.argv[1]}
rng = np.random.default_rng(5)
for name, nt, nph, lo, L, s, rows, opt, tag in SHAPES:
    block = rng.normal(size=(50, nt, nph)) + 1j * rng.normal(size=(50, nt, nph))
    f = np.ascontiguousarray(np.tile(block, (rows // 50, 1, 1)))
    if opt:
        ctx.option(opt, 1)
    engine.map2salm(f, s, L, ell_min=lo, ctx=ctx)  # warm: tables, code objects, work space
    ctx.enable_timing(True)
    ctx.get_timing(reset=True)
    n = 5
    for _ in range(n):
        engine.map2salm(f, s, L, ell_min=lo, ctx=ctx)
    t = ctx.get_timing(reset=True)
    ctx.enable_timing(False)
    if opt:
        ctx.option(opt, 0)
    live = {k: v for k, v in t.items() if v[1]}
    assert tag in live, (name, sorted(live))
    res[name] = {k: round(v[0] / n, 5) for k, v in live.items()}
print("SPEED " + json.dumps(res), flush=True)
ctx.close()
