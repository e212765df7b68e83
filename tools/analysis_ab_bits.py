"""usage: SCRI_AMD_LIB_PATH=LIB python tools/analysis_ab_bits.py OUT.json -- sha256 of every output of group A (engine.map2salm over
analysis_cases.A_CASES) and group B (the boosted transforms) of tests/test_gpu_analysis_edges.py; run once per build and compare the files"""
import hashlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scri_amd
from scri_amd import _lib, engine
from tests.helpers import analysis_cases as an
from tests import test_gpu_analysis_edges as te

OPT = te.ROUTE_OPTIONS
ctx = _lib.Context(0)
print("library", _lib.LIB_PATH, flush=True)

def set_route(env):
    for key, name in OPT.items():
        ctx.option(name, 1 if key == env else 0)

def h(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()

out = {}
for c in an.A_CASES:
    seed = c.n_theta * 1009 + c.n_phi * 31 + c.L * 7 + c.ell_min + 3 * (c.spin + 4)
    if c.kind == "noise":
        f = an.noise_rows(c.rows, c.n_theta, c.n_phi, seed)
    elif c.kind == "one_hot":
        f = an.one_hot_rows(an.one_hot_pixels(c.n_theta, c.n_phi), c.n_theta, c.n_phi)
    else:
        f = an.band_limited_rows(c.rows, c.n_theta, c.n_phi, c.spin, c.L, c.ell_min, seed)[1]
    set_route(c.env)
    got = engine.map2salm(f, c.spin, c.L, ell_min=c.ell_min, ctx=ctx)
    assert np.isfinite(got).all(), an.case_id(c)
    out["A " + an.case_id(c)] = h(got)
print("group A", len(out), flush=True)
for n_theta, n_phi in an.B_GRIDS + an.B_NOT_FUSED:
    for name in an.B_TYPES:
        _, w_g = te._pair(ctx, name, seed=n_theta * 64 + n_phi)
        kw = dict(boost_velocity=np.array(an.B_BOOST), n_theta=n_theta, n_phi=n_phi, ell_max=an.B_ELL_MAX)
        aux = {}
        if name in ("psi0", "psi1", "psi2", "psi3"):
            for n in range(int(name[-1]) + 1, 5):
                aux[f"psi{n}_modes"] = te._pair(ctx, f"psi{n}", seed=1000 + n)[1]
        for env in ((None, "NO_SPLIT") if (n_theta, n_phi) in an.B_GRIDS else (None,)):
            set_route(env)
            got = w_g.transform(**kw, **aux)
            assert np.isfinite(got.data).all()
            out[f"B {name} {n_theta}x{n_phi} {env}"] = h(got.data) + h(got.t)
set_route(None)
print("all", len(out), flush=True)
json.dump(out, open(sys.argv[1], "w"), indent=0)
ctx.close()
