"""Oracle parity for every build of the two fallback rotation kernels (scri_amd/csrc/engine_rotate.hip cuts the l range of a call
into segments: the LDS-resident kernel takes l <= 27 where its plan fits, the staged MFMA kernel what is left while ell_max <= 33,
the VALU kernel what is left up to ell_max = 79).

Builds and what reaches them:
  rotate_modes_kernel (VALU)        4 / 3 / 2 / 1 waves per workgroup for ell_max <= 19 / 20..26 / 27..39 / 40..79
                                    (rotate_waves_per_block); by default only for ell_max >= 34, below that through ROTATE_VALU
  rotate_modes_mfma_kernel<2|3|5>   ell_max <= 15 / 16..23 / 24..33; <2> and <3> prefetch the next l into registers; by default
                                    only for l = 28..33, below that through ROTATE_STAGED

Every case asserts from Context.rotate_stats() which kernel ran (and the VALU wave count): a case written for one build fails if the
routing sends it elsewhere.  The reference is oracle.rotations_ref (rotate_by_series; rotate_by_constant with the oracle's D for a
constant rotor), computed once per shape and shared by the tests of that shape.  The bound is the one tests/test_gpu_kernels.py
holds these kernels to: max|got - expect| < 1e-13 max(ell_max, 1) for data with unit-normal real and imaginary parts.

The rotors of a case are random unit quaternions with special rotors written over the first row, the last row and the rows either
side of every 16-step boundary (which covers the 32- and 64-step ones): +-identity, pure z rotations (Rb = 0), flips (Ra = 0) and
|Rb| resp. |Ra| in {1e-16, 9e-16, 1.1e-15, 1e-12, 1e-8, 1e-4}, i.e. on both sides of the kernels' 1e-15 threshold of the exact
branches.  Before the oracle is trusted on a set, its result is checked to keep the norm of every l block of every row to 1e-13.

Measured on an MI355X (worst max|got - expect| over the cases of a build, series and constant rotors; bound 1e-13 ell_max):

  build                    series, worst case             constant rotor   bound at that case
  VALU, 4 waves            7.7e-14  (5, 19, 127)          6.2e-15          1.9e-12
  VALU, 3 waves            1.04e-13 (19, 20, 97)          1.9e-14          2.0e-12
  VALU, 2 waves            1.43e-13 (36, 39, 33)          2.4e-14          3.9e-12
  VALU, 1 wave             1.81e-13 (40, 41, 40)          3.5e-14          4.1e-12
  VALU, 1 wave at l = 79   1.44e-13 (78, 79, 3)           --               7.9e-12
  staged <2>               5.3e-14  (0, 15, 130)          1.0e-14          1.5e-12
  staged <3>               9.4e-14  (2, 23, 70)           3.3e-14          2.3e-12
  staged <5>               9.6e-14  (24, 24, 33)          3.4e-14          2.4e-12

The identity rows were bit-equal to the input and a second run gave the same bits in every case; no case found a fault.
Wall time of the module run alone: 27.5 s for its 48 tests (13 s of that is the first import of torch and the start of the
runtime in test_constant_rotor, which a run of the whole suite has paid before); the (79, 79, 3) case takes 4.7 s, nearly all of
it the oracle.
"""
import functools

import numpy as np
import pytest

from oracle import rotations_ref, wigner

pytestmark = pytest.mark.gpu

STAGED, VALU = "SCRI_AMD_ROTATE_STAGED", "SCRI_AMD_ROTATE_VALU"
RESIDENT_KERNEL, STAGED_KERNEL, VALU_KERNEL = 0, 1, 2
TINY = (1e-16, 9e-16, 1.1e-15, 1e-12, 1e-8, 1e-4)


def _special_rotors():
    """(Ra, Rb) pairs, normalised: see the module docstring"""
    out = [(1.0 + 0j, 0j), (-1.0 + 0j, 0j)]
    out += [(np.exp(1j * a), 0j) for a in (0.3, 1.7, -2.9)]
    out += [(0j, np.exp(1j * b)) for b in (0.4, -1.3, 2.6)]
    for k, e in enumerate(TINY):
        big, small = np.sqrt(1.0 - e * e) * np.exp(1j * (0.5 + k)), e * np.exp(1j * (2.0 - 0.7 * k))
        out += [(big, small), (small, big)]  # |Rb| = e, then |Ra| = e
    return out


SPECIAL = _special_rotors()
IDENTITY_ROW = 0  # index into SPECIAL


def _special_rows(n):
    rows = {0, n - 1}
    for k in range(16, n, 16):
        rows |= {k - 1, k}
    return sorted(rows)


def _rotor_set(n, rng, first_special):
    """spinors complex [n, 2] and {row: index into SPECIAL}; the cycle over SPECIAL starts at `first_special`, which differs from case
    to case so that the short cases do not all see the same few rotors"""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    sp = np.stack([q[:, 0] + 1j * q[:, 3], q[:, 2] + 1j * q[:, 1]], axis=-1)
    which = {}
    for i, row in enumerate(_special_rows(n)):
        k = (first_special + i) % len(SPECIAL)
        sp[row] = SPECIAL[k]
        which[row] = k
    return sp, which


def _block_norms(a, ell_min, ell_max):
    return np.stack([np.linalg.norm(a[:, l * l - ell_min**2 : (l + 1) ** 2 - ell_min**2], axis=1) for l in range(ell_min, ell_max + 1)], axis=1)


@functools.lru_cache(maxsize=None)
def _case(ell_min, ell_max, n):
    """data, spinors, special rows and the oracle's rotation of a shape -- computed once, shared and never written to"""
    rng = np.random.default_rng(1000 * ell_max + 10 * ell_min + n)
    nm = (ell_max + 1) ** 2 - ell_min**2
    data = rng.normal(size=(n, nm)) + 1j * rng.normal(size=(n, nm))
    sp, which = _rotor_set(n, rng, first_special=_FIRST_SPECIAL.get((ell_min, ell_max, n), 0))
    expect = rotations_ref.rotate_by_series(data, sp, ell_min, ell_max)
    # the oracle on this rotor set is a rotation: the norm of every l block of every row is kept
    n_in, n_out = _block_norms(data, ell_min, ell_max), _block_norms(expect, ell_min, ell_max)
    assert np.abs(n_out / n_in - 1.0).max() < 1e-13
    for a in (data, sp, expect):
        a.setflags(write=False)
    return data, sp, which, expect


def _case_79():
    """(79, 79, 3): the l = 79 columns of the shared (78, 79, 3) reference (a rotation acts on each l block alone)"""
    data, sp, which, expect = _case(78, 79, 3)
    c0 = 79 * 79 - 78 * 78
    return np.ascontiguousarray(data[:, c0:]), sp, which, np.ascontiguousarray(expect[:, c0:])


def _set_route(route, name):
    """name: STAGED, VALU or None (the default route); the other switch is cleared (the suite may run with one exported)"""
    for other in (STAGED, VALU):
        if other != name:
            route(other, None)
    if name:
        route(name)


def _waves(ell_max):
    return 4 if ell_max <= 19 else 3 if ell_max <= 26 else 2 if ell_max <= 39 else 1


def _assert_stats(stats, kernel, ell_max, resident_too=False):
    """exactly one launch of `kernel` (and of no other, but for leading resident segments where the case has them)"""
    res, staged, valu, waves = stats
    assert (res >= 1) if resident_too else (res == 0), stats
    assert staged == (1 if kernel == STAGED_KERNEL else 0), stats
    assert valu == (1 if kernel == VALU_KERNEL else 0), stats
    assert waves == (_waves(ell_max) if kernel == VALU_KERNEL else 0), stats


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _run_series(ctx, data, sp, ell_min, ell_max):
    from scri_amd import engine

    ctx.rotate_stats(reset=True)
    got = engine.rotate_series(data.copy(), ell_min, ell_max, sp, ctx=ctx)
    return got, ctx.rotate_stats(reset=True)


# (build, route, (ell_min, ell_max, n), kernel, leading resident segments)
CASES = [
    ("valu4", VALU, (0, 3, 1), VALU_KERNEL, False),
    ("valu4", VALU, (2, 8, 129), VALU_KERNEL, False),
    ("valu4", VALU, (5, 19, 127), VALU_KERNEL, False),
    ("valu3", VALU, (19, 20, 97), VALU_KERNEL, False),
    ("valu3", VALU, (2, 26, 50), VALU_KERNEL, False),
    ("valu2", VALU, (26, 27, 65), VALU_KERNEL, False),
    ("valu2", None, (34, 35, 97), VALU_KERNEL, False),
    ("valu2", None, (36, 39, 33), VALU_KERNEL, False),
    ("valu2", None, (0, 34, 5), VALU_KERNEL, True),  # resident segments, then a VALU tail 28..34
    ("valu1", None, (40, 41, 40), VALU_KERNEL, False),
    ("staged2", STAGED, (0, 0, 3), STAGED_KERNEL, False),
    ("staged2", STAGED, (1, 1, 17), STAGED_KERNEL, False),
    ("staged2", STAGED, (2, 8, 65), STAGED_KERNEL, False),
    ("staged2", STAGED, (14, 15, 63), STAGED_KERNEL, False),
    ("staged2", STAGED, (0, 15, 130), STAGED_KERNEL, False),
    ("staged3", STAGED, (15, 16, 64), STAGED_KERNEL, False),
    ("staged3", STAGED, (22, 23, 1), STAGED_KERNEL, False),
    ("staged3", STAGED, (2, 23, 70), STAGED_KERNEL, False),
    ("staged5", STAGED, (23, 24, 65), STAGED_KERNEL, False),
    ("staged5", STAGED, (24, 24, 33), STAGED_KERNEL, False),
    ("staged5", STAGED, (2, 33, 20), STAGED_KERNEL, False),
    ("staged5", None, (28, 33, 65), STAGED_KERNEL, False),
    ("staged5", None, (0, 30, 5), STAGED_KERNEL, True),  # resident segments, then a staged tail 28..30
    ("valu2", STAGED, (33, 34, 10), VALU_KERNEL, False),  # staged asked for but impossible at l = 34: the VALU kernel serves it
]

# the smallest multi-tile shape of each build, for the further tests
MULTI_TILE = [
    ("valu4", VALU, (2, 8, 129), VALU_KERNEL),
    ("valu3", VALU, (19, 20, 97), VALU_KERNEL),
    ("valu2", VALU, (26, 27, 65), VALU_KERNEL),
    ("valu1", None, (40, 41, 40), VALU_KERNEL),
    ("staged2", STAGED, (2, 8, 65), STAGED_KERNEL),
    ("staged3", STAGED, (2, 23, 70), STAGED_KERNEL),
    ("staged5", STAGED, (23, 24, 65), STAGED_KERNEL),
]


# where the cycle over SPECIAL starts in each case: where the previous case of the same build left it, so that the cases of a build
# together see as much of the set as their rows allow ((78, 79, 3) carries the l = 79 case of the 1-wave VALU build)
_FIRST_SPECIAL = {}
_next = {}
for _build, _shape in [(c[0], c[2]) for c in CASES] + [("valu1", (78, 79, 3))]:
    _FIRST_SPECIAL[_shape] = _next.get(_build, 0) % len(SPECIAL)
    _next[_build] = _next.get(_build, 0) + len(_special_rows(_shape[2]))


def _id(c):
    return f"{c[0]}-{'default' if c[1] is None else c[1].split('_')[-1].lower()}-{'_'.join(map(str, c[2]))}"


def _check_series(ctx, build, route_name, shape, kernel, resident_too, data, sp, which, expect):
    ell_min, ell_max, n = shape
    got, stats = _run_series(ctx, data, sp, ell_min, ell_max)
    _assert_stats(stats, kernel, ell_max, resident_too)
    err = np.abs(got - expect).max()
    print(f"ROUTES {build} {route_name or 'default'} {shape} series err {err:.3e} bound {1e-13 * max(ell_max, 1):.1e}")
    assert err < 1e-13 * max(ell_max, 1)
    for row, k in which.items():  # the kernels' headers promise it: the identity leaves a row as it is
        if k == IDENTITY_ROW:
            assert _same_bits(got[row], data[row]), row
    again, stats2 = _run_series(ctx, data, sp, ell_min, ell_max)
    assert stats2 == stats and _same_bits(again, got)


@pytest.mark.parametrize("build,route_name,shape,kernel,resident_too", CASES, ids=[_id(c) for c in CASES])
def test_series_matches_the_oracle_on_its_kernel_build(ctx, route, build, route_name, shape, kernel, resident_too):
    _set_route(route, route_name)
    _check_series(ctx, build, route_name, shape, kernel, resident_too, *_case(*shape))


def test_last_supported_ell_79(ctx, route):
    """(79, 79, 3): the 1-wave VALU build where its LDS holds 162 816 of 163 840 bytes.  Alone in a test: the oracle needs
    4.7 s for it (its cost grows like l^3 per l however few the rows; the reference is shared with the table-growth test)."""
    _set_route(route, None)
    _check_series(ctx, "valu1", None, (79, 79, 3), VALU_KERNEL, False, *_case_79())


@functools.lru_cache(maxsize=None)
def _constant_case(ell_min, ell_max):
    """four constant rotors (generic, identity, pure z rotation, flip) as quaternions, and the oracle's D of each (one call)"""
    q = np.array([[0.3, 0.1, -0.7, 0.2], [1.0, 0.0, 0.0, 0.0], [np.cos(0.6), 0.0, 0.0, np.sin(0.6)], [0.0, np.sin(1.1), np.cos(1.1), 0.0]])
    q[0] /= np.linalg.norm(q[0])
    D = wigner.wigner_D_matrices(q[:, 0] + 1j * q[:, 3], q[:, 2] + 1j * q[:, 1], ell_min, ell_max)
    return q, D


@pytest.mark.parametrize("build,route_name,shape,kernel", MULTI_TILE, ids=[_id(c) for c in MULTI_TILE])
def test_constant_rotor(ctx, route, build, route_name, shape, kernel):
    """rotor_stride 0; the exact branches (identity, pure z rotation, flip) run on every row of every tile -- through the host
    entry (engine.rotate_const) and, device-resident, through rotate_device(quaternion=...)"""
    import torch

    from scri_amd import engine

    ell_min, ell_max, n = shape
    _set_route(route, route_name)
    data = _case(*shape)[0]
    q, D = _constant_case(ell_min, ell_max)
    for k, name in enumerate(("generic", "identity", "z", "flip")):
        expect = rotations_ref.rotate_by_constant(data, ell_min, ell_max, D[k])
        ctx.rotate_stats(reset=True)
        got = engine.rotate_const(data.copy(), ell_min, ell_max, q[k], ctx=ctx)
        _assert_stats(ctx.rotate_stats(reset=True), kernel, ell_max)
        err = np.abs(got - expect).max()
        print(f"ROUTES {build} {route_name or 'default'} {shape} constant-{name} err {err:.3e} bound {1e-13 * max(ell_max, 1):.1e}")
        assert err < 1e-13 * max(ell_max, 1)
        if name == "identity":
            assert _same_bits(got, data)
        d = torch.from_numpy(data.copy()).to("cuda:0")
        torch.cuda.synchronize()
        engine.rotate_device(d.data_ptr(), n, data.shape[1], ell_min, ell_max, quaternion=q[k], ctx=ctx)
        ctx.synchronize()
        _assert_stats(ctx.rotate_stats(reset=True), kernel, ell_max)
        assert _same_bits(d.cpu().numpy(), got)


@pytest.mark.parametrize("build,route_name,shape,kernel", MULTI_TILE, ids=[_id(c) for c in MULTI_TILE])
def test_device_resident_with_a_wide_row_stride(ctx, route, build, route_name, shape, kernel):
    """ld = n_modes + 3: the three pad columns and 40 rows past the end come back as they were, the mode columns match the oracle"""
    import torch

    from scri_amd import engine

    ell_min, ell_max, n = shape
    _set_route(route, route_name)
    data, sp, which, expect = _case(*shape)
    nm = data.shape[1]
    ld = nm + 3
    sentinel = complex(-7.25e300, 3.5e-300)
    host = np.full((n + 40, ld), sentinel, dtype=complex)
    host[:n, :nm] = data
    d = torch.from_numpy(host).to("cuda:0")
    d_sp = torch.from_numpy(sp.copy()).to("cuda:0")
    torch.cuda.synchronize()
    ctx.rotate_stats(reset=True)
    engine.rotate_device(d.data_ptr(), n, ld, ell_min, ell_max, spinors_ptr=d_sp.data_ptr(), ctx=ctx)
    ctx.synchronize()
    _assert_stats(ctx.rotate_stats(reset=True), kernel, ell_max)
    back = d.cpu().numpy()
    assert _same_bits(back[:n, nm:], host[:n, nm:]) and _same_bits(back[n:], host[n:])
    assert np.abs(back[:n, :nm] - expect).max() < 1e-13 * max(ell_max, 1)


@pytest.mark.parametrize("build,route_name,shape,kernel", MULTI_TILE, ids=[_id(c) for c in MULTI_TILE])
def test_rows_are_isolated(ctx, route, build, route_name, shape, kernel):
    """NaN in every mode of one mid-tile row and of the last row: every other row has the bits of the run without them"""
    ell_min, ell_max, n = shape
    _set_route(route, route_name)
    data, sp, which, expect = _case(*shape)
    clean, stats = _run_series(ctx, data, sp, ell_min, ell_max)
    _assert_stats(stats, kernel, ell_max)
    bad = [7, n - 1]
    poisoned = data.copy()
    poisoned[bad] = complex(np.nan, np.nan)
    got, stats = _run_series(ctx, poisoned, sp, ell_min, ell_max)
    _assert_stats(stats, kernel, ell_max)
    keep = np.setdiff1d(np.arange(n), bad)
    assert _same_bits(got[keep], clean[keep])
    assert np.abs(clean - expect).max() < 1e-13 * max(ell_max, 1)


def test_tables_grow_and_a_larger_table_serves_a_smaller_call(route):
    """ensure_delta / ensure_delta_mfma on a context of the test's own: ell_max 12, 39, 20, 79 through the VALU kernel, then 12, 33, 16
    through the staged one -- a later call that asks for a larger l regrows the table, a smaller one reuses the larger table"""
    from scri_amd import _lib

    _set_route(route, VALU)
    own = _lib.Context(0)  # (created with the switch exported: it starts with it)
    try:
        for name, kernel, shapes in ((VALU, VALU_KERNEL, [(11, 12, 5), (38, 39, 5), (19, 20, 97), (78, 79, 3)]),
                                     (STAGED, STAGED_KERNEL, [(11, 12, 5), (32, 33, 5), (15, 16, 64)])):
            _set_route(route, name)
            for shape in shapes:
                ell_min, ell_max, n = shape
                data, sp, which, expect = _case(*shape)
                got, stats = _run_series(own, data, sp, ell_min, ell_max)
                _assert_stats(stats, kernel, ell_max)
                err = np.abs(got - expect).max()
                print(f"ROUTES growth {name.split('_')[-1]} {shape} err {err:.3e}")
                assert err < 1e-13 * ell_max, (name, shape)
    finally:
        own.close()


def test_refusal_beyond_79_is_decided_on_the_host(ctx, route):
    """(80, 80, 2): unsupported, before any launch; the data is untouched and the stats stay zero"""
    from scri_amd import engine

    _set_route(route, None)
    rng = np.random.default_rng(80)
    data = rng.normal(size=(2, 161)) + 1j * rng.normal(size=(2, 161))
    sp = _rotor_set(2, rng, 0)[0]
    work = data.copy()
    ctx.rotate_stats(reset=True)
    with pytest.raises(NotImplementedError, match="too large for the rotation kernels"):
        engine.rotate_series(work, 80, 80, sp, ctx=ctx)
    assert ctx.rotate_stats(reset=True) == (0, 0, 0, 0)
    assert _same_bits(work, data)
