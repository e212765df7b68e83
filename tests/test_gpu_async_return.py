"""Stream-ordered return of bms_transform_modes / bms_transform_modes_shard (include/scri_amd.h): a warm call on
device-resident data, on a stream the caller gave, returns without waiting for the device; its result is ordered on that stream.

Shape: h, l = 2..4, supertranslation + frame rotation + boost on the 13 x 13 grid (the dense route with the evaluating product),
n = 70 and 200 rows: more than one 64-row tile of the product, and the straddle rows between tiles.

What is checked: the results are the bits of the same calls made with the option off, for calls queued back to back into ten
outputs and into one reused output read back through the stream; the counter of bms_ctx_get_async_stats rises by the number of warm
calls and stays where it is for a cold call, for host memory, for a context on its own stream, for a call that runs in several
chunks, and with the option off; an invalid argument still fails at the call.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ELL_MIN, ELL_MAX, N_CALLS = 2, 4, 10
N_MODES = (ELL_MAX + 1) ** 2 - ELL_MIN**2


def _case(n):
    """(t, [N_CALLS different inputs], transformation)"""
    from scri_amd import engine, synthetic

    t, data, spec = synthetic.workload("cfg3", n_times=n)
    data = np.ascontiguousarray(data[:, :N_MODES])
    rng = np.random.default_rng(n)
    inputs = [data * (rng.normal(size=N_MODES) + 1j * rng.normal(size=N_MODES)) for _ in range(N_CALLS)]
    kw = spec["kwargs"]
    lst = int(round(np.sqrt(len(kw["supertranslation"])))) - 1
    n_theta = 2 * (ELL_MAX + lst) + 1
    assert n_theta == 13
    tr = engine.make_transformation(kw["supertranslation"], kw["frame_rotation"], kw["boost_velocity"], n_theta, n_theta, ELL_MAX)
    return t, inputs, tr


def _call(ctx, t, x, tr, out, **kw):
    """one device-resident call: (t_out, n_new)"""
    from scri_amd import engine

    return engine.transform_modes(t, x.data_ptr(), ELL_MIN, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=ctx, device=True, ld=N_MODES,
                                  out_ptr=out.data_ptr(), **kw)


class _Side:
    """a torch side stream made current, and a context on it"""

    def __init__(self, **ctx_kw):
        import torch

        from scri_amd import _lib

        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.stream = torch.cuda.Stream(device=self.dev)
        self.guard = torch.cuda.stream(self.stream)
        self.guard.__enter__()
        self.ctx = _lib.Context(0, stream=self.stream.cuda_stream, **ctx_kw)

    def tensors(self, inputs, n, n_out_buffers):
        torch = self.torch
        xs = [torch.from_numpy(x).to(self.dev) for x in inputs]
        nan = complex(float("nan"), float("nan"))
        outs = [torch.full((n, N_MODES), nan, dtype=torch.complex128, device=self.dev) for _ in range(n_out_buffers)]
        self.stream.synchronize()
        return xs, outs

    def close(self):
        self.ctx.synchronize()
        self.ctx.close()
        self.guard.__exit__(None, None, None)


@pytest.fixture
def side():
    made = []

    def make(**kw):
        made.append(_Side(**kw))
        return made[-1]

    yield make
    for s in reversed(made):  # (the stream guards nest: the last one entered leaves first)
        s.close()


def _reference(s, t, xs, tr, out):
    """every call with the option off, waited for and read back: [(t_out, rows)]"""
    s.ctx.option("ASYNC_RETURN", 0)
    s.ctx.async_stats(reset=True)
    refs = []
    for x in [xs[0]] + xs:  # (the first call is the cold one)
        t_out, n_new = _call(s.ctx, t, x, tr, out)
        s.ctx.synchronize()
        refs.append((t_out.copy(), out[:n_new].cpu().numpy().copy()))
    assert s.ctx.async_stats() == (0, False), "the option is off: every call waits"
    return refs[1:]


@pytest.mark.parametrize("n", [70, 200])
def test_queued_calls_equal_the_waiting_calls_bit_for_bit(side, n):
    s = side()
    t, inputs, tr = _case(n)
    xs, outs = s.tensors(inputs, n, N_CALLS + 1)
    refs = _reference(s, t, xs, tr, outs[N_CALLS])
    s.ctx.option("ASYNC_RETURN", 1)  # (setting an option drops the kept tables: the next call is cold)
    _call(s.ctx, t, xs[0], tr, outs[N_CALLS])
    assert s.ctx.async_stats(reset=False)[0] == 0, "a cold call uploads its tables from host memory and waits"
    got = [_call(s.ctx, t, xs[i], tr, outs[i]) for i in range(N_CALLS)]  # no wait in between
    count, pending = s.ctx.async_stats(reset=False)
    assert count == N_CALLS and pending
    s.ctx.synchronize()
    assert s.ctx.async_stats() == (N_CALLS, False)
    for i, (t_out, n_new) in enumerate(got):
        assert n_new == refs[i][1].shape[0] and 8 < n_new <= n
        assert np.array_equal(t_out, refs[i][0])
        rows = outs[i][:n_new].cpu().numpy()
        assert np.isfinite(rows.view(float)).all()
        assert np.array_equal(rows, refs[i][1]), f"call {i}"
    assert not np.array_equal(refs[0][1], refs[1][1])  # (the inputs differ)


@pytest.mark.parametrize("n", [70, 200])
def test_one_output_buffer_reused_and_read_back_through_the_stream(side, n):
    import torch

    s = side()
    t, inputs, tr = _case(n)
    xs, (out,) = s.tensors(inputs, n, 1)
    refs = _reference(s, t, xs, tr, out)
    s.ctx.option("ASYNC_RETURN", 1)
    _call(s.ctx, t, xs[0], tr, out)  # cold
    host = [torch.empty((n, N_MODES), dtype=torch.complex128).pin_memory() for _ in range(N_CALLS)]
    n_new = []
    for i in range(N_CALLS):
        n_new.append(_call(s.ctx, t, xs[i], tr, out)[1])
        host[i].copy_(out, non_blocking=True)  # (on the current stream = the context's: behind call i, ahead of call i + 1)
    assert s.ctx.async_stats(reset=False)[0] == N_CALLS
    s.stream.synchronize()
    for i in range(N_CALLS):
        assert np.array_equal(host[i][: n_new[i]].numpy(), refs[i][1]), f"call {i}"


def test_calls_that_keep_the_host_side_wait(side):
    from scri_amd import _lib, engine

    n = 200
    t, inputs, tr = _case(n)
    # a context on a caller's stream: device calls count once warm, host-memory calls never do
    s = side()
    xs, (out,) = s.tensors(inputs, n, 1)
    for i in range(3):
        _call(s.ctx, t, xs[i], tr, out)
    assert s.ctx.async_stats(reset=False)[0] == 2
    for i in range(2):
        t_h, rows_h = engine.transform_modes(t, inputs[i], ELL_MIN, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=s.ctx)
    assert s.ctx.async_stats(reset=False)[0] == 2, "host memory in and out: the call waits"
    s.ctx.synchronize()
    _, n_new = _call(s.ctx, t, xs[1], tr, out)
    assert s.ctx.async_stats()[0] == 3
    s.ctx.synchronize()
    assert rows_h.shape == (n_new, N_MODES) and np.abs(out[:n_new].cpu().numpy() - rows_h).max() <= 1e-13 * np.abs(rows_h).max()
    # an invalid argument fails at the call, warm or not (a row stride smaller than the number of modes; a NULL result)
    with pytest.raises(ValueError):
        engine.transform_modes(t, xs[0].data_ptr(), ELL_MIN, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=s.ctx, device=True, ld=N_MODES - 1,
                               out_ptr=out.data_ptr())
    with pytest.raises(ValueError):
        engine.transform_modes(t, xs[0].data_ptr(), ELL_MIN, ELL_MAX, -2, -1, engine.BMS_TERM_H, tr, ctx=s.ctx, device=True, ld=N_MODES, out_ptr=0)
    assert s.ctx.async_stats()[0] == 0
    _call(s.ctx, t, xs[2], tr, out)  # (and the context goes on working)
    assert s.ctx.async_stats()[0] == 1
    # the context's own stream: the caller has no handle to order on
    s.ctx.synchronize()
    own = _lib.Context(0)
    try:
        for i in range(3):
            _call(own, t, xs[i], tr, out)
        assert own.async_stats() == (0, False)
    finally:
        own.close()
    # a work-space cap that cuts the call into several chunks
    n_long = 600
    t_l, inputs_l, tr_l = _case(n_long)
    small = side(workspace_limit=3_400_000)
    small.ctx.enable_timing(True)
    xl, (out_l,) = small.tensors(inputs_l[:3], n_long, 1)
    for i in range(3):
        _call(small.ctx, t_l, xl[i], tr_l, out_l)
    launches = small.ctx.get_timing()["gemm_synthesis"][1]
    assert launches >= 2 * 3, f"{launches} product launches in 3 calls: the cap did not cut them into chunks"
    assert small.ctx.async_stats() == (0, False)
    # the option off, from the environment of the context's creation or by bms_ctx_set_option
    off = side()
    off.ctx.option("ASYNC_RETURN", 0)
    for i in range(3):
        _call(off.ctx, t, xs[i], tr, out)
    assert off.ctx.async_stats() == (0, False)
    assert off.ctx.option("ASYNC_RETURN") == 0 and s.ctx.option("ASYNC_RETURN") == 1


def test_environment_switches_the_default_off(side, monkeypatch):
    monkeypatch.setenv("SCRI_AMD_NO_ASYNC_RETURN", "1")
    s = side()
    assert s.ctx.option("ASYNC_RETURN") == 0
    monkeypatch.delenv("SCRI_AMD_NO_ASYNC_RETURN")
    assert side().ctx.option("ASYNC_RETURN") == 1
