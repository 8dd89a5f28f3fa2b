"""The one-launch lf_free's block of launch-invariant arguments (lf_free.h: FreeBlock; lfmcmc.hip: free_block): uploaded on
first use and whenever its bytes change - a reallocated buffer, an option - and never in steady state; every result bitwise
equal to a fresh context's with the same settings, on any stream."""
import numpy as np
import pytest

from lf_testlib import make_inputs, synth

pytestmark = pytest.mark.gpu

N = 200003


@pytest.fixture(scope="module")
def inp():
    return make_inputs("free", N, seed=311)


def _ctx(inp, opts=()):
    from lumfuncmcmc_amd.capi import LFContext
    ctx = LFContext(inp)
    ctx.set_option("persistent", 2)
    for k, v in opts:
        ctx.set_option(k, v)
    return ctx


def _fresh(inp, opts, th):
    ctx = _ctx(inp, opts)
    out = ctx.lnprob_batch(th)
    ctx.close()
    return out


def _rows(B, seed):
    th = synth.walkers("free", B, seed=seed)
    th[1, 0] = 40.2                 # underflow zone: -inf
    th[2, 1] = 6.0                  # outside the prior
    return th


def test_steady_state_makes_no_uploads(inp):
    ctx = _ctx(inp)
    th = [_rows(128, 320 + i) for i in range(3)]
    first = [ctx.lnprob_batch(t) for t in th]
    info = ctx.last_launch()
    assert info["fused"] and info["kernel"] == "lf_free<%d>" % info["st"], info
    n0 = ctx.free_block_uploads()
    assert n0 >= 1
    again = [ctx.lnprob_batch(th[i % 3]) for i in range(12)]
    assert ctx.free_block_uploads() == n0
    for i, a in enumerate(again):
        np.testing.assert_array_equal(a, first[i % 3])
    ctx.close()


def test_changes_upload_the_block_and_match_a_fresh_context(inp):
    ctx = _ctx(inp)
    opts = {}
    steps = [(None, 128), (("cells", 0), 128), (("cells", 1), 128), (("grid_shortcut", 0), 128), (("grid_shortcut", 1), 128),
             (None, 256), (None, 128), (("poll", 0), 128), (("poll", 1), 128)]
    seen = ctx.free_block_uploads()
    for i, (opt, B) in enumerate(steps):
        if opt is not None:
            ctx.set_option(*opt)
            opts[opt[0]] = opt[1]
        th = _rows(B, 330 + i)
        got = ctx.lnprob_batch(th)
        assert ctx.last_launch()["fused"], (opt, B)
        n = ctx.free_block_uploads()
        # the first use and an option that changes the arguments each bring a new block; 256 rows grow the partial-sum
        # buffers (a new block unless the allocator hands back the same addresses); the way back to 128 rows keeps them
        if opt is not None or i == 0:
            assert n == seen + 1, (opt, B, seen, n)
        elif B == 256:
            assert n in (seen, seen + 1), (opt, B, seen, n)
        else:
            assert n == seen, (opt, B, seen, n)
        seen = n
        want = _fresh(inp, sorted(opts.items()), th)
        assert np.isfinite(got).sum() > B // 2
        np.testing.assert_array_equal(got, want, err_msg=str((opt, B)))
        again = ctx.lnprob_batch(th)
        assert ctx.free_block_uploads() == seen
        np.testing.assert_array_equal(again, got)
    ctx.close()


def test_stream_switches(inp):
    import torch
    ctx = _ctx(inp)
    th = [_rows(128, 340 + i) for i in range(4)]
    want = [ctx.lnprob_batch(t) for t in th]
    n0 = ctx.free_block_uploads()
    dth = [torch.from_numpy(t).cuda() for t in th]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((128,), np.nan, dtype=torch.float64, device="cuda") for _ in range(8)]
    for i in range(8):
        with torch.cuda.stream(streams[i % 2]):
            ctx.lnprob_torch(dth[i % 4], out=outs[i])
        if i == 3:
            ctx.lnprob_batch(th[0])                     # the context's own stream in between
    torch.cuda.synchronize()
    for i in range(8):
        np.testing.assert_array_equal(outs[i].cpu().numpy(), want[i % 4])
    assert ctx.free_block_uploads() == n0
    ctx.close()
