"""GPU: ctx->chain_buf grows in the middle of a queue. The companion of tests/test_gpu_call_sequences.py::test_scratch_grows_mid_queue for the
chain buffer, which grows through the same vszip_reserve (csrc/ctx.hip) as the scratch buffer and the XPSNR block sums: synchronise, free,
reallocate, in the middle of whatever is queued."""
import numpy as np
import pytest

import fixtures as fx
from test_gpu_call_sequences import _differ, _same

pytestmark = pytest.mark.gpu


def test_chain_buffer_grows_mid_queue():
    """Three vszip_chain_run calls on one context with no host synchronise in between - u8 planes of 64 x 48, then of 256 x 192, then of
    64 x 48 again, each with its own content; BoxBlur r = 2 then Limiter on all planes, so every plane has two writers and goes through its
    intermediates. Expected: the same call made alone on a fresh context."""
    import vszip_amd

    stages = [{"boxblur": (2, 1, 2, 1)}, {"limiter": ([16.0, 16.0, 16.0], [235.0, 240.0, 240.0])}]
    calls = [[fx.splitmix64_plane(7000 + 10 * c + i, shape, np.uint8) for i in range(3)] for c, shape in enumerate([(48, 64), (192, 256), (48, 64)])]

    def run(d, calls):
        tables = [([d.upload(p) for p in planes], [d.empty(p.shape[0], p.shape[1], np.uint8) for p in planes]) for planes in calls]  # (uploads synchronise: all before the first call)
        for srcs, dsts in tables:
            d.chain_run(stages, srcs, dsts, [0, 1, 2])
        return [[d.download(o) for o in dsts] for _, dsts in tables]

    d = vszip_amd.Device(0)
    try:
        got = run(d, calls)
    finally:
        d.close()
    for c, planes in enumerate(calls):
        alone = vszip_amd.Device(0)
        try:
            want = run(alone, [planes])[0]
        finally:
            alone.close()
        for i, (g, w) in enumerate(zip(got[c], want)):
            assert _same(g, w), f"call {c} plane {i}: {_differ(g, w)} bytes differ from the call alone"
        assert not any(_same(w, p) for w, p in zip(want, planes))  # (the stages did something)
