"""engine.HostStage, the pinned ring the masked-image models stage their index tables through: every upload arrives whole, in
the dtypes it was given, on the current stream, and stays untouched until the ring comes round.

(The file's name sorts after test_gpu_offstream.py: the default-stream control case there depends on how many pool streams the
session has created before it, and the side stream below would be one more.)"""
import contextlib

import numpy as np
import pytest
import torch

from _offstream import hold

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOTS = 4


def tables(call):
    """int32[5], uint8[7], int32[0], int32[64]: other contents in every call"""
    rng = np.random.default_rng(100 + call)
    i32 = lambda n: rng.integers(-2 ** 31, 2 ** 31 - 1, n, dtype=np.int32)      # noqa: E731
    return [i32(5), rng.integers(0, 256, 7, dtype=np.uint8), i32(0), i32(64)]


@pytest.mark.parametrize("where", ["default stream", "side stream"])
def test_uploads_arrive_and_last_for_a_turn_of_the_ring(where):
    from vitssl_hip.engine import HostStage
    stage, calls = HostStage(slots=SLOTS), []
    side = where == "side stream"
    if side:      # the default stream is busy throughout: a copy that strayed onto it would not have run when the views are read
        hold(200.0)
    with torch.cuda.stream(torch.cuda.Stream()) if side else contextlib.nullcontext():
        for call in range(6):
            calls.append((tables(call), stage.upload(tables(call), DEV)))
            for back, (arrays, views) in enumerate(reversed(calls[-SLOTS:])):      # this call's views and those of the three before
                assert len(views) == len(arrays)
                for a, v in zip(arrays, views):
                    assert v.device == DEV and v.shape == (a.size,) and v.dtype == torch.from_numpy(a).dtype, (call, back)
                    assert np.array_equal(v.cpu().numpy(), a), (call, back, a.dtype, a.size)
    torch.cuda.synchronize()
