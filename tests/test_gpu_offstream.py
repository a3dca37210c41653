"""The off-stream fixture of tests/_offstream.py can fail: its gate is as long as it claims, a launch on another stream than the
current one fails the body, and a host wait after the call trips the `pre` event.  Float inputs only, every access inside the
arena's one allocation: nothing here can fault."""
import ctypes as C
import time

import pytest
import torch

from _arena import Arena
from _offstream import GATE_MS, hold, offstream  # noqa: F401  (offstream is a fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16 = torch.bfloat16


def _cast_body(handle=None):
    """vitssl_cast_bf16 of 300 x 64 floats on the current stream, or on the stream whose handle is given"""
    from vitssl_hip import _lib as L
    torch.manual_seed(3)
    a = Arena(DEV, mib=8)
    rows, cols = 300, 64
    n = rows * cols
    v = torch.randn(rows, cols)
    src, dst = a.put("src", v), a.empty("dst", (rows, cols), BF16)
    s = torch.cuda.current_stream().cuda_stream if handle is None else handle
    L.call("vitssl_cast_bf16", C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), n, C.c_void_p(s))
    torch.cuda.synchronize()
    a.check()
    assert torch.equal(dst.cpu(), v.to(BF16)), "dst is not the cast of src"


def test_gate_holds_its_stream_and_not_the_host():
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hold()                                              # calibrates on first use
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        w = time.perf_counter()
        hold()
        t1.record()
        host_ms = (time.perf_counter() - w) * 1e3
        assert not t1.query() and host_ms < GATE_MS / 2, f"enqueueing the gate took the host {host_ms:.1f} ms"
        t1.synchronize()
    print(f"gate: {t0.elapsed_time(t1):.1f} ms on the stream, {host_ms:.2f} ms on the host")
    assert t0.elapsed_time(t1) >= GATE_MS


@pytest.mark.parametrize("mode", ["gate", "graph"])
def test_right_stream_passes(mode, offstream):
    offstream(mode, _cast_body)


def test_control_launch_on_the_default_stream_fails_the_body(offstream):
    """(a) the default stream's handle in place of the current one: the kernel runs at once, on the NaN the fixture put into `src`,
    and the restore behind the gate then puts the 0xFF poison back over `dst`: the body's equality check must fail."""
    with pytest.raises(AssertionError, match="dst is not the cast of src"):
        offstream("gate", _cast_body, torch.cuda.default_stream().cuda_stream)


def test_control_host_wait_trips_the_pre_event(offstream):
    """(b) a wait for the side stream right after the wrapped call, as an entry point that synchronises would do it"""
    with pytest.raises(AssertionError, match="vitssl_cast_bf16 returned only after"):
        offstream("gate", _cast_body, inject=lambda: torch.cuda.current_stream().synchronize())
