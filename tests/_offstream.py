"""Arena test bodies again, off the default stream: the header promises that an entry point enqueues on its `stream` argument,
never synchronises and never allocates (include/vitssl_hip.h), and every arena test takes that argument from
torch.cuda.current_stream().  The `offstream` fixture of this module (a plain module, imported by the test files; no conftest)
runs such a body unchanged with a side stream current and turns a launch on another stream, or a host wait, into a failure.

    offstream(mode, body, *args)          mode: "gate" | "graph"

First the body runs once on the default stream (the first use of a kernel loads code objects and sets function attributes);
that run also records which launching calls were refused.  Then it runs with a non-blocking pool stream current, every Arena
it creates registered, and every launching function of the library wrapped (vitssl_hip._lib.lib() hands out the wrappers, so
_lib.call and the direct `L.lib().vitssl_x(...)` calls of some bodies both pass through them).

gate, per wrapped call: synchronise; clone every arena; fill every fp32 / bf16 / e4m3 region with 0xFF (NaN), inputs and outputs
alike; synchronise; enqueue on the side stream a gate of >= GATE_MS that holds the stream without blocking the host, then the
device-to-device restore of the clones, then event `pre`; make the call; assert `not pre.query()`.
  * A launch on any other stream runs at once, on NaN inputs, and the restore then puts the poison back over its outputs: the
    body's own NaN / parity / repeat-bits assertions fail.
  * An entry point that waits for its stream or the device returns after `pre` has completed: the assertion names it.
Integer regions (int32, int64, uint8) are never poisoned: indices, labels and device job tables hold offsets and pointers, and
a stray kernel must read NaN, not a wild address.

graph, per wrapped call: clone; capture the call on the side stream with torch.cuda.graph (a legacy-stream operation, a
synchronisation or an allocation inside the entry point fails the capture); poison; restore; replay once; synchronise.  Calls the
warm-up saw refused, and the atomic (workspace = NULL) form of the two single TN GEMMs, are made directly: the one launches
nothing, the other is parity-only.

The gate length is a condition, not a tolerance: sized once per session with events; a case whose call returns late fails."""
import functools
import glob
import os
import re

import pytest
import torch

from _arena import POISON, Arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_MS = 50.0
MAX_ARENA_MIB = 128                     # larger arenas may stay out of the twins (two clones of the arena per wrapped call)
POISONED = (torch.float32, torch.bfloat16, torch.float8_e4m3fn)
ATOMIC_TN = ("vitssl_gemm_bf16_tn", "vitssl_gemm_fp8_tn")           # (..., workspace, workspace_floats, stream)
MODES = ("gate", "graph")


# ------------------------------------------------------------------------------------------------ the headers
def headers():
    return sorted(glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "include_ext", "*.h")))


def prototypes(path):
    """name -> parameter text of every function a header declares"""
    txt = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    txt = re.sub(r"//.*$", "", txt, flags=re.M)
    return {m.group(2): m.group(3) for m in re.finditer(r"\b(int|int64_t|const char\s*\*)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def launching(path=None):
    """the functions that take a `void* stream` (of one header, or of all of them)"""
    paths = [path] if path else headers()
    return {n for p in paths for n, args in prototypes(p).items() if re.search(r"void\s*\*\s*stream\b", args)}


# ------------------------------------------------------------------------------------------------ the gate
_cycles_per_ms = None


def _spin_ms(cycles):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    torch.cuda._sleep(int(cycles))
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def hold(ms=GATE_MS):
    """Enqueue on the current stream a kernel that spins for at least `ms` milliseconds; the host does not wait.  The spin is
    calibrated once per session against an event pair, and the calibrated GATE_MS gate is itself timed before it is trusted."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        cycles = 1 << 20
        _spin_ms(cycles)                                    # loads the spin kernel
        t = _spin_ms(cycles)
        while t < 5.0:                                      # long enough for the event pair to resolve
            cycles *= 4
            t = _spin_ms(cycles)
        rate = cycles / t
        for _ in range(8):
            got = _spin_ms(rate * GATE_MS * 1.25)
            if got >= GATE_MS * 1.1:
                break
            rate *= 1.5
        assert got >= GATE_MS, f"the gate lasts {got:.1f} ms, {GATE_MS} ms are required"
        _cycles_per_ms = rate
    torch.cuda._sleep(int(_cycles_per_ms * ms * 1.25))


# ------------------------------------------------------------------------------------------------ the wrappers
class _Lib:
    """stands for the ctypes library: launching functions come out wrapped, everything else as it is"""

    def __init__(self, real, wrap, names):
        self._real, self._wrap, self._names = real, wrap, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        return functools.partial(self._wrap, name, fn) if name in self._names else fn


_WARM = {}          # body and case -> [(entry point, return code)] of its launching calls in order, from the default-stream run


class OffStream:
    def __init__(self, monkeypatch):
        self.mp, self.arenas, self.side, self.inject = monkeypatch, [], None, None
        self.log, self.k = None, 0

    # ---- what the wrappers do
    def _record(self, name, fn, *args):
        rc = fn(*args)
        self.log.append((name, rc))
        return rc

    def _save(self):
        return [(a, a.buf.clone()) for a in self.arenas]

    def _poison(self):
        for a in self.arenas:
            for (_, s, e, _), dt in zip(a.regions, a.dtypes):
                if dt in POISONED:
                    a.buf[s:e].fill_(POISON)

    @staticmethod
    def _restore(saved):
        for a, c in saved:
            a.buf.copy_(c)

    def _gated(self, name, fn, *args):
        torch.cuda.synchronize()
        saved = self._save()
        self._poison()
        torch.cuda.synchronize()
        hold(GATE_MS)
        self._restore(saved)
        pre = torch.cuda.Event()
        pre.record()
        rc = fn(*args)
        if self.inject is not None:
            self.inject()
        assert not pre.query(), (f"{name} returned only after the work enqueued in front of it on its stream had finished "
                                 f"(a gate of >= {GATE_MS} ms): it waits for the stream or the device")
        return rc

    def _graphed(self, name, fn, *args):
        assert self.k < len(self.log) and self.log[self.k][0] == name, f"call {self.k} is {name}, the default-stream run made {self.log[self.k:self.k + 1]}"
        refused = self.log[self.k][1] != 0
        self.k += 1
        if refused or (name in ATOMIC_TN and not getattr(args[-3], "value", args[-3])):
            return fn(*args)
        torch.cuda.synchronize()
        saved = self._save()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=self.side):
            rc = fn(*args)
        assert rc == 0, f"{name} returned {rc} under capture and 0 on the default stream"
        self._poison()
        torch.cuda.synchronize()
        self._restore(saved)
        g.replay()
        torch.cuda.synchronize()
        return rc

    # ---- the run
    def __call__(self, mode, body, *args, inject=None):
        from vitssl_hip import _lib
        assert mode in MODES
        real, names = _lib.lib(), launching()
        key = (body.__module__, body.__qualname__, tuple(getattr(a, "id", a) for a in args if not callable(a)))
        if key not in _WARM:
            self.log = []
            with self.mp.context() as m:
                m.setattr(_lib, "lib", lambda: _Lib(real, self._record, names))
                body(*args)
            torch.cuda.synchronize()
            _WARM[key] = self.log
        self.log, self.k, self.inject = _WARM[key], 0, inject
        self.side = torch.cuda.Stream()                     # a pool stream: non-blocking, the null stream does not wait for it
        init, arenas = Arena.__init__, self.arenas

        def registering(a, *p, **kw):
            init(a, *p, **kw)
            arenas.append(a)
        wrap = self._gated if mode == "gate" else self._graphed
        try:
            with self.mp.context() as m:
                m.setattr(Arena, "__init__", registering)
                m.setattr(_lib, "lib", lambda: _Lib(real, wrap, names))
                with torch.cuda.stream(self.side):
                    body(*args)
        finally:
            torch.cuda.synchronize()                        # a gate left behind by a failed call drains here
            del self.arenas[:]


@pytest.fixture
def offstream(monkeypatch):
    return OffStream(monkeypatch)


def twin_of(test, modes=MODES):
    """Decorator for `<test>_off_stream`: the marks of `test` (its parametrisation, the gpu marker) and the mode as one parameter
    more.  tests/test_abi_arena.py (no GPU) checks that every arena test has such a twin."""
    def mark(twin):
        twin.pytestmark = list(getattr(test, "pytestmark", [])) + [pytest.mark.parametrize("mode", list(modes)).mark]
        return twin
    return mark
