#!/usr/bin/env python3
"""Launch trace of engine.EncoderStack on the host: no GPU, no library.

`engine.ops` is replaced by a recorder and the stack runs forward / backward on CPU tensors.  Every public `ops` call becomes one
line: the call's name and its arguments by parameter name (bound to the real signature, so positional and keyword spellings of one
call read alike).  A tensor is logged as dtype, shape and the buffer it is a view of, with its element offset: the name given to
`Workspace.get`, a weight image of the store (`w:` / `w8:` + key), `flat` / `gflat`, the fp8 scale state (`gs[key].field`) or the
step's inputs `x` / `g`.  A dropout descriptor is logged by its fields.  Arguments that are None or NO_DROP are left out.
`reducer.ready` ranges are lines too.  No line holds an address, so two trees that print the same digests enqueue the same
launches on the same operands in the same order.

The store's cast plans are stubs (their launches belong to FlatStore, not to the stack) and `droppath_table` returns its `out`;
`make_dropout` and `attn_family` run for real.

usage: python tools/stack_trace.py            one line per case: launches and sha256 of the trace
       python tools/stack_trace.py --dump     the full lines as well
       python tools/stack_trace.py --write    rewrite tests/golden/stack_schedule.json (call names and digest per case)"""
import contextlib
import ctypes
import hashlib
import inspect
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "stack_schedule.json")
BLOCKS, D, H, F, B, T = 3, 128, 2, 256, 2, 5
STEPS = 2

# name -> (operands, EncoderStack arguments, what one step runs)
CASES = {
    "bf16 plain": ("bf16", dict(p_drop=0.0), "step"),
    "bf16 dropout": ("bf16", dict(p_drop=0.1), "step"),
    "bf16 dropout droppath": ("bf16", dict(p_drop=0.1, drop_path=[0.0, 0.1, 0.2]), "step"),
    "bf16 droppath layerscale": ("bf16", dict(p_drop=0.0, drop_path=[0.0, 0.1, 0.2], layer_scale=True), "step"),
    "bf16 input_grad_only": ("bf16", dict(p_drop=0.1), "input_grad_only"),
    "bf16 forward only": ("bf16", dict(p_drop=0.1), "forward_only"),
    "bf16 return_attn": ("bf16", dict(p_drop=0.1), "return_attn"),
    "fp8 plain": ("fp8", dict(p_drop=0.0), "step"),
    "fp8 dropout": ("fp8", dict(p_drop=0.1), "step"),
    "fp8 two slots one scale_key": ("fp8", dict(p_drop=0.1), "two_slots"),
}


class _Names:
    """storage -> name of the buffer a tensor is a view of (the latest owner of an address wins: a freed buffer's address is reused)"""

    def __init__(self):
        self.by_ptr = {}
        self.late = []       # callables yielding (name, tensor) of buffers that appear while the stack runs

    def add(self, name, t):
        self.by_ptr[t.untyped_storage().data_ptr()] = name
        return t

    def of(self, t):
        ptr = t.untyped_storage().data_ptr()
        for src in self.late:
            for name, base in src():
                if base.untyped_storage().data_ptr() == ptr:
                    return name
        return self.by_ptr.get(ptr, "-")


class _StubPlan:
    """FlatStore's cast plans: the images exist, nothing is launched"""
    alpha = None

    def run(self, jobs):
        if self.alpha is None or self.alpha.numel() != len(jobs):
            self.alpha = torch.ones(len(jobs))


class Recorder:
    """Stands in for the module vitssl_hip.ops inside vitssl_hip.engine."""

    def __init__(self, real, names):
        self._real, self._names, self.lines = real, names, []
        self.NO_DROP, self.make_dropout, self.attn_family = real.NO_DROP, real.make_dropout, real.attn_family
        self.FP8, self.HD_SUPPORTED = real.FP8, real.HD_SUPPORTED
        self.CastPlan = self.CastPlanLd = self.Fp8WeightPlan = _StubPlan

    def _desc(self, v):
        if isinstance(v, torch.Tensor):
            off = f"+{v.storage_offset()}" if v.storage_offset() else ""
            return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}@{self._names.of(v)}{off}"
        if isinstance(v, ctypes.Structure):
            return type(v).__name__ + "(" + ",".join(f"{f[0]}={getattr(v, f[0])!r}" for f in v._fields_) + ")"
        if isinstance(v, (list, tuple)):
            return "(" + ",".join("None" if e is None else self._desc(e) for e in v) + ")"
        return repr(v)

    def log(self, name, bound):
        args = [f"{k}={self._desc(v)}" for k, v in bound.items() if v is not None and v is not self.NO_DROP]
        self.lines.append(name + " " + " ".join(args))

    def __getattr__(self, name):
        fn = getattr(self._real, name)       # an unknown name fails here as it would on the module
        if name.startswith("_") or not inspect.isfunction(fn):
            raise AttributeError(f"the stack reached for ops.{name}, which is not a public launch")
        sig = inspect.signature(fn)

        def call(*a, **kw):
            self.log(name, sig.bind(*a, **kw).arguments)
            return kw.get("out", a[3] if len(a) > 3 else None) if name == "droppath_table" else None
        return call


class _Block(nn.Module):
    """the parameter names and order of vit_core.encoder_block.EncoderBlock"""

    def __init__(self, layer_scale):
        super().__init__()
        att, ff = nn.Module(), nn.Module()
        att.w_query, att.w_key, att.w_value = (nn.Linear(D, D, bias=False) for _ in range(3))
        att.final_linear = nn.Linear(D, D, bias=False)
        ff.linear_in, ff.linear_out = nn.Linear(D, F), nn.Linear(F, D)
        self.self_attention, self.feed_forward = att, ff
        self.layer_norm1, self.layer_norm2 = nn.LayerNorm(D), nn.LayerNorm(D)
        if layer_scale:
            for k in (1, 2):
                ls = nn.Module()
                ls.gamma = nn.Parameter(torch.full((D,), 1e-5))
                setattr(self, f"layer_scale{k}", ls)


@contextlib.contextmanager
def _recording(operands):
    from vitssl_hip import engine
    names = _Names()
    rec = Recorder(engine.ops, names)
    real_ops, real_get, real_kind = engine.ops, engine.Workspace.get, engine._LINEAR_OPERANDS

    def get(self, name, shape, dtype, device):
        return names.add(name, real_get(self, name, shape, dtype, device))
    engine.ops, engine.Workspace.get = rec, get
    engine.set_linear_operands(operands)
    try:
        yield engine, rec, names
    finally:
        engine.ops, engine.Workspace.get, engine._LINEAR_OPERANDS = real_ops, real_get, real_kind


def trace(case):
    """-> the lines of one case"""
    operands, kw, mode = CASES[case]
    with _recording(operands) as (engine, rec, names):
        torch.manual_seed(0)
        model = nn.Module()
        model.encoder_blocks = nn.ModuleList(_Block(kw.get("layer_scale", False)) for _ in range(BLOCKS))
        dev = torch.device("cpu")
        st = engine.FlatStore(model, dev)
        stack = engine.EncoderStack(st, [f"encoder_blocks.{i}." for i in range(BLOCKS)], D, H, F, **kw)
        st.refresh_weights()
        names.add("flat", st.flat), names.add("gflat", st.gflat)
        for k, t in st._bf16.items():
            names.add("w:" + k, t)
        for k, t in st._fp8.items():
            names.add("w8:" + k, t)
        if st._fp8_plan is not None:
            names.add("alpha", st._fp8_plan.alpha)
        names.late.append(lambda: [(f"gs[{key}].{f}", t) for key, gs in stack._gs_by_slot.items() for f, t in gs.items() if f != "valid"])
        reducer = engine.GradReducer(st.gflat)
        assert reducer.world == 1
        ready = reducer.ready
        reducer.ready = lambda lo, hi: (rec.lines.append(f"reducer.ready {lo} {hi}"), ready(lo, hi))[1]
        x, g = names.add("x", torch.zeros(B * T, D)), names.add("g", torch.zeros(B * T, D))
        for step in range(STEPS):
            seed = 1000 + step
            rec.lines.append(f"# step {step}")
            reducer.begin()
            if mode == "forward_only":
                stack.forward(x, B, T, training=bool(step), seed=seed, save=False)
            elif mode == "two_slots":
                for slot in ("a", "b"):
                    stack.forward(x, B, T, training=True, seed=seed, save=True, slot=slot)
                for slot in ("b", "a"):
                    stack.backward(g, slot=slot, reducer=reducer, scale_key="k")
            else:
                stack.forward(x, B, T, training=True, seed=seed, save=True, return_attn=mode == "return_attn")
                stack.backward(g, reducer=reducer, input_grad_only=mode == "input_grad_only")
        return rec.lines


def summary(lines):
    """-> (names of the launches in order, sha256 of the full lines)"""
    calls = [l.split(" ", 1)[0] for l in lines if not l.startswith("#")]
    return calls, hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main(argv):
    out = {}
    for case in CASES:
        lines = trace(case)
        calls, digest = summary(lines)
        out[case] = {"calls": calls, "sha256": digest}
        print(f"{case:30s} {len(calls):4d} launches  {digest}")
        if "--dump" in argv:
            print("\n".join("    " + l for l in lines))
    if "--write" in argv:
        with open(GOLDEN, "w") as f:
            json.dump(out, f, separators=(",", ":"))
            f.write("\n")
        print("wrote", GOLDEN)


if __name__ == "__main__":
    main(sys.argv[1:])
