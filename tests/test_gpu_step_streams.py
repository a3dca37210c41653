"""Fused train steps of tiny models: the same bits run to run, the same bits on a side stream, and no host wait inside a step.

Every configuration is built from one saved state_dict, one fixed batch, one fixed mask / keep table and one seed of torch's CPU
generator (the source of vit_core._runtime.next_seed, so the dropout keys repeat).  Compared with torch.equal: the flat
parameters, exp_avg, exp_avg_sq and the last gflat after 3 steps of FusedAdamW.  The loss scalars are sums of per-row float
atomics and are compared at 1e-6 relative.

  reproducible        two fresh models, 3 steps each on the default stream
  stream-independent  a third model, the same 3 steps under torch.cuda.stream(side); its batch is written on the side stream behind
                      a gate (tests/_offstream.hold) over NaN, so a launch that strays to another stream reads NaN or stale data
  never blocking      a fourth model: 2 warm steps, then a gate on the side stream of >= 10 x the host time of a warm step and
                      >= 100 ms, event `pre`, one train_step with a prepared mask and device-resident inputs; `pre` must still be
                      pending when train_step returns.  Steps that cannot pass would be listed in BLOCKS with the line that waits;
                      none is.

The shapes keep the steps off the launches that are order-dependent by design: the DINO head has K = 1024 (split-K of the NT
GEMM needs K >= 4096 and fewer than 64 tiles) and every weight gradient runs with a workspace (the TN GEMM's atomic form is the
workspace = NULL one).  The DINO local crops have another grid than the global ones, so the bicubic resize of the positional
embedding and its backward are in the step."""
import contextlib
import functools
import time

import pytest
import torch

from _offstream import hold

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPS, SEED = 3, 1234
CONFIGS = ["simmim-bf16", "simmim-fp8", "vit", "mae", "dino"]
BLOCKS = {}             # configuration -> "file:line that waits for the device", for a step that cannot pass never-blocking


@contextlib.contextmanager
def operands(name):
    from vitssl_hip import engine
    engine.set_linear_operands("fp8" if name.endswith("fp8") else "bf16")
    try:
        yield
    finally:
        engine.set_linear_operands("bf16")


def construct(name):
    torch.manual_seed(11)
    if name.startswith("simmim"):
        from vit_core.ssl.simmim.model import SimMIMViT
        return SimMIMViT(num_blocks=2, input_shape=(3, 64, 64), embed_dim=128, patch_size=16, num_heads=2, mlp_dim=256, dropout=0.1)
    if name == "vit":
        from vit_core.vit import ViT
        return ViT(num_classes=10, num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=256, dropout=0.0)
    if name == "mae":
        from vit_core.ssl.mae import MAEViT
        return MAEViT(num_blocks=2, input_shape=(3, 32, 32), patch_size=8, embed_dim=64, num_heads=1, mlp_dim=128, decoder_embed_dim=64,
                      decoder_blocks=1, decoder_heads=2, mask_ratio=0.75, norm_pix_loss=True)
    from vit_core.ssl.dino import DINOViT
    return DINOViT(num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=256, dropout=0.0, output_dim=1024,
                   center_momentum=0.9)


@functools.lru_cache(maxsize=None)
def fixed(name):
    """-> (state_dict, host inputs): computed once per configuration, never changed"""
    sd = {k: v.detach().clone() for k, v in construct(name).state_dict().items()}
    g = torch.Generator().manual_seed(7)
    if name.startswith("simmim"):
        mask = torch.zeros(4, 16, dtype=torch.bool)
        mask[:, 1::2] = True
        mask[0, :3] = True
        return sd, dict(x=torch.rand(4, 3, 64, 64, generator=g), mask=mask)
    if name == "vit":
        return sd, dict(x=torch.rand(5, 3, 32, 32, generator=g), y=torch.randint(0, 10, (5,), generator=g))
    if name == "mae":
        from vit_core.ssl.mae import masking as Mk
        keep, restore = Mk.draw_keep(5, 16, 4, generator=torch.Generator().manual_seed(5))
        return sd, dict(x=torch.rand(5, 3, 32, 32, generator=g), keep=keep, restore=restore)
    return sd, dict(views=[torch.rand(4, 3, 32, 32, generator=g) for _ in range(2)] + [torch.rand(4, 3, 16, 16, generator=g) for _ in range(2)])


def fresh(name):
    from vitssl_hip.optim import FusedAdamW
    model = construct(name)
    model.load_state_dict(fixed(name)[0])
    model = model.to(DEV).train()
    store = model.trainable_store() if name == "dino" else model.flat_store()
    return model, store, FusedAdamW(store, lr=1e-3, weight_decay=0.05)


def upload(name, gated):
    """the device copies of the float inputs (and labels); `gated`: written behind a gate on the current stream, over NaN"""
    host = fixed(name)[1]
    src = host["views"] if name == "dino" else [host["x"]]
    dst = [torch.full(t.shape, float("nan"), device=DEV) for t in src]
    pinned = [t.pin_memory() for t in src]
    torch.cuda.synchronize()
    if gated:
        hold()
    for d, p in zip(dst, pinned):
        d.copy_(p, non_blocking=True)
    dev = dict(views=dst) if name == "dino" else dict(x=dst[0])
    if name == "vit":
        dev["y"] = host["y"].to(DEV)
    dev["_pinned"] = pinned                                 # alive until the copies have run
    return dev


def step(name, model, opt, dev, prepared=None):
    host = fixed(name)[1]
    if name.startswith("simmim"):
        return model.train_step(dev["x"], opt, mask_cpu=None if prepared is not None else host["mask"], prepared=prepared)
    if name == "vit":
        return model.train_step(dev["x"], dev["y"], opt, label_smoothing=0.1)
    if name == "mae":
        return model.train_step(dev["x"], opt, keep_cpu=None if prepared is not None else host["keep"], prepared=prepared)
    from vit_core.ssl.dino.loss import DINOLoss
    return model.train_step(dev["views"], 2, DINOLoss(0.04, 0.1), opt, None, teacher_momentum=0.99)


def prepare(name, model):
    host = fixed(name)[1]
    if name.startswith("simmim"):
        return model.runtime(DEV).prepare_mask(host["mask"], DEV)
    if name == "mae":
        return model.runtime(DEV).prepare(host["keep"], host["restore"], DEV)
    return None


def run(name, side=None):
    """3 steps of a fresh model on the default stream or under torch.cuda.stream(side) -> the bits the runs are compared by"""
    with operands(name), (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
        model, store, opt = fresh(name)
        dev = upload(name, gated=side is not None)
        torch.manual_seed(SEED)
        losses = torch.stack([step(name, model, opt, dev).detach().reshape(()) for _ in range(STEPS)])
        torch.cuda.synchronize()
        bits = {k: t.detach().cpu().view(torch.int32).clone() for k, t in (("flat", store.flat), ("exp_avg", opt.exp_avg),
                                                                            ("exp_avg_sq", opt.exp_avg_sq), ("gflat", store.gflat))}
        return bits, losses.cpu().double(), store.offsets


@functools.lru_cache(maxsize=None)
def baseline(name):
    return run(name)


def same(name, what, got, ref):
    (bits, losses, offsets), (rbits, rlosses, _) = got, ref
    assert bool(torch.isfinite(losses).all()) and bool((rbits["gflat"] != 0).any()), f"{name}: the steps did not train"
    for k in ("gflat", "exp_avg", "exp_avg_sq", "flat"):
        if torch.equal(bits[k], rbits[k]):
            continue
        diff = (bits[k] != rbits[k]).nonzero().flatten()
        first = int(diff[0])
        owner = next((n for n, (o, cnt) in offsets.items() if o <= first < o + cnt), "padding")
        raise AssertionError(f"{name}, {what}: {k} differs in {diff.numel()} of {bits[k].numel()} floats, first at {first} ({owner})")
    rel = float(((losses - rlosses).abs() / rlosses.abs()).max())
    assert rel <= 1e-6, f"{name}, {what}: losses {losses.tolist()} against {rlosses.tolist()}"


@pytest.mark.parametrize("name", CONFIGS)
def test_steps_are_reproducible(name):
    same(name, "second run on the default stream", run(name), baseline(name))


@pytest.mark.parametrize("name", CONFIGS)
def test_steps_do_not_depend_on_the_stream(name):
    same(name, "side stream", run(name, torch.cuda.Stream()), baseline(name))


@pytest.mark.parametrize("name", CONFIGS)
def test_step_never_blocks_the_host(name):
    assert name not in BLOCKS, BLOCKS.get(name)
    side = torch.cuda.Stream()
    with operands(name), torch.cuda.stream(side):
        model, store, opt = fresh(name)
        dev = upload(name, gated=False)
        torch.manual_seed(SEED)
        step(name, model, opt, dev)
        torch.cuda.synchronize()
        w = time.perf_counter()
        step(name, model, opt, dev, prepare(name, model))
        host_ms = (time.perf_counter() - w) * 1e3
        torch.cuda.synchronize()
        gate_ms = max(100.0, 10.0 * host_ms)
        prepared = prepare(name, model)
        torch.cuda.synchronize()
        hold(gate_ms)
        pre = torch.cuda.Event()
        pre.record()
        loss = step(name, model, opt, dev, prepared)
        pending = not pre.query()
        torch.cuda.synchronize()
        print(f"{name}: warm step {host_ms:.2f} ms on the host, gate {gate_ms:.0f} ms")
        assert pending, f"{name}: train_step returned only after a gate of {gate_ms:.0f} ms in front of it had run out: something in it waits"
        assert bool(torch.isfinite(loss))
