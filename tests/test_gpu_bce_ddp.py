"""The fused step with loss="bce" under data parallelism, built as tests/test_gpu_classify_ddp.py builds its case (frozen
backbone; 2 ranks, gloo rendezvous, both on cuda:0 -- RCCL refuses two ranks on one device): 2 ranks of batch 4 equal one
process of batch 8 -- every rank normalises by its own n_valid, the reducer averages -- and the reducer was handed the
trainable ranges only."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_classify_ddp import _build
from test_gpu_ddp import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from _util import rel_l2
        from vitssl_hip.engine import GradReducer
        from vitssl_hip.optim import FusedAdamW
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(3)
        x = torch.rand(8, 3, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 10, (8,), generator=g).to(dev)
        per = 8 // world

        model = _build(dev)
        store = model.flat_store()
        if rank == 1:                                   # prove the broadcast matters
            store.flat.add_(1.0)
        dist.broadcast(store.flat, 0)
        store.mark_dirty()
        ranges = model.reduce_ranges()
        assert ranges == [store.span("patch_embedding.cls_token", "patch_embedding.conv.bias"),
                          store.span("classification_head.norm.weight", "classification_head.linear.bias")]
        red = GradReducer(store.gflat, bucket_mb=0.5, expect=ranges)
        opt = FusedAdamW(store, lr=1e-3, weight_decay=1e-3)
        sl = slice(rank * per, (rank + 1) * per)
        loss = model.train_step(x[sl], y[sl], opt, red, label_smoothing=0.1, loss="bce")
        torch.cuda.synchronize()
        buckets, nbytes = red.stats()                   # only the trainable ranges went through the collective
        assert nbytes == 4 * sum(hi - lo for lo, hi in ranges) < 4 * store.gflat.numel() // 4 and 1 <= buckets <= 2
        flats = [torch.empty_like(store.flat) for _ in range(world)]
        dist.all_gather(flats, store.flat)
        assert torch.equal(flats[0], flats[1])          # replicas stay bit-identical
        grads = store.gflat * red.grad_scale
        losses = [torch.zeros(1, device=dev) for _ in range(world)]
        dist.all_gather(losses, loss.reshape(1))

        if rank == 0:                                   # single-process reference on the whole batch
            ref = _build(dev)
            rstore = ref.flat_store()
            ropt = FusedAdamW(rstore, lr=1e-3, weight_decay=1e-3)
            rloss = ref.train_step(x, y, ropt, None, label_smoothing=0.1, loss="bce")
            torch.cuda.synchronize()
            assert abs(float(sum(losses)) / world - float(rloss)) < 1e-4
            for n, p in zip(rstore.names, rstore.params):
                if p.requires_grad:
                    o, cnt = rstore.offsets[n]
                    assert rel_l2(grads[o:o + cnt], rstore.gflat[o:o + cnt]) < 2e-2, n
        open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_bce_equal_single_process(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))
