"""The fused MAE step under data parallelism, in the manner of tests/test_gpu_classify_ddp.py: 2 ranks (gloo rendezvous, both on
cuda:0 -- RCCL refuses two ranks on one device) of batch 4 equal one process of batch 8 on the same keep table, the reducer was
handed the whole gradient buffer, and the replicas stay bit-identical."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_ddp import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(dev):
    from vit_core.ssl.mae import MAEViT
    torch.manual_seed(7)
    return MAEViT(2, (3, 24, 24), 64, 8, num_heads=1, mlp_dim=128, decoder_embed_dim=64, decoder_blocks=1, decoder_heads=2).to(dev).train()


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from _util import rel_l2
        from vit_core.ssl.mae.masking import draw_keep
        from vitssl_hip.engine import GradReducer
        from vitssl_hip.optim import FusedAdamW
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(3)
        x = torch.rand(8, 3, 24, 24, generator=g).to(dev)
        keep, _ = draw_keep(8, 9, 2, generator=g)
        per = 8 // world

        model = _build(dev)
        store = model.flat_store()
        if rank == 1:                                   # prove the broadcast matters
            store.flat.add_(1.0)
        dist.broadcast(store.flat, 0)
        store.mark_dirty()
        red = GradReducer(store.gflat, bucket_mb=0.05)  # expect: the whole buffer; finish() checks that every range came once
        opt = FusedAdamW(store, lr=1e-3, weight_decay=1e-3)
        sl = slice(rank * per, (rank + 1) * per)
        loss = model.train_step(x[sl], opt, red, keep_cpu=keep[sl])
        torch.cuda.synchronize()
        buckets, nbytes = red.stats()
        assert buckets >= 2 and 4 * (store.gflat.numel() - 64 * len(store.names)) <= nbytes <= 4 * store.gflat.numel()
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
            rloss = ref.train_step(x, ropt, None, keep_cpu=keep)
            torch.cuda.synchronize()
            assert abs(float(sum(losses)) / world - float(rloss)) < 1e-4 * float(rloss)      # equal rows per rank: the mean of the means
            for n in rstore.names:
                o, cnt = rstore.offsets[n]
                assert rel_l2(grads[o:o + cnt], rstore.gflat[o:o + cnt]) < 2e-2, n
        open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_single_process(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"ok{r}").exists() for r in range(world))
