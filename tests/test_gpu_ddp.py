"""Data-parallel correctness on the GPU: 2 ranks (gloo rendezvous, both on cuda:0 --
RCCL refuses two ranks on one device; the driver's multi-GPU run uses nccl) each take
half of a batch.  After one fused step (a) both ranks hold bit-identical weights,
(b) the all-reduced, 1/world-scaled gradients equal a single-process step on the whole
batch with the same masks, within the bf16 tolerance of test_gpu_models."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(dev):
    from vit_core.ssl.simmim import SimMIMViT
    torch.manual_seed(7)
    return SimMIMViT(num_blocks=2, input_shape=(3, 32, 32), embed_dim=128, patch_size=8, num_heads=2, mlp_dim=192,
                     dropout=0.0, mask_ratio=0.6).to(dev).train()


def _worker(rank, world, port, out_dir):
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from _util import rel_l2
        from vit_core.ssl.simmim.masking import draw_mask
        from vitssl_hip.engine import GradReducer
        from vitssl_hip.optim import FusedAdamW
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(3)
        x = torch.rand(8, 3, 32, 32, generator=g).to(dev)
        torch.manual_seed(11)
        mask = draw_mask(8, 16, 0.6)
        per = 8 // world

        model = _build(dev)
        store = model.flat_store()
        if rank == 1:                                   # prove the broadcast matters
            store.flat.add_(1.0)
        dist.broadcast(store.flat, 0)
        store.mark_dirty()
        red = GradReducer(store.gflat, bucket_mb=0.5)
        opt = FusedAdamW(store, lr=1e-3, weight_decay=1e-3)
        sl = slice(rank * per, (rank + 1) * per)
        loss = model.train_step(x[sl], opt, red, mask_cpu=mask[sl])
        torch.cuda.synchronize()
        assert len(red.launched) >= 2
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
            rloss = ref.train_step(x, ropt, None, mask_cpu=mask)
            torch.cuda.synchronize()
            assert abs(float(sum(losses)) / world - float(rloss)) < 1e-4
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


def _rccl_worker(port, out_dir):
    """world_size 1 over the real `nccl` (= RCCL) backend: the communicator is created with
    device_id, and the reducer's bucketed side-stream all-reduce runs through RCCL kernels.
    A one-rank sum is the identity, so the step must equal a reducer-less step."""
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from vit_core.ssl.simmim.masking import draw_mask
        from vitssl_hip.engine import GradReducer
        from vitssl_hip.optim import FusedAdamW
        g = torch.Generator().manual_seed(3)
        x = torch.rand(8, 3, 32, 32, generator=g).to(dev)
        torch.manual_seed(11)
        mask = draw_mask(8, 16, 0.6)
        outs = []
        for use_reducer in (True, False):
            model = _build(dev)
            store = model.flat_store()
            red = None
            if use_reducer:
                dist.broadcast(store.flat, 0)
                red = GradReducer(store.gflat, bucket_mb=0.5)
                red.world = 2                 # force the collective path; one rank's sum = identity
            opt = FusedAdamW(store, lr=1e-3, weight_decay=1e-3)
            loss = model.train_step(x, opt, red, mask_cpu=mask)
            dist.barrier()
            torch.cuda.synchronize()
            if use_reducer:
                assert len(red.launched) >= 2
            outs.append((float(loss), store.gflat.clone()))
        from _util import rel_l2
        assert abs(outs[0][0] - outs[1][0]) < 1e-6
        # all-reduce over one rank changes nothing (float atomics in the bias / LayerNorm
        # gradient sums make two runs differ in the last bits, hence not torch.equal)
        assert rel_l2(outs[0][1], outs[1][1]) < 1e-5
        open(os.path.join(out_dir, "ok_rccl"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_rccl_single_rank_side_stream_allreduce(tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), str(tmp_path)))
    p.start()
    p.join(300)
    assert p.exitcode == 0 and os.path.exists(tmp_path / "ok_rccl")


def _dino_build(dev):
    from vit_core.ssl.dino import DINOViT
    torch.manual_seed(9)
    return DINOViT(2, (3, 32, 32), 64, 8, 1, 128, 0.0, 256, 0.9).to(dev).train()


def _dino_worker(rank, world, port, out_dir):
    """DINO under data parallelism: the centre update must use the GLOBAL teacher batch mean
    (all-reduced column sums), the student gradient is averaged, teacher EMA stays local."""
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from _util import rel_l2
        from vit_core.ssl.dino.loss import DINOLoss
        from vitssl_hip.engine import GradReducer
        from vitssl_hip.optim import FusedAdamW
        dev = torch.device("cuda:0")
        g = torch.Generator().manual_seed(4)
        B = 4
        views = [torch.rand(B, 3, 32, 32, generator=g).to(dev) for _ in range(2)] + [torch.rand(B, 3, 16, 16, generator=g).to(dev) for _ in range(2)]
        per = B // world
        sl = slice(rank * per, (rank + 1) * per)
        crit = DINOLoss(0.04, 0.1)

        model = _dino_build(dev)
        store = model.trainable_store()
        for s in model.all_stores():
            dist.broadcast(s.flat, 0)
            s.mark_dirty()
        red = GradReducer(store.gflat, bucket_mb=0.25)
        opt = FusedAdamW(store, lr=1e-3, weight_decay=1e-3)
        loss = model.train_step([v[sl] for v in views], 2, crit, opt, red, 0.99)
        torch.cuda.synchronize()
        centers = [torch.empty_like(model.center) for _ in range(world)]
        dist.all_gather(centers, model.center)
        assert torch.equal(centers[0], centers[1])                      # one centre everywhere
        flats = [torch.empty_like(store.flat) for _ in range(world)]
        dist.all_gather(flats, store.flat)
        assert torch.equal(flats[0], flats[1])                          # replicas stay identical
        losses = [torch.zeros(1, device=dev) for _ in range(world)]
        dist.all_gather(losses, loss.reshape(1))
        grads = store.gflat * red.grad_scale
        # reference: the whole batch in one model.  Both ranks run it (the centre update
        # all-reduces whenever a process group exists; two identical contributions over
        # 2 x rows give the same mean), rank 0 compares.
        ref = _dino_build(dev)
        rstore = ref.trainable_store()
        ropt = FusedAdamW(rstore, lr=1e-3, weight_decay=1e-3)
        rloss = ref.train_step(views, 2, crit, ropt, None, 0.99)
        torch.cuda.synchronize()
        if rank == 0:
            assert rel_l2(model.center, ref.center) < 1e-5              # global teacher mean
            assert abs(float(sum(losses)) / world - float(rloss)) < 2e-3 * abs(float(rloss)) + 1e-6
            assert rel_l2(grads, rstore.gflat) < 3e-2
        open(os.path.join(out_dir, f"dino_ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_dino_two_ranks_share_one_centre(tmp_path):
    world = 2
    mp.spawn(_dino_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"dino_ok{r}").exists() for r in range(world))


@pytest.mark.parametrize("model,dtype", [("vit_tiny", "bf16"), ("vit_s", "fp8")])
def test_bench_two_rank_path_reports_its_collectives(tmp_path, model, dtype):
    """bench.py's N > 1 path, rehearsed with two ranks on one GPU (gloo rendezvous, --share-gpu): the
    JSON line carries the self-diagnosis block (world size as the collective sees it, buckets, exposed
    communication) the first real multi-GPU run will be read by."""
    import json
    import subprocess
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--model", model, "--dtype", dtype, "--batch", "8", "--img", "64", "--backend", "gloo", "--share-gpu", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 16 and d["scaling"] == "weak"
    dp = d["data_parallel"]
    assert dp["world_size"] == 2 and dp["allreduce_of_ones"] == 2.0 and dp["backend"] == "gloo"
    assert dp["buckets_per_step"] >= 1 and dp["reduced_bytes_per_step"] >= 0.99 * dp["grad_bytes"] - 64 * 4 * 200
    assert "exposed_comm_ms" in dp and d["roofline"]["hbm"]["ln_fwd"]["launches"] > 0


def _entry_worker(rank, world, port, out_dir):
    """The reference's entry path under torch.distributed.run (train.py:107-128): setup_device() -> build_model ->
    trainer -> fit, with nothing else creating the process group.  Rehearsed on one card: VITSSL_SHARE_GPU binds both
    ranks to cuda:0, VITSSL_DIST_BACKEND=gloo (RCCL refuses two ranks on one device)."""
    for p in (ROOT, os.path.join(ROOT, "vit-ssl_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      VITSSL_DIST_BACKEND="gloo", VITSSL_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    from utils import build_model, setup_device
    from utils.trainers import SimMIMTrainer
    from vitssl_hip.optim import FusedAdamW
    device = setup_device()
    try:
        assert device == torch.device("cuda:0") and dist.is_initialized() and dist.get_world_size() == world
        cfg = {"training": {"type": "simmim", "num_epochs": 1, "warmup_epochs": 1, "warmup_initial_learning_rate": 1e-6,
                            "warmup_final_learning_rate": 1e-3, "criterion": {"name": "L1Loss", "params": {"reduction": "mean"}},
                            "optimizer": {"name": "AdamW", "params": {"lr": 1e-3, "weight_decay": 1e-3}},
                            "lr_scheduler": {"main": {"name": "CosineAnnealingLR", "params": {"eta_min": 1e-6}}, "warmup": {"params": {}}}},
               "eval": {}, "data": {"img_size": 32},
               "model": {"in_channels": 3, "patch_size": 8, "embed_dim": 128, "num_blocks": 2, "num_heads": 2, "mlp_dim": 192,
                         "dropout": 0.1, "mask_ratio": 0.6}}
        torch.manual_seed(50 + rank)                    # per-rank init, per-rank data, per-rank masks / dropout
        model = build_model(cfg).to(device)
        data = [torch.rand(8, 3, 32, 32) for _ in range(3)]
        tr = SimMIMTrainer(model, os.path.join(out_dir, f"r{rank}"), cfg, data, data[:1], device)
        assert tr.world == world and tr.reducer is not None and isinstance(tr.optimizer, FusedAdamW) and tr._fused_ok()
        store = model.flat_store()
        w0 = store.flat.clone()
        tr.fit(1)
        torch.cuda.synchronize()
        flats = [torch.empty_like(store.flat) for _ in range(world)]
        dist.all_gather(flats, store.flat)
        assert torch.equal(flats[0], flats[1]) and not torch.equal(flats[0], w0)
        assert len(tr.reducer.launched) >= 1
        open(os.path.join(out_dir, f"entry_ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


def test_entry_point_path_is_data_parallel(tmp_path):
    world = 2
    mp.spawn(_entry_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all((tmp_path / f"entry_ok{r}").exists() for r in range(world))
