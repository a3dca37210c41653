"""Kernel code that runs only at production size, compared with plain fp64 references on the CPU.

Attention: the persistent forward (129-256 tokens) and backward (129-224 tokens) run min(B*H, CUs) workgroups that sweep the
(batch, head) items blockIdx.x, +grid, ...; the prefetch of the next item, the double-buffer index, the two-row lse buffer and the
counted waits that leave the previous item's stores in flight exist only for the second and later items.  The reserve of
vitssl_set_reserved_cus (library state read at every launch) shrinks the grid to 8 workgroups, so a few dozen items give 3-4
items per workgroup; one launch at the real CU count covers the production schedule.  Every (batch, head) item is checked on its
own, and a launch at the reduced grid must equal one-item-per-workgroup launches bit for bit: no item's arithmetic depends on
where it sits in a sweep.  The start-up stagger of the fused (<= 128 tokens) and pipelined (225-256) kernels engages only above
2 x CUs x workgroups-per-CU items (forward: only with VITSSL_ATTN_STAGGER_FWD set, tests/test_gpu_knobs.py).

DINO: vitssl_dino_loss picks its kernels by K (generic three-pass kernels; register-resident rows for K = 4096, 8192; four row
slices for the teacher at 16384-65536); every branch against the oracle's DINOLoss in fp64 with autograd, per student row.
The loss value is a float atomicAdd over the student rows, so only the gradient is asserted bit-repeatable.  The DINO-head
kernels (row / weight normalisation, centre) at the ViT-B head's size and at a ragged one."""
import ctypes as C
import math

import pytest
import torch

from _util import rel_l2, max_abs
from oracle import vit_oracle as O
from test_gpu_ops import close_bf16

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DH = 64
FP8 = torch.float8_e4m3fn
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def reserve():
    """set(n) -> vitssl_set_reserved_cus(n); the count in force before the test is restored afterwards, also on failure."""
    from vitssl_hip import _lib as L
    lib = L.lib()
    old = lib.vitssl_get_reserved_cus()

    def set_(n):
        L.call("vitssl_set_reserved_cus", C.c_int(n))
        assert lib.vitssl_get_reserved_cus() == n
    yield set_
    torch.cuda.synchronize()
    L.call("vitssl_set_reserved_cus", C.c_int(old))
    assert lib.vitssl_get_reserved_cus() == old


def _last_fwd_grid():
    from vitssl_hip import _lib as L
    return L.lib().vitssl_debug_last_attn_fwd_grid()


# ----------------------------------------------------------------------------- attention helpers
def _qkv(B, N, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * N, 3 * H * DH, generator=g).to(torch.bfloat16)


def _ref_fwd(qkv, B, N, H, images=None):
    """fp64 forward of the images `images` (all by default): out [b, N, H, dh] (P rounded to bf16 before P.V, as the kernel
    does), lse [b, H, N], probs [b, H, N, N]."""
    x = qkv.double().view(B, N, 3, H, DH)
    if images is not None:
        x = x[images]
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-2, -1)) / math.sqrt(DH)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    o = p.to(torch.bfloat16).double() @ v
    return o.transpose(1, 2), lse, p


def _ref_bwd(qkv, dout, B, N, H, images=None):
    """fp64 d(sum(out * dout))/d(qkv) of the images `images`: [b, N, 3, H, dh]"""
    x = qkv.double().view(B, N, 3, H, DH)
    d = dout.double().view(B, N, H, DH)
    if images is not None:
        x, d = x[images], d[images]
    x = x.clone().requires_grad_(True)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    o = torch.softmax((q @ k.transpose(-2, -1)) / math.sqrt(DH), dim=-1) @ v
    (o.transpose(1, 2) * d).sum().backward()
    return x.grad


def _empty(shape, dtype=torch.bfloat16):
    if dtype == FP8:
        t = torch.empty(shape, dtype=torch.uint8, device=DEV).fill_(0x7F)     # e4m3fn NaN
        return t.view(FP8)
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _fwd(ops, qkv_d, B, N, H, probs=False, fp8=False):
    out = _empty((B * N, H * DH))
    lse = _empty((B, H, N), torch.float32)
    pr = _empty((B, H, N, N), torch.float32) if probs else None
    o8 = _empty((B * N, H * DH), FP8) if fp8 else None
    ops.attn_fwd(qkv_d, out, lse, B, N, H, DH, probs=pr, out_fp8=o8)
    return out, lse, pr, o8


def _bwd(ops, qkv_d, out, dout_d, lse, B, N, H, mode="bf16", scale=16.0):
    """mode: "bf16"; "fp8" (bf16 dqkv and its e4m3 image); "fp8_only" (e4m3 image, dqkv = NULL).  -> (dqkv or None, image, amax)"""
    dq = None if mode == "fp8_only" else _empty((B * N, 3 * H * DH))
    if mode == "bf16":
        ops.attn_bwd(qkv_d, out, dout_d, lse, dq, torch.empty(B, H, N, device=DEV), B, N, H, DH)
        return dq, None, None
    d8 = _empty((B * N, 3 * H * DH), FP8)
    sc = torch.tensor([scale], device=DEV)
    amax = torch.zeros(1, device=DEV)
    ops.attn_bwd(qkv_d, out, dout_d, lse, dq, None, B, N, H, DH, dqkv_fp8=d8, scale=sc, amax=amax)
    return dq, d8, amax


def _check_fwd_items(out, lse, probs, ref, B, N, H, images):
    """every (b, h) item of images `images` against the fp64 forward, at the bars of test_gpu_ops.test_attention_fwd_bwd"""
    ro, rl, rp = ref
    got_o = out.float().cpu().view(B, N, H, DH)[images]
    got_l = lse.cpu()[images]
    got_p = probs.cpu()[images] if probs is not None else None
    for i, b in enumerate(images):
        for h in range(H):
            what = f"item (b={b}, h={h}) = {b * H + h}"
            close_bf16(got_o[i, :, h], ro[i, :, h].to(torch.bfloat16), atol=4e-3, what=f"out {what}")
            assert max_abs(got_l[i, h], rl[i, h]) < 1e-4, f"lse {what}"
            if got_p is not None:
                assert rel_l2(got_p[i, h], rp[i, h]) < 1e-3 and max_abs(got_p[i, h], rp[i, h]) < 2e-4, f"probs {what}"


def _check_bwd_items(dqkv, ref, B, N, H, images):
    """each of q / k / v of every (b, h) item on its own (the bar of test_attention_fwd_bwd, per item instead of per tensor)"""
    got = dqkv.float().cpu().view(B, N, 3, H, DH)[images]
    assert not torch.isnan(got).any()
    for i, b in enumerate(images):
        for h in range(H):
            for j, name in enumerate("qkv"):
                err = rel_l2(got[i, :, j, h], ref[i, :, j, h])
                assert err < 2e-2, f"d{name} of item (b={b}, h={h}) = {b * H + h}: rel-L2 {err:.3e}"


def _assert_no_nan8(t8):
    assert not torch.isnan(t8.cpu().float()).any()


def _equal8(a, b):
    return torch.equal(a.cpu().view(torch.uint8), b.cpu().view(torch.uint8))


# ----------------------------------------------------------------------------- A.1 sweeps against fp64, per item
ITEMS = [(3, 3), (4, 6), (9, 3)]          # 9, 24, 27 items on 8 workgroups: 1-2, 3 and 3-4 items per workgroup


@pytest.mark.parametrize("BH", ITEMS, ids=lambda bh: f"B{bh[0]}H{bh[1]}")
@pytest.mark.parametrize("N", [129, 145, 160, 196, 197, 224, 225, 256])
def test_attn_persistent_sweep_parity(ops, cus, reserve, N, BH):
    B, H = BH
    reserve(cus - 8)
    qkv = _qkv(B, N, H, seed=N * 100 + B * H)
    qkv_d = qkv.to(DEV)
    out, lse, probs, _ = _fwd(ops, qkv_d, B, N, H, probs=True)
    assert _last_fwd_grid() == min(B * H, 8)
    images = list(range(B))
    _check_fwd_items(out, lse, probs, _ref_fwd(qkv, B, N, H), B, N, H, images)
    out2, lse2, _, _ = _fwd(ops, qkv_d, B, N, H)                   # the plain wait variant
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    if N > 224:                                                    # 225-256: the backward is the pipelined kernel (one item each)
        return
    dout = _qkv(B, N, H, seed=N * 100 + B * H + 1)[:, : H * DH].contiguous()
    dq, _, _ = _bwd(ops, qkv_d, out, dout.to(DEV), lse, B, N, H)
    _check_bwd_items(dq, _ref_bwd(qkv, dout, B, N, H), B, N, H, images)


# ----------------------------------------------------------------------------- A.2 schedule independence, bit for bit
@pytest.mark.parametrize("N", [129, 197, 224, 256])
def test_attn_fwd_schedule_independent(ops, cus, reserve, N):
    """27 items on 8 workgroups (3-4 each) against 27 workgroups of one item: the three wait variants of the persistent
    forward (probs, plain, e4m3 image) give the same bits."""
    B, H = 9, 3
    assert B * H <= cus
    qkv_d = _qkv(B, N, H, seed=N + 7).to(DEV)
    res = {}
    for rsv in (0, cus - 8):
        reserve(rsv)
        runs = [_fwd(ops, qkv_d, B, N, H, probs=True), _fwd(ops, qkv_d, B, N, H), _fwd(ops, qkv_d, B, N, H, fp8=True)]
        assert _last_fwd_grid() == min(B * H, cus - rsv)
        res[rsv] = runs
    for v, (one, swept) in enumerate(zip(res[0], res[cus - 8])):
        assert not torch.isnan(one[0].float()).any() and not torch.isnan(one[1]).any()
        assert torch.equal(one[0], swept[0]), f"out, variant {v}"
        assert torch.equal(one[1], swept[1]), f"lse, variant {v}"
        if one[2] is not None:
            assert torch.equal(one[2], swept[2]), "probs"
        if one[3] is not None:
            _assert_no_nan8(one[3])
            assert _equal8(one[3], swept[3]), "e4m3 image of out"
        assert torch.equal(one[0], res[0][0][0]), "the wait variants differ in out"


@pytest.mark.parametrize("N", [129, 197, 224])
def test_attn_bwd_schedule_independent(ops, cus, reserve, N):
    """The three store variants of the persistent backward (bf16 dqkv; e4m3 image with dqkv; e4m3 image alone, dqkv = NULL:
    one or two dQ stores behind the counted waits) on 27 items over 8 workgroups against one item per workgroup."""
    B, H = 9, 3
    qkv_d = _qkv(B, N, H, seed=N + 11).to(DEV)
    dout_d = (_qkv(B, N, H, seed=N + 12)[:, : H * DH]).contiguous().to(DEV)
    reserve(0)
    out, lse, _, _ = _fwd(ops, qkv_d, B, N, H)
    res = {}
    for rsv in (0, cus - 8):
        reserve(rsv)
        res[rsv] = [_bwd(ops, qkv_d, out, dout_d, lse, B, N, H, mode) for mode in ("bf16", "fp8", "fp8_only")]
    (a0, _, _), (a1, a8, am), (_, b8, bm) = res[0]
    assert not torch.isnan(a0.float()).any()
    assert torch.equal(a0, a1)                                     # the e4m3 image does not change the bf16 result
    _assert_no_nan8(a8)
    assert _equal8(a8, b8) and torch.equal(am, bm)                 # nor does dropping the bf16 store
    assert float(am) > 0
    for mode, one, swept in zip(("bf16", "fp8", "fp8_only"), res[0], res[cus - 8]):
        if one[0] is not None:
            assert torch.equal(one[0], swept[0]), f"dqkv, {mode}"
        if one[1] is not None:
            assert _equal8(one[1], swept[1]), f"e4m3 dqkv, {mode}"
            assert torch.equal(one[2], swept[2]), f"amax, {mode}"


# ----------------------------------------------------------------------------- A.3 the production schedule
def test_attn_production_launch(ops, cus, reserve):
    """ViT-B's 12 heads at 197 tokens, 67 images: 804 items on every CU (at 256 CUs the first 36 workgroups sweep 4 items, the
    rest 3), bit-identical to per-image launches (12 workgroups of one item) and, per item, against fp64 for every item at
    index >= 2 x grid and a sample of the earlier ones."""
    B, H, N = 67, 12, 197
    reserve(0)
    grid = min(B * H, cus)
    qkv = _qkv(B, N, H, seed=197)
    dout = _qkv(B, N, H, seed=198)[:, : H * DH].contiguous()
    qkv_d, dout_d = qkv.to(DEV), dout.to(DEV)
    out, lse, _, _ = _fwd(ops, qkv_d, B, N, H)
    assert _last_fwd_grid() == grid
    dq, _, _ = _bwd(ops, qkv_d, out, dout_d, lse, B, N, H)
    for b in range(B):
        rows = slice(b * N, (b + 1) * N)
        o1, l1, _, _ = _fwd(ops, qkv_d[rows].contiguous(), 1, N, H)
        assert torch.equal(o1, out[rows]) and torch.equal(l1, lse[b:b + 1]), f"forward of image {b}"
        d1, _, _ = _bwd(ops, qkv_d[rows].contiguous(), out[rows].contiguous(), dout_d[rows].contiguous(), lse[b:b + 1].contiguous(), 1, N, H)
        assert torch.equal(d1, dq[rows]), f"backward of image {b}"
    first = (2 * grid) // H                                        # the first image holding an item >= 2 x grid
    images = sorted(set(range(0, first, 7)) | set(range(first, B)))
    _check_fwd_items(out, lse, None, _ref_fwd(qkv, B, N, H, images), B, N, H, images)
    _check_bwd_items(dq, _ref_bwd(qkv, dout, B, N, H, images), B, N, H, images)


# ----------------------------------------------------------------------------- A.4 start-up stagger
@pytest.mark.parametrize("N", [37, 50, 65, 128, 225, 256])
def test_attn_stagger_paths(ops, cus, reserve, N):
    """60 items: above the stagger threshold of the fused kernels (2 x 8 CUs x 3 or 2 workgroups per CU) and of the pipelined
    backward (2 x 8) under the reserve, below it at the full CU count.  Against fp64 and bit for bit across the two."""
    B, H = 5, 12
    qkv = _qkv(B, N, H, seed=N + 300)
    dout = _qkv(B, N, H, seed=N + 301)[:, : H * DH].contiguous()
    qkv_d, dout_d = qkv.to(DEV), dout.to(DEV)
    res = {}
    for rsv in (cus - 8, 0):
        reserve(rsv)
        out, lse, probs, _ = _fwd(ops, qkv_d, B, N, H, probs=True)
        dq, _, _ = _bwd(ops, qkv_d, out, dout_d, lse, B, N, H)
        res[rsv] = (out, lse, probs, dq)
    images = list(range(B))
    out, lse, probs, dq = res[cus - 8]
    _check_fwd_items(out, lse, probs, _ref_fwd(qkv, B, N, H), B, N, H, images)
    _check_bwd_items(dq, _ref_bwd(qkv, dout, B, N, H), B, N, H, images)
    for name, a, b in zip(("out", "lse", "probs", "dqkv"), res[cus - 8], res[0]):
        assert torch.equal(a, b), name


# ----------------------------------------------------------------------------- B. DINO loss on every dispatch branch
DINO_K = [4100, 12288, 4096, 8192, 16384, 32768, 65536]    # generic (2), register rows (2), four teacher slices (3)
DINO_GVB = [(1, 1, 1), (1, 9, 3), (2, 2, 8), (2, 10, 3)]
T_TEMP, S_TEMP, GSCALE = 0.04, 0.1, 1000.0


def _dino_inputs(G, V, B, K, seed):
    g = torch.Generator().manual_seed(seed)
    teacher = torch.randn(G, B, K, generator=g) * 3
    student = torch.randn(V, B, K, generator=g) * 3
    center = torch.randn(K, generator=g) * 0.5 + torch.linspace(-1.0, 2.0, K)
    teacher[0, 0] = center                                   # (t - c) / tau = 0 exactly: a uniform teacher row
    student[V - 1, 0] = 0.25                                 # a uniform student row (with G = V = B = 1: both uniform, gradient 0)
    if B > 1:
        for x, r in ((teacher, G - 1), (student, V - 1)):
            x[r, B - 1, K - 1] = x[r, B - 1].max() + 1.0      # maximum in the last float4 of the last slice
            x[0, 1, 5] = x[0, 1].max() + 1.0                  # maximum in slice 0 (the first quarter of the row)
    else:
        if G > 1:
            teacher[1, 0, K - 1] = teacher[1, 0].max() + 1.0
        if V > 1:
            student[0, 0, 5] = student[0, 0].max() + 1.0
    return teacher, student, center


def _dino_ref(teacher, student, center):
    """fp64 loss, d(loss)/d(student) by autograd, and the magnitude of the two terms the gradient is the difference of,
    |d/ds| (G p + T) with p the student softmax and T = sum_g teacher softmax (fp32 error of the kernel scales with it)"""
    G, B, K = teacher.shape
    s = student.double().requires_grad_(True)
    loss = O.dino_loss_naive(teacher.double(), s, center.double(), T_TEMP, S_TEMP)
    loss.backward()
    T = torch.softmax((teacher.double() - center.double()) / T_TEMP, dim=-1).sum(0)
    mag = (G * torch.softmax(student.double() / S_TEMP, dim=-1) + T) / (S_TEMP * G * B * K)
    return float(loss.detach()), s.grad, mag


def _close_rows(got, ref, rtol, floor, what, mag=None, mtol=0.0):
    """elementwise |got - ref| <= rtol |ref| + floor x max |ref| of the same row (+ mtol x mag): a wrong column chunk of one
    row cannot hide in an aggregate"""
    got = got.double().cpu().reshape(-1, got.shape[-1])
    ref = ref.double().cpu().reshape(-1, ref.shape[-1])
    lim = rtol * ref.abs() + floor * ref.abs().amax(dim=1, keepdim=True) + 1e-30
    if mag is not None:
        lim = lim + mtol * mag.double().cpu().reshape(ref.shape)
    bad = ((got - ref).abs() > lim) | torch.isnan(got)
    if bad.any():
        r = int(bad.any(dim=1).nonzero()[0])
        c = int(bad[r].nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements in {int(bad.any(dim=1).sum())} rows out of tolerance; "
                             f"first at row {r} col {c}: got {float(got[r, c])}, want {float(ref[r, c])}")


@pytest.mark.parametrize("GVB", DINO_GVB, ids=lambda x: "G%dV%dB%d" % x)
@pytest.mark.parametrize("K", DINO_K)
def test_dino_loss_dispatch_branches(ops, K, GVB):
    G, V, B = GVB
    teacher, student, center = _dino_inputs(G, V, B, K, seed=K + 10 * G + V + B)
    ref_loss, ref_grad, mag = _dino_ref(teacher, student, center)
    td, sd, cd = teacher.view(G * B, K).to(DEV), student.view(V * B, K).to(DEV), center.to(DEV)
    nws = ops.dino_tws_floats(G, B, K)
    assert nws == B * K + 8 * G * B

    def run(with_grad, loss_sum=None):
        t_ws = torch.full((nws,), NAN, device=DEV)
        loss_sum = torch.zeros(1, device=DEV) if loss_sum is None else loss_sum
        ds = torch.full((V * B, K), NAN, dtype=torch.bfloat16, device=DEV) if with_grad else None
        ops.dino_loss(td, sd, cd, t_ws, loss_sum, ds, G, V, B, K, T_TEMP, S_TEMP, GSCALE)
        return loss_sum, ds

    loss, ds = run(True)
    assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
    run(True, loss)                                           # loss_sum accumulates
    assert abs(float(loss) - 2 * ref_loss) <= 1e-5 * abs(2 * ref_loss), (float(loss), 2 * ref_loss)
    loss_ng, _ = run(False)                                   # GRAD = false: its own instantiation, same loss
    assert abs(float(loss_ng) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss_ng), ref_loss)
    # dstudent = gscale * d(loss)/d(student): one bf16 rounding (2^-9 relative) of gs (G p - T), whose fp32 terms carry the
    # error of the fast exponentials at logits / tau of a few hundred (~1e-5 relative) -- it shows where G p and T cancel
    _close_rows(ds.float().view(V, B, K), GSCALE * ref_grad, 2.0 ** -8, 1e-5, f"dstudent K={K} G={G} V={V} B={B}",
                mag=GSCALE * mag, mtol=1e-4)
    _, ds2 = run(True)
    assert torch.equal(ds, ds2)


def test_dino_loss_rejects_bad_scratch_and_k(ops):
    from vitssl_hip import _lib as L
    G, V, B, K = 2, 3, 2, 16384
    td, sd, cd = torch.zeros(G * B, K, device=DEV), torch.zeros(V * B, K, device=DEV), torch.zeros(K, device=DEV)
    loss = torch.zeros(1, device=DEV)
    short = torch.zeros(ops.dino_tws_floats(G, B, K) - 1, device=DEV)
    with pytest.raises(L.VitsslError):
        ops.dino_loss(td, sd, cd, short, loss, None, G, V, B, K, T_TEMP, S_TEMP)
    K2 = 4098
    td2, sd2, cd2 = torch.zeros(G * B, K2, device=DEV), torch.zeros(V * B, K2, device=DEV), torch.zeros(K2, device=DEV)
    ws = torch.zeros(B * K2 + 8 * G * B, device=DEV)
    with pytest.raises(L.VitsslError):
        ops.dino_loss(td2, sd2, cd2, ws, loss, None, G, V, B, K2, T_TEMP, S_TEMP)
    torch.cuda.synchronize()
    assert float(loss) == 0.0


def test_dino_loss_module_fullsize_gradient():
    """the user-facing DINOLoss at K = 65536 (2 global + 8 local views): student.grad against the oracle in fp64"""
    from vit_core.ssl.dino.loss import DINOLoss
    G, V, B, K = 2, 10, 4, 65536
    teacher, student, center = _dino_inputs(G, V, B, K, seed=65)
    ref_loss, ref_grad, mag = _dino_ref(teacher, student, center)
    s = student.to(DEV).requires_grad_(True)
    loss = DINOLoss(T_TEMP, S_TEMP)(teacher.to(DEV), s, center.to(DEV))
    loss.backward()
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * abs(ref_loss)
    assert s.grad.shape == (V, B, K)
    _close_rows(s.grad, ref_grad, 2.0 ** -8, 1e-5, "student.grad", mag=mag, mtol=1e-4)


# ----------------------------------------------------------------------------- C. DINO head kernels
@pytest.mark.parametrize("rows,D", [(160, 768), (83, 300)])
def test_rownorm_fwd_bwd(ops, rows, D):
    g = torch.Generator().manual_seed(rows + D)
    z = torch.randn(rows, D, generator=g) * 2
    z[1] *= 1e-3                                              # a short row
    zn = torch.full((rows, D), NAN, dtype=torch.bfloat16, device=DEV)
    inv = torch.full((rows,), NAN, device=DEV)
    ops.rownorm_fwd(z.to(DEV), zn, inv)
    z64 = z.double()
    nrm = z64.norm(dim=1).clamp_min(1e-12)
    _close_rows(zn.float(), z64 / nrm[:, None], 2.0 ** -8, 0.0, "rownorm zn")
    assert float(((inv.cpu().double() - 1 / nrm).abs() / (1 / nrm)).max()) < 1e-5
    # backward on the stored bf16 image, as the kernel computes it
    dzn = torch.randn(rows, D, generator=g)
    dz = torch.full((rows, D), NAN, dtype=torch.bfloat16, device=DEV)
    ops.rownorm_bwd(dzn.to(DEV), zn, inv, dz)
    n64 = zn.cpu().double()
    d64 = dzn.double()
    ref = inv.cpu().double()[:, None] * (d64 - n64 * (n64 * d64).sum(1, keepdim=True))
    _close_rows(dz.float(), ref, 2.0 ** -8, 1e-4, "rownorm dz")
    # and the autograd of F.normalize itself, at bf16 precision
    zr = z64.clone().requires_grad_(True)
    torch.nn.functional.normalize(zr, dim=1, eps=1e-12).mul(d64).sum().backward()
    assert rel_l2(dz.float(), zr.grad) < 1e-2


@pytest.mark.parametrize("K,D", [(65536, 768), (1031, 300)])
def test_weightnorm_fold_bwd(ops, K, D):
    gen = torch.Generator().manual_seed(K + D)
    v = torch.randn(K, D, generator=gen) * 0.05
    g = torch.rand(K, generator=gen) + 0.5
    w = torch.full((K, D), NAN, device=DEV)
    inv = torch.full((K,), NAN, device=DEV)
    ops.weightnorm_fold(g.to(DEV), v.to(DEV), w, inv)
    v64, g64 = v.double(), g.double()
    vn = v64.norm(dim=1)
    _close_rows(w, g64[:, None] * v64 / vn[:, None], 1e-5, 1e-6, "weightnorm w")
    assert float(((inv.cpu().double() - 1 / vn).abs() * vn).max()) < 1e-5
    # accumulating backward against autograd of torch's weight_norm formula
    dw = torch.randn(K, D, generator=gen)
    dg0 = torch.randn(K, generator=gen)
    dv0 = torch.randn(K, D, generator=gen) * 0.1
    dg, dv = dg0.to(DEV), dv0.to(DEV)
    ops.weightnorm_bwd(dw.to(DEV), g.to(DEV), v.to(DEV), inv, dg, dv)
    vr, gr = v64.clone().requires_grad_(True), g64.clone().requires_grad_(True)
    (gr[:, None] * vr / vr.norm(dim=1, keepdim=True) * dw.double()).sum().backward()
    # dg: a length-D fp32 dot product, error relative to sum |dW vhat|
    dg_err = (dg.cpu().double() - (dg0.double() + gr.grad)).abs()
    assert bool((dg_err <= 1e-5 * (dw.double() * v64 / vn[:, None]).abs().sum(1)).all()), float(dg_err.max())
    _close_rows(dv - dv0.to(DEV), vr.grad, 1e-4, 1e-5, "weightnorm dv increment")
    _close_rows(dv, dv0.double() + vr.grad, 1e-5, 1e-6, "weightnorm dv")


@pytest.mark.parametrize("rows,K", [(160, 65536), (83, 1032)])
def test_colsum_and_center_ema(ops, rows, K):
    gen = torch.Generator().manual_seed(rows + K)
    x = torch.randn(rows, K, generator=gen) * 3 + 1
    out = torch.full((K,), NAN, device=DEV)
    ops.colsum_f32(x.to(DEV), out)
    ref = x.double().sum(0)
    err = (out.cpu().double() - ref).abs()
    assert not torch.isnan(out).any()
    assert bool((err <= 1e-6 * x.double().abs().sum(0) + 1e-30).all()), float(err.max())
    center0 = torch.randn(K, generator=gen)
    center = center0.to(DEV)
    mom, inv_rows = 0.9, 1.0 / rows
    ops.center_ema(center, out, mom, inv_rows)
    mom32, inv32 = (float(torch.tensor(x, dtype=torch.float32)) for x in (mom, inv_rows))    # the values the kernel receives
    a, b = mom32 * center0.double(), (1 - mom32) * out.cpu().double() * inv32
    err = (center.cpu().double() - (a + b)).abs()
    assert bool((err <= 1e-6 * (a.abs() + b.abs()) + 1e-30).all()), float(err.max())
