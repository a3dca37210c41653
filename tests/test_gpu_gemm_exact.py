"""Every NT / TN GEMM variant and the deterministic sums beside them, bit for bit on small-integer operands (tests/_gemm_exact.py).

The tolerance tests judge these kernels over whole matrices (rel-L2 1e-5, 2^-7 |ref| + 5e-3 per bf16 element, rel-L2 1e-3 for column
sums) because random floats make the summation order visible.  Here the arithmetic is exact in any order, so every element of every
output must equal an integer reference as bits, outputs are filled with a sentinel first, and a mismatch names its (row, col), 16 x 16
blocks and 256 x 256 tiles.  Paths (csrc/gemm_nt.hip launch_nt / launch_cfg_parts / launch_splitk_f32, csrc/gemm_tn.hip tn_plan /
tn_batch_plan; 256 CUs unless a case reserves some), per case id:

  NT, fewer than 64 tiles of 256 x 256 -> 256 x 128 tiles, two-phase kernel (gemm_nt_kernel), persistent for K <= 512
    small-37x12x64        one ragged tile, N % 8 == 4, a single K-step
    small-300x260x128     2 x 3 tiles, ragged M and N, N % 8 == 4
    round-257x264x192     one row into the second tile row; an odd count of K-steps for the two buffers
    round-300x520x512     N % 8 == 0 changes nothing here (four waves: no ping-pong form)
    small-1100x772x64-G8  8 CUs: 35 tiles on 16 workgroup slots, every workgroup walks 2-3 tiles
  NT, 64 tiles or more -> 8-wave tiles; 192 rows by the cost model at 256 CUs (one round either way, 0.78 of the loop time)
    small-3900x1028x64    N % 8 == 4: gemm_nt_kernel with 192 x 256 tiles, ragged last tile row and column
    small-3330x1160x128   N % 8 == 0: ping-pong kernel, line-shaped stores, 192-row tiles (3330 % 192 = 66), last column 136 wide
    round-3330x1160x192   the same, three K-steps, outputs that round
    small-3330x1160x64-G8 8 CUs: 256-row tiles (9 rounds each way), 70 tiles on 8 workgroups = 8-9 tiles each, raster groups of
                          4 + 1 tile columns, so every workgroup crosses group boundaries
    round-3330x1160x512-G75  75 CUs: 224-row tiles (75 tiles = one round; 3330 % 224 = 194: the last tile is ragged inside its
                          last 32 rows)
    (192- and 224-row tiles for EVERY shape: tests/test_gpu_knobs.py runs this file under VITSSL_NT_TILE=3 and =4)
  NT split-K (fewer than 64 tiles, K >= 4096, EPI_F32 without column sums): atomics into a zeroed output, bias by slice 0
  TN: slab (splits > 1), direct (one split: M <= 64, or more tiles than CUs under a reserve), atomic; the batch with splits > 1,
      with single owners (no workspace) and with helper workgroups after one and after two splits; e4m3 twins of all of them."""
import ctypes as C
import functools
import math
import os

import pytest
import torch

import _gemm_exact as X

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF16, F32, FP8 = X.BF16, X.F32, X.FP8
SENT = 7.0                        # every output starts as this: an element the kernel does not write is a mismatch
DROPS = [0.0, 0.5]                # at p = 0.5 the survivor scale 65536 / 32768 is exactly 2

NT_CASES = [                      # regime, M, N, K, usable CUs (None = all), the tile launch_nt picks without knobs
    ("small", 37, 12, 64, None, ("small", 256)),
    ("small", 300, 260, 128, None, ("small", 256)),
    ("round", 257, 264, 192, None, ("small", 256)),
    ("round", 300, 520, 512, None, ("small", 256)),
    ("small", 1100, 772, 64, 8, ("small", 256)),
    ("small", 3900, 1028, 64, None, ("big", 192)),
    ("small", 3330, 1160, 128, None, ("big", 192)),
    ("round", 3330, 1160, 192, None, ("big", 192)),
    ("small", 3330, 1160, 64, 8, ("big", 256)),
    ("round", 3330, 1160, 512, 75, ("big", 224)),
]


def _id(c):
    return f"{c[0]}-{c[1]}x{c[2]}x{c[3]}" + (f"-G{c[4]}" if c[4] else "")


nt_cases = pytest.mark.parametrize("case", NT_CASES, ids=_id)
drops = pytest.mark.parametrize("p", DROPS, ids=lambda p: f"p{p}")


@pytest.fixture(scope="module")
def ops():
    from vitssl_hip import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from vitssl_hip import _lib
    return _lib


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture
def usable(L, cus):
    """set(G) -> the persistent grids of the library may occupy G CUs (vitssl_set_reserved_cus(CUs - G)); the reserve in force
    before the test is restored afterwards, also on failure."""
    lib = L.lib()
    old = lib.vitssl_get_reserved_cus()

    def set_(G):
        if G is None:
            return cus - lib.vitssl_get_reserved_cus()
        L.call("vitssl_set_reserved_cus", C.c_int(cus - G))
        assert lib.vitssl_get_reserved_cus() == cus - G
        return G
    yield set_
    torch.cuda.synchronize()
    L.call("vitssl_set_reserved_cus", C.c_int(old))
    assert lib.vitssl_get_reserved_cus() == old


def _knob(name):
    return int(os.environ.get(name, "0") or 0)


@functools.lru_cache(maxsize=None)
def _nt_ref(case):
    """operands and the exact accumulator of a case, computed once and shared by the tests of all epilogues (left unchanged)"""
    regime, M, N, K = case[:4]
    hi = X.regime_hi(regime, K)
    A, B, bias = X.operands(M, N, K, seed=M + N + K, hi=hi, colsum=regime == "small")
    acc = X.ref_nt(A, B, fp32=M * N * K > 1 << 30)
    return {"A": A.to(DEV), "B": B.to(DEV), "bias": bias.to(DEV), "bias64": bias.double(), "acc": acc, "small": regime == "small"}


def _filled(shape, dtype, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _check_grid(L, cus, case, G):
    """what the case id promises about the launch: the tile the cost model picks; under a reserve of all but 8 CUs a grid smaller
    than the tile count; for the ping-pong kernel the grid names the tile height that ran"""
    _, M, N, K, want_G, want_tile = case
    kind, rows = X.nt_tile_rows(M, N, G)
    if want_G is not None or cus == 256:
        assert (kind, rows) == want_tile, (kind, rows, want_tile)
    tiles256 = math.ceil(M / 256) * math.ceil(N / 256)
    if want_G == 8:
        slots = G * (2 if kind == "small" and not _knob("VITSSL_NT_TILE") else 1)
        assert slots < tiles256, (slots, tiles256)              # fewer slots than tiles of any height: workgroups walk several tiles
    if N % 8 == 0 and (kind == "big" or _knob("VITSSL_NT_TILE") in (1, 3, 4)):
        rows = {0: rows, 1: 256, 3: 192, 4: 224}[_knob("VITSSL_NT_TILE")]
        tiles = math.ceil(M / rows) * math.ceil(N / 256)
        assert L.lib().vitssl_debug_last_nt_grid() == min(tiles, G), (rows, tiles, G)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32), b.view(torch.int16 if b.dtype == BF16 else torch.int32))


# ----------------------------------------------------------------------------- NT, bf16 operands
@nt_cases
def test_nt_exact_bf16_and_f32(ops, L, cus, usable, case):
    r = _nt_ref(case)
    M, N = case[1], case[2]
    G = usable(case[4])
    full = r["acc"] + r["bias64"]
    outs = []
    for _ in range(2):                                           # the default path twice: identical bits
        out = _filled((M, N), BF16)
        ops.gemm_nt(r["A"], r["B"], out, L.EPI_BF16, bias=r["bias"])
        outs.append(out)
    _check_grid(L, cus, case, G)
    X.check_exact(outs[0], X.bf16_rne(full), "EPI_BF16 + bias")
    assert _same_bits(outs[0], outs[1]), "EPI_BF16: two runs differ"
    out = _filled((M, N), BF16)
    ops.gemm_nt(r["A"], r["B"], out, L.EPI_BF16)
    X.check_exact(out, X.bf16_rne(r["acc"]), "EPI_BF16, no bias")

    out32 = _filled((M, N), F32)
    ops.gemm_nt(r["A"], r["B"], out32, L.EPI_F32, bias=r["bias"])
    X.check_exact(out32, X.to_f32_exact(full), "EPI_F32 + bias")
    if r["small"]:                                               # column sums, accumulated into a non-zero vector by two calls
        cs0 = X.int_values((N,), -5, 5, seed=N)
        for epi, dtype in ((L.EPI_BF16, BF16), (L.EPI_F32, F32)):
            cs, out = cs0.to(DEV), _filled((M, N), dtype)
            ops.gemm_nt(r["A"], r["B"], out, epi, bias=r["bias"], colsum=cs)
            X.check_exact(cs, X.to_f32_exact(cs0.double() + full.sum(0)), f"epilogue {epi}: column sums")
            ops.gemm_nt(r["A"], r["B"], out, epi, bias=r["bias"], colsum=cs)
            X.check_exact(cs, X.to_f32_exact(cs0.double() + 2 * full.sum(0)), f"epilogue {epi}: column sums accumulated by a second call")
            X.check_exact(out, X.to_f32_exact(full).to(dtype), f"epilogue {epi} with column sums")


@drops
@nt_cases
def test_nt_exact_resid(ops, L, usable, case, p):
    r = _nt_ref(case)
    M, N = case[1], case[2]
    usable(case[4])
    drop = ops.make_dropout(p, seed=5, site=11)
    keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
    assert p == 0 or 0.4 < float(keep.mean()) < 0.6 or M * N < 1000
    res = X.int_values((M, N), -100, 100, seed=M)
    out = _filled((M, N), F32)
    ops.gemm_nt(r["A"], r["B"], out, L.EPI_RESID, bias=r["bias"], aux=res.to(DEV), drop=drop)
    want = res.double() + (r["acc"] + r["bias64"]) * keep * (2.0 if p else 1.0)
    X.check_exact(out, X.to_f32_exact(want), f"EPI_RESID p={p}")


@nt_cases
def test_nt_exact_dgelu(ops, L, usable, case):
    r = _nt_ref(case)
    M, N = case[1], case[2]
    usable(case[4])
    aux = X.dgelu_aux(M, N, seed=N)
    want = r["acc"] * aux.double()
    out = _filled((M, N), BF16)
    ops.gemm_nt(r["A"], r["B"], out, L.EPI_DGELU, aux=aux.to(DEV))
    X.check_exact(out, X.bf16_rne(want), "EPI_DGELU")
    if r["small"]:
        cs0 = X.int_values((N,), -5, 5, seed=N + 1)
        cs, out = cs0.to(DEV), _filled((M, N), BF16)
        ops.gemm_nt(r["A"], r["B"], out, L.EPI_DGELU, aux=aux.to(DEV), colsum=cs)
        X.check_exact(cs, X.to_f32_exact(cs0.double() + want.sum(0)), "EPI_DGELU column sums")
        X.check_exact(out, X.bf16_rne(want), "EPI_DGELU with column sums")


@drops
@nt_cases
def test_nt_exact_gelu(ops, L, usable, case, p):
    """u = bf16(acc + bias) is known exactly, so the bar of test_gemm_nt_epilogues holds WITHOUT its 1.13 scale |u| 2^-7 term (which
    only covers a u one ulp off); the cases hold u = 0, |u| >= 16 (the end of the ping-pong kernel's table) and negative u."""
    r = _nt_ref(case)
    M, N = case[1], case[2]
    usable(case[4])
    u = X.bf16_rne(r["acc"] + r["bias64"]).double()
    assert bool((u == 0).any()) and bool((u.abs() >= 16).any()) and bool((u < 0).any())
    drop = ops.make_dropout(p, seed=5, site=11)
    ks = ops.dropout_mask(M, N, drop, DEV).cpu().double() * (2.0 if p else 1.0)
    gp, a = _filled((M, N), BF16), _filled((M, N), BF16)
    ops.gemm_nt(r["A"], r["B"], gp, L.EPI_GELU, bias=r["bias"], out1=a, drop=drop)
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    ref_a = ks * u * cdf
    ref_gp = ks * (cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi))
    for name, got, ref in (("out1 = gelu(u)", a, ref_a), ("out0 = gelu'(u)", gp, ref_gp)):
        err = (got.cpu().double() - ref).abs()
        lim = ref.abs() * 2.0 ** -7 + 2e-3
        worst = int((err - lim).argmax())
        print(f"EPI_GELU p={p} {name}: max error {float(err.max()):.3e}, max excess over the bar {float((err - lim).max()):.3e}")
        assert bool((err <= lim).all()), (f"EPI_GELU p={p} {name}: {int((err > lim).sum())} elements over the bar, worst at (row {worst // N}, "
                                          f"col {worst % N}): u = {float(u.view(-1)[worst])}, got {float(got.view(-1)[worst])}, want {float(ref.view(-1)[worst])}")


@pytest.mark.parametrize("tok_offset,use_mask", [(0, True), (1, False), (0, False), (1, True)])
@pytest.mark.parametrize("Bimg,tokens,N,K", [(3, 16, 132, 64), (3, 100, 264, 128), (5, 197, 388, 128)],
                         ids=["48x132x64", "300x264x128", "985x388x128"])
def test_nt_exact_embed(ops, L, Bimg, tokens, N, K, tok_offset, use_mask):
    M = Bimg * tokens
    A, B, bias = X.operands(M, N, K, seed=M + N, hi=1)
    full = X.ref_nt(A, B) + bias.double()
    out_tokens = tokens + tok_offset
    pos, mtok = X.int_values((out_tokens, N), -8, 8, seed=1).double(), X.int_values((N,), -8, 8, seed=2).double()
    mask = (X.int_values((M,), 0, 1, seed=3) > 0) if use_mask else None
    out = _filled((Bimg * out_tokens, N), F32, -SENT)
    ops.gemm_nt(A.to(DEV), B.to(DEV), out, L.EPI_EMBED, bias=bias.to(DEV),
                embed=(None if mask is None else mask.to(torch.uint8).to(DEV), mtok.float().to(DEV), pos.float().to(DEV), tokens, out_tokens, tok_offset))
    tok = full.view(Bimg, tokens, N)
    if mask is not None:
        tok = torch.where(mask.view(Bimg, tokens, 1), mtok, tok)
    want = torch.full((Bimg, out_tokens, N), -SENT, dtype=torch.float64)            # the CLS slot stays untouched
    want[:, tok_offset:] = tok + pos[tok_offset:]
    X.check_exact(out, X.to_f32_exact(want.view(-1, N)), f"EPI_EMBED tok_offset={tok_offset} mask={use_mask}")


@pytest.mark.parametrize("M,N,K", [(130, 68, 4160), (300, 264, 4096)], ids=["130x68x4160", "300x264x4096"])
def test_nt_exact_splitk(ops, L, M, N, K):
    """1 and 6 tiles, K >= 4096: split-K slices (the last one shorter at K = 4160) add into the output the launcher zeroes; the atomics
    are exact here, and the bias is added exactly once"""
    A, B, bias = X.operands(M, N, K, seed=K)
    acc = X.ref_nt(A, B)
    for b in (bias, None):
        outs = []
        for _ in range(2):
            out = _filled((M, N), F32)
            ops.gemm_nt(A.to(DEV), B.to(DEV), out, L.EPI_F32, bias=None if b is None else b.to(DEV))
            outs.append(out)
        X.check_exact(outs[0], X.to_f32_exact(acc + (0 if b is None else b.double())), f"split-K EPI_F32, bias {b is not None}")
        assert _same_bits(outs[0], outs[1])


# ----------------------------------------------------------------------------- TN, bf16 and e4m3 operands
def _scalar(v):
    return None if v is None else torch.tensor([v], device=DEV)


def _tn_twice(run, C0, prod, what):
    Cd = C0.to(DEV)
    run(Cd)
    X.check_exact(Cd, X.to_f32_exact(C0.double() + prod), what)
    run(Cd)
    X.check_exact(Cd, X.to_f32_exact(C0.double() + 2 * prod), what + ", second call")
    return Cd


def _tn_id(kind, rest):
    """the bf16 cases keep the ids they had before the e4m3 cases joined them"""
    return ("" if kind == "bf16" else kind + "-") + rest


TN_CASES = [                                                     # kind, M, N1, N2, usable CUs, mode
    ("bf16", 1, 264, 8, None, "direct"), ("bf16", 63, 264, 8, None, "direct"), ("bf16", 64, 8, 264, None, "direct"),      # one chunk of 64 rows: one split
    ("bf16", 65, 264, 8, None, "slab"),                          # two chunks, the second of one row
    ("bf16", 3000, 264, 520, None, "slab"),                      # 6 tiles, 47 chunks in 24 splits of 2: the last split and the last chunk ragged
    ("bf16", 300, 520, 776, 8, "direct"),                        # 12 tiles on 8 CUs: one owner per tile walks all 5 chunks
    ("bf16", 1000, 264, 8, 8, "slab"),                           # 2 tiles on 8 CUs: 4 splits of 4 chunks
    # e4m3: chunks of 128 rows, widths multiples of 16
    ("e4m3", 100, 272, 16, None, "direct"), ("e4m3", 127, 272, 16, None, "direct"), ("e4m3", 128, 16, 272, None, "direct"),    # one chunk
    ("e4m3", 129, 272, 16, None, "slab"),                        # two splits, the second of one row
    ("e4m3", 1000, 272, 16, None, "slab"),                       # 2 tiles, 8 splits of one chunk, the last ragged
    ("e4m3", 3000, 272, 528, None, "slab"),                      # 6 tiles, 24 splits of one chunk
    ("e4m3", 600, 528, 784, 8, "direct"),                        # 12 tiles on 8 CUs: one owner per tile walks all 5 chunks
    ("e4m3", 2000, 272, 16, 8, "slab"),                          # 2 tiles on 8 CUs: 4 splits of 4 chunks
]


@pytest.mark.parametrize("kind,M,N1,N2,G,mode", TN_CASES, ids=[_tn_id(c[0], "-".join(str(v) for v in c[1:])) for c in TN_CASES])
def test_tn_exact(ops, L, usable, kind, M, N1, N2, G, mode):
    """first and second (accumulating) call, two independent runs with the same bits, and the atomic mode; e4m3 operands once with
    alpha x alpha2 = 0.25 x 8 (the factor 2 is part of the exactness bound of operands_tn) and once without scalars"""
    fp8 = kind == "e4m3"
    A, B, C0 = X.operands_tn(M, N1, N2, seed=M + (N2 if fp8 else N1), scale=2.0 if fp8 else 1.0)
    prod = X.ref_tn(A, B)
    Ad, Bd = (X.to_fp8(A).to(DEV), X.to_fp8(B).to(DEV)) if fp8 else (A.to(DEV), B.to(DEV))
    G = usable(G)
    _, splits, _ = X.tn_plan(M, N1, N2, G, km=128 if fp8 else 64)
    assert (splits == 1) == (mode == "direct"), (splits, mode)
    query = L.lib().vitssl_gemm_fp8_tn_workspace_floats if fp8 else L.lib().vitssl_gemm_tn_workspace_floats
    assert query(M, N1, N2) == splits * N1 * N2
    gemm, name = (ops.gemm_fp8_tn, "gemm_fp8_tn") if fp8 else (ops.gemm_tn, "gemm_tn")
    variants = [(", alpha 0.25 x 8", 2.0, dict(alpha=_scalar(0.25), alpha2=_scalar(8.0))), (", no scalars", 1.0, {})] if fp8 else [("", 1.0, {})]
    for tag, s, kw in variants:
        c_a = _tn_twice(lambda Cd: gemm(Ad, Bd, Cd, **kw), C0, s * prod, f"{name} {mode}{tag}")
        c_b = _tn_twice(lambda Cd: gemm(Ad, Bd, Cd, **kw), C0, s * prod, f"{name} {mode}{tag}, again")
        assert _same_bits(c_a, c_b)
        _tn_twice(lambda Cd: gemm(Ad, Bd, Cd, atomic=True, **kw), C0, s * prod, f"{name} atomic{tag}")


JOBS8 = [(264, 520), (8, 264), (512, 264), (256, 8), (8, 8), (264, 8), (72, 136), (16, 520)]     # 6 + 2 + 4 + 1 | + 1 + 2 + 1 + 3 tiles
JOBS11 = [(264, 520), (512, 264), (256, 8)]                                                        # 6 + 4 + 1 tiles
_W16 = {264: 272, 8: 16, 520: 528, 72: 80, 136: 144}                                               # the same lists in multiples of 16 (e4m3)
JOBS8_16 = [(_W16.get(a, a), _W16.get(b, b)) for a, b in JOBS8]
JOBS11_16 = [(_W16.get(a, a), _W16.get(b, b)) for a, b in JOBS11]
FP8_SCALES = [(0.25, 8.0), (None, None), (2.0, None), (None, 0.5)]                                 # (alpha, alpha2) of job j % 4: |product| <= 2

TN_BATCH_CASES = [                                 # kind, M, dims, usable CUs, plan, id
    ("bf16", 300, JOBS8[4:5], None, "splits", "1job"),                      # one job, one tile, 5 chunks in 5 splits
    ("bf16", 1700, JOBS8[:4], None, "splits", "4jobs"),                     # four jobs, 13 tiles, ragged last chunk
    ("bf16", 1700, JOBS8, None, "splits", "8jobs"),                         # eight jobs, 20 tiles
    ("bf16", 1700, JOBS8[:4], 8, "owners", "4jobs-G8-owners"),              # 13 tiles on 8 CUs: single owners, two rounds, workspace requirement 0
    ("bf16", 1700, JOBS8[:4], 24, "helpers", "4jobs-G24-helpers"),          # 13 tiles on 24 CUs: one split of 22 chunks, the last 5 chunks of every tile by 11 helpers
    ("bf16", 3100, JOBS11, 32, "helpers", "3jobs-G32-helpers"),             # 11 tiles on 32 CUs: two splits of 22 chunks + 5 chunks by 10 helpers
    # e4m3 (chunks of 128 rows): the same plans at twice the rows
    ("e4m3", 600, JOBS8_16[4:5], None, "splits", "1job"),                   # 5 splits of one chunk
    ("e4m3", 1700, JOBS8_16[:4], None, "splits", "4jobs-1700"),             # 14 chunks in 3 splits of 5, the last split and chunk ragged
    ("e4m3", 3400, JOBS8_16[:4], None, "splits", "4jobs"),                  # 4 splits of 7 chunks
    ("e4m3", 3400, JOBS8_16[:4], 8, "owners", "4jobs-G8-owners"),           # single owners of 27 chunks, workspace requirement 0
    ("e4m3", 3400, JOBS8_16[:4], 24, "helpers", "4jobs-G24-helpers"),       # one split of 22 chunks + 5 chunks by helpers
    ("e4m3", 6200, JOBS11_16, 32, "helpers", "3jobs-G32-helpers"),          # two splits of 22 chunks + 5 chunks by helpers
]


@pytest.mark.parametrize("kind,M,dims,G,plan", [c[:5] for c in TN_BATCH_CASES], ids=[_tn_id(c[0], c[5]) for c in TN_BATCH_CASES])
def test_tn_exact_batch(ops, L, usable, kind, M, dims, G, plan):
    fp8 = kind == "e4m3"
    G = usable(G)
    ops_in = [X.operands_tn(M, N1, N2, seed=M + (5 if fp8 else 7) * j, scale=2.0 if fp8 else 1.0) for j, (N1, N2) in enumerate(dims)]
    scales = [FP8_SCALES[j % 4] if fp8 else (None, None) for j in range(len(dims))]
    prods = [(a or 1.0) * (a2 or 1.0) * X.ref_tn(A, B) for (A, B, _), (a, a2) in zip(ops_in, scales)]
    T = sum(math.ceil(N1 / 256) * math.ceil(N2 / 256) for N1, N2 in dims)
    knobs = dict(forced=_knob("VITSSL_TN_BATCH_SPLITS"), use_rem=os.environ.get("VITSSL_TN_BATCH_REM", "1") != "0", km=128 if fp8 else 64)
    S, cps, rem = X.tn_batch_plan(M, T, G, **knobs)
    if not knobs["forced"] and knobs["use_rem"]:                 # the plan the case id names (the knob child forces another one)
        assert {"splits": S > 1 and rem == 0, "owners": S == 1 and rem == 0, "helpers": rem > 0}[plan], (S, cps, rem)
    if fp8:
        jobs = [(X.to_fp8(A).to(DEV), X.to_fp8(B).to(DEV), C0.to(DEV), _scalar(a), _scalar(a2)) for (A, B, C0), (a, a2) in zip(ops_in, scales)]
        arr, batch, query = (L.Fp8TnJob * len(jobs))(), ops.gemm_fp8_tn_batch, L.lib().vitssl_gemm_fp8_tn_batch_workspace_floats
    else:
        jobs = [(A.to(DEV), B.to(DEV), C0.to(DEV)) for A, B, C0 in ops_in]
        arr, batch, query = (L.TnJob * len(jobs))(), ops.gemm_tn_batch, L.lib().vitssl_gemm_tn_batch_workspace_floats
    for j, job in enumerate(jobs):
        A, B, Cd = job[:3]
        ptrs = dict(A8=A.data_ptr(), B8=B.data_ptr()) if fp8 else dict(A=A.data_ptr(), B=B.data_ptr())
        for field, v in dict(ptrs, C=Cd.data_ptr(), N1=A.shape[1], N2=B.shape[1]).items():
            setattr(arr[j], field, v)
    assert query(arr, len(jobs), M) == X.tn_batch_workspace(M, T, G, **knobs)
    for call in (1, 2):
        batch(jobs)
        for j, ((_, _, C0), prod, job) in enumerate(zip(ops_in, prods, jobs)):
            X.check_exact(job[2], X.to_f32_exact(C0.double() + call * prod), f"{batch.__name__} {plan}: job {j} {dims[j]}, call {call}")


# ----------------------------------------------------------------------------- fp8 operands (always the ping-pong kernel)
@pytest.mark.parametrize("regime,M,N,K", [("small", 300, 264, 128), ("round", 1000, 520, 256)], ids=["small-300x264x128", "round-1000x520x256"])
def test_fp8_exact_nt(ops, L, regime, M, N, K):
    s = 2.0                                                      # alpha x alpha2
    A, B, bias = X.operands(M, N, K, seed=M + K, hi=X.regime_hi(regime, K), scale=s)
    A8, B8 = X.to_fp8(A).to(DEV), X.to_fp8(B).to(DEV)
    sc = dict(alpha=_scalar(0.25), alpha2=_scalar(8.0))
    acc = X.ref_nt(A, B) * s
    full = acc + bias.double()
    out = _filled((M, N), BF16)
    ops.gemm_fp8_nt(A8, B8, out, L.EPI_BF16, bias=bias.to(DEV), **sc)
    X.check_exact(out, X.bf16_rne(full), "fp8 EPI_BF16")
    out32 = _filled((M, N), F32)
    ops.gemm_fp8_nt(A8, B8, out32, L.EPI_F32, bias=bias.to(DEV), **sc)
    X.check_exact(out32, X.to_f32_exact(full), "fp8 EPI_F32")
    out32 = _filled((M, N), F32)
    ops.gemm_fp8_nt(A8, B8, out32, L.EPI_F32)
    X.check_exact(out32, X.to_f32_exact(X.ref_nt(A, B)), "fp8 EPI_F32, no scalars, no bias")
    res = X.int_values((M, N), -100, 100, seed=M)
    for p in DROPS:
        drop = ops.make_dropout(p, seed=9, site=3)
        keep = ops.dropout_mask(M, N, drop, DEV).cpu().double()
        out32 = _filled((M, N), F32)
        ops.gemm_fp8_nt(A8, B8, out32, L.EPI_RESID, bias=bias.to(DEV), aux=res.to(DEV), drop=drop, **sc)
        X.check_exact(out32, X.to_f32_exact(res.double() + full * keep * (2.0 if p else 1.0)), f"fp8 EPI_RESID p={p}")


@pytest.mark.parametrize("regime,M,N,K", [("small", 300, 264, 128), ("round", 1000, 520, 256)], ids=["small-300x264x128", "round-1000x520x256"])
def test_fp8_exact_nt_dgelu_image(ops, L, regime, M, N, K):
    """out0 = bf16(alpha alpha2 acc aux) and its e4m3 image e4m3(value x out_scale), both ONE rounding of the exact value (torch's own
    float8_e4m3fn conversion), and max |value| exactly"""
    s, s_out = 0.5, 0.5
    A, B, _ = X.operands(M, N, K, seed=M + K, hi=X.regime_hi(regime, K))
    aux = X.dgelu_aux(M, N, seed=K)
    want = X.to_f32_exact(X.ref_nt(A, B) * s * aux.double())
    assert float(want.abs().max()) * s_out <= 448
    out, out8, amax = _filled((M, N), BF16), _filled((M, N), BF16).to(FP8), torch.zeros(1, device=DEV)
    ops.gemm_fp8_nt(X.to_fp8(A).to(DEV), X.to_fp8(B).to(DEV), out, L.EPI_DGELU, alpha=_scalar(2.0), alpha2=_scalar(0.25), aux=aux.to(DEV),
                    out_fp8=out8, out_scale=_scalar(s_out), out_amax=amax)
    X.check_exact(out, want.to(BF16), "fp8 EPI_DGELU out0")
    X.check_exact(out8, (want * s_out).to(FP8), "fp8 EPI_DGELU e4m3 image")
    assert float(amax) == float(want.abs().max())
    if regime == "small":
        cs0 = X.int_values((N,), -5, 5, seed=N)
        cs = cs0.to(DEV)
        ops.gemm_fp8_nt(X.to_fp8(A).to(DEV), X.to_fp8(B).to(DEV), out, L.EPI_DGELU, alpha=_scalar(2.0), alpha2=_scalar(0.25), aux=aux.to(DEV), colsum=cs)
        X.check_exact(cs, X.to_f32_exact(cs0.double() + want.double().sum(0)), "fp8 EPI_DGELU column sums")


# ----------------------------------------------------------------------------- deterministic sums beside the GEMMs
@pytest.mark.parametrize("cols", [260, 384])
@pytest.mark.parametrize("rows", [1, 301, 4102])
def test_exact_column_sums(ops, rows, cols):
    """colsum_bf16 and the column sums of grad_mask_cast (p = 0 and 0.5), accumulated into a non-zero vector: one lost row is an
    integer off (the rel-L2 1e-4 of the tolerance tests cannot see it)"""
    x = X.int_values((rows, cols), -3, 3, seed=rows + cols)
    out0 = X.int_values((cols,), -5, 5, seed=cols)
    assert rows * 2 * 3 + 5 < X.EXACT
    outs = []
    for _ in range(2):
        out = out0.to(DEV)
        ops.colsum_bf16(x.to(BF16).to(DEV), out)
        outs.append(out)
    X.check_exact(outs[0], X.to_f32_exact(out0.double() + x.double().sum(0)), "colsum_bf16")
    assert _same_bits(outs[0], outs[1])
    for p in DROPS:
        drop = ops.make_dropout(p, seed=3, site=7)
        keep = ops.dropout_mask(rows, cols, drop, DEV).cpu().double()
        gm, cs = _filled((rows, cols), BF16), out0.to(DEV)
        ops.grad_mask_cast(x.to(DEV), gm, gm_colsum=cs, drop=drop)
        want = x.double() * keep * (2.0 if p else 1.0)
        X.check_exact(gm, X.bf16_rne(want), f"grad_mask_cast p={p}")
        X.check_exact(cs, X.to_f32_exact(out0.double() + want.sum(0)), f"grad_mask_cast column sums p={p}")
        ops.grad_mask_cast(x.to(DEV), gm, gm_colsum=cs, drop=drop)
        X.check_exact(cs, X.to_f32_exact(out0.double() + 2 * want.sum(0)), f"grad_mask_cast column sums p={p}, second call")


@pytest.mark.parametrize("n", [4, 1028, 4 * 57821])          # n % 4 == 0 is the entry point's contract; none a multiple of a block
def test_exact_l1_loss_sum(ops, n):
    pred, target = X.int_values((n,), -5, 5, seed=n), X.int_values((n,), -5, 5, seed=n + 1)
    assert 2 * n * 10 + 9 < X.EXACT
    total = (pred.double() - target.double()).abs().sum().view(1)
    loss = torch.full((1,), 9.0, device=DEV)
    ops.l1_loss(pred.to(DEV), target.to(DEV), loss)
    X.check_exact(loss, X.to_f32_exact(9.0 + total), "l1_loss loss_sum")
    ops.l1_loss(pred.to(DEV), target.to(DEV), loss)
    X.check_exact(loss, X.to_f32_exact(9.0 + 2 * total), "l1_loss loss_sum, second call")
