"""Every launching entry point of include/vitssl_hip.h on guarded-arena tensors (tests/_arena.py).

Per case of CASES, in this order:
  1. one call on arena tensors (rc == 0); entry points with a workspace get EXACTLY the floats their sizing function promises;
  2. arena.check(): no byte outside a tensor was written; no NaN in any output the header says is written (the documented
     exceptions are asserted to have stayed 0xFF by the case itself);
  3. parity with a plain fp64 reference (bit-exact oracle for the uint8 / gather work) at the bar of the op's existing test,
     named in Case.bar: no tolerance is introduced here;
  4. where the header promises the same bits in every run (Case.det): a second call whose outputs and workspace were filled
     with zeros instead of 0xFF gives the same bits -- nothing depends on what the scratch held before;
  5. workspace entry points: one float less, and workspace = NULL where one is required, raise VitsslError naming the sizing
     function, and every output and guard byte is still 0xFF (nothing was launched).

The two controls at the end show that the harness can fail.  All their accesses stay inside the arena's one allocation.
test_abi_case_off_stream runs the same body with a side stream current, behind a gate and through a captured graph
(tests/_offstream.py).  tests/test_abi_arena.py (no GPU) checks that every entry point of the header has a case here, on the
default stream and off it."""
import ctypes as C
import math
import zlib

import pytest
import torch

from _arena import Arena, ArenaError
from _offstream import MAX_ARENA_MIB, offstream, twin_of  # noqa: F401  (offstream is a fixture)
from _util import rel_l2, max_abs

DEV = torch.device("cuda:0")
BF16, F32, FP8, U8, I32, I64 = torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.uint8, torch.int32, torch.int64
DH = 64
gpu = pytest.mark.gpu


def _L():
    from vitssl_hip import _lib
    return _lib


def call(name, *args):
    _L().call(name, *args)


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bf(x):
    return x.to(BF16)


def q8(x32):
    return x32.clamp(-448.0, 448.0).to(FP8)


def f8(t8):
    return t8.cpu().float()


def drop_of(p, seed=5, site=11):
    return _L().Dropout(float(p), site, seed)


def drop_scale(p):
    return 1.0 if p == 0 else 65536.0 / (65536 - round(p * 65536))


def keep_of(rows, cols, drop):
    from vitssl_hip import ops
    return ops.dropout_mask(rows, cols, drop, DEV).cpu().double()


def close_bf16(got, ref, atol=2e-3, what=""):
    from test_gpu_ops import close_bf16 as f
    f(got, ref, atol=atol, what=what)


def sum_ws(rows, cols):
    return int(_L().lib().vitssl_sum_workspace_floats(rows, cols))


class Spec:
    """What a case builder hands to the driver.
    run(wsp, wsn): the call (wsp / wsn: workspace pointer and float count, ignored by entry points without one)
    outs:    name -> tensor the call overwrites (poisoned before every run, NaN-checked after; partial = names the case checks itself)
    accs:    name -> (tensor, value) the caller initialises and the call accumulates into / updates in place
    scratch: tensors without a size argument that the call may use as it likes (attention's delta_ws)
    ws_floats / ws_fn: promised workspace size and the sizing function's name; null: "refused" | "atomic" | None (not tried)"""

    def __init__(self, run, outs, verify, accs=None, scratch=(), ws_floats=None, ws_fn=None, null="refused", partial=()):
        self.run, self.outs, self.verify, self.accs, self.scratch = run, outs, verify, accs or {}, scratch
        self.ws_floats, self.ws_fn, self.null, self.partial = ws_floats, ws_fn, null, partial


# ============================================================================================ builders
def b_dropout_mask(a, rows, cols, p):
    keep = a.empty("keep", (rows, cols), U8)
    d = drop_of(p)

    def verify():
        from test_dropout_stream import keep_mask             # the NumPy restatement of the mixer
        want = torch.from_numpy(keep_mask(rows, cols, p, d.seed, d.site).astype("uint8")).view(rows, cols)
        assert torch.equal(keep.cpu(), want)
    return Spec(lambda w, n: call("vitssl_dropout_mask", P(keep), rows, cols, d, S()), {"keep": keep}, verify)


def _ln_inputs(a, rows, cols):
    x = torch.randn(rows, cols) * 2 + 0.5
    gamma, beta = torch.rand(cols) + 0.5, torch.randn(cols) * 0.1
    return x, gamma, beta, a.put("x", x), a.put("gamma", gamma), a.put("beta", beta)


def b_ln_fwd(a, rows, cols, fp8=False, y16=True):
    x, gamma, beta, xd, gd, bd = _ln_inputs(a, rows, cols)
    y = a.empty("y", (rows, cols), BF16) if y16 else None
    mean, rstd = a.empty("mean", (rows,), F32), a.empty("rstd", (rows,), F32)
    outs = {"mean": mean, "rstd": rstd}
    if y16:
        outs["y"] = y
    if fp8:
        y8 = outs["y8"] = a.empty("y8", (rows, cols), FP8)

    def run(w, n):
        if fp8:
            call("vitssl_layernorm_fwd_fp8", P(xd), P(gd), P(bd), P(y), P(y8), P(mean), P(rstd), rows, cols, C.c_float(1e-5), S())
        else:
            call("vitssl_layernorm_fwd", P(xd), P(gd), P(bd), P(y), P(mean), P(rstd), rows, cols, C.c_float(1e-5), S())

    def verify():
        x64 = x.double()
        ref = torch.nn.functional.layer_norm(x64, (cols,), gamma.double(), beta.double(), 1e-5)
        if y16:
            close_bf16(y, bf(ref.float()), what="ln fwd")
        assert max_abs(mean, x64.mean(-1)) < 1e-5
        assert rel_l2(rstd, torch.rsqrt(x64.var(-1, unbiased=False) + 1e-5)) < 1e-5
        if fp8:
            same = (y8.cpu().view(U8) == q8(ref.float()).view(U8)).float().mean()
            assert float(same) > 0.995 and rel_l2(f8(y8), ref) < 4e-2
    return Spec(run, outs, verify)


def b_ln_bwd(a, rows, cols, p=0.25, cs=True, gm16=True, fp8=False):
    x, gamma, beta, xd, gd, _ = _ln_inputs(a, rows, cols)
    mean32, rstd32 = x.mean(-1), torch.rsqrt(x.var(-1, unbiased=False) + 1e-5)
    dy, g_res = bf(torch.randn(rows, cols)), torch.randn(rows, cols)
    dyd, grd, md, rd = a.put("dy", dy), a.put("g_res", g_res), a.put("mean", mean32), a.put("rstd", rstd32)
    g_out = a.empty("g_out", (rows, cols), F32)
    outs = {"g_out": g_out}
    gm = outs["gm"] = a.empty("gm", (rows, cols), BF16) if gm16 else None
    if not gm16:
        del outs["gm"]
    accs = {"dgamma": (a.empty("dgamma", (cols,), F32), 0.0), "dbeta": (a.empty("dbeta", (cols,), F32), 0.0)}
    csum = None
    if cs:
        csum = a.empty("gm_colsum", (cols,), F32)
        accs["gm_colsum"] = (csum, 0.0)
    drop = drop_of(p, 99, 7)
    s_q = 2.0 ** 3
    if fp8:
        gm8 = outs["gm8"] = a.empty("gm8", (rows, cols), FP8)
        qs = a.put("qscale", torch.tensor([s_q]))
        amax = a.empty("qamax", (1,), F32)
        accs["qamax"] = (amax, 0.0)
    dg, db = accs["dgamma"][0], accs["dbeta"][0]

    def run(w, n):
        if fp8:
            call("vitssl_layernorm_bwd_fp8", P(dyd), P(xd), P(md), P(rd), P(gd), P(grd), P(g_out), P(gm), P(gm8), P(qs), P(amax), P(dg),
                 P(db), P(csum), drop, rows, cols, w, n, S())
        else:
            call("vitssl_layernorm_bwd", P(dyd), P(xd), P(md), P(rd), P(gd), P(grd), P(g_out), P(gm), P(dg), P(db), P(csum), drop, rows,
                 cols, w, n, S())

    def verify():
        xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
        (torch.nn.functional.layer_norm(xr, (cols,), gr, br, 1e-5) * dy.double()).sum().backward()
        ref_g = xr.grad + g_res.double()
        assert rel_l2(g_out, ref_g) < 1e-5
        assert rel_l2(dg, gr.grad) < 1e-4 and rel_l2(db, br.grad) < 1e-4
        ref_gm = ref_g * keep_of(rows, cols, drop) * drop_scale(p)
        if gm16:
            close_bf16(gm, bf(ref_gm.float()), what="ln bwd gm")
        if cs:
            assert rel_l2(csum, ref_gm.sum(0)) < 1e-3
        if fp8:
            assert abs(float(amax) - float(ref_gm.abs().max())) <= 1e-4 * float(amax)
            from test_gpu_fp8 import _same_e4m3
            assert float(_same_e4m3(gm8, q8((ref_gm * s_q).float())).float().mean()) > 0.999
    return Spec(run, outs, verify, accs, ws_floats=sum_ws(rows, cols), ws_fn="vitssl_sum_workspace_floats")


def b_grad_mask_cast(a, rows, cols, p=0.0, cs=True, fp8=False):
    g = torch.randn(rows, cols)
    gd = a.put("g", g)
    gm = a.empty("gm", (rows, cols), BF16)
    outs, accs = {"gm": gm}, {}
    csum = None
    if cs:
        csum = a.empty("gm_colsum", (cols,), F32)
        accs["gm_colsum"] = (csum, 0.0)
    drop = drop_of(p, 3, 2)
    s_q = 2.0 ** 4
    if fp8:
        gm8 = outs["gm8"] = a.empty("gm8", (rows, cols), FP8)
        qs = a.put("qscale", torch.tensor([s_q]))
        amax = a.empty("qamax", (1,), F32)
        accs["qamax"] = (amax, 0.0)

    def run(w, n):
        if fp8:
            call("vitssl_grad_mask_cast_fp8", P(gd), P(gm), P(gm8), P(qs), P(amax), P(csum), drop, rows, cols, w, n, S())
        else:
            call("vitssl_grad_mask_cast", P(gd), P(gm), P(csum), drop, rows, cols, w, n, S())

    def verify():
        ref = g.double() * keep_of(rows, cols, drop) * drop_scale(p)
        if p == 0:
            assert torch.equal(gm.cpu(), bf(g))
        else:
            close_bf16(gm, bf(ref.float()), what="grad_mask_cast gm")
        if cs:
            assert rel_l2(csum, ref.sum(0)) < 1e-4
        if fp8:
            from test_gpu_fp8 import _same_e4m3
            assert float(_same_e4m3(gm8, q8((ref * s_q).float())).float().mean()) > 0.999
            assert abs(float(amax) - float(ref.abs().max())) <= 1e-4 * float(amax)
    if not cs:
        return Spec(run, outs, verify, accs)
    return Spec(run, outs, verify, accs, ws_floats=sum_ws(rows, cols), ws_fn="vitssl_sum_workspace_floats")


def _gelu64(u):
    cdf = 0.5 * (1 + torch.erf(u / math.sqrt(2)))
    return u * cdf, cdf + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def b_gemm_nt(a, M, N, K, epi, cs=False, p=0.0, bias=True, embed=None):
    """epi: "bf16" | "f32" | "gelu" | "dgelu" | "resid" | "embed"; embed = (images, tok_offset, use_mask)"""
    L = _L()
    A, B = bf(torch.randn(M, K) * 0.5), bf(torch.randn(N, K) * 0.5)
    bias_t = torch.randn(N) if bias and epi != "dgelu" else None
    acc = A.double() @ B.double().t()
    ref = acc + (bias_t.double() if bias_t is not None else 0.0)
    g = L.Gemm()
    Ad, Bd, biasd = a.put("A", A), a.put("B", B), (a.put("bias", bias_t) if bias_t is not None else None)
    g.A, g.B, g.M, g.N, g.K, g.bias = P(Ad), P(Bd), M, N, K, P(biasd)
    g.epilogue = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "gelu": L.EPI_GELU, "resid": L.EPI_RESID, "dgelu": L.EPI_DGELU,
                  "embed": L.EPI_EMBED}[epi]
    drop = drop_of(p)
    g.drop = drop
    outs, accs, partial = {}, {}, ()
    if epi == "embed":
        imgs, tok_offset, use_mask = embed
        tokens = M // imgs
        out_tokens = tokens + tok_offset
        pos, mtok = torch.rand(out_tokens, N), torch.randn(N)
        mask = (torch.rand(M) < 0.5).to(U8) if use_mask else None
        posd, mtokd, maskd = a.put("pos", pos), a.put("mask_token", mtok), (a.put("mask", mask) if use_mask else None)
        e = L.Embed()
        e.mask, e.mask_token, e.pos, e.tokens, e.out_tokens, e.tok_offset = P(maskd), P(mtokd), P(posd), tokens, out_tokens, tok_offset
        g.embed = e
        out0 = a.empty("out0", (imgs * out_tokens, N), F32)
        partial = ("out0",) if tok_offset else ()
    else:
        out0 = a.empty("out0", (M, N), F32 if epi in ("f32", "resid") else BF16)
    outs["out0"] = out0
    g.out0 = P(out0)
    if epi == "gelu":
        out1 = outs["out1"] = a.empty("out1", (M, N), BF16)
        g.out1 = P(out1)
    if epi == "resid":
        res = torch.randn(M, N)
        resd = a.put("aux", res)
        g.aux = P(resd)
    if epi == "dgelu":
        gp = bf(torch.rand(M, N) * 1.2)
        gpd = a.put("aux", gp)
        g.aux = P(gpd)
    if cs:
        csum = a.empty("colsum", (N,), F32)
        accs["colsum"] = (csum, 0.0)
        g.colsum = P(csum)
    keepalive = [Ad, Bd]

    def run(w, n):
        g.workspace, g.workspace_floats = (w, n) if cs else (C.c_void_p(0), 0)
        call("vitssl_gemm_bf16_nt", C.byref(g), S())

    def verify():
        assert keepalive
        sc = drop_scale(p)
        if epi == "bf16":
            close_bf16(out0, bf(ref.float()), atol=5e-3, what="EPI_BF16")
            if cs:
                assert rel_l2(csum, ref.sum(0)) < 1e-3
        elif epi == "f32":
            assert rel_l2(out0, ref) < 1e-5
        elif epi == "resid":
            assert rel_l2(out0, res.double() + ref * keep_of(M, N, drop) * sc) < 1e-5
        elif epi == "dgelu":
            ref_du = acc * gp.double()
            close_bf16(out0, bf(ref_du.float()), atol=5e-3, what="EPI_DGELU")
            if cs:
                assert rel_l2(csum, ref_du.sum(0)) < 2e-3
        elif epi == "gelu":
            keep = keep_of(M, N, drop)
            u = bf(ref.float()).double()
            ga, gd_ = _gelu64(u)
            slack = 2e-3 + 1.13 * sc * u.abs() * 2.0 ** -7        # test_gemm_nt_epilogues: u may sit one bf16 ulp away
            for got, want, what in ((out0, gd_ * keep * sc, "g'"), (out1, ga * keep * sc, "a")):
                err = (got.cpu().double() - want).abs()
                assert bool((err <= want.abs() * 2.0 ** -7 + slack).all()), f"EPI_GELU {what}: max excess {float((err - want.abs() * 2.0 ** -7 - slack).max())}"
        else:
            tok = ref.view(imgs, tokens, N).clone()
            if mask is not None:
                tok = torch.where(mask.view(imgs, tokens, 1).bool(), mtok.double(), tok)
            tok = tok + pos.double()[tok_offset:]
            got = out0.view(imgs, out_tokens, N)
            assert not torch.isnan(got[:, tok_offset:]).any()
            assert rel_l2(got[:, tok_offset:], tok) < 1e-5
            if tok_offset:
                assert Arena.untouched(got[:, 0].contiguous()), "the CLS slot belongs to the caller"
    if cs:
        return Spec(run, outs, verify, accs, ws_floats=sum_ws(M, N), ws_fn="vitssl_sum_workspace_floats", partial=partial)
    return Spec(run, outs, verify, accs, partial=partial)


def b_gemm_fp8_nt(a, M, N, K, epi, cs=False, p=0.0, image=False, out16=True):
    """bars of test_gemm_fp8_epilogues / test_gemm_fp8_dgelu_with_scaled_image"""
    L = _L()
    A, B = q8(torch.randn(M, K) * 2), q8(torch.randn(N, K) * 100)
    al, s_out = 2.0 ** -7, 0.5
    bias_t = torch.randn(N) if epi != "dgelu" else None
    acc = (A.float().double() @ B.float().double().t()) * al
    ref = acc + (bias_t.double() if bias_t is not None else 0.0)
    g, q = L.Gemm(), L.Fp8Gemm()
    Ad, Bd, ald = a.put("A8", A), a.put("B8", B), a.put("alpha", torch.tensor([al]))
    biasd = a.put("bias", bias_t) if bias_t is not None else None
    g.A, g.B, g.M, g.N, g.K, g.bias = P(Ad), P(Bd), M, N, K, P(biasd)
    g.epilogue = {"bf16": L.EPI_BF16, "f32": L.EPI_F32, "gelu": L.EPI_GELU, "resid": L.EPI_RESID, "dgelu": L.EPI_DGELU}[epi]
    q.alpha = P(ald)
    drop = drop_of(p, 11, 3)
    g.drop = drop
    outs, accs = {}, {}
    out0 = out1 = None
    if not (epi == "dgelu" and not out16):
        out0 = outs["out0"] = a.empty("out0", (M, N), F32 if epi in ("f32", "resid") else BF16)
    g.out0 = P(out0)
    if epi == "gelu" and out16:
        out1 = outs["out1"] = a.empty("out1", (M, N), BF16)
    g.out1 = P(out1)
    if epi == "resid":
        res = torch.randn(M, N)
        resd = a.put("aux", res)
        g.aux = P(resd)
    if epi == "dgelu":
        gp = bf(torch.rand(M, N) * 1.2)
        gpd = a.put("aux", gp)
        g.aux = P(gpd)
    if image:
        o8 = outs["out_fp8"] = a.empty("out_fp8", (M, N), FP8)
        osd = a.put("out_scale", torch.tensor([s_out]))
        amax = a.empty("out_amax", (1,), F32)
        accs["out_amax"] = (amax, 0.0)
        q.out_fp8, q.out_scale, q.out_amax = P(o8), P(osd), P(amax)
    if cs:
        csum = a.empty("colsum", (N,), F32)
        accs["colsum"] = (csum, 0.0)
        g.colsum = P(csum)

    def run(w, n):
        g.workspace, g.workspace_floats = (w, n) if cs else (C.c_void_p(0), 0)
        call("vitssl_gemm_fp8_nt", C.byref(g), C.byref(q), S())

    def verify():
        from test_gpu_fp8 import _same_e4m3
        sc = drop_scale(p)
        img_ref = None
        if epi == "f32":
            assert rel_l2(out0, ref) < 2e-5
        elif epi == "bf16":
            assert rel_l2(out0, ref) < 4e-3
            if cs:
                assert rel_l2(csum, ref.sum(0)) < 1e-4
        elif epi == "resid":
            assert rel_l2(out0, res.double() + ref * keep_of(M, N, drop) * sc) < 2e-5
        elif epi == "dgelu":
            img_ref = acc * gp.double()
            if out0 is not None:
                assert rel_l2(out0, img_ref) < 4e-3
            if cs:
                assert rel_l2(csum, img_ref.sum(0)) < 1e-4
        else:
            keep = keep_of(M, N, drop)
            ga, gd_ = _gelu64(bf(ref.float()).double())
            img_ref = ga * keep * sc
            assert rel_l2(out0, gd_ * keep * sc) < 4e-3
            if out1 is not None:
                assert rel_l2(out1, img_ref) < 4e-3
        if image:
            assert rel_l2(f8(o8) / s_out, img_ref) < 4e-2
            assert float(_same_e4m3(o8, q8((img_ref * s_out).float())).float().mean()) > 0.99
            assert abs(float(amax) - float(img_ref.abs().max())) <= 1e-4 * float(amax)
    if cs:
        return Spec(run, outs, verify, accs, ws_floats=sum_ws(M, N), ws_fn="vitssl_sum_workspace_floats")
    return Spec(run, outs, verify, accs)


def b_gemm_tn(a, M, N1, N2, fp8=False):
    lib = _L().lib()
    if fp8:
        A, B = q8(torch.randn(M, N1) * 3), q8(torch.randn(M, N2) * 2)
        al, al2 = 2.0 ** -5, 0.75
        ald, al2d = a.put("alpha", torch.tensor([al])), a.put("alpha2", torch.tensor([al2]))
    else:
        A, B = bf(torch.randn(M, N1) * 0.5), bf(torch.randn(M, N2) * 0.5)
        al = al2 = 1.0
    C0 = torch.randn(N1, N2)
    Ad, Bd = a.put("A", A), a.put("B", B)
    Cd = a.empty("C", (N1, N2), F32)
    fn = "vitssl_gemm_fp8_tn_workspace_floats" if fp8 else "vitssl_gemm_tn_workspace_floats"
    nws = int(getattr(lib, fn)(M, N1, N2))

    def run(w, n):
        if fp8:
            call("vitssl_gemm_fp8_tn", P(Ad), P(Bd), P(Cd), M, N1, N2, P(ald), P(al2d), w, n, S())
        else:
            call("vitssl_gemm_bf16_tn", P(Ad), P(Bd), P(Cd), M, N1, N2, w, n, S())

    def verify():
        ref = C0.double() + (A.float().double().t() @ B.float().double()) * (al * al2)
        assert rel_l2(Cd, ref) < (2e-5 if fp8 else 1e-5)
    return Spec(run, {}, verify, {"C": (Cd, C0)}, ws_floats=nws, ws_fn=fn, null="atomic")


def b_gemm_tn_batch(a, M, shapes, fp8=False):
    L = _L()
    lib = L.lib()
    arr = ((L.Fp8TnJob if fp8 else L.TnJob) * len(shapes))()
    host, accs, keepalive = [], {}, []
    for j, (N1, N2) in enumerate(shapes):
        if fp8:
            A, B = q8(torch.randn(M, N1) * 3), q8(torch.randn(M, N2) * 2)
            al = 2.0 ** -(3 + j)
            ald = a.put(f"alpha{j}", torch.tensor([al]))
        else:
            A, B = bf(torch.randn(M, N1) * 0.5), bf(torch.randn(M, N2) * 0.5)
            al = 1.0
        C0 = torch.randn(N1, N2)
        Ad, Bd, Cd = a.put(f"A{j}", A), a.put(f"B{j}", B), a.empty(f"C{j}", (N1, N2), F32)
        keepalive += [Ad, Bd]
        if fp8:
            arr[j].A8, arr[j].B8, arr[j].alpha, arr[j].alpha2 = Ad.data_ptr(), Bd.data_ptr(), ald.data_ptr(), 0
        else:
            arr[j].A, arr[j].B = Ad.data_ptr(), Bd.data_ptr()
        arr[j].C, arr[j].N1, arr[j].N2 = Cd.data_ptr(), N1, N2
        accs[f"C{j}"] = (Cd, C0)
        host.append((A, B, C0, al, Cd))
    fn = "vitssl_gemm_fp8_tn_batch_workspace_floats" if fp8 else "vitssl_gemm_tn_batch_workspace_floats"
    nws = int(getattr(lib, fn)(arr, len(shapes), M))
    entry = "vitssl_gemm_fp8_tn_batch" if fp8 else "vitssl_gemm_bf16_tn_batch"

    def verify():
        for j, (A, B, C0, al, Cd) in enumerate(host):
            ref = C0.double() + (A.float().double().t() @ B.float().double()) * al
            if fp8:     # test_gemm_fp8_tn_batch_matches_single_launches
                assert float((Cd.double().cpu() - ref).abs().max()) < 2e-5 * float(ref.abs().max()), j
            else:       # test_gemm_tn
                assert rel_l2(Cd, ref) < 1e-5, j
    return Spec(lambda w, n: call(entry, arr, len(shapes), M, w, n, S()), {}, verify, accs, ws_floats=nws, ws_fn=fn)


def b_attn_fwd(a, N, B, H, probs=True, fp8=False):
    from test_gpu_schedules import _ref_fwd, _check_fwd_items
    qkv = bf(torch.randn(B * N, 3 * H * DH))
    qd = a.put("qkv", qkv)
    out, lse = a.empty("out", (B * N, H * DH), BF16), a.empty("lse", (B, H, N), F32)
    outs = {"out": out, "lse": lse}
    pr = outs["probs"] = a.empty("probs", (B, H, N, N), F32) if probs else None
    if not probs:
        del outs["probs"]
    if fp8:
        o8 = outs["out_fp8"] = a.empty("out_fp8", (B * N, H * DH), FP8)

    def run(w, n):
        if fp8:
            call("vitssl_attn_fwd_fp8", P(qd), P(out), P(o8), P(lse), P(pr), B, N, H, DH, S())
        else:
            call("vitssl_attn_fwd", P(qd), P(out), P(lse), P(pr), B, N, H, DH, S())

    def verify():
        ref = _ref_fwd(qkv, B, N, H)
        _check_fwd_items(out, lse, pr, ref, B, N, H, list(range(B)))
        if fp8:     # test_attention_fwd_fp8_image
            assert rel_l2(f8(o8), ref[0].reshape(B * N, H * DH)) < 4e-2
            assert float((o8.cpu().view(U8) == q8(out.cpu().float()).view(U8)).float().mean()) > 0.95
    return Spec(run, outs, verify)


def b_attn_bwd(a, N, B, H, fp8=False, dq16=True):
    from test_gpu_schedules import _ref_fwd, _ref_bwd, _check_bwd_items
    qkv = bf(torch.randn(B * N, 3 * H * DH))
    dout = bf(torch.randn(B * N, H * DH) * (1e-3 if fp8 else 1.0))
    ro, rl, _ = _ref_fwd(qkv, B, N, H)
    qd, dod = a.put("qkv", qkv), a.put("dout", dout)
    od, ld = a.put("out", bf(ro.reshape(B * N, H * DH).float())), a.put("lse", rl.float())
    outs, accs = {}, {}
    dq = None
    if dq16:
        dq = outs["dqkv"] = a.empty("dqkv", (B * N, 3 * H * DH), BF16)
    s_q = 2.0 ** 13
    if fp8:
        d8 = outs["dqkv_fp8"] = a.empty("dqkv_fp8", (B * N, 3 * H * DH), FP8)
        qs = a.put("qscale", torch.tensor([s_q]))
        amax = a.empty("qamax", (1,), F32)
        accs["qamax"] = (amax, 0.0)
        scratch = ()
    else:
        delta = a.empty("delta_ws", (B, H, N), F32)         # exactly [B, H, N]
        scratch = (delta,)

    def run(w, n):
        if fp8:
            call("vitssl_attn_bwd_fp8", P(qd), P(od), P(dod), P(ld), P(dq), P(d8), P(qs), P(amax), B, N, H, DH, S())
        else:
            call("vitssl_attn_bwd", P(qd), P(od), P(dod), P(ld), P(dq), P(delta), B, N, H, DH, S())

    def verify():
        ref = _ref_bwd(qkv, dout, B, N, H)
        if dq16:
            _check_bwd_items(dq, ref, B, N, H, list(range(B)))
        if fp8:     # test_attention_bwd_fp8_image
            r2 = ref.reshape(B * N, 3 * H * DH)
            if not dq16:        # no bf16 tensor to compare with: the e4m3 bar of the image tests against the fp64 gradient
                assert not torch.isnan(f8(d8)).any() and rel_l2(f8(d8) / s_q, r2) < 4e-2
            if dq16:
                assert abs(float(amax) - float(dq.float().abs().max())) <= 2.0 ** -8 * float(amax)
                assert float((d8.cpu().view(U8) == q8(dq.cpu().float() * s_q).view(U8)).float().mean()) > 0.95
                assert rel_l2(f8(d8) / s_q, dq.cpu().float()) < 4e-2
    return Spec(run, outs, verify, accs, scratch=scratch)


def b_patchify(a, B, Cc, H, W, Pp):
    from oracle import vit_oracle as O
    img = torch.rand(B, Cc, H, W)
    ref = O.patchify(img, Pp).reshape(-1, Cc * Pp * Pp)
    imd = a.put("img", img)
    out = a.empty("patches", ref.shape, BF16)

    def verify():
        assert torch.equal(out.cpu(), bf(ref))
    return Spec(lambda w, n: call("vitssl_patchify_bf16", P(imd), P(out), B, Cc, H, W, Pp, S()), {"patches": out}, verify)


def b_gather_patches(a, B, Cc, H, W, Pp, n_idx):
    from oracle import vit_oracle as O
    img = torch.rand(B, Cc, H, W)
    ref = O.patchify(img, Pp).reshape(-1, Cc * Pp * Pp)
    idx = torch.randperm(ref.shape[0])[:n_idx].to(I32)
    idx[-1] = ref.shape[0] - 1                                  # the last patch of the last image
    imd, ixd = a.put("img", img), a.put("idx", idx)
    out = a.empty("out", (n_idx, ref.shape[1]), F32)

    def verify():
        assert torch.equal(out.cpu(), ref[idx.long()])
    return Spec(lambda w, n: call("vitssl_gather_patches_f32", P(imd), P(ixd), P(out), n_idx, Cc, H, W, Pp, S()), {"out": out}, verify)


def b_gather_rows(a, rows, cols, n_idx):
    x = torch.randn(rows, cols)
    idx = torch.randperm(rows)[:n_idx].to(I32)
    idx[-1] = rows - 1
    xd, ixd = a.put("x", x), a.put("idx", idx)
    out = a.empty("out", (n_idx, cols), BF16)

    def verify():
        assert torch.equal(out.cpu(), bf(x[idx.long()]))
    return Spec(lambda w, n: call("vitssl_gather_rows_bf16", P(xd), P(ixd), P(out), n_idx, cols, S()), {"out": out}, verify)


def b_scatter_rows(a, rows, cols, n_src):
    src = bf(torch.randn(n_src, cols))
    sel = torch.randperm(rows)[:n_src]
    sel[-1] = rows - 1
    sel = torch.unique(sel)
    inv = torch.full((rows,), -1, dtype=I32)
    inv[sel] = torch.arange(sel.numel(), dtype=I32)
    sd, ivd = a.put("src", src), a.put("inv", inv)
    g = a.empty("g", (rows, cols), F32)

    def verify():                                               # g = 0 except g[idx[i]] = src[i]: every row is written
        ref = torch.zeros(rows, cols)
        ref[sel] = src[:sel.numel()].float()
        assert torch.equal(g.cpu(), ref)
    return Spec(lambda w, n: call("vitssl_scatter_rows_f32", P(sd), P(ivd), P(g), rows, cols, S()), {"g": g}, verify)


def b_cls(a, B, T, D, scatter):
    if not scatter:
        x = torch.randn(B * T, D)
        xd = a.put("x", x)
        out = a.empty("out", (B, D), F32)

        def verify():
            assert torch.equal(out.cpu(), x.view(B, T, D)[:, 0])
        return Spec(lambda w, n: call("vitssl_gather_cls_f32", P(xd), P(out), B, T, D, S()), {"out": out}, verify)
    gc = torch.randn(B, D)
    gd = a.put("gcls", gc)
    g = a.empty("g", (B * T, D), F32)

    def verify():
        ref = torch.zeros(B, T, D)
        ref[:, 0] = gc
        assert torch.equal(g.cpu().view(B, T, D), ref)
    return Spec(lambda w, n: call("vitssl_scatter_cls_f32", P(gd), P(g), B, T, D, S()), {"g": g}, verify)


def b_embed_bwd(a, B, tokens, tok_offset, use_mask, D):
    T_out = tokens + tok_offset
    dtok = torch.randn(B * T_out, D)
    mask = (torch.rand(B * tokens) < 0.6).to(U8) if use_mask else None
    dd, md = a.put("dtok", dtok), (a.put("mask", mask) if use_mask else None)
    dproj = a.empty("dproj", (B * tokens, D), BF16)
    accs = {"dpos": (a.empty("dpos", (T_out, D), F32), 0.0), "dbias": (a.empty("dbias", (D,), F32), 0.0)}
    if use_mask:
        accs["dmask_token"] = (a.empty("dmask_token", (D,), F32), 0.0)
    if tok_offset:
        accs["dcls"] = (a.empty("dcls", (D,), F32), 0.0)
    t_ = lambda k: accs[k][0] if k in accs else None
    nws = int(_L().lib().vitssl_embed_bwd_workspace_floats(B, tokens, tok_offset, D))

    def run(w, n):
        call("vitssl_embed_bwd", P(dd), P(md), P(dproj), P(t_("dpos")), P(t_("dmask_token")), P(t_("dbias")), P(t_("dcls")), B, tokens,
             tok_offset, D, w, n, S())

    def verify():                                               # test_embed_bwd
        d3 = dtok.double().view(B, T_out, D)
        assert rel_l2(t_("dpos"), d3.sum(0)) < 1e-5
        rows = d3[:, tok_offset:].reshape(B * tokens, D)
        ref = rows.clone()
        if use_mask:
            mb = mask.bool()
            assert rel_l2(t_("dmask_token"), rows[mb].sum(0)) < 1e-5 and rel_l2(t_("dbias"), rows[~mb].sum(0)) < 1e-5
            ref[mb] = 0
        else:
            assert rel_l2(t_("dbias"), rows.sum(0)) < 1e-5
        assert torch.equal(dproj.cpu(), bf(ref.float()))
        if tok_offset:
            assert rel_l2(t_("dcls"), d3[:, 0].sum(0)) < 1e-5
    return Spec(run, {"dproj": dproj}, verify, accs, ws_floats=nws, ws_fn="vitssl_embed_bwd_workspace_floats")


def b_l1_loss(a, n, grad=True):
    pred, tgt = torch.randn(n), torch.rand(n)
    pred[:2] = tgt[:2]                                           # exact ties -> zero gradient
    pd, td = a.put("pred", pred), a.put("target", tgt)
    loss = a.empty("loss_sum", (1,), F32)
    dp = a.empty("dpred", (n,), BF16) if grad else None

    def verify():                                               # test_l1_loss
        assert abs(float(loss) / n - float((pred.double() - tgt.double()).abs().mean())) < 1e-6
        if grad:
            assert torch.equal(dp.cpu(), bf(torch.sign(pred - tgt) / n))
    return Spec(lambda w, nn: call("vitssl_l1_loss", P(pd), P(td), P(loss), P(dp), C.c_float(1.0 / n), n, w, nn, S()),
                {"dpred": dp} if grad else {}, verify, {"loss_sum": (loss, 0.0)}, ws_floats=sum_ws(n, 1),
                ws_fn="vitssl_sum_workspace_floats")


def b_cross_entropy(a, B, Cn):
    logits, labels = torch.randn(B, Cn) * 3, torch.randint(0, Cn, (B,))
    ld, lbd = a.put("logits", logits), a.put("labels", labels)
    loss = a.empty("loss_sum", (1,), F32)
    dl = a.empty("dlogits", (B, Cn), BF16)

    def verify():                                               # test_cross_entropy
        leaf = logits.double().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(leaf, labels)
        ref.backward()
        assert abs(float(loss) / B - float(ref)) < 1e-5
        close_bf16(dl, bf(leaf.grad.float()), atol=1e-4, what="ce grad")
    return Spec(lambda w, n: call("vitssl_cross_entropy", P(ld), P(lbd), P(loss), P(dl), C.c_float(1.0 / B), B, Cn, S()), {"dlogits": dl},
                verify, {"loss_sum": (loss, 0.0)})


def b_colsum_bf16(a, rows, cols):
    x = bf(torch.randn(rows, cols))
    xd = a.put("x", x)
    out = a.empty("out", (cols,), F32)
    o0 = torch.randn(cols)

    def verify():                                               # column sums of a bf16 matrix: the grad_mask_cast bar of _layernorm_case
        assert rel_l2(out, o0.double() + x.double().sum(0)) < 1e-4
    return Spec(lambda w, n: call("vitssl_colsum_bf16", P(xd), P(out), rows, cols, w, n, S()), {}, verify, {"out": (out, o0)},
                ws_floats=sum_ws(rows, cols), ws_fn="vitssl_sum_workspace_floats")


def b_cast_bf16(a, n):
    v = torch.randn(n)
    vd = a.put("src", v)
    d = a.empty("dst", (n,), BF16)

    def verify():
        assert torch.equal(d.cpu(), bf(v))
    return Spec(lambda w, nn: call("vitssl_cast_bf16", P(vd), P(d), n, S()), {"dst": d}, verify)


def b_cast_transpose(a, R, Cn, plain=True, transposed=True):
    src = torch.randn(R, Cn)
    sd = a.put("src", src)
    outs = {}
    dst = dst_t = None
    if plain:
        dst = outs["dst"] = a.empty("dst", (R, Cn), BF16)
    if transposed:
        dst_t = outs["dst_t"] = a.empty("dst_t", (Cn, R), BF16)

    def verify():                                               # test_casts
        assert dst is None or torch.equal(dst.cpu(), bf(src))
        assert dst_t is None or torch.equal(dst_t.cpu(), bf(src).t())
    return Spec(lambda w, n: call("vitssl_cast_transpose_bf16", P(sd), P(dst), P(dst_t), R, Cn, S()), outs, verify)


def _job_table(a, jobs):
    """device job table of vitssl_cast_job_t / vitssl_fp8_weight_job_t (same layout) and its tile_start, inside the arena"""
    import numpy as np
    rec = np.zeros(len(jobs), dtype=np.dtype([("src", "<u8"), ("dst", "<u8"), ("dst_t", "<u8"), ("R", "<i4"), ("C", "<i4")]))
    starts = np.zeros(len(jobs) + 1, dtype=np.int32)
    for i, (s, d, t) in enumerate(jobs):
        R, Cn = s.shape
        rec[i] = (s.data_ptr(), 0 if d is None else d.data_ptr(), 0 if t is None else t.data_ptr(), R, Cn)
        starts[i + 1] = starts[i] + ((R + 63) // 64) * ((Cn + 63) // 64)
    return a.put("jobs", torch.from_numpy(rec.view(np.uint8).copy())), a.put("tile_start", torch.from_numpy(starts)), int(starts[-1])


def b_cast_batch(a, shapes, fp8=False):
    dt = FP8 if fp8 else BF16
    srcs = [torch.randn(R, Cn) * (10.0 ** (i - 2)) for i, (R, Cn) in enumerate(shapes)]
    outs, jobs = {}, []
    for i, s in enumerate(srcs):
        d = None if i == 1 else a.empty(f"dst{i}", s.shape, dt)
        t = None if i == 2 else a.empty(f"dst_t{i}", s.shape[::-1], dt)
        for k, v in ((f"dst{i}", d), (f"dst_t{i}", t)):
            if v is not None:
                outs[k] = v
        jobs.append((a.put(f"src{i}", s), d, t))
    tab, starts, total = _job_table(a, jobs)
    nj = len(jobs)
    if fp8:
        amax_ws, alpha = a.empty("amax_ws", (nj,), F32), a.empty("alpha", (nj,), F32)
        outs["alpha"] = alpha
        accs = {"amax_ws": (amax_ws, 0.0)}      # Fp8WeightPlan hands over a zeroed amax table
        run = lambda w, n: call("vitssl_fp8_quantize_weights", P(tab), P(starts), nj, total, P(amax_ws), P(alpha), S())
    else:
        accs = {}
        run = lambda w, n: call("vitssl_cast_transpose_batch", P(tab), P(starts), nj, total, S())

    def verify():
        from oracle import vit_oracle as O
        for i, s in enumerate(srcs):
            if fp8:     # test_fp8_weight_images_bit_exact
                k = O.fp8_scale_exp(float(s.abs().max()))
                assert float(alpha[i]) == 2.0 ** -k, i
                want = q8(s * (2.0 ** k)).view(U8)
            else:       # test_casts
                want = bf(s)
            _, d, t = jobs[i]
            if d is not None:
                assert torch.equal(d.cpu().view(want.dtype), want), i
            if t is not None:
                assert torch.equal(t.cpu().view(want.dtype), want.t().contiguous()), i
    return Spec(run, outs, verify, accs)


def b_quantize_fp8(a, n, scaled):
    x = bf(torch.randn(n) * torch.exp2(torch.randint(-12, 10, (n,)).float()))
    xd = a.put("x", x)
    y = a.empty("y8", (n,), FP8)
    if not scaled:
        def verify():                                           # test_quantize_fp8_bit_exact
            assert torch.equal(y.cpu().view(U8), q8(x.float()).view(U8))
        return Spec(lambda w, nn: call("vitssl_quantize_fp8", P(xd), P(y), n, S()), {"y8": y}, verify)
    s = 2.0 ** 3
    sd = a.put("qscale", torch.tensor([s]))
    amax = a.empty("qamax", (1,), F32)

    def verify():                                               # test_quantize_fp8_scaled_and_amax
        assert torch.equal(y.cpu().view(U8), q8(x.float() * s).view(U8))
        assert float(amax) == float(x.float().abs().max())
    return Spec(lambda w, nn: call("vitssl_quantize_fp8_scaled", P(xd), P(y), n, P(sd), P(amax), S()), {"y8": y}, verify,
                {"qamax": (amax, 0.0)})


def b_adamw(a, n):
    from oracle import vit_oracle as O
    p0, gr = torch.randn(n), torch.randn(n)
    lr, wd = 1e-3, 1e-3
    pd, gd = a.empty("p", (n,), F32), a.put("g", gr)
    md, vd = a.empty("m", (n,), F32), a.empty("v", (n,), F32)

    def verify():                                               # test_adamw_matches_torch_golden (first step, zero moments)
        z = torch.zeros(n, dtype=torch.float64)
        rp, rm, rv = O.adamw_step(p0.double(), gr.double(), z, z.clone(), 1, lr, wd=wd)
        assert max_abs(pd, rp) < 2e-6 and max_abs(md, rm) < 2e-6 and max_abs(vd, rv) < 2e-6
    return Spec(lambda w, nn: call("vitssl_adamw", P(pd), P(gd), P(md), P(vd), n, C.c_float(lr), C.c_float(0.9), C.c_float(0.999),
                                   C.c_float(1e-8), C.c_float(wd), 1, C.c_float(1.0), S()), {}, verify,
                {"p": (pd, p0), "m": (md, 0.0), "v": (vd, 0.0)})


def b_ema(a, n):
    from oracle import vit_oracle as O
    tt, ss = torch.randn(n), torch.randn(n)
    td, sd = a.empty("teacher", (n,), F32), a.put("student", ss)

    def verify():                                               # test_ema
        assert max_abs(td, O.ema_update(tt, ss, 0.996)) < 1e-6
    return Spec(lambda w, nn: call("vitssl_ema", P(td), P(sd), n, C.c_float(0.996), S()), {}, verify, {"teacher": (td, tt)})


def b_rownorm(a, rows, D, bwd):
    from test_gpu_schedules import _close_rows
    z = torch.randn(rows, D) * 2
    z64 = z.double()
    nrm = z64.norm(dim=1).clamp_min(1e-12)
    if not bwd:
        zd = a.put("z", z)
        zn, inv = a.empty("zn", (rows, D), BF16), a.empty("inv_norm", (rows,), F32)

        def verify():                                           # test_rownorm_fwd_bwd
            _close_rows(zn.float(), z64 / nrm[:, None], 2.0 ** -8, 0.0, "rownorm zn")
            assert float(((inv.cpu().double() - 1 / nrm).abs() / (1 / nrm)).max()) < 1e-5
        return Spec(lambda w, n: call("vitssl_rownorm_fwd", P(zd), P(zn), P(inv), rows, D, S()), {"zn": zn, "inv_norm": inv}, verify)
    zn, inv, dzn = bf((z64 / nrm[:, None]).float()), (1 / nrm).float(), torch.randn(rows, D)
    znd, invd, dd = a.put("zn", zn), a.put("inv_norm", inv), a.put("dzn", dzn)
    dz = a.empty("dz", (rows, D), BF16)

    def verify():
        n64, d64 = zn.double(), dzn.double()
        _close_rows(dz.float(), inv.double()[:, None] * (d64 - n64 * (n64 * d64).sum(1, keepdim=True)), 2.0 ** -8, 1e-4, "rownorm dz")
    return Spec(lambda w, n: call("vitssl_rownorm_bwd", P(dd), P(znd), P(invd), P(dz), rows, D, S()), {"dz": dz}, verify)


def b_weightnorm(a, K, D, bwd):
    from test_gpu_schedules import _close_rows
    v, g = torch.randn(K, D) * 0.05, torch.rand(K) + 0.5
    v64, g64 = v.double(), g.double()
    vn = v64.norm(dim=1)
    gd, vd = a.put("g", g), a.put("v", v)
    if not bwd:
        w_, inv = a.empty("w", (K, D), F32), a.empty("inv_vnorm", (K,), F32)

        def verify():                                           # test_weightnorm_fold_bwd
            _close_rows(w_, g64[:, None] * v64 / vn[:, None], 1e-5, 1e-6, "weightnorm w")
            assert float(((inv.cpu().double() - 1 / vn).abs() * vn).max()) < 1e-5
        return Spec(lambda w, n: call("vitssl_weightnorm_fold", P(gd), P(vd), P(w_), P(inv), K, D, S()), {"w": w_, "inv_vnorm": inv}, verify)
    dw, dg0, dv0 = torch.randn(K, D), torch.randn(K), torch.randn(K, D) * 0.1
    dwd, invd = a.put("dw", dw), a.put("inv_vnorm", (1 / vn).float())
    dg, dv = a.empty("dg", (K,), F32), a.empty("dv", (K, D), F32)

    def verify():
        vr, gr = v64.clone().requires_grad_(True), g64.clone().requires_grad_(True)
        (gr[:, None] * vr / vr.norm(dim=1, keepdim=True) * dw.double()).sum().backward()
        dg_err = (dg.cpu().double() - (dg0.double() + gr.grad)).abs()
        assert bool((dg_err <= 1e-5 * (dw.double() * v64 / vn[:, None]).abs().sum(1)).all()), float(dg_err.max())
        _close_rows(dv, dv0.double() + vr.grad, 1e-5, 1e-6, "weightnorm dv")
    return Spec(lambda w, n: call("vitssl_weightnorm_bwd", P(dwd), P(gd), P(vd), P(invd), P(dg), P(dv), K, D, S()), {}, verify,
                {"dg": (dg, dg0), "dv": (dv, dv0)})


def b_dino_loss(a, G, V, B, K):
    from test_gpu_schedules import _dino_inputs, _dino_ref, _close_rows, T_TEMP, S_TEMP, GSCALE
    teacher, student, center = _dino_inputs(G, V, B, K, seed=K + 10 * G + V + B)
    td, sd, cd = a.put("teacher", teacher.view(G * B, K)), a.put("student", student.view(V * B, K)), a.put("center", center)
    loss = a.empty("loss_sum", (1,), F32)
    ds = a.empty("dstudent", (V * B, K), BF16)
    nws = int(_L().lib().vitssl_dino_loss_workspace_floats(G, B, K))

    def run(w, n):
        call("vitssl_dino_loss", P(td), P(sd), P(cd), w, n, P(loss), P(ds), G, V, B, K, C.c_float(T_TEMP), C.c_float(S_TEMP),
             C.c_float(GSCALE), S())

    def verify():                                               # test_dino_loss_dispatch_branches
        ref_loss, ref_grad, mag = _dino_ref(teacher, student, center)
        assert abs(float(loss) - ref_loss) <= 1e-5 * abs(ref_loss), (float(loss), ref_loss)
        _close_rows(ds.float().view(V, B, K), GSCALE * ref_grad, 2.0 ** -8, 1e-5, f"dstudent K={K}", mag=GSCALE * mag, mtol=1e-4)
    # the loss value is an atomic sum over the student rows: only the gradient is compared bit for bit (Case.det = "outs")
    return Spec(run, {"dstudent": ds}, verify, {"loss_sum": (loss, 0.0)}, ws_floats=nws, ws_fn="vitssl_dino_loss_workspace_floats")


def b_colsum_f32(a, rows, K):
    x = torch.randn(rows, K) * 3 + 1
    xd = a.put("x", x)
    out = a.empty("out", (K,), F32)

    def verify():                                               # test_colsum_and_center_ema
        err = (out.cpu().double() - x.double().sum(0)).abs()
        assert bool((err <= 1e-6 * x.double().abs().sum(0) + 1e-30).all()), float(err.max())
    return Spec(lambda w, n: call("vitssl_colsum_f32", P(xd), P(out), rows, K, S()), {"out": out}, verify)


def b_center_ema(a, K):
    c0, cs = torch.randn(K), torch.randn(K) * 50
    cd, sd = a.empty("center", (K,), F32), a.put("colsum", cs)
    mom, inv_rows = 0.9, 1.0 / 83

    def verify():
        m32, i32 = (float(torch.tensor(v, dtype=F32)) for v in (mom, inv_rows))
        x, y = m32 * c0.double(), (1 - m32) * cs.double() * i32
        err = (cd.cpu().double() - (x + y)).abs()
        assert bool((err <= 1e-6 * (x.abs() + y.abs()) + 1e-30).all()), float(err.max())
    return Spec(lambda w, n: call("vitssl_center_ema", P(cd), P(sd), K, C.c_float(mom), C.c_float(inv_rows), S()), {}, verify,
                {"center": (cd, c0)})


def b_bicubic(a, g0, g1, D, bwd):
    from oracle import vit_oracle as O
    if not bwd:
        src = torch.randn(g0[0] * g0[1], D)
        sd = a.put("src", src)
        dst = a.empty("dst", (g1[0] * g1[1], D), F32)

        def verify():                                           # test_bicubic_resize_matches_aten_and_oracle
            ora = O.bicubic_resize(src.reshape(1, g0[0], g0[1], D).permute(0, 3, 1, 2), g1[0], g1[1]).permute(0, 2, 3, 1).reshape(-1, D)
            assert max_abs(dst, ora) < 2e-5
        return Spec(lambda w, n: call("vitssl_bicubic_resize_fwd", P(sd), P(dst), g0[0], g0[1], g1[0], g1[1], D, S()), {"dst": dst}, verify)
    gout, d0 = torch.randn(g1[0] * g1[1], D), torch.randn(g0[0] * g0[1], D)
    gd = a.put("ddst", gout)
    dsrc = a.empty("dsrc", (g0[0] * g0[1], D), F32)

    def verify():
        leaf = torch.zeros(g0[0] * g0[1], D, dtype=torch.float64, requires_grad=True)
        r = torch.nn.functional.interpolate(leaf.reshape(1, g0[0], g0[1], D).permute(0, 3, 1, 2), size=g1, mode="bicubic")
        r.permute(0, 2, 3, 1).reshape(-1, D).backward(gout.double())
        assert max_abs(dsrc.cpu() - d0, leaf.grad) < 5e-5
    return Spec(lambda w, n: call("vitssl_bicubic_resize_bwd", P(gd), P(dsrc), g0[0], g0[1], g1[0], g1[1], D, S()), {}, verify,
                {"dsrc": (dsrc, d0)})


def b_augment(a, stage, B, H, W, Sz, scale):
    """the three uint8 stages against oracle/augment_oracle.py, bit-exact (test_stages_bit_exact_against_oracle)"""
    import numpy as np
    from oracle import augment_oracle as AO
    from data.multicrop import ViewSpec, pack_params, sample_view_params
    from test_gpu_augment import _images
    imgs = _images(B, H, W, Sz)
    spec = ViewSpec(size=Sz, scale=scale, gray_p=0.5)
    gen = torch.Generator().manual_seed(Sz + H)
    prm = [sample_view_params(spec, H, W, gen) for _ in range(B)]
    ip, fp = pack_params(prm, 7)
    ipd, fpd = a.put("iparams", torch.from_numpy(ip)), a.put("fparams", torch.from_numpy(fp))
    ref1 = [AO.resized_crop_u8(imgs[b], p["top"], p["left"], p["h"], p["w"], Sz, Sz, p["flip"]) for b, p in enumerate(prm)]
    if stage == "crop":
        src = a.put("src", torch.from_numpy(imgs))
        tmp, dst = a.empty("tmp", (B, H, Sz, 3), U8), a.empty("dst", (B, Sz, Sz, 3), U8)

        def verify():
            assert np.array_equal(dst.cpu().numpy(), np.stack(ref1))
        return Spec(lambda w, n: call("vitssl_aug_resized_crop_u8", P(src), P(ipd), P(tmp), P(dst), B, H, W, Sz, S()), {"dst": dst}, verify,
                    scratch=(tmp,))
    ref2 = []
    for b, p in enumerate(prm):
        x = ref1[b]
        for fn in p["order"]:
            x = (AO.adjust_brightness(x, p["brightness"]) if fn == 0 else AO.adjust_contrast(x, p["contrast"]) if fn == 1
                 else AO.adjust_saturation(x, p["saturation"]) if fn == 2 else AO.adjust_hue(x, p["hue"]))
        ref2.append(AO.to_grayscale3(x) if p["gray"] else x)
    if stage == "color":
        img = a.empty("img", (B, Sz, Sz, 3), U8)

        def verify():
            assert np.array_equal(img.cpu().numpy(), np.stack(ref2))
        return Spec(lambda w, n: call("vitssl_aug_color_u8", P(img), P(ipd), P(fpd), B, Sz, S()), {}, verify,
                    {"img": (img, torch.from_numpy(np.stack(ref1)))})
    img = a.put("img", torch.from_numpy(np.stack(ref2)))
    out = a.empty("out", (B, 3, Sz, Sz), F32)

    def verify():
        ref3 = np.stack([AO.to_tensor(AO.gaussian_blur_u8(ref2[b], 7, p["sigma"])) for b, p in enumerate(prm)])
        assert np.array_equal(out.cpu().numpy(), ref3)
    return Spec(lambda w, n: call("vitssl_aug_blur_to_tensor", P(img), P(fpd), P(out), B, Sz, 7, S()), {"out": out}, verify)


# ============================================================================================ the table
class Case:
    def __init__(self, cid, entry, build, kw, bar, ws=False, det=False, mib=64, reserve=False, ws_zero_ok=False):
        self.id, self.entry, self.build, self.kw, self.bar = cid, entry, build, kw, bar
        self.ws, self.det, self.mib, self.reserve, self.ws_zero_ok = ws, det, mib, reserve, ws_zero_ok or reserve


CASES = []


def case(cid, entry, build, bar, ws=False, det=False, mib=64, reserve=False, ws_zero_ok=False, **kw):
    CASES.append(Case(cid, entry, build, kw, bar, ws, det, mib, reserve, ws_zero_ok))


case("dropout_mask-ragged", "vitssl_dropout_mask", b_dropout_mask, "tests/test_dropout_stream.py (bit-exact)", rows=301, cols=260, p=0.1)
case("dropout_mask-min", "vitssl_dropout_mask", b_dropout_mask, "tests/test_dropout_stream.py (bit-exact)", rows=1, cols=4, p=0.5)

for _r, _c in ((301, 64), (1, 4), (301, 768), (77, 2048), (301, 260)):
    case(f"ln_fwd-{_r}x{_c}", "vitssl_layernorm_fwd", b_ln_fwd, "_layernorm_case", rows=_r, cols=_c)
case("ln_fwd_fp8-301x260", "vitssl_layernorm_fwd_fp8", b_ln_fwd, "test_layernorm_fwd_fp8_images", rows=301, cols=260, fp8=True)
case("ln_fwd_fp8-only8-33x768", "vitssl_layernorm_fwd_fp8", b_ln_fwd, "test_layernorm_fwd_fp8_images", rows=33, cols=768, fp8=True, y16=False)
for _r, _c in ((302, 384), (301, 384), (2, 384), (301, 64), (1, 4), (301, 768), (77, 2048), (4096 + 7, 260)):
    case(f"ln_bwd-{_r}x{_c}", "vitssl_layernorm_bwd", b_ln_bwd, "_layernorm_case", ws=True, det=True, mib=128, rows=_r, cols=_c)
case("ln_bwd-nocolsum-302x384", "vitssl_layernorm_bwd", b_ln_bwd, "_layernorm_case", ws=True, det=True, rows=302, cols=384, cs=False, p=0.0)
case("ln_bwd-nogm-301x768", "vitssl_layernorm_bwd", b_ln_bwd, "_layernorm_case", ws=True, det=True, rows=301, cols=768, cs=False, gm16=False)
for _r, _c in ((4098, 384), (4097, 768)):
    case(f"ln_bwd-reserved-{_r}x{_c}", "vitssl_layernorm_bwd", b_ln_bwd, "_layernorm_case", ws=True, det=True, reserve=True, mib=128, rows=_r, cols=_c)
case("ln_bwd_fp8-301x768", "vitssl_layernorm_bwd_fp8", b_ln_bwd, "test_layernorm_bwd_fp8_image", ws=True, det=True, rows=301, cols=768, fp8=True)
case("ln_bwd_fp8-only8-302x384", "vitssl_layernorm_bwd_fp8", b_ln_bwd, "test_layernorm_bwd_fp8_image", ws=True, det=True, rows=302, cols=384,
     fp8=True, gm16=False, cs=False)
case("grad_mask_cast-301x260", "vitssl_grad_mask_cast", b_grad_mask_cast, "_layernorm_case", ws=True, det=True, rows=301, cols=260, p=0.25)
case("grad_mask_cast-min", "vitssl_grad_mask_cast", b_grad_mask_cast, "_layernorm_case", ws=True, det=True, rows=1, cols=4)
case("grad_mask_cast-nocolsum", "vitssl_grad_mask_cast", b_grad_mask_cast, "_layernorm_case", rows=301, cols=260, cs=False)
case("grad_mask_cast_fp8-301x260", "vitssl_grad_mask_cast_fp8", b_grad_mask_cast, "test_layernorm_bwd_fp8_image", ws=True, det=True, rows=301,
     cols=260, p=0.1, fp8=True)

NT_SHAPES = [(1000, 260, 128), (333, 776, 256), (66000, 512, 128), (25216, 768, 64), (50000, 768, 64)]
for _M, _N, _K in NT_SHAPES:
    _mib = 64 + (_M * _N * 8 + _M * _K * 2) // (1 << 20) + 16
    _t = f"{_M}x{_N}x{_K}"
    case(f"nt-bf16-colsum-{_t}", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", ws=True, det=True, mib=_mib, M=_M, N=_N, K=_K,
         epi="bf16", cs=True)
    case(f"nt-dgelu-colsum-{_t}", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", ws=True, det=True, mib=_mib, M=_M, N=_N, K=_K,
         epi="dgelu", cs=True)
    case(f"nt-gelu-drop-{_t}", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", mib=_mib, M=_M, N=_N, K=_K, epi="gelu", p=0.3)
case("nt-bf16-colsum-reserved-66000x512x128", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", ws=True, det=True, reserve=True,
     mib=400, M=66000, N=512, K=128, epi="bf16", cs=True)
case("nt-bf16-colsum-reserved-333x776x256", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", ws=True, det=True, reserve=True,
     M=333, N=776, K=256, epi="bf16", cs=True)
case("nt-bf16-min-1x4x64", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", ws=True, det=True, M=1, N=4, K=64, epi="bf16", cs=True)
case("nt-f32-splitk-130x64x4160", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_splitk_f32", M=130, N=64, K=4160, epi="f32")
case("nt-f32-333x776x256", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", M=333, N=776, K=256, epi="f32")
case("nt-resid-drop-333x776x256", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_epilogues", M=333, N=776, K=256, epi="resid", p=0.3)
for _off, _mask in ((0, True), (1, False), (1, True), (0, False)):
    case(f"nt-embed-off{_off}-mask{int(_mask)}", "vitssl_gemm_bf16_nt", b_gemm_nt, "test_gemm_nt_embed_epilogue", M=3 * 49, N=132, K=192,
         epi="embed", embed=(3, _off, _mask))

for _epi in ("f32", "bf16", "resid"):
    case(f"fp8nt-{_epi}-517x264x1024", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_epilogues", M=517, N=264, K=1024, epi=_epi,
         p=0.25 if _epi == "resid" else 0.0)
case("fp8nt-gelu-image-517x264x1024", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_epilogues", M=517, N=264, K=1024, epi="gelu",
     p=0.25, image=True)
case("fp8nt-gelu-only8-301x136x128", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_epilogues", M=301, N=136, K=128, epi="gelu",
     image=True, out16=False)
case("fp8nt-dgelu-colsum-image-1001x264x128", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_dgelu_with_scaled_image", ws=True, det=True,
     M=1001, N=264, K=128, epi="dgelu", cs=True, image=True)
case("fp8nt-dgelu-colsum-only8-1001x264x128", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_dgelu_with_scaled_image", ws=True, det=True,
     M=1001, N=264, K=128, epi="dgelu", cs=True, image=True, out16=False)
case("fp8nt-bf16-colsum-min-1x8x128", "vitssl_gemm_fp8_nt", b_gemm_fp8_nt, "test_gemm_fp8_dgelu_with_scaled_image", ws=True, det=True,
     M=1, N=8, K=128, epi="bf16", cs=True)

for _M, _N1, _N2 in ((63, 8, 8), (545, 776, 264), (5001, 192, 768), (1, 8, 8)):
    case(f"tn-{_M}x{_N1}x{_N2}", "vitssl_gemm_bf16_tn", b_gemm_tn, "test_gemm_tn", ws=True, det=True, M=_M, N1=_N1, N2=_N2)
for _M, _N1, _N2 in ((301, 16, 16), (4101, 784, 272), (1, 16, 16)):
    case(f"fp8tn-{_M}x{_N1}x{_N2}", "vitssl_gemm_fp8_tn", b_gemm_tn, "test_gemm_fp8_tn_weight_gradient", ws=True, det=True, M=_M, N1=_N1,
         N2=_N2, fp8=True)
TNB = [(192, 584), (192, 192), (200, 768), (768, 192)]
case("tn_batch-4001", "vitssl_gemm_bf16_tn_batch", b_gemm_tn_batch, "test_gemm_tn", ws=True, det=True, M=4001, shapes=TNB)
case("tn_batch-min", "vitssl_gemm_bf16_tn_batch", b_gemm_tn_batch, "test_gemm_tn", ws=True, det=True, ws_zero_ok=True, M=1, shapes=[(8, 8)])
case("tn_batch-reserved-4001", "vitssl_gemm_bf16_tn_batch", b_gemm_tn_batch, "test_gemm_tn", ws=True, det=True, reserve=True, M=4001, shapes=TNB)
TNB8 = [(192, 592), (192, 192), (208, 768), (768, 192)]
case("fp8_tn_batch-4001", "vitssl_gemm_fp8_tn_batch", b_gemm_tn_batch, "test_gemm_fp8_tn_batch_matches_single_launches", ws=True, det=True,
     M=4001, shapes=TNB8, fp8=True)
case("fp8_tn_batch-reserved-4001", "vitssl_gemm_fp8_tn_batch", b_gemm_tn_batch, "test_gemm_fp8_tn_batch_matches_single_launches", ws=True,
     det=True, reserve=True, M=4001, shapes=TNB8, fp8=True)

for _N in (1, 5, 37, 128, 129, 197, 224, 225, 256):
    case(f"attn_fwd-probs-N{_N}", "vitssl_attn_fwd", b_attn_fwd, "_check_fwd_items", det=True, N=_N, B=2, H=3)
    case(f"attn_bwd-N{_N}", "vitssl_attn_bwd", b_attn_bwd, "_check_bwd_items", det=True, N=_N, B=2, H=3)
for _N in (257, 319, 383, 385, 577, 2047):
    case(f"attn_fwd-probs-N{_N}", "vitssl_attn_fwd", b_attn_fwd, "_check_fwd_items", det=True, mib=256, N=_N, B=1, H=2)
    case(f"attn_bwd-N{_N}", "vitssl_attn_bwd", b_attn_bwd, "_check_bwd_items", det=True, mib=128, N=_N, B=1, H=2)
for _N in (37, 197, 256, 319, 2047):
    case(f"attn_fwd-noprobs-N{_N}", "vitssl_attn_fwd", b_attn_fwd, "_check_fwd_items", det=True, N=_N, B=1, H=3, probs=False)
for _N in (5, 129, 197, 256):
    case(f"attn_fwd_fp8-N{_N}", "vitssl_attn_fwd_fp8", b_attn_fwd, "test_attention_fwd_fp8_image", det=True, N=_N, B=2, H=3, fp8=True,
         probs=_N == 197)
    case(f"attn_bwd_fp8-N{_N}", "vitssl_attn_bwd_fp8", b_attn_bwd, "test_attention_bwd_fp8_image", det=True, N=_N, B=2, H=3, fp8=True,
         dq16=_N != 129)

case("patchify-3x3x32x48-p8", "vitssl_patchify_bf16", b_patchify, "test_patch_and_gather_kernels", B=3, Cc=3, H=32, W=48, Pp=8)
case("patchify-min", "vitssl_patchify_bf16", b_patchify, "test_patch_and_gather_kernels", B=1, Cc=1, H=4, W=4, Pp=4)
case("gather_patches-7", "vitssl_gather_patches_f32", b_gather_patches, "test_patch_and_gather_kernels", B=3, Cc=3, H=32, W=48, Pp=8, n_idx=7)
case("gather_patches-min", "vitssl_gather_patches_f32", b_gather_patches, "test_patch_and_gather_kernels", B=1, Cc=1, H=4, W=4, Pp=4, n_idx=1)
case("gather_rows-51x196", "vitssl_gather_rows_bf16", b_gather_rows, "test_patch_and_gather_kernels", rows=51, cols=196, n_idx=7)
case("gather_rows-min", "vitssl_gather_rows_bf16", b_gather_rows, "test_patch_and_gather_kernels", rows=1, cols=4, n_idx=1)
case("scatter_rows-51x196", "vitssl_scatter_rows_f32", b_scatter_rows, "test_patch_and_gather_kernels", rows=51, cols=196, n_src=7)
case("scatter_rows-min", "vitssl_scatter_rows_f32", b_scatter_rows, "test_patch_and_gather_kernels", rows=1, cols=4, n_src=1)
for _sc in (False, True):
    _e = "vitssl_scatter_cls_f32" if _sc else "vitssl_gather_cls_f32"
    case(f"{_e[7:]}-5x17x68", _e, b_cls, "test_patch_and_gather_kernels", B=5, T=17, D=68, scatter=_sc)
    case(f"{_e[7:]}-min", _e, b_cls, "test_patch_and_gather_kernels", B=1, T=1, D=4, scatter=_sc)
for _B, _tok, _off, _mask, _D in ((5, 16, 0, True, 128), (5, 16, 1, False, 128), (3, 49, 1, True, 132), (37, 49, 0, True, 132),
                                  (37, 49, 1, False, 132), (1, 1, 0, False, 4)):
    case(f"embed_bwd-B{_B}-t{_tok}-off{_off}-mask{int(_mask)}-D{_D}", "vitssl_embed_bwd", b_embed_bwd, "test_embed_bwd", ws=True, det=True, B=_B,
         tokens=_tok, tok_offset=_off, use_mask=_mask, D=_D)
for _n in (4, 2048 * 256 * 4 + 4 * 333, 117 * 4):
    case(f"l1_loss-{_n}", "vitssl_l1_loss", b_l1_loss, "test_l1_loss", ws=True, det=True, mib=128, n=_n)
case("l1_loss-nograd-468", "vitssl_l1_loss", b_l1_loss, "test_l1_loss", ws=True, det=True, n=468, grad=False)
case("cross_entropy-33x10", "vitssl_cross_entropy", b_cross_entropy, "test_cross_entropy", B=33, Cn=10)
case("cross_entropy-min", "vitssl_cross_entropy", b_cross_entropy, "test_cross_entropy", B=1, Cn=2)
for _r in (1, 129, 65537):
    case(f"colsum_bf16-{_r}x260", "vitssl_colsum_bf16", b_colsum_bf16, "_layernorm_case (column sum of grad_mask_cast)", ws=True, det=True,
         mib=128, rows=_r, cols=260)
case("colsum_bf16-min", "vitssl_colsum_bf16", b_colsum_bf16, "_layernorm_case (column sum of grad_mask_cast)", ws=True, det=True, rows=1, cols=4)
for _n in (4, 1003, 2048 * 256 * 4 + 7):
    case(f"cast_bf16-{_n}", "vitssl_cast_bf16", b_cast_bf16, "test_casts", mib=128, n=_n)
for _R, _C in ((100, 37), (65, 64), (1, 1), (130, 191)):
    case(f"cast_transpose-{_R}x{_C}", "vitssl_cast_transpose_bf16", b_cast_transpose, "test_casts", R=_R, Cn=_C)
case("cast_transpose-only_t-100x37", "vitssl_cast_transpose_bf16", b_cast_transpose, "test_casts", R=100, Cn=37, plain=False)
case("cast_transpose-only_plain-100x37", "vitssl_cast_transpose_bf16", b_cast_transpose, "test_casts", R=100, Cn=37, transposed=False)
case("cast_transpose_batch", "vitssl_cast_transpose_batch", b_cast_batch, "test_casts", shapes=[(130, 191), (100, 37), (65, 64), (1, 5), (192, 128)])
case("fp8_quantize_weights", "vitssl_fp8_quantize_weights", b_cast_batch, "test_fp8_weight_images_bit_exact",
     shapes=[(130, 191), (100, 37), (65, 64), (1, 5), (192, 128)], fp8=True)
for _n in (4, (1 << 16) + 5):
    case(f"quantize_fp8-{_n}", "vitssl_quantize_fp8", b_quantize_fp8, "test_quantize_fp8_bit_exact", n=_n, scaled=False)
    case(f"quantize_fp8_scaled-{_n}", "vitssl_quantize_fp8_scaled", b_quantize_fp8, "test_quantize_fp8_scaled_and_amax", n=_n, scaled=True)
for _n in (4, 1001):
    case(f"adamw-{_n}", "vitssl_adamw", b_adamw, "test_adamw_matches_torch_golden", n=_n)
    case(f"ema-{_n}", "vitssl_ema", b_ema, "test_ema", n=_n)
for _bwd in (False, True):
    _s = "bwd" if _bwd else "fwd"
    case(f"rownorm_{_s}-83x300", f"vitssl_rownorm_{_s}", b_rownorm, "test_rownorm_fwd_bwd", rows=83, D=300, bwd=_bwd)
    case(f"rownorm_{_s}-min", f"vitssl_rownorm_{_s}", b_rownorm, "test_rownorm_fwd_bwd", rows=1, D=4, bwd=_bwd)
    _e = "vitssl_weightnorm_bwd" if _bwd else "vitssl_weightnorm_fold"
    case(f"{_e[7:]}-1031x300", _e, b_weightnorm, "test_weightnorm_fold_bwd", K=1031, D=300, bwd=_bwd)
    case(f"{_e[7:]}-min", _e, b_weightnorm, "test_weightnorm_fold_bwd", K=1, D=4, bwd=_bwd)
    case(f"bicubic_{_s}-5x7-to-14x14", f"vitssl_bicubic_resize_{_s}", b_bicubic, "test_bicubic_resize_matches_aten_and_oracle", g0=(5, 7),
         g1=(14, 14), D=196, bwd=_bwd)
    case(f"bicubic_{_s}-6x6-to-3x5", f"vitssl_bicubic_resize_{_s}", b_bicubic, "test_bicubic_resize_matches_aten_and_oracle", g0=(6, 6),
         g1=(3, 5), D=4, bwd=_bwd)
for _K in (4100, 4096, 16384):          # generic / register rows / four teacher slices (test_dino_loss_dispatch_branches)
    case(f"dino_loss-K{_K}", "vitssl_dino_loss", b_dino_loss, "test_dino_loss_dispatch_branches", ws=True, det="outs", G=2, V=10, B=3, K=_K)
case("dino_loss-min-K4096", "vitssl_dino_loss", b_dino_loss, "test_dino_loss_dispatch_branches", ws=True, det="outs", G=1, V=1, B=1, K=4096)
case("colsum_f32-83x1032", "vitssl_colsum_f32", b_colsum_f32, "test_colsum_and_center_ema", rows=83, K=1032)
case("colsum_f32-min", "vitssl_colsum_f32", b_colsum_f32, "test_colsum_and_center_ema", rows=1, K=4)
case("center_ema-1032", "vitssl_center_ema", b_center_ema, "test_colsum_and_center_ema", K=1032)
case("center_ema-min", "vitssl_center_ema", b_center_ema, "test_colsum_and_center_ema", K=4)
for _st, _e in (("crop", "vitssl_aug_resized_crop_u8"), ("color", "vitssl_aug_color_u8"), ("blur", "vitssl_aug_blur_to_tensor")):
    case(f"aug_{_st}-160x120-to-96", _e, b_augment, "test_stages_bit_exact_against_oracle", stage=_st, B=3, H=160, W=120, Sz=96, scale=(0.3, 1.0))
    case(f"aug_{_st}-96x96-to-48", _e, b_augment, "test_stages_bit_exact_against_oracle", stage=_st, B=1, H=96, W=96, Sz=48, scale=(0.08, 0.4))

assert len({c.id for c in CASES}) == len(CASES)


# ============================================================================================ the driver
@pytest.fixture
def reserve():
    """as tests/test_gpu_schedules.py::reserve: the count in force before the test is restored afterwards, also on failure"""
    L = _L()
    lib = L.lib()
    old = lib.vitssl_get_reserved_cus()

    def set_(n):
        L.call("vitssl_set_reserved_cus", C.c_int(n))
        assert lib.vitssl_get_reserved_cus() == n
    yield set_
    torch.cuda.synchronize()
    L.call("vitssl_set_reserved_cus", C.c_int(old))
    assert lib.vitssl_get_reserved_cus() == old


def _is_float(t):
    return t.dtype in (F32, BF16, FP8)


def _snapshot(s, with_accs=True):
    ts = list(s.outs.items()) + ([(k, v[0]) for k, v in s.accs.items()] if with_accs else [])
    return {k: Arena.bytes_of(t).clone() for k, t in ts}


def _prepare(s, ws, byte, accs_byte=None):
    for t in list(s.outs.values()) + list(s.scratch) + ([ws] if ws is not None else []):
        Arena.fill(t, byte)
    for t, init in s.accs.values():
        if accs_byte is not None:
            Arena.fill(t, accs_byte)
        elif isinstance(init, torch.Tensor):
            t.copy_(init.view(t.shape))
        else:
            t.fill_(init)


@gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_abi_case(c, reserve):
    L = _L()
    if c.reserve:
        reserve(torch.cuda.get_device_properties(0).multi_processor_count - 8)
    torch.manual_seed(zlib.crc32(c.id.encode()))
    a = Arena(DEV, mib=c.mib)
    s = c.build(a, **c.kw)
    assert (s.ws_floats is not None) == c.ws, "Case.ws out of step with its builder"
    ws = a.empty("workspace", (s.ws_floats,), F32) if c.ws else None
    wsp, wsn = P(ws), (s.ws_floats if c.ws else 0)

    # 1 + 2: exact-size workspace, guards, no NaN left in an output
    _prepare(s, ws, 0xFF)
    s.run(wsp, wsn)
    torch.cuda.synchronize()
    a.check()
    for name, t in list(s.outs.items()) + [(k, v[0]) for k, v in s.accs.items()]:
        if _is_float(t) and name not in s.partial:
            assert not torch.isnan(t.float()).any(), f"{name}: NaN left in an output ({int(torch.isnan(t.float()).sum())} elements)"
    # 3: parity
    s.verify()
    # 4: same bits from zero-filled outputs and workspace
    if c.det:
        first = _snapshot(s, with_accs=c.det is True)
        _prepare(s, ws, 0x00)
        s.run(wsp, wsn)
        torch.cuda.synchronize()
        a.check()
        for k, v in _snapshot(s, with_accs=c.det is True).items():
            if k in s.partial:
                continue
            assert torch.equal(first[k], v), f"{k}: bits depend on what outputs / workspace held before the call"
    # 5: refused before anything is launched
    if c.ws and s.ws_floats == 0:
        assert c.ws_zero_ok, "a workspace case must need a workspace (only one row or a reduced grid makes every tile single-owner)"
    elif c.ws:
        tries = [("one float short", wsp, wsn - 1)]
        if s.null == "refused":
            tries.append(("NULL", C.c_void_p(0), wsn))
        for what, p_, n_ in tries:
            _prepare(s, ws, 0xFF, accs_byte=0xFF)
            with pytest.raises(L.VitsslError, match=s.ws_fn):
                s.run(p_, n_)
            torch.cuda.synchronize()
            a.check()
            for name, t in list(s.outs.items()) + [(k, v[0]) for k, v in s.accs.items()]:
                assert Arena.untouched(t), f"{name} was written by a call that refused its workspace ({what})"
        if s.null == "atomic":         # the documented atomic path of the TN GEMMs: parity only
            _prepare(s, ws, 0xFF)
            s.run(C.c_void_p(0), 0)
            torch.cuda.synchronize()
            a.check()
            s.verify()


# The same body off the default stream (tests/_offstream.py).  Left out: arenas above MAX_ARENA_MIB (the fixture clones the arena
# at every call) and the cases that change the reserved CUs; tests/test_abi_arena.py checks that no entry point loses its last case.
OFF_STREAM_CASES = [c for c in CASES if c.mib <= MAX_ARENA_MIB and not c.reserve]


@gpu
@pytest.mark.parametrize("mode", ["gate", "graph"])
@pytest.mark.parametrize("c", OFF_STREAM_CASES, ids=lambda c: c.id)
def test_abi_case_off_stream(c, mode, reserve, offstream):
    offstream(mode, test_abi_case, c, reserve)


# ============================================================================================ controls
@gpu
def test_control_write_past_output_is_caught():
    """vitssl_cast_bf16 told 301 rows of 64 on a destination carved 300 rows long: the last row lands in the guard behind `dst`
    and check() must say so.  The guard is >= 128 rows of the tensor's row and >= 64 KiB, so the stray 128 bytes stay inside
    the arena's single allocation: nothing outside an allocation is touched and nothing can fault."""
    a = Arena(DEV, mib=8)
    rows, cols = 300, 64
    src = a.put("src", torch.randn(rows + 1, cols))
    dst = a.empty("dst", (rows, cols), BF16)
    assert a.guard_bytes(dst.shape, dst.dtype) >= 128 * cols * 2
    call("vitssl_cast_bf16", P(src), P(dst), (rows + 1) * cols, S())
    torch.cuda.synchronize()
    with pytest.raises(ArenaError, match=r"0 bytes after the end of 'dst'") as e:
        a.check()
    assert f"{cols * 2} guard bytes" in str(e.value)
    assert torch.equal(dst.cpu(), bf(src.cpu()[:rows]))


@gpu
def test_control_read_past_input_is_seen():
    """vitssl_colsum_bf16 told rows + 1 on an input of `rows` rows: the extra row is the NaN guard behind `x` (inside the
    arena's single allocation, guard >= 128 rows), so every column sum must come out NaN; the right row count gives none."""
    a = Arena(DEV, mib=8)
    rows, cols = 129, 64
    x = a.put("x", bf(torch.randn(rows, cols)))
    out = a.zeros("out", (cols,), F32)
    assert a.guard_bytes(x.shape, x.dtype) >= 128 * cols * 2
    n = sum_ws(rows + 1, cols)
    ws = a.empty("workspace", (n,), F32)
    call("vitssl_colsum_bf16", P(x), P(out), rows, cols, P(ws), n, S())
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    out.zero_()
    call("vitssl_colsum_bf16", P(x), P(out), rows + 1, cols, P(ws), n, S())
    torch.cuda.synchronize()
    a.check()
    assert bool(torch.isnan(out).all())
