"""LayerNorm forward / backward (csrc/layernorm.hip), every entry point: each output element and each column sum on its own.

What runs only on a wave's second and later rows: the kernels are grid-stride with one row (PAIR: one row pair) per wave and
request the next row before they reduce the current one -- `fetch(row + row_step)`, the `nxt[]` / `nx[] ngr[] ndy[] nbr[]` operand
copies, the prefetched statistics `nmu nrs nmuB nrsB` and row scales `nsc nscB`, and the column-sum registers that carry from one
visit to the next.  The forward grid is capped at 4096 blocks, so that code needs more than 16384 rows; the backward grid is one
block per CU the library may occupy (two for rows of <= 512 columns), 256 or 512 blocks of four rows on an MI355X.  The reserve of
vitssl_set_reserved_cus (library state read at every launch, as in tests/test_gpu_schedules.py) leaves 8 CUs: 8 or 16 blocks, so
101 / 197 / 202 / 203 rows give every wave 3 to 4 rows with a ragged last trip, and the slot-row workspace (re-queried per call by
ops._ln_bwd) shrinks with it.  One launch per form at the unreduced grid must give the reduced grid's bits.

Backward, bit for bit: the planted cases of tests/_ln_exact.py are exact in fp32 in any order, so g_out, the bf16 / e4m3 operand,
dgamma, dbeta, gm_colsum, dls and amax are compared for equality with an fp64 reference; outputs start as NaN (0x7F bytes for
e4m3), the column-sum targets as planted integers (the sums accumulate).  Forward and a real-valued backward: rows of seven
families (offset >> spread, constant, spread << sqrt(eps), spread >> 1, one massive activation), neighbours always of different
families, each row against fp64 within bounds derived from the any-order summation bound (tests/_ln_exact.py, fwd_bounds /
bwd_ref); the largest observed error / bound ratios are printed (`LN_MARGIN ...`) and recorded in profiles/ln_rows_margins.txt.
Every launch is enqueued on a side stream."""
import ctypes as C

import pytest
import torch

import _ln_exact as X
from _gemm_exact import BF16, F32, FP8, check_exact

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")
_SIDE = []


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


def _side():
    """One side stream for the whole file.  torch hands out its 32 pool streams round-robin, and which hardware queue a later
    test's side stream shares with the null stream follows from its place in that round (the controls of
    tests/test_gpu_offstream.py need a launch on the null stream to overtake a gated side stream): one full round is taken here,
    so every test after this file gets the streams it would get without it."""
    if not _SIDE:
        ring = [torch.cuda.Stream() for _ in range(32)]
        assert len({s.cuda_stream for s in ring}) == 32, "torch's stream pool is no longer a round of 32"
        _SIDE.append(ring[0])
    return _SIDE[0]


def _off_stream(fn):
    """run the launches of fn on a side stream: operands were written on the default stream, so that drains first"""
    torch.cuda.synchronize()
    with torch.cuda.stream(_side()):
        fn()
    _side().synchronize()


def _nan(shape, dtype=F32):
    if dtype == FP8:
        return torch.empty(shape, dtype=torch.uint8, device=DEV).fill_(0x7F).view(FP8)
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


# =============================================================================================== backward, bit for bit
_DEVCASE = {}


def _dev(c):
    key = (c.rows, c.cols)
    if key not in _DEVCASE:
        if len(_DEVCASE) > 8:
            _DEVCASE.clear()
        names = ("x", "mean", "rstd", "gamma", "dy", "g_res", "g", "rowscale", "lsgamma", "branch")
        _DEVCASE[key] = {n: getattr(c, n).to(DEV).contiguous() for n in names}
    return _DEVCASE[key]


def _launch(ops, c, form, o):
    """one launch of `form` with the operands the options select -> {name: device tensor} keyed as _ln_exact.expected"""
    d = _dev(c)
    ln, ls, q8, rws = form.startswith("ln"), form.endswith("_ls"), form.endswith("_fp8"), form.endswith("_rows")
    rows, cols = c.rows, c.cols
    out = {}
    if o["gm"]:
        out["gm"] = _nan((rows, cols), BF16)
    if o["cs"]:
        out["cs"] = c.init["cs"].to(DEV)
    if ln:
        out["g_out"] = _nan((rows, cols))
        out["dgamma"], out["dbeta"] = c.init["dgamma"].to(DEV), c.init["dbeta"].to(DEV)
    if q8:
        out["gm8"] = _nan((rows, cols), FP8)
        out["amax"] = torch.tensor([X.AMAX0], device=DEV)
        scale = torch.tensor([X.QSCALE], device=DEV)
    if ls and o["dls"]:
        out["dls"] = c.init["dls"].to(DEV)
    drop = ops.make_dropout(X.DROP_P, seed=X.DROP_SEED, site=X.DROP_SITE) if o["drop"] else ops.NO_DROP
    kw = {}
    if rws or (ls and o["rows"]):
        kw["rows"] = (d["rowscale"], c.rpg)
    if ls:
        kw["cols"] = d["lsgamma"]
        if o["dls"]:
            kw.update(branch=d["branch"], dls=out["dls"])
    gm, cs = out.get("gm"), out.get("cs")

    def go():
        if ln:
            head = (d["dy"], d["x"], d["mean"], d["rstd"], d["gamma"], d["g_res"] if o["res"] else None, out["g_out"], gm)
            if q8:
                ops.layernorm_bwd_fp8(*head, out["gm8"], scale, out["amax"], out["dgamma"], out["dbeta"], cs, drop)
            else:
                ops.layernorm_bwd(*head, out["dgamma"], out["dbeta"], cs, drop, **kw)
        elif q8:
            ops.grad_mask_cast_fp8(d["g"], gm, out["gm8"], scale, out["amax"], cs, drop)
        else:
            ops.grad_mask_cast(d["g"], gm, cs, drop, **kw)
    _off_stream(go)
    return out


def _check(got, want, what):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k, w in want.items():
        if w.dim() == 2:
            check_exact(got[k], w, f"{what}: {k}")
        else:                                                   # column sums and amax: the bits
            g = got[k].cpu()
            assert torch.equal(g, w), \
                f"{what}: {k} differs at {(g != w).nonzero().flatten()[:8].tolist()}: got {g[g != w][:8].tolist()}, want {w[g != w][:8].tolist()}"


@pytest.mark.parametrize("case", X.sweep_cases(), ids=X.case_id)
def test_backward_sweep_exact(ops, cus, reserve, case):
    """8 CUs: 8 or 16 blocks, every wave sweeps 3 to 4 rows (row pairs), the last trip ragged"""
    form, cols, rows, o = case
    reserve(cus - X.SWEEP_CUS)
    c = X.cached_case(rows, cols)
    _check(_launch(ops, c, form, o), X.expected(c, form, o), X.case_id(case))


@pytest.mark.parametrize("cols", X.WIDTHS)
@pytest.mark.parametrize("form", X.NARROW_FORMS)
def test_backward_few_rows_exact(ops, form, cols):
    """1, 2, 3, 5, 6 rows: idle waves in the LDS reduce, a second block with one or two rows; 2 and 6 rows of 384 columns are PAIR"""
    o = X.options(form)[0]
    for rows in X.SMALL_ROWS:
        c = X.cached_case(rows, cols)
        _check(_launch(ops, c, form, o), X.expected(c, form, o), f"{form} {rows} x {cols}")


@pytest.mark.parametrize("cols", [384, 1280])
@pytest.mark.parametrize("form", X.FORMS)
def test_backward_grid_independent(ops, cus, reserve, form, cols):
    """the same rows on every CU (one row per wave, 26 or 51 slot rows) and on 8 CUs: the reference's bits both times"""
    rows = X.sweep_rows(cols)[0]
    c = X.cached_case(rows, cols)
    o = X.options(form)[0]
    want = X.expected(c, form, o)
    from vitssl_hip import _lib as L
    ws_floats = L.lib().vitssl_layerscale_workspace_floats          # four sums x one slot row per block the grid may hold
    reserve(0)
    assert int(ws_floats(rows, cols)) == 4 * min((rows + 3) // 4, 2 * cus) * cols
    full = _launch(ops, c, form, o)
    _check(full, want, f"{form} {rows} x {cols}, every CU")
    reserve(cus - X.SWEEP_CUS)
    assert int(ws_floats(rows, cols)) == 4 * 2 * X.SWEEP_CUS * cols, "the reserve is not in force"
    swept = _launch(ops, c, form, o)
    for k in want:
        a, b = full[k], swept[k]
        if a.dtype == FP8:
            a, b = a.view(torch.uint8), b.view(torch.uint8)
        assert torch.equal(a, b), f"{form} {rows} x {cols}: {k} depends on the grid"


# =============================================================================================== forward, per row against fp64
FWD_CASES = [(w, X.FWD_ROWS, 1e-5) for w in X.FWD_WIDTHS] + [(384, X.FWD_ROWS, 1e-6)] + [(w, X.FWD_LONG, 1e-5) for w in X.FWD_LONG_WIDTHS]
CHUNK = 4096


def _report(kind, cols, rows, ratios):
    for (fam, name), q in sorted(ratios.items()):
        print(f"LN_MARGIN {kind} cols={cols} rows={rows} family={fam} output={name} ratio={q:.4g}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("cols,rows,eps", FWD_CASES)
def test_forward_rows(ops, cols, rows, eps, fp8):
    x, fam, _ = X.family_rows(rows, cols, seed=cols)
    gamma, beta = X.affine(cols, seed=cols + 1)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y, mean, rstd = _nan((rows, cols), BF16), _nan((rows,)), _nan((rows,))
    y8 = _nan((rows, cols), FP8) if fp8 else None
    if fp8:
        _off_stream(lambda: ops.layernorm_fwd_fp8(xd, gd, bd, y, y8, mean, rstd, eps))
        y8b, mean_b, rstd_b = _nan((rows, cols), FP8), _nan((rows,)), _nan((rows,))
        _off_stream(lambda: ops.layernorm_fwd_fp8(xd, gd, bd, None, y8b, mean_b, rstd_b, eps))     # the e4m3 image alone
        assert torch.equal(y8.view(torch.uint8), y8b.view(torch.uint8)) and torch.equal(mean, mean_b) and torch.equal(rstd, rstd_b)
    else:
        _off_stream(lambda: ops.layernorm_fwd(xd, gd, bd, y, mean, rstd, eps))
    yc, mc, rc = y.cpu(), mean.cpu(), rstd.cpu()
    y8c = y8.cpu() if fp8 else None
    worst = {}
    for r0 in range(0, rows, CHUNK):                              # the fp64 reference in chunks; the check stays per row
        r1 = min(r0 + CHUNK, rows)
        s = slice(r0, r1)
        for k, q in X.fwd_ratios(x[s], gamma, beta, eps, mc[s], rc[s], yc[s], fam[s]).items():
            worst[k] = max(worst.get(k, 0.0), q)
        if fp8:
            bad, share = X.fp8_excluded(x[s], gamma, beta, mc[s], rc[s], y8c[s])
            assert share <= 0.02, f"rows {r0}..{r1}: {share:.3f} of a row's elements left out of the e4m3 comparison"
            assert bad == 0, f"rows {r0}..{r1}: {bad} e4m3 bytes are not the rounding of the launch's own fp32 value"
    _report("fwd_fp8" if fp8 else "fwd", cols, rows, worst)
    assert len(worst) == 18
    over = {k: q for k, q in worst.items() if not q <= 1.0}
    assert not over, over


# =============================================================================================== backward on the same rows
@pytest.mark.parametrize("cols", X.FWD_WIDTHS)
def test_backward_rows(ops, cus, reserve, cols):
    """mean / rstd are the fp32 roundings of the fp64 statistics (the forward kernel is not in the loop); 67 rows on 8 CUs:
    two or three trips, the last one of three rows"""
    rows, eps = X.FWD_ROWS, 1e-5
    x, fam, _ = X.family_rows(rows, cols, seed=cols)
    gamma, beta = X.affine(cols, seed=cols + 1)
    rm, rr, _ = X.fwd_ref(x, gamma, beta, eps)
    mean, rstd = rm.float(), rr.float()
    g = torch.Generator().manual_seed(cols + 5)
    dy = torch.randn(rows, cols, generator=g).to(BF16)
    g_res = torch.randn(rows, cols, generator=g)
    refs, bounds = X.bwd_ref(x, mean, rstd, gamma, dy, g_res)
    reserve(cus - X.SWEEP_CUS)
    g_out, gm = _nan((rows, cols)), _nan((rows, cols), BF16)
    sums = [torch.zeros(cols, device=DEV) for _ in range(3)]
    ins = [t.to(DEV) for t in (dy, x, mean, rstd, gamma, g_res)]
    _off_stream(lambda: ops.layernorm_bwd(*ins, g_out, gm, sums[0], sums[1], sums[2]))
    assert torch.equal(gm, g_out.to(BF16)), "the bf16 operand is not the rounding of g_out"
    q = (g_out.cpu().double() - refs[0]).abs() / bounds[0]
    q[torch.isnan(q)] = float("inf")
    ratios = {(name, "g_out"): float(q[fam == i].max()) for i, name in enumerate(X.FAMILIES)}
    for name, got, ref, b in zip(("dgamma", "dbeta", "gm_colsum"), sums, refs[1:], bounds[1:]):
        qc = (got.cpu().double() - ref).abs() / b
        qc[torch.isnan(qc)] = float("inf")
        ratios[("all", name)] = float(qc.max())
    _report("bwd", cols, rows, ratios)
    over = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not over, over
