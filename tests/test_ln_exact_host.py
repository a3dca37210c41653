"""The builders of tests/_ln_exact.py, proved on the CPU: the planted backward cases are exact in every output type, an fp32
restatement of the kernel's formula reproduces the fp64 reference bit for bit whatever the column order and whether products are
rounded or fused, and every planted fault moves at least one output element of every case that can express it.  For the
real-valued rows: the derived bounds admit a faithful fp32 restatement of the forward, reject three wrong ones, and leave at most
2 % of a row's elements out of the e4m3 comparison."""
import numpy as np
import pytest
import torch

import _ln_exact as X


def _width_form_rows():
    seen, out = set(), []
    for form, cols, rows, _ in X.sweep_cases():
        if (form, cols, rows) not in seen:
            seen.add((form, cols, rows))
            out.append((form, cols, rows))
    return out


SWEEPS = _width_form_rows()


@pytest.mark.parametrize("cols", X.WIDTHS)
def test_widths_divide_exactly(cols):
    X.check_width(cols)


def test_refused_widths():
    for cols in (28, 52, 56):
        with pytest.raises(AssertionError):
            X.check_width(cols)


def test_sweep_geometry():
    """on the reserved grid every wave takes 3 to 4 rows and the last trip is ragged; the small counts leave waves and blocks idle"""
    for form, cols, rows in SWEEPS:
        pair, grid = X.launch_plan(form, rows, cols, X.SWEEP_CUS)
        assert pair == (cols == 384 and rows % 2 == 0 and form in ("ln", "ln_rows", "ln_ls"))
        assert grid == (8 if pair or cols > 512 else 16), (form, cols, rows, grid)
        krows = rows // 2 if pair else rows
        assert X.sweeps(form, rows, cols, X.SWEEP_CUS) == 4 and 0 < krows % (4 * grid) < 4 * grid, (form, cols, rows)
        assert X.launch_plan(form, rows, cols, 256)[1] == (krows + 3) // 4          # unreduced: one row per wave


@pytest.mark.parametrize("case", X.sweep_cases(), ids=X.case_id)
def test_reference_is_exact_and_restated(case):
    """`expected` asserts representability itself; the restatement at the launch's layout gives its bits"""
    form, cols, rows, o = case
    c = X.cached_case(rows, cols)
    want = X.expected(c, form, o)
    assert X.same_bits(want, X.restate(c, form, o, cus=X.SWEEP_CUS)) == []
    assert set(want) == set(X.restate(c, form, o, cus=X.SWEEP_CUS))


@pytest.mark.parametrize("form,cols,rows", SWEEPS, ids=lambda v: str(v))
def test_any_order_any_contraction(form, cols, rows):
    c = X.cached_case(rows, cols)
    o = X.options(form)[0]
    want = X.expected(c, form, o)
    rng = np.random.default_rng(cols + rows)
    for k in range(3):
        order = rng.permutation(cols)
        for fma in (False, True):
            for cus in (X.SWEEP_CUS, 256):
                assert X.same_bits(want, X.restate(c, form, o, cus=cus, order=order, fma=fma)) == [], (k, fma, cus)


@pytest.mark.parametrize("cols", X.WIDTHS)
@pytest.mark.parametrize("form", X.NARROW_FORMS)
def test_small_row_counts(form, cols):
    for rows in X.SMALL_ROWS:
        c = X.cached_case(rows, cols)
        o = X.options(form)[0]
        want = X.expected(c, form, o)
        assert X.same_bits(want, X.restate(c, form, o, cus=X.SWEEP_CUS)) == [], rows
        pair, grid = X.launch_plan(form, rows, cols, X.SWEEP_CUS)
        for fault in X.FAULTS:
            if X.fault_applies(fault, c, form, o, pair, grid):
                assert X.same_bits(want, X.restate(c, form, o, cus=X.SWEEP_CUS, fault=fault)) != [], (rows, fault)


@pytest.mark.parametrize("form,cols,rows", SWEEPS, ids=lambda v: str(v))
def test_planted_faults_move_an_output(form, cols, rows):
    c = X.cached_case(rows, cols)
    tried = set()
    for o in X.options(form, "matrix" if cols in X.FULL_WIDTHS else "all"):
        want = X.expected(c, form, o)
        pair, grid = X.launch_plan(form, rows, cols, X.SWEEP_CUS)
        for fault in X.FAULTS:
            if X.fault_applies(fault, c, form, o, pair, grid):
                tried.add(fault)
                assert X.same_bits(want, X.restate(c, form, o, cus=X.SWEEP_CUS, fault=fault)) != [], (fault, X.opt_id(o))
    # every fault the form can express at all was expressed by this case
    ln, ls, rws = form.startswith("ln"), form.endswith("_ls"), form.endswith("_rows")
    must = {"slot_dropped"}
    if ln:
        must.add("neigh_stats")
    if ln and (ls or rws):
        must.add("scale_g_out")
    if ls:
        must.add("dls_scaled")
    if cols == 384:
        must.add("stride_768")
        if rows % 2 == 0 and form in ("ln", "ln_rows", "ln_ls"):
            must |= {"pair_swap", "m1_other", "drop_pair_row"}
    assert must <= tried, (must - tried)


# =============================================================================================== real-valued rows
def _fwd_case(cols, eps=1e-5):
    x, fam, _ = X.family_rows(X.FWD_ROWS, cols, seed=cols)
    gamma, beta = X.affine(cols, seed=cols + 1)
    return x, fam, gamma, beta, eps


@pytest.mark.parametrize("cols", X.FWD_WIDTHS)
def test_bounds_admit_the_faithful_restatement(cols):
    x, fam, gamma, beta, eps = _fwd_case(cols)
    assert bool((gamma == 0).any()) and bool((beta != 0).all())
    mean, rstd, y = X.fwd_restate(x, gamma, beta, eps)
    ratios = X.fwd_ratios(x, gamma, beta, eps, mean, rstd, y, fam)
    assert len(ratios) == 18 and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("cols", X.FWD_WIDTHS)
@pytest.mark.parametrize("wrong,families", [("one_pass", "bc"), ("prev_row", "abcefg"), ("no_eps", "de")])
def test_bounds_bite(cols, wrong, families):
    """each wrong restatement breaks the bounds in at least one of the families expected to show it"""
    x, fam, gamma, beta, eps = _fwd_case(cols)
    mean, rstd, y = X.fwd_restate(x, gamma, beta, eps, wrong=wrong)
    broken = set()
    try:
        ratios = X.fwd_ratios(x, gamma, beta, eps, mean, rstd, y, fam)
    except AssertionError:
        broken.add("d")                                           # the bit-exact checks of the constant rows
        keep = fam != 3
        ratios = X.fwd_ratios(x[keep], gamma, beta, eps, mean[keep], rstd[keep], y[keep], fam[keep])
    broken |= {f for (f, _), q in ratios.items() if not q <= 1.0}
    assert broken & set(families), (wrong, broken, ratios)


@pytest.mark.parametrize("cols", X.FWD_WIDTHS)
def test_e4m3_exclusion_cap(cols):
    """the reference alone: at most 2 % of a row's elements sit within their bound of an e4m3 rounding boundary"""
    x, fam, gamma, beta, eps = _fwd_case(cols)
    mean, rstd, _ = X.fwd_restate(x, gamma, beta, eps)
    _, share = X.fp8_excluded(x, gamma, beta, mean, rstd, None)
    assert share <= 0.02, share
    # and the restated fp32 value, rounded once, passes the comparison it defines
    o = (x.numpy() - mean.numpy()[:, None]) * rstd.numpy()[:, None] * gamma.numpy()[None, :] + beta.numpy()[None, :]
    y8 = torch.from_numpy(o.astype(np.float32)).clamp(-448, 448).to(torch.float8_e4m3fn)
    bad, _ = X.fp8_excluded(x, gamma, beta, mean, rstd, y8)
    assert bad == 0


@pytest.mark.parametrize("cols", X.FWD_WIDTHS)
def test_backward_bounds_admit_fp32(cols):
    """the backward formula evaluated in fp32 (NumPy's pairwise sums) stays inside the derived bounds"""
    x, fam, gamma, beta, eps = _fwd_case(cols)
    rm, rr, _ = X.fwd_ref(x, gamma, beta, eps)
    mean, rstd = rm.float(), rr.float()
    g = torch.Generator().manual_seed(cols + 5)
    dy = torch.randn(X.FWD_ROWS, cols, generator=g).to(torch.bfloat16)
    g_res = torch.randn(X.FWD_ROWS, cols, generator=g)
    refs, bounds = X.bwd_ref(x, mean, rstd, gamma, dy, g_res)
    f = np.float32
    xh = (x.numpy() - mean.numpy()[:, None]) * rstd.numpy()[:, None]
    dyg = dy.float().numpy() * gamma.numpy()[None, :]
    inv = f(1) / f(cols)
    m1, m2 = dyg.sum(1, dtype=f) * inv, (dyg * xh).sum(1, dtype=f) * inv
    g_out = (dyg - m1[:, None] - xh * m2[:, None]) * rstd.numpy()[:, None] + g_res.numpy()
    got = (g_out, (dy.float().numpy() * xh).sum(0, dtype=f), dy.float().numpy().sum(0, dtype=f), g_out.sum(0, dtype=f))
    for name, a, r, b in zip(("g_out", "dgamma", "dbeta", "cs"), got, refs, bounds):
        q = float(((torch.from_numpy(a).double() - r).abs() / b).max())
        assert q <= 1.0, (name, q)
    # a neighbour's statistics break them
    xh2 = (x.numpy() - np.roll(mean.numpy(), 1)[:, None]) * np.roll(rstd.numpy(), 1)[:, None]
    q = float(((torch.from_numpy((dy.float().numpy() * xh2).sum(0, dtype=f)).double() - refs[1]).abs() / bounds[1]).max())
    assert q > 1.0
