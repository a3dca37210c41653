"""No GPU needed: include/vitssl_attention_hd.h is exported and bound and the ABI of vitssl_hip.h is what it was; the argument
checks of both entry points and of the dispatcher come before any launch; the oracle's bf16 emulation alone passes, for every
(head dim, length) pair of tests/test_gpu_attention_hd.py, the checks that file applies to the kernels; and the per-row checker
fails a flash pipeline with one localised fault, a wrong scale or a non-zero pad column at dh = 32 and dh = 96."""
import ctypes
import os
import re
import sys

import pytest
import torch

import _attn_hd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_attention_hd.h")


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


# ---------------------------------------------------------------------------------------------- header completeness
def test_header_is_bound_and_exported(built):
    from vitssl_hip import _lib, ops
    protos = _prototypes()
    assert set(protos) == {"vitssl_attn_hd_fwd", "vitssl_attn_hd_bwd"}
    table = {n: a for n, (r, a) in _lib.REGISTRY["attention_hd"].items()}
    assert set(_lib.header_symbols("attention_hd")) == set(protos) == set(table)
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for n, args in table.items():
        assert hasattr(raw, n), f"{n} declared in include/vitssl_attention_hd.h but not exported"
        assert re.search(r"void\s*\*\s*stream", protos[n]), n
        assert len(args) == len([a for a in protos[n].split(",") if a.strip()]), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype is ctypes.c_int
    # same argument lists as the dh = 64 entry points
    assert _lib.REGISTRY["attention_hd"]["vitssl_attn_hd_fwd"] == _lib.REGISTRY["hip"]["vitssl_attn_fwd"]
    assert _lib.REGISTRY["attention_hd"]["vitssl_attn_hd_bwd"] == _lib.REGISTRY["hip"]["vitssl_attn_bwd"]
    # the ABI of include/vitssl_hip.h is what it was
    assert not set(protos) & set(_lib.header_symbols()) and not set(protos) & set(_lib.REGISTRY["hip"])
    assert set(_lib.header_symbols()) >= {"vitssl_attn_fwd", "vitssl_attn_bwd"} and lib.vitssl_version() == _lib.ABI_VERSION == 3
    assert callable(ops.attn_hd_fwd) and callable(ops.attn_hd_bwd)
    import __graft_entry__ as ge
    assert "attention_hd.hip" in ge.SOURCES


def test_argument_errors_come_before_any_launch(built):
    lib = built.lib()
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused

    def fwd(qkv=one, out=one, lse=one, probs=None, B=2, N=5, H=3, dh=32):
        return lib.vitssl_attn_hd_fwd(qkv, out, lse, probs, B, N, H, dh, None)

    def bwd(qkv=one, out=one, dout=one, lse=one, dqkv=one, ws=one, B=2, N=5, H=3, dh=32):
        return lib.vitssl_attn_hd_bwd(qkv, out, dout, lse, dqkv, ws, B, N, H, dh, None)

    for fn, name, ptrs in ((fwd, b"attn_hd_fwd", ("qkv", "out", "lse")), (bwd, b"attn_hd_bwd", ("qkv", "out", "dout", "lse", "dqkv"))):
        for p in ptrs:
            assert fn(**{p: None}) == -1 and name in lib.vitssl_last_error() and p.encode() + b" is NULL" in lib.vitssl_last_error()
        for kw, msg in [(dict(B=0), b"B=0"), (dict(N=0), b"N=0"), (dict(H=0), b"H=0"), (dict(N=2049), b"N=2049"), (dict(dh=0), b"dh=0"),
                        (dict(dh=12), b"dh=12"), (dict(dh=136), b"dh=136"), (dict(dh=4), b"dh=4"),
                        (dict(qkv=ctypes.c_void_p(264)), b"qkv must be 16-byte aligned"),
                        (dict(out=ctypes.c_void_p(264)), b"out must be 16-byte aligned")]:
            assert fn(**kw) == -1 and msg in lib.vitssl_last_error(), (name, kw, lib.vitssl_last_error())
    assert bwd(ws=None) == -1 and b"delta_ws is NULL" in lib.vitssl_last_error()
    assert bwd(dqkv=ctypes.c_void_p(264)) == -1 and b"dqkv must be 16-byte aligned" in lib.vitssl_last_error()
    # the dh = 64 entry points still refuse everything else
    assert lib.vitssl_attn_fwd(one, one, one, None, 1, 4, 1, 32, None) == -1 and b"head dim 32 unsupported" in lib.vitssl_last_error()


def test_dispatcher(built):
    from vitssl_hip import _lib, ops
    assert ops.attn_family(64) == (ops.attn_fwd, ops.attn_bwd)
    for dh in range(8, 129, 8):
        if dh != 64:
            assert ops.attn_family(dh) == (ops.attn_hd_fwd, ops.attn_hd_bwd)
    import numpy as np
    assert ops.attn_family(np.int64(32)) == (ops.attn_hd_fwd, ops.attn_hd_bwd) and ops.attn_family(np.int64(64)) == (ops.attn_fwd, ops.attn_bwd)
    for dh in (12, 136, 0, 4, 7, 129, 32.0, None):
        with pytest.raises(_lib.VitsslError, match=r"head dims 8, 16, \.\.\., 128"):
            ops.attn_family(dh)
        with pytest.raises(_lib.VitsslError, match=r"head dims 8, 16, \.\.\., 128"):     # before any tensor is looked at
            ops.attn_fwd_any(None, None, None, 1, 4, 1, dh)
        with pytest.raises(_lib.VitsslError, match=r"head dims 8, 16, \.\.\., 128"):
            ops.attn_bwd_any(None, None, None, None, None, None, 1, 4, 1, dh)


def test_engine_refuses_before_any_launch(built, monkeypatch):
    """EncoderStack.check_tokens: an unsupported head dim, and fp8 operands with a head dim other than 64 (the message names bf16
    operands as the way out), without a GPU"""
    from vitssl_hip import _lib, engine
    st = engine.EncoderStack.__new__(engine.EncoderStack)
    st.D, st.H, st.dh, st.fp8 = 96, 8, 12, False
    with pytest.raises(_lib.VitsslError, match="head dim 12"):
        st.check_tokens(17)
    st.D, st.H, st.dh, st.fp8 = 128, 4, 32, True
    with pytest.raises(_lib.VitsslError, match="bf16"):
        st.check_tokens(17)
    st.fp8 = False
    st.check_tokens(17)
    st.D, st.H, st.dh, st.fp8 = 128, 2, 64, True
    st.check_tokens(17)


# ---------------------------------------------------------------------------------------------- the emulation passes the GPU checks
WHOLE_PAIRS = ([(dh, N) for dh in A.WHOLE_DHS for N in A.WHOLE_NS] + [(64, N) for N in A.CROSS_NS] + [A.POISON] + A.BOUNDS)


@pytest.mark.parametrize("dh,N", WHOLE_PAIRS)
def test_emulation_passes_the_whole_tensor_bars(dh, N):
    (q, k, v, dout, _), ref = A.randn_case(dh, N)
    A.check_whole(A.emu(q, k, v, dout, full=True), ref, f"emulation dh={dh} N={N}", inputs=(q, k, v, dout))


@pytest.mark.parametrize("dh,N", A.LARGE)
def test_emulation_passes_the_large_logit_bars(dh, N):
    from _util import max_abs, rel_l2
    (q, k, v, dout, _), ref = A.randn_case(dh, N, scale=4.0, Bn=2, Hn=2)
    em = A.emu(q, k, v, dout, full=True)
    assert max_abs(em["lse"], ref["lse"]) < 1e-2 and rel_l2(em["out"], ref["out"]) < 2e-2
    assert rel_l2(torch.stack([em[n] for n in ("dq", "dk", "dv")]), torch.stack([ref[n] for n in ("dq", "dk", "dv")])) < 4e-2


ROW_PAIRS = [(dh, N) for dh in A.ROW_DHS for N in A.ROW_NS] + [(64, N) for N in A.CROSS_NS] + A.ROW_LONG


@pytest.mark.parametrize("perm", A.PERMS)
@pytest.mark.parametrize("dh,N", ROW_PAIRS)
def test_emulation_passes_the_row_checker(dh, N, perm):
    case = A.planted_case(dh, N, perm)
    (q, k, v, dout), ref, em, bar, worst = case
    # a bar of 3 x this still means something (a dropped key or row is an error of 0.5 and more).  The worst are dq / dk at dh = 8:
    # |k|^2 has 8 degrees of freedom, a few planted queries are large and their rows nearly saturated
    assert all(0 <= worst[n] < (0.1 if dh == 8 else 5e-2) for n in worst), worst
    if N > 1:
        assert all(worst[n] > 0 for n in worst), worst
    got = dict(em, lse=ref["lse"])
    A.check_rows(got, case, f"emulation dh={dh} N={N} {perm}")            # trivially, with the margin
    A.check_rows(dict(A.flash(q, k, v, dout), lse=ref["lse"]), case, f"flash dh={dh} N={N} {perm}")   # the carrier of the faults below


# ---------------------------------------------------------------------------------------------- negative controls
def positions(N):
    return sorted({i for i in (0, 15, 16, 63, 64, N - 1) if i < N})


@pytest.mark.parametrize("mutation", A.MUTATIONS)
@pytest.mark.parametrize("perm", A.PERMS)
@pytest.mark.parametrize("dh", [32, 96])
def test_one_fault_fails_the_row_checker(dh, perm, mutation):
    N = 129
    (q, k, v, dout), ref, em, bar, _ = A.planted_case(dh, N, perm)
    pm = A.perm_of(perm, N)
    delta = (dout.double() * ref["out"]).sum(-1)[A.ITEM]
    for i in positions(N):
        j = int(pm[i])
        if mutation == "stale_delta" and abs(float(delta[i] - delta[(i + 1) % N])) < 0.5:
            continue                                                      # the neighbour's delta is (nearly) the same: no fault
        bad = A.failures(A.flash(q, k, v, dout, mutation=mutation, i=i, j=j), ref, bar, tensors=("out", "dq", "dv"))
        assert bad, f"{mutation} at row {i}, key {j} passes the checker"
        for n, (err, (b, h, r)) in bad.items():
            assert (b, h) == A.ITEM, (mutation, n, (b, h, r))
            if mutation in ("drop_pair", "key_off_by_one", "stale_delta"):   # found where it was planted
                assert r == (j if n == "dv" else i), (mutation, i, j, n, err, (b, h, r))
        if mutation in ("scale_eighth", "pad_nonzero"):
            break                                                         # these do not depend on (i, j)
