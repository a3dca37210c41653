"""No GPU needed: everything that hangs on include/vitssl_mixup.h is exported and bound and every other header's ABI is what
it was, the argument checks of both entry points come before any launch, the fp64 restatement the GPU tests use
(tests/_mixup_ref.py) is torch's own cross entropy with probability targets, the host's draws (data.sample_mix_params) follow
timm's Mixup, and the trainer refuses `training.mixup` without the fused step."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _classify_ref as R
import _mixup_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vitssl_mixup.h")


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip


def _prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(?:int|int64_t)\s+(vitssl_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


# ---------------------------------------------------------------------------------------------- header completeness
def test_mixup_header_is_bound_and_exported(built):
    from vitssl_hip import _lib
    protos = _prototypes()
    sizing = {"vitssl_classify_loss_mix_workspace_floats"}
    launching = {n: a for n, (r, a) in _lib.REGISTRY["mixup"].items() if r is ctypes.c_int}
    assert set(_lib.header_symbols("mixup")) == set(protos) == set(_lib.REGISTRY["mixup"]) == set(launching) | sizing
    assert {n for n, a in protos.items() if re.search(r"void\s*\*\s*stream", a)} == set(launching)
    raw = ctypes.CDLL(built.LIB_PATH)
    lib = built.lib()
    for n in protos:
        assert hasattr(raw, n), f"{n} declared in include/vitssl_mixup.h but not exported"
    for n, args in launching.items():
        assert len(args) == len([a for a in protos[n].split(",") if a.strip()]), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype is ctypes.c_int
    assert lib.vitssl_classify_loss_mix_workspace_floats.restype is ctypes.c_int64
    others = {n for key in _lib.HEADERS if key != "mixup" for n in _lib.header_symbols(key)}
    assert not set(protos) & others                                          # disjoint from every other header ...
    assert set(_lib.header_symbols("classify")) == {"vitssl_classify_loss", "vitssl_classify_loss_workspace_floats"}      # ... which are what they were
    assert lib.vitssl_version() == _lib.ABI_VERSION == 3
    import __graft_entry__ as ge
    assert "mixup.hip" in ge.SOURCES


def test_sizing_and_argument_errors(built):
    """Pointer, geometry, overlap and workspace checks come before any launch: they can be exercised without a GPU."""
    from vitssl_hip import _lib, ops
    lib = built.lib()
    wsf = lib.vitssl_classify_loss_mix_workspace_floats
    for B, C in [(1, 2), (33, 10), (3, 65536), (0, 10), (4, 1), (4, 65537)]:
        assert wsf(B, C) == lib.vitssl_classify_loss_workspace_floats(B, C)
    one = ctypes.c_void_p(256)                                               # never dereferenced: every call below is refused
    far = ctypes.c_void_p(1 << 30)
    fn = lib.vitssl_classify_loss_mix

    def loss(logits=one, labels=one, partner=one, lam=one, B=33, C=10, ld=64, eps=0.1, ign=-100, up=1.0, out=one, dl=one, ld_out=64,
             db=one, pred=one, cnt=one, bad=one, ws=one, wsn=1 << 20):
        return fn(logits, labels, partner, lam, B, C, ld, eps, ign, up, out, dl, ld_out, db, pred, cnt, bad, ws, wsn, None)

    for kw, msg in [(dict(logits=None), b"null pointer"), (dict(partner=None), b"null pointer"), (dict(lam=None), b"null pointer"),
                    (dict(B=0), b"1 <= B"), (dict(C=1), b"2 <= C <= 65536"), (dict(C=100), b"ld >= C"), (dict(ld=62), b"multiple of 4"),
                    (dict(ld_out=32), b"multiple of 64"), (dict(eps=1.5), b"label_smoothing"),
                    (dict(logits=ctypes.c_void_p(260)), b"16-byte aligned"), (dict(partner=ctypes.c_void_p(258)), b"4-byte aligned"),
                    (dict(ws=None), b"vitssl_classify_loss_mix_workspace_floats"),
                    (dict(wsn=wsf(33, 10) - 1), b"vitssl_classify_loss_mix_workspace_floats")]:
        assert loss(**kw) == -1 and msg in lib.vitssl_last_error() and b"classify_loss_mix" in lib.vitssl_last_error(), (kw, lib.vitssl_last_error())

    def mix(x=one, out=far, ip=one, lam=one, B=4, C=3, H=8, W=8):
        return lib.vitssl_mix_batch(x, out, ip, lam, B, C, H, W, None)

    nbytes = 4 * 3 * 8 * 8 * 4
    for kw, msg in [(dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(ip=None), b"null pointer"),
                    (dict(lam=None), b"null pointer"), (dict(B=0), b">= 1"), (dict(C=0), b">= 1"), (dict(H=0), b">= 1"), (dict(W=0), b">= 1"),
                    (dict(C=1 << 11, H=1 << 10, W=1 << 10), b"C * H * W < 2^31"), (dict(x=ctypes.c_void_p(260)), b"16-byte aligned"),
                    (dict(out=ctypes.c_void_p((1 << 30) + 8)), b"16-byte aligned"), (dict(lam=ctypes.c_void_p(258)), b"4-byte aligned"),
                    (dict(out=one), b"overlaps"), (dict(out=ctypes.c_void_p(256 + nbytes - 16)), b"overlaps"),
                    (dict(x=ctypes.c_void_p(256 + nbytes - 16), out=one), b"overlaps")]:
        assert mix(**kw) == -1 and msg in lib.vitssl_last_error() and b"mix_batch" in lib.vitssl_last_error(), (kw, lib.vitssl_last_error())
    x = torch.zeros(4, 3, 8, 8)
    with pytest.raises(_lib.VitsslError, match="CUDA"):                      # no CPU fallback in the wrappers either
        ops.mix_batch(x, torch.zeros_like(x), torch.zeros(4, 6, dtype=torch.int32), torch.ones(4))
    z, y = torch.zeros(4, 64), torch.zeros(4, dtype=torch.int64)
    out = (torch.zeros(2), torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.VitsslError, match="CUDA"):
        ops.classify_loss_mix(z, y, torch.zeros(4, dtype=torch.int32), torch.ones(4), 10, *out)
    with pytest.raises(_lib.VitsslError, match="2 <= C"):
        ops.classify_loss_mix(z, y, torch.zeros(4, dtype=torch.int32), torch.ones(4), 65, *out)


# ---------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("rot", [0, 3])
@pytest.mark.parametrize("B,C,ld", M.LOSS_SHAPES, ids=str)
def test_loss_restatement_is_torch_cross_entropy_with_probability_targets(B, C, ld, rot, eps):
    z, y, partner, lam, _ = M.make_loss_case(B, C, ld, rot=rot)
    ref = M.loss_reference(z, y, partner, lam, C, eps)
    t, valid = M.soft_targets(y, partner, lam, C)
    assert ref["n_valid"] == int(valid.sum()) >= 1 and ref["n_bad"] == 0 and (ref["valid"] == valid).all()
    if B >= 3:
        assert (y == M.IGNORE).any() and (y[partner][y != M.IGNORE] == M.IGNORE).any()      # own and partner labels ignored
        assert y[0] != y[2] and partner[0] == 2 == partner[2] and ref["valid"][0]             # a two-label row (the tie), a row with a == b
        assert ((t[0] > 0).sum() == 2) == (0 < lam[0] < 1) and (rot != 0 or lam[0] == np.float32(0.3))
    zt = torch.from_numpy(z[:, :C].astype(np.float64)[valid]).requires_grad_(True)
    loss = F.cross_entropy(zt, torch.from_numpy(t), label_smoothing=eps)
    loss.backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
    assert np.abs(ref["grad"][valid] - zt.grad.numpy()).max() <= 1e-15       # torch's p - t carries the cancellation, not more
    assert not ref["grad"][~valid].any()
    assert ref["correct"] == int((z[:, :C].argmax(1)[valid] == y[valid]).sum())              # against the row's own label


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,C,ld", M.LOSS_SHAPES, ids=str)
def test_loss_restatement_with_lam_one_is_the_one_label_restatement(B, C, ld, eps):
    z, y, _ = R.make_case(B, C, ld)
    want = R.reference(z, y, C, eps)
    for partner in (np.arange(B, dtype=np.int32), np.zeros(B, np.int32) + (B - 1) // 3 * 3):      # self; one valid row for all
        got = M.loss_reference(z, y, partner, np.ones(B, np.float32), C, eps)
        assert got["loss_sum"] == want["loss_sum"] and got["n_valid"] == want["n_valid"] and got["correct"] == want["correct"]
        assert np.array_equal(got["grad"], want["grad"]) and np.array_equal(got["pred"], want["pred"])


def test_loss_restatement_counts_bad_rows_and_reads_nothing_through_them():
    B, C = 33, 10
    z, y, partner, lam, _ = M.make_loss_case(B, C, 64)
    base = M.loss_reference(z, y, partner, lam, C, 0.1)
    rows = np.flatnonzero(base["valid"])[:5]
    y2, p2, l2 = y.copy(), partner.copy(), lam.copy()
    y2[rows[0]] = C                                                          # also the partner label of whoever mixes with that row
    p2[rows[1]], p2[rows[2]] = -1, B
    l2[rows[3]], l2[rows[4]] = np.nan, 1.5
    got = M.loss_reference(z, y2, p2, l2, C, 0.1)
    hit = set(rows.tolist()) | {i for i in range(B) if p2[i] == rows[0] and 0 <= p2[i] < B}
    assert got["n_bad"] == len(hit) and got["n_valid"] == base["n_valid"] - len(hit & set(np.flatnonzero(base["valid"]).tolist()))
    assert not got["grad"][sorted(hit)].any()


def test_mix_restatement():
    x = M.mix_input(3, 2, 6, 8)
    ip = np.array([[M.BLEND, 2, 0, 0, 0, 0], [M.PASTE, 0, 1, 4, 2, 99], [7, 1, 0, 6, 0, 8]], np.int32)
    lam = np.array([0.25, 0.5, 0.5], np.float32)
    out, bound = M.mix_reference(x, ip, lam)
    assert np.allclose(out[0], 0.25 * x[0].astype(np.float64) + 0.75 * x[2]) and bound[0].all() and not bound[1:].any()
    assert np.array_equal(out[1][:, 1:4, 2:], x[0][:, 1:4, 2:]) and np.array_equal(out[1][:, :1], x[1][:, :1])
    assert np.array_equal(out[1][:, :, :2], x[1][:, :, :2]) and np.array_equal(out[2], x[2])
    for B, _, H, W in M.MIX_SHAPES:
        kinds, seen = set(), set()
        for ip, lam in M.mix_tables(B, H, W):
            kinds |= set(ip[:, 0].tolist())
            seen |= {tuple(r[2:]) for r in ip.tolist() if r[0] == M.PASTE}
            assert (ip[:, 1] == B - 1 - np.arange(B)).all() and not ((ip[:, 0] == M.BLEND) & (lam == 1)).any()
            if B >= 3:
                assert set(ip[:, 0].tolist()) == {0, 1, 2}
        assert kinds == {0, 1, 2} and seen == set(M.boxes(H, W))
        bx = M.boxes(H, W)
        assert any(b[0] >= b[1] for b in bx) and (0, H, 0, W) in bx and any((b[1] - b[0]) * (b[3] - b[2]) == 1 for b in bx)
        assert {b[2] % 4 for b in bx} >= {0, 1, 2, 3} and any(0 < b[3] - b[2] < 4 for b in bx)
        assert any(b[0] == 0 and b[1] < H for b in bx) and any(b[1] == H and b[0] > 0 for b in bx)
        assert any(b[2] == 0 and b[3] < W for b in bx) and any(b[3] == W and b[2] > 0 for b in bx)


# ---------------------------------------------------------------------------------------------- the host's draws
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_sample_mix_params_boxes_and_lam(built):
    from data import MixSpec, sample_mix_params
    H, W, B = 24, 40, 16
    kinds = set()
    for seed in range(40):
        for mode in ("batch", "elem"):
            p = sample_mix_params(MixSpec(mode=mode), B, H, W, _gen(seed))
            assert all(p[k].dtype == np.int32 and p[k].shape == (B,) for k in ("kind", "partner", "y0", "y1", "x0", "x1"))
            assert p["lam"].dtype == np.float32 and ((p["lam"] >= 0) & (p["lam"] <= 1)).all()
            assert (p["partner"] == B - 1 - np.arange(B)).all()
            paste, blend, copy = p["kind"] == 2, p["kind"] == 1, p["kind"] == 0
            assert (paste | blend | copy).all()
            assert (0 <= p["y0"]).all() and (p["y0"] <= p["y1"]).all() and (p["y1"] <= H).all()
            assert (0 <= p["x0"]).all() and (p["x0"] <= p["x1"]).all() and (p["x1"] <= W).all()
            area = (p["y1"] - p["y0"]).astype(np.int64) * (p["x1"] - p["x0"])
            assert (area[paste] > 0).all()
            assert np.array_equal(p["lam"][paste], (1.0 - area[paste].astype(np.float64) / (H * W)).astype(np.float32))
            assert (p["lam"][copy] == 1).all() and (p["lam"][blend] < 1).all()
            if mode == "batch":
                rows = np.stack([p[k] for k in ("kind", "y0", "y1", "x0", "x1")] + [p["lam"].view(np.int32)], 1)
                assert len(np.unique(rows, axis=0)) == 1                     # one distinct parameter row
            else:
                kinds |= set(p["kind"].tolist())
    assert kinds >= {1, 2}
    p = sample_mix_params(MixSpec(mode="elem"), 256, H, W, _gen(3))          # elem: rows i and B-1-i share nothing
    assert len(np.unique(p["lam"])) > 100 and not np.array_equal(p["lam"], p["lam"][::-1])


def test_sample_mix_params_switches(built):
    from data import MixSpec, sample_mix_params
    H, W, B = 24, 40, 64
    for mode in ("batch", "elem"):
        p = sample_mix_params(MixSpec(prob=0.0, mode=mode), B, H, W, _gen(1))
        assert not p["kind"].any() and (p["lam"] == 1).all()                 # prob = 0: all copy, lam 1
        for seed in range(8):
            assert not (sample_mix_params(MixSpec(switch_prob=0.0, mode=mode), B, H, W, _gen(seed))["kind"] == 2).any()
            assert not (sample_mix_params(MixSpec(switch_prob=1.0, mode=mode), B, H, W, _gen(seed))["kind"] == 1).any()
            assert not (sample_mix_params(MixSpec(cutmix_alpha=0.0, mode=mode), B, H, W, _gen(seed))["kind"] == 2).any()
            assert not (sample_mix_params(MixSpec(mixup_alpha=0.0, mode=mode), B, H, W, _gen(seed))["kind"] == 1).any()
        assert not sample_mix_params(MixSpec(mixup_alpha=0.0, cutmix_alpha=0.0, mode=mode), B, H, W, _gen(1))["kind"].any()
    e = sample_mix_params(MixSpec(prob=0.5, mode="elem"), 512, H, W, _gen(5))
    assert 150 < int((e["kind"] == 0).sum()) < 362                           # about half the rows mix
    e = sample_mix_params(MixSpec(mode="elem"), 512, H, W, _gen(5))
    assert 150 < int((e["kind"] == 2).sum()) < 362                           # switch_prob = 0.5


def test_sample_mix_params_follow_the_torch_generator(built):
    from data import MixSpec, sample_mix_params
    spec = MixSpec(mode="elem")
    a, b, c = (sample_mix_params(spec, 32, 24, 40, _gen(s)) for s in (11, 11, 12))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    torch.manual_seed(4)
    d = sample_mix_params(spec, 32, 24, 40)
    torch.manual_seed(4)
    e = sample_mix_params(spec, 32, 24, 40)
    f = sample_mix_params(spec, 32, 24, 40)                                  # the global generator has moved on
    assert all(np.array_equal(d[k], e[k]) for k in d) and any(not np.array_equal(d[k], f[k]) for k in d)
    g = _gen(9)
    state = g.get_state()
    sample_mix_params(spec, 32, 24, 40, g)
    one_draw = g.get_state()
    g.set_state(state)
    torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, generator=g)
    assert torch.equal(one_draw, g.get_state())                              # exactly one int64 is taken from it


def test_mix_spec_from_config(built):
    from data import MixSpec
    assert MixSpec.from_config({}) == MixSpec() == MixSpec(0.8, 1.0, 1.0, 0.5, "batch")
    assert MixSpec.from_config({"mixup_alpha": 0.2, "mode": "elem"}) == MixSpec(mixup_alpha=0.2, mode="elem")
    for bad, msg in [({"alpha": 1.0}, "unknown key"), ({"mode": "pair"}, "mode must be"), ({"prob": 1.5}, r"\[0, 1\]"),
                     ({"mixup_alpha": -1}, ">= 0")]:
        with pytest.raises(ValueError, match=msg):
            MixSpec.from_config(bad)


# ---------------------------------------------------------------------------------------------- trainer
def test_trainer_refuses_mixup_without_the_fused_path(built):
    from test_classify_host import _StubModel, _cfg
    from utils.trainers import SupervisedTrainer
    data = [(torch.rand(4, 4), torch.tensor([0, 1, 2, 0]))]
    for cfg in (_cfg(mixup={"mixup_alpha": 0.8}), _cfg(fused=False, mixup={}), _cfg(fused=True, mixup={"mode": "elem"})):      # the last: SGD
        with pytest.raises(ValueError, match=r"training\.mixup needs .*training\.fused_step"):
            SupervisedTrainer(_StubModel(), "unused", cfg, data, data, "cpu")
    tr = SupervisedTrainer(_StubModel(), "unused", _cfg(fused=True), data, data, "cpu")      # without the key nothing changes
    assert tr.mixup is None
    with pytest.raises(ValueError, match="unknown key"):
        SupervisedTrainer(_StubModel(), "unused", _cfg(fused=True, mixup={"alpha": 1.0}), data, data, "cpu")
