"""The launching entry point of include/vitssl_transforms.h on guarded-arena tensors (tests/_arena.py), in the manner of
tests/test_gpu_abi_bounds.py.  Per case of CASES:
  1. one call on exact-size, poisoned (0xFF) arena tensors: rc == 0;
  2. arena.check(): no byte outside a tensor was written; no NaN left in the output (every element was stored);
  3. bit-exact parity with the Pillow-pinned oracle (oracle/augment_oracle.py: resized_crop_u8 + to_tensor) -- the bar of
     tests/test_gpu_transforms.py::test_equals_oracle, named in Case.bar;
  4. a second call on a zero-filled output gives the same bits;
  5. refused calls (null pointer, empty batch, empty shape, a shape beyond the LDS limit) return VITSSL_ERR_ARG, say why
     through vitssl_last_error, and leave the output and every guard byte 0xFF.
tests/test_transforms_host.py (no GPU) checks that every launching entry point of the header has a case here."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from _arena import Arena
from _offstream import offstream, twin_of  # noqa: F401  (offstream is a fixture)
from oracle import augment_oracle as AO

DEV = torch.device("cuda:0")
F32, U8, I32 = torch.float32, torch.uint8, torch.int32
ENTRY = "vitssl_tf_resized_crop_to_tensor"
gpu = pytest.mark.gpu


def _L():
    from vitssl_hip import _lib
    return _lib


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def boxes_for(rng, B, H, W, kind):
    """[B, 5] int32 boxes inside an H x W image: "full" (Resize), "rows" (one-row and one-column boxes first), "random" """
    ip = np.zeros((B, 5), np.int32)
    for b in range(B):
        if kind == "full":
            ip[b] = (0, 0, H, W, 0)
            continue
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        if kind == "rows" and b == 0:
            h = 1
        if kind == "rows" and b == 1:
            w = 1
        ip[b] = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, int(rng.integers(0, 2)))
    return ip


def oracle_batch(imgs, ip, SH, SW):
    return np.stack([AO.to_tensor(AO.resized_crop_u8(imgs[b], int(p[0]), int(p[1]), int(p[2]), int(p[3]), SH, SW, bool(p[4])))
                     for b, p in enumerate(ip)])


class Case:
    def __init__(self, cid, entry, bar, **kw):
        self.id, self.entry, self.bar, self.kw = cid, entry, bar, kw


_BAR = "test_equals_oracle"
CASES = [
    Case("tf-120x160-to-64x48-rows", ENTRY, _BAR, B=3, H=120, W=160, SH=64, SW=48, kind="rows"),          # rectangular both ways
    Case("tf-32x32-to-224x224", ENTRY, _BAR, B=2, H=32, W=32, SH=224, SW=224, kind="random"),             # upscaling, 32-row tiles
    Case("tf-300x250-to-96x96", ENTRY, _BAR, B=2, H=300, W=250, SH=96, SW=96, kind="random"),             # downscaling, wide taps
    Case("tf-96x96-to-192x192-resize", ENTRY, _BAR, B=2, H=96, W=96, SH=192, SW=192, kind="full"),        # Resize
    Case("tf-40x30-to-7x5-vec1-stores", ENTRY, _BAR, B=2, H=40, W=30, SH=7, SW=5, kind="random"),       # SW % 4 != 0, ragged tile
    Case("tf-1x1-to-1x1", ENTRY, _BAR, B=1, H=1, W=1, SH=1, SW=1, kind="full"),                           # the smallest call
]
assert len({c.id for c in CASES}) == len(CASES)


@gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_transforms_abi_case(c):
    L = _L()
    lib = L.lib()
    k = c.kw
    B, H, W, SH, SW = k["B"], k["H"], k["W"], k["SH"], k["SW"]
    rng = np.random.default_rng(zlib.crc32(c.id.encode()))
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    ip = boxes_for(rng, B, H, W, k["kind"])
    a = Arena(DEV, mib=16)
    src, ipd = a.put("src", torch.from_numpy(imgs)), a.put("iparams", torch.from_numpy(ip))
    out = a.empty("out", (B, 3, SH, SW), F32)
    fn = lib.vitssl_tf_resized_crop_to_tensor

    def run():
        L.call(ENTRY, P(src), P(ipd), P(out), B, H, W, SH, SW, S())
        torch.cuda.synchronize()
        a.check()

    # 1 + 2
    assert Arena.untouched(out)
    run()
    assert not torch.isnan(out).any(), f"{int(torch.isnan(out).sum())} output elements were never stored"
    # 3
    want = torch.from_numpy(oracle_batch(imgs, ip, SH, SW))
    first = out.cpu()
    assert torch.equal(first, want)
    assert torch.equal(src.cpu(), torch.from_numpy(imgs)) and torch.equal(ipd.cpu(), torch.from_numpy(ip))     # inputs are inputs
    # 4
    Arena.fill(out, 0)
    run()
    assert torch.equal(Arena.bytes_of(out).cpu(), Arena.bytes_of(first)), "bits depend on what the output held before the call"
    # 5
    Arena.fill(out)
    refused = [((P(None), P(ipd), P(out), B, H, W, SH, SW), b"null pointer"), ((P(src), P(None), P(out), B, H, W, SH, SW), b"null pointer"),
               ((P(src), P(ipd), P(None), B, H, W, SH, SW), b"null pointer"), ((P(src), P(ipd), P(out), 0, H, W, SH, SW), b"empty batch"),
               ((P(src), P(ipd), P(out), B, 0, W, SH, SW), b"bad shape"), ((P(src), P(ipd), P(out), B, H, W, SH, 0), b"bad shape"),
               ((P(src), P(ipd), P(out), B, 50000, 8, 512, 512), b"the limit is 65536"),
               ((P(src), P(ipd), P(out), B, 166, 8, 2, 8355968), b"the limit is 65536"),      # 2^32 + 928 bytes of LDS
               ((P(src), P(ipd), P(out), B, 96, 4096, 96, 32), b"more than 127x")]
    for args, msg in refused:
        assert fn(*args, S()) == -1 and msg in lib.vitssl_last_error(), (msg, lib.vitssl_last_error())
    with pytest.raises(L.VitsslError, match="null pointer"):
        L.call(ENTRY, P(None), P(ipd), P(out), B, H, W, SH, SW, S())
    torch.cuda.synchronize()
    a.check()
    assert Arena.untouched(out), "a refused call wrote to its output"


# ============================================================================================ off the default stream (tests/_offstream.py)
@twin_of(test_transforms_abi_case)
def test_transforms_abi_case_off_stream(c, mode, offstream):
    offstream(mode, test_transforms_abi_case, c)
