"""include/vitssl_patch.h without a GPU: the library exports every symbol of the header, the Python table mirrors it, and every
entry point reports argument errors by name before anything is launched (tests/test_cabi_exports.py for the new header)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    import vitssl_hip
    return vitssl_hip.lib()


def test_exports_every_symbol_of_the_patch_header(lib):
    from vitssl_hip import _lib
    syms = _lib.header_symbols("patch")
    assert len(syms) == 5
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), f"{s} declared in include/vitssl_patch.h but not exported"
    assert set(syms) == set(_lib.REGISTRY["patch"]), "Python prototypes out of sync with the header"
    assert not set(syms) & set(_lib.header_symbols()), "vitssl_hip.h keeps its symbol list"
    assert lib.vitssl_version() == _lib.ABI_VERSION == 3


def test_argument_errors_are_reported(lib):
    one = ctypes.c_void_p(256)          # never dereferenced: every check precedes the launch
    null = ctypes.c_void_p(0)
    err = lambda: lib.vitssl_last_error()   # noqa: E731
    cases = [
        ("vitssl_patchify_ld_bf16", (null, one, 1, 3, 42, 42, 14, 640, None), b"null pointer"),
        ("vitssl_patchify_ld_bf16", (one, one, 1, 3, 42, 42, 14, 586, None), b"ld=586 is smaller"),
        ("vitssl_patchify_ld_bf16", (one, one, 1, 1, 28, 28, 7, 49, None), b"ld=49 must be a multiple of 2"),
        ("vitssl_patchify_ld_bf16", (one, one, 1, 3, 42, 40, 14, 640, None), b"image 42x40 not divisible by patch 14"),
        ("vitssl_patchify_ld_bf16", (one, one, 1, 3, 42, 42, 0, 640, None), b"patch size 0"),
        ("vitssl_patchify_ld_bf16", (one, one, 0, 3, 42, 42, 14, 640, None), b"empty image batch"),
        ("vitssl_patchify_ld_bf16", (one, ctypes.c_void_p(258), 1, 3, 42, 42, 14, 640, None), b"4-byte aligned"),
        ("vitssl_patchify_ld_bf16", (one, one, 1, 4, 128, 128, 128, 65536, None), b"must fit the LDS tile"),
        ("vitssl_gather_patches_any_f32", (one, null, one, 4, 3, 42, 42, 14, None), b"null pointer"),
        ("vitssl_gather_patches_any_f32", (one, one, one, 0, 3, 42, 42, 14, None), b"n_idx=0"),
        ("vitssl_gather_patches_any_f32", (one, one, one, 4, 3, 43, 42, 14, None), b"image 43x42 not divisible by patch 14"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, null, one, 128, 0.5, 4, 75, one, 1 << 20, None), b"null pointer"),
        ("vitssl_l1_loss_ld", (one, 74, one, 75, one, one, 128, 0.5, 4, 75, one, 1 << 20, None), b"ld_p=74"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, one, one, 74, 0.5, 4, 75, one, 1 << 20, None), b"ld_d=74 smaller"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, one, one, 77, 0.5, 4, 75, one, 1 << 20, None), b"ld_d=77 must be a multiple of 2"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, one, one, 128, 0.5, 0, 75, one, 1 << 20, None), b"empty problem"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, one, one, 128, 0.5, 4, 75, null, 0, None), b"vitssl_sum_workspace_floats"),
        ("vitssl_l1_loss_ld", (one, 75, one, 75, one, one, 128, 0.5, 4, 75, one, 16, None), b"vitssl_sum_workspace_floats"),
        ("vitssl_accumulate_ld_f32", (null, one, 4, 75, 128, None), b"null pointer"),
        ("vitssl_accumulate_ld_f32", (one, one, 4, 75, 74, None), b"ld=74 smaller than cols=75"),
        ("vitssl_accumulate_ld_f32", (one, one, 4, 0, 74, None), b"empty problem"),
        ("vitssl_cast_transpose_batch_ld", (null, one, 1, 1, None), b"null pointer"),
        ("vitssl_cast_transpose_batch_ld", (one, one, 0, 1, None), b"njobs=0"),
    ]
    for name, args, msg in cases:
        rc = getattr(lib, name)(*args)
        assert rc == -1 and msg in err(), (name, args, rc, err())


def test_patch_geometry_widths():
    from vitssl_hip.engine import PatchGeometry
    for (C, P), (native, pdp, npw) in {(3, 16): (True, 768, 768), (3, 8): (True, 192, 192), (3, 14): (False, 640, 588), (1, 7): (False, 64, 64),
                                       (3, 5): (False, 128, 128), (3, 4): (False, 64, 48), (1, 2): (False, 64, 4), (4, 10): (False, 448, 400),
                                       (64, 1): (False, 64, 64)}.items():
        g = PatchGeometry(C, P)
        assert (g.native, g.Pdp, g.Np) == (native, pdp, npw), (C, P, g.native, g.Pdp, g.Np)


def test_a_patch_beyond_the_lds_tile_is_refused_by_name():
    from vitssl_hip import _lib
    from vitssl_hip.engine import PatchGeometry
    assert PatchGeometry(3, 59).Pdp == 10496 and PatchGeometry(3, 64).native          # 64: the unchanged path, no such limit
    with pytest.raises(_lib.VitsslError, match="patch_size=60"):
        PatchGeometry(3, 60)
