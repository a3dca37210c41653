"""Geometries of the patch-path tests (include/vitssl_patch.h): (C, P, H, W), chosen for what can go wrong.
Pd = C * P * P: 48 one partial K chunk; 588 nine full chunks + 12; 49 odd; 75 Pd % 4 == 3; 4 the smallest; 28 x 42 rectangular."""
import torch

SQUARE = [(3, 4, 16, 16), (3, 6, 24, 24), (3, 12, 36, 36), (3, 14, 42, 42), (1, 7, 28, 28), (3, 5, 15, 15), (4, 10, 30, 30), (1, 2, 8, 8)]
RECT = [(3, 14, 28, 42)]
NATIVE = [(3, 16, 32, 32), (3, 8, 24, 24)]          # P % 4 == 0 and Pd % 64 == 0: the unchanged path
KERNEL_CASES = SQUARE + RECT + NATIVE


def pd_of(C, P):
    return C * P * P


def padded(pd):
    return (pd + 63) // 64 * 64


def image(B, C, H, W, seed):
    """fp32 image batch with full mantissas (a copy that drops or rounds a value shows)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, H, W, generator=g)


def bits16(x):
    return x.detach().cpu().contiguous().view(torch.int16)
