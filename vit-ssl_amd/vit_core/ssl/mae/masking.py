"""MAE random masking (He et al., "Masked Autoencoders Are Scalable Vision Learners", section 3 and the per-sample shuffle of
its published code): one uniform noise value per patch, patches sorted by noise, the first K of the shuffle kept.

Like SimMIM's `draw_mask` the draw stays on the host: `torch.rand(B, N)` from the default CPU generator (so torch.manual_seed
makes runs reproducible) and two argsorts; only the int32 index tables are uploaded.  The token work (gather of the kept
patches, assembly, un-shuffle) runs in HIP (include_ext/vitssl_mae.h)."""
import numpy as np
import torch


def num_kept(num_patches: int, mask_ratio: float) -> int:
    """K = int(N * (1 - mask_ratio)), the paper's len_keep"""
    return int(num_patches * (1 - mask_ratio))


def shuffle_tables(noise: torch.Tensor, K: int):
    """noise f32 [B, N] -> (keep int64 [B, K]: the kept patch indices in shuffle order, restore int64 [B, N]: position of patch
    n in the shuffle; < K means kept)"""
    shuffle = torch.argsort(noise, dim=1)
    return shuffle[:, :K], torch.argsort(shuffle, dim=1)


def draw_keep(batch_size: int, num_patches: int, K: int, generator=None):
    """One draw of the step's masking: (keep [B, K], restore [B, N]), int64 on the CPU."""
    return shuffle_tables(torch.rand(batch_size, num_patches, generator=generator), K)


def restore_from_keep(keep: torch.Tensor, num_patches: int) -> torch.Tensor:
    """restore [B, N] of a given keep table [B, K] (distinct indices per row): kept patch keep[b, j] sits at position j, the
    masked ones follow in ascending patch order."""
    keep_np = np.asarray(keep, dtype=np.int64)
    B, K = keep_np.shape
    if K < 1 or K > num_patches - 1 or keep_np.min() < 0 or keep_np.max() >= num_patches:
        raise ValueError(f"keep must be [B, K] with 1 <= K <= N-1 = {num_patches - 1} and indices in [0, {num_patches}), got shape {keep_np.shape}")
    restore = np.full((B, num_patches), -1, dtype=np.int64)
    rows = np.arange(B)[:, None]
    restore[rows, keep_np] = np.arange(K)[None, :]
    masked = restore < 0
    if int(masked.sum()) != B * (num_patches - K):
        raise ValueError("keep holds a patch index twice in one row")
    restore[masked] = (K + np.cumsum(masked, axis=1) - 1)[masked]
    return torch.from_numpy(restore)


def bool_mask(restore: torch.Tensor, K: int) -> torch.Tensor:
    """mask[b, n] = patch n of image b is masked"""
    return restore >= K


class MAEIndices:
    """The int32 tables one step uploads, as NumPy arrays (single-threaded on purpose, as SimMIM's `mask_indices_np`):
      keep [B*K]        kept patch indices in shuffle order            restore [B*N]   position of patch n in the shuffle
      keep_rows [B*K]   the kept patches as rows b * N + n of the patch matrix
      midx [Mm]         the masked patches as rows b * N + n, ascending: the order of pred / targets (SimMIM's order)
      mrows [Mm]        the same patches as rows b * (N+1) + 1 + n of the decoder's token matrix
      inv [B*(N+1)]     decoder row -> its row of pred, or -1"""
    NAMES = ("keep", "restore", "keep_rows", "midx", "mrows", "inv")

    def __init__(self, keep, restore, K: int):
        keep = np.ascontiguousarray(np.asarray(keep, dtype=np.int64))
        restore = np.ascontiguousarray(np.asarray(restore, dtype=np.int64))
        B, N = restore.shape
        if keep.shape != (B, K) or not 1 <= K <= N - 1:
            raise ValueError(f"keep {keep.shape} / restore {restore.shape} do not fit K = {K}")
        self.B, self.N, self.K, self.Mm = B, N, K, B * (N - K)
        flat = (restore >= K).reshape(-1)
        if int(flat.sum()) != self.Mm or not np.array_equal(np.take_along_axis(restore, keep, 1), np.broadcast_to(np.arange(K), (B, K))):
            raise ValueError("keep / restore are not the two halves of one shuffle")
        self.keep = keep.reshape(-1).astype(np.int32)
        self.restore = restore.reshape(-1).astype(np.int32)
        self.keep_rows = (keep + np.arange(B, dtype=np.int64)[:, None] * N).reshape(-1).astype(np.int32)
        midx = np.flatnonzero(flat)
        self.midx = midx.astype(np.int32)
        self.mrows = (midx + midx // N + 1).astype(np.int32)          # b * N + n -> b * (N + 1) + 1 + n
        inv = np.full(B * (N + 1), -1, dtype=np.int32)
        inv[self.mrows] = np.arange(self.Mm, dtype=np.int32)
        self.inv = inv

    def tables(self):
        return [getattr(self, n) for n in self.NAMES]
