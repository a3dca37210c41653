"""MAE trainer: SimMIMTrainer's epoch loop over an MAEViT (no counterpart in the reference; shaped like its SimMIM trainer so
that configs, loaders, metrics and checkpoints carry over).

With nn.MSELoss(mean) and the fused AdamW or LAMB the whole step runs fused in the HIP engine (MAEViT.train_step: the
mean squared error against the per-patch normalised pixels is include_ext/vitssl_mae.h's loss kernel); any other criterion or
optimizer takes the autograd path through the same kernels.  With `model.norm_pix_loss: true` the targets are normalised
patches, not pixels, so `metrics: [PSNR, SSIM]` is refused; without normalisation they work as for SimMIM."""
import logging

from torch import nn

from .simmim_trainer import SimMIMTrainer

logger = logging.getLogger(__name__)


class MAETrainer(SimMIMTrainer):
    def __init__(self, model, save_path: str, config, train_loader, val_loader, device):
        super().__init__(model, save_path, config, train_loader, val_loader, device)
        if getattr(model, "norm_pix_loss", False) and (self._listed("PSNR") or self._listed("SSIM")):
            raise ValueError("MAETrainer: metrics PSNR / SSIM compare pixels, but with model.norm_pix_loss: true the targets are "
                             "per-patch normalised; drop the metrics or set norm_pix_loss: false")

    def _fused_ok(self):
        return self._is_fused() and isinstance(self.criterion, nn.MSELoss) and self.criterion.reduction == "mean"
