"""Model factory (reference: utils/model_builder.py:11-184).  Same entry points and mode
dispatch; returns the bare module (the reference wraps it in torch.compile, whose
checkpoints carry an ``_orig_mod.`` key prefix -- accepted here on load)."""
import logging
import os

import torch

from vit_core.vit import ViT
from vit_core.ssl.dino.model import DINOViT
from vit_core.ssl.mae.model import MAEViT
from vit_core.ssl.simmim.model import SimMIMViT

from ._config import cfg_get

logger = logging.getLogger(__name__)


_COMPILE_PREFIX = "_orig_mod."                 # key prefix of checkpoints saved from a torch.compile-wrapped model
_SSL_ONLY = ("simmim_head", "mask_token")      # tensors that exist only while pre-training
_MAE_MARK = "decoder_pred.weight"              # a checkpoint that holds it is an MAEViT's (`_place`, mae=True)


def strip_compile_prefix(state_dict):
    return {k.removeprefix(_COMPILE_PREFIX): v for k, v in state_dict.items()}


def _place_mae(key, tensor, target, fits):
    """`_place` for a tensor of an MAEViT checkpoint going into a ViT: the patch projection is the embedder's convolution (the
    unfold order is (c, kh, kw), so the reshape is the same linear map), CLS token and position table carry over, the encoder
    blocks keep their keys; the final norm, the mask token and the decoder exist only while pre-training."""
    conv = "patch_embedding.conv.weight"
    if key == "projection.weight" and conv in target:
        slot = target[conv]
        if tensor.dim() == 2 and tensor.shape[0] == slot.shape[0] and tensor.shape[1] == slot[0].numel():
            return conv, tensor.reshape(slot.shape)
        return None, f"projection {tuple(tensor.shape)} cannot seed the convolution {tuple(slot.shape)}"
    moved = {"projection.bias": "patch_embedding.conv.bias", "cls_token": "patch_embedding.cls_token",
             "pos_embed": "patch_embedding.positional_embedding"}
    if key in moved and moved[key] in target:
        return fits(moved[key], tensor)
    if key == "mask_token" or key.startswith(("norm.", "decoder_")):
        return None, "pre-training-only tensor"
    if key in target:
        return fits(key, tensor)
    return None, "no such parameter in the model"


def _place(key, tensor, target, mae=False):
    """Where a checkpoint tensor goes in a model with state `target`.
    Returns (destination key, tensor) or (None, reason).  `mae`: the checkpoint is an MAEViT's (it holds decoder_pred.weight)
    and the model is not one; every other placement is untouched by it."""
    def fits(dst_key, t):
        if t.shape == target[dst_key].shape:
            return dst_key, t
        return None, f"shape {tuple(t.shape)} != model's {tuple(target[dst_key].shape)} for {dst_key}"

    if mae:
        return _place_mae(key, tensor, target, fits)
    if key in target:
        return fits(key, tensor)
    embedded = f"patch_embedding.{key}"
    if key.startswith("projection.") and embedded in target:           # SimMIM patch projection -> ViT embedder
        return fits(embedded, tensor)
    if key == "positional_embedding" and embedded in target:           # SimMIM table has no CLS row: add a zero one
        slot = target[embedded]
        if tensor.shape[1] + 1 == slot.shape[1] and tensor.shape[2] == slot.shape[2]:
            grown = torch.zeros_like(slot)
            grown[:, 1:] = tensor
            return embedded, grown
        return None, f"positional table {tuple(tensor.shape)} cannot seed {tuple(slot.shape)}"
    if any(tag in key for tag in _SSL_ONLY) or key.startswith(("teacher.", "center")):
        return None, "pre-training-only tensor"
    return None, "no such parameter in the model"


def load_weights(model, checkpoint_path: str):
    """Initialise `model` from a checkpoint written by the reference or by this package
    (reference: utils/model_builder.py:11-89).  Accepts bare state dicts and trainer
    checkpoints, with or without the torch.compile key prefix, and carries SimMIM
    pre-training weights over to the fine-tuning ViT layout (see `_place`)."""
    if not os.path.exists(checkpoint_path):
        raise FileNotFoundError(f"Checkpoint file not found: {checkpoint_path}")
    payload = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    source = strip_compile_prefix(payload.get("model_state_dict", payload))
    target = model.state_dict()
    accepted, skipped = {}, {}
    mae = _MAE_MARK in source and _MAE_MARK not in target      # MAE pre-training weights into another model (see `_place_mae`)
    for key, tensor in source.items():
        dst_key, result = _place(key, tensor, target, mae=mae)
        if dst_key is None:
            skipped[key] = result
        else:
            accepted[dst_key] = result
    missing, unexpected = model.load_state_dict(accepted, strict=False)
    logger.info("loaded %d tensors from %s (%d skipped)", len(accepted), checkpoint_path, len(skipped))
    for key, why in skipped.items():
        logger.info("  skipped %s: %s", key, why)
    if missing:
        logger.warning("parameters left at their initial values: %s", list(missing))
    if unexpected:
        logger.warning("tensors the model did not take: %s", list(unexpected))
    return model


def freeze_backbone(model: ViT):
    """Linear-probe setting of the reference (utils/model_builder.py:92-101): only the
    classification head and the CLS token keep training."""
    frozen = list(model.encoder_blocks.parameters())
    frozen += [p for name, p in model.patch_embedding.named_parameters() if "cls_token" not in name]
    for p in frozen:
        p.requires_grad = False
    logger.info("backbone frozen: %d tensors", len(frozen))


def _resolve_mode(config) -> str:
    mode = cfg_get(config, "training", "type") or cfg_get(config, "eval", "mode")
    if mode is None:
        raise ValueError("Could not determine mode. Set either 'training.type' or 'eval.mode' in config.")
    return mode.lower()


def _make_mae(m, backbone):
    """MAEViT from the backbone keys and the MAE keys under `model` (mask_ratio, decoder_embed_dim, decoder_blocks,
    decoder_heads, decoder_mlp_dim, norm_pix_loss), each optional (absent: MAEViT's own default).  The model takes no dropout
    (absent counts as 0), drop path or LayerScale: it raises ValueError for them."""
    extra = [k for k in ("drop_path_rate", "layer_scale_init") if k in backbone]
    if extra:
        raise ValueError(f"mode 'mae': model.{extra[0]} is not built for MAEViT; remove the key")
    keys = ("mask_ratio", "decoder_embed_dim", "decoder_blocks", "decoder_heads", "decoder_mlp_dim", "norm_pix_loss")
    return MAEViT(**{**backbone, "dropout": backbone["dropout"] or 0.0}, **{k: m(k) for k in keys if m(k) is not None})


def build_model(config):
    """config -> module, by mode (reference: utils/model_builder.py:104-184)."""
    mode = _resolve_mode(config)
    m = lambda key: cfg_get(config, "model", key)  # noqa: E731
    side = cfg_get(config, "data", "img_size")
    backbone = dict(input_shape=(m("in_channels"), side, side), patch_size=m("patch_size"), embed_dim=m("embed_dim"),
                    num_blocks=m("num_blocks"), num_heads=m("num_heads"), mlp_dim=m("mlp_dim"), dropout=m("dropout"))
    rate = cfg_get(config, "model", "drop_path_rate")      # optional: stochastic depth (absent or 0: the models as they always were)
    if rate:
        backbone["drop_path_rate"] = float(rate)
    init = cfg_get(config, "model", "layer_scale_init")    # optional: LayerScale (absent or null: no new parameter, key or launch)
    if init is not None:
        backbone["layer_scale_init"] = init                # (checked by the models: a finite float > 0, else ValueError)
    pool = cfg_get(config, "model", "global_pool")         # optional: cls | avg, what the ViT's head reads (absent: cls)
    if pool is not None and mode not in ("supervised", "finetune"):
        raise ValueError(f"mode '{mode}': model.global_pool belongs to the supervised / finetune ViT; remove the key")
    head = {} if pool is None else {"global_pool": pool}   # (checked by ViT: anything but cls / avg is a ValueError)
    makers = {
        "supervised": lambda: ViT(num_classes=m("num_classes"), **backbone, **head),
        "simmim": lambda: SimMIMViT(mask_ratio=m("mask_ratio"), **backbone),
        "dino": lambda: DINOViT(output_dim=m("output_dim"), center_momentum=m("center_momentum"), **backbone),
        "mae": lambda: _make_mae(m, backbone),
    }
    makers["finetune"], makers["eval_dino"] = makers["supervised"], makers["dino"]
    if mode not in makers:
        raise ValueError(f"Unknown model-building mode: {mode}")
    logger.info("building a %s model", mode)
    model = makers[mode]()
    if mode == "finetune":
        load_weights(model, cfg_get(config, "training", "pretrained_path"))
        if cfg_get(config, "training", "freeze_backbone"):
            freeze_backbone(model)
    elif mode == "eval_dino":
        load_weights(model, os.path.join(cfg_get(config, "eval", "experiment_path"), "best_model.pth"))
    return model
