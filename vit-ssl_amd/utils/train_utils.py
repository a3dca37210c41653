"""Factories that turn the `training:` section of a config into objects.

Same entry points and config keys as the reference (utils/train_utils.py:12-51:
`setup_device`, `make_criterion`, `make_optimizer`, `make_schedulers`; keys `criterion`,
`optimizer`, `lr_scheduler.{main,warmup}`, `warmup_*`), different machinery: every section is
read through `_spec` into a (name, kwargs) pair, and an AdamW request over a model that exposes
its flat parameter store is answered with the fused flat-buffer optimizer kernel instead of
torch.optim.AdamW, and a Lamb request (torch.optim has none) with the fused LAMB over the same store; the optional keys
`training.clip_grad_norm`, `training.no_weight_decay` and `training.layer_decay` reach either fused optimizer as its per-parameter
settings (`_group_options`) and are refused with any other.  `get_transforms` returns callables with the reference's per-image semantics that also carry the
GPU multi-crop recipe (`.view_spec`, see `data.ViewSpec.from_config`) or, for the crop / flip / ToTensor and Resize / ToTensor
lists, the recipe of the fused transform kernel (`.transform_spec`, see `data.TransformSpec.from_config`).
"""
import fnmatch
import logging
import os

import torch
from torch import nn, optim
from torch.optim import lr_scheduler

from ._config import cfg_get
from .schedulers import LinearWarmupScheduler

logger = logging.getLogger(__name__)
_FUSED_ADAMW_KEYS = {"lr", "betas", "eps", "weight_decay"}
_FUSED_LAMB_KEYS = _FUSED_ADAMW_KEYS | {"always_adapt", "trust_clip"}
_LAMB_NAMES = ("Lamb", "LAMB", "lamb")
_GROUP_KEYS = ("clip_grad_norm", "no_weight_decay", "layer_decay")


def _spec(config, *path):
    """(name, kwargs) of a `{name: ..., params: {...}}` config node."""
    node = cfg_get(config, *path)
    return cfg_get(node, "name"), dict(cfg_get(node, "params", default={}) or {})


class _NeedsTorchvision:
    """Stand-in for one transform list on a host without torchvision: carries the GPU recipes (`view_spec`, `transform_spec`), and says what
    is missing when a dataset calls it the way the reference's datasets do (`self.transform(image)`,
    `self.transforms["globals"](image)`: data/datasets.py:36-38,119-123)."""

    def __init__(self, key, sequence, view_spec, transform_spec=None):
        self.key, self.sequence, self.view_spec, self.transform_spec = key, list(sequence), view_spec, transform_spec

    def __call__(self, image):
        from vitssl_hip import VitsslError
        names = ", ".join(str(e["name"]) for e in self.sequence)
        raise VitsslError(
            f"transforms[{self.key!r}] ({names}) was called on the CPU, but torchvision is not installed on this host. "
            "The reference builds these lists from torchvision.transforms (utils/train_utils.py:54-68). Either install "
            "torchvision, or feed uint8 [B,H,W,3] batches and let data.GPUMultiCrop (from this object's .view_spec) or "
            "data.GPUTransform (from its .transform_spec) render them on the GPU (INTEGRATION.md section 4).")

    def __repr__(self):
        return f"_NeedsTorchvision({self.key!r}, view_spec={self.view_spec}, transform_spec={self.transform_spec})"


def _view_spec_or_none(sequence):
    """The GPU multi-crop recipe of a transform list, or None when the list is not a DINO view recipe."""
    from data import ViewSpec
    try:
        return ViewSpec.from_config(sequence)
    except (ValueError, KeyError, TypeError):
        return None


def _transform_spec_or_none(sequence):
    """The fused-kernel recipe of a crop / flip / ToTensor or Resize / ToTensor list, or None for any other list."""
    from data import TransformSpec
    try:
        return TransformSpec.from_config(sequence)
    except (ValueError, KeyError, TypeError):
        return None


def get_transforms(config):
    """`transforms:` section -> {name: callable}, the reference's contract (utils/train_utils.py:54-68: every list becomes
    a torchvision Compose built with getattr(T, name)(**params), which the datasets call per image on the CPU).  Each
    returned callable ALSO carries `.view_spec`: the same list reduced to the numbers `data.GPUMultiCrop` needs to render
    the DINO views for a whole batch on the GPU (None for lists that are not crop / flip / jitter / gray / blur recipes),
    and `.transform_spec`: the numbers `data.GPUTransform` needs (None unless the list is RandomResizedCrop, RandomHorizontalFlip,
    ToTensor or Resize, ToTensor).
    Without torchvision the callables refuse to run with a message naming the GPU route."""
    try:
        from torchvision import transforms as T
    except ImportError:
        T = None
    out = {}
    for key, sequence in dict(cfg_get(config, "transforms") or {}).items():
        sequence = [dict(name=cfg_get(e, "name"), params=dict(cfg_get(e, "params", default={}) or {})) for e in sequence]
        spec, tspec = _view_spec_or_none(sequence), _transform_spec_or_none(sequence)
        if T is None:
            out[key] = _NeedsTorchvision(key, sequence, spec, tspec)
            continue
        pipeline = T.Compose([getattr(T, e["name"])(**e["params"]) for e in sequence])
        pipeline.view_spec = spec
        pipeline.transform_spec = tspec
        out[key] = pipeline
    return out


def init_data_parallel(device=None, backend=None):
    """Join the data-parallel job `torch.distributed.run` started, once: when WORLD_SIZE > 1 and no process group exists yet,
    size RCCL to the CUs the persistent GEMM grids leave free (`engine.configure_collectives`, must precede the
    communicator) and call `init_process_group` (backend "nccl" = RCCL, bound to `device`; VITSSL_DIST_BACKEND overrides,
    e.g. "gloo" for a rehearsal on CPU or on one GPU).  An already initialised group is left alone.  Returns the world size.
    The reference has no multi-GPU path (train.py:107 only calls setup_device()); this is the "DDP added" of SURVEY 8(b):
    with it `BaseTrainer` finds an initialised group and builds its GradReducer."""
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if not dist.is_available():
        if world > 1:
            raise RuntimeError(f"WORLD_SIZE={world} but this torch build has no torch.distributed")
        return 1
    if dist.is_initialized():
        return dist.get_world_size()
    if world <= 1:
        return 1
    backend = backend or os.environ.get("VITSSL_DIST_BACKEND", "nccl")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if "MASTER_PORT" not in os.environ or "RANK" not in os.environ:
        raise RuntimeError(f"WORLD_SIZE={world} but RANK / MASTER_PORT are not set: launch with "
                           "`python -m torch.distributed.run --nproc-per-node N train.py ...` (one process per GPU)")
    kwargs = {}
    if backend == "nccl":
        from vitssl_hip.engine import configure_collectives
        configure_collectives()
        if device is not None:
            kwargs["device_id"] = torch.device(device)
    dist.init_process_group(backend, rank=int(os.environ["RANK"]), world_size=world, **kwargs)
    logger.info("data parallel: rank %d of %d over %s", dist.get_rank(), dist.get_world_size(), backend)
    return dist.get_world_size()


def setup_device():
    """One process per GPU: binds this process to cuda:LOCAL_RANK (torch.distributed.run exports it; 0 when run alone),
    joins the data-parallel job when there is one (`init_data_parallel`: nothing else on the reference's entry path,
    train.py:107-128, would) and returns the device.  The reference returns bare "cuda" or "cpu"
    (utils/train_utils.py:12-16); the engine has no CPU path, so unlike the reference this refuses to hand out 'cpu'.
    VITSSL_SHARE_GPU=1 (rehearsal of N ranks on one card, with VITSSL_DIST_BACKEND=gloo) binds every rank to cuda:0."""
    if not torch.cuda.is_available():
        raise RuntimeError("no GPU visible: this engine runs the vit_core hot path on MI355X only (no CPU fallback)")
    index = int(os.environ.get("LOCAL_RANK", "0") or 0)
    if os.environ.get("VITSSL_SHARE_GPU", "0") not in ("", "0"):
        index = 0
    if not 0 <= index < torch.cuda.device_count():
        raise RuntimeError(f"LOCAL_RANK={index} but {torch.cuda.device_count()} GPU(s) are visible")
    torch.cuda.set_device(index)                            # bind the GPU before RCCL sees the process
    device = torch.device(f"cuda:{index}")
    init_data_parallel(device)
    logger.info("Using device: %s", device)
    return device


def make_criterion(config):
    """`training.criterion: {name, params}`: a criterion of utils.losses (BinaryCrossEntropy), else one of torch.nn."""
    from . import losses
    name, kwargs = _spec(config, "training", "criterion")
    cls = losses.CRITERIA.get(name)
    return (getattr(nn, name) if cls is None else cls)(**kwargs)


def _group_options(config, store):
    """The optional keys beside `training.optimizer` as FusedAdamW's / FusedLamb's keyword arguments ({} when none is present):
    `clip_grad_norm` (> 0), `no_weight_decay` (true, or a list of fnmatch patterns over parameter names) and
    `layer_decay` (0 < d <= 1: lr multiplier d ** (L + 1 - layer_id), see vitssl_hip.engine.layer_id).  `store` is the
    FlatStore whose names they are keyed by, or None when only the presence of the keys is asked for."""
    present = {key: cfg_get(config, "training", key) for key in _GROUP_KEYS}
    present = {key: value for key, value in present.items() if value is not None and value is not False}
    if not present or store is None:
        return present
    from vitssl_hip.engine import exempt_from_weight_decay, layer_id, num_layers
    out = {}
    if "clip_grad_norm" in present:
        clip = float(present["clip_grad_norm"])
        if not clip > 0.0:
            raise ValueError(f"training.clip_grad_norm = {present['clip_grad_norm']!r} must be a positive number")
        out["max_grad_norm"] = clip
    if "no_weight_decay" in present:
        rule = present["no_weight_decay"]
        if rule is True:
            ndim = {name: p.dim() for name, p in zip(store.names, store.params)}
            exempt = {name for name in store.names if exempt_from_weight_decay(name, ndim[name])}
        elif isinstance(rule, str) or not hasattr(rule, "__iter__"):
            raise ValueError(f"training.no_weight_decay = {rule!r} must be true or a list of name patterns")
        else:
            patterns = [str(pattern) for pattern in rule]
            exempt = {name for name in store.names if any(fnmatch.fnmatchcase(name, pattern) for pattern in patterns)}
        _, kwargs = _spec(config, "training", "optimizer")
        decay = float(kwargs.get("weight_decay", 1e-2))        # the default of both fused optimizers
        out["weight_decay_of"] = lambda name: 0.0 if name in exempt else decay
    if "layer_decay" in present:
        d = float(present["layer_decay"])
        if not 0.0 < d <= 1.0:
            raise ValueError(f"training.layer_decay = {present['layer_decay']!r} must satisfy 0 < d <= 1")
        layers = num_layers(store.names)
        out["lr_scale"] = lambda name: d ** (layers + 1 - layer_id(name, layers))
    return out


def make_optimizer(config, model):
    name, kwargs = _spec(config, "training", "optimizer")
    if name == "AdamW" and hasattr(model, "flat_store") and set(kwargs) <= _FUSED_ADAMW_KEYS:
        from vitssl_hip.optim import FusedAdamW
        store = model.trainable_store() if hasattr(model, "trainable_store") else model.flat_store()
        return FusedAdamW(store, **kwargs, **_group_options(config, store))
    if name in _LAMB_NAMES:
        # torch.optim has no Lamb: the fused one is the only one there is, so what it cannot take is refused here
        if not hasattr(model, "flat_store"):
            raise ValueError(f"training.optimizer.name = {name} is the fused LAMB (vitssl_hip.optim.FusedLamb), which steps a model's "
                             f"flat parameter store; {type(model).__name__} has no flat_store()")
        unknown = sorted(set(kwargs) - _FUSED_LAMB_KEYS)
        if unknown:
            raise ValueError(f"training.optimizer.params {unknown} are unknown to the fused LAMB; it takes {sorted(_FUSED_LAMB_KEYS)}")
        from vitssl_hip.optim import FusedLamb
        store = model.trainable_store() if hasattr(model, "trainable_store") else model.flat_store()
        return FusedLamb(store, **kwargs, **_group_options(config, store))
    ignored = _group_options(config, None)
    if ignored:
        raise ValueError(f"training.{' / training.'.join(sorted(ignored))} need the fused AdamW or the fused LAMB (optimizer name AdamW "
                         f"with only {sorted(_FUSED_ADAMW_KEYS)} under params, or Lamb with only {sorted(_FUSED_LAMB_KEYS)}, over a "
                         f"model with a flat store); the optimizer configured here is {name} with params {sorted(kwargs)}")
    return getattr(optim, name)((p for p in model.parameters() if p.requires_grad), **kwargs)


def make_schedulers(config, optimizer, num_epochs, warmup_steps):
    """{"main": per-epoch torch scheduler, "warmup": per-step linear ramp}"""
    train = lambda key: cfg_get(config, "training", key)  # noqa: E731
    main_name, main_kwargs = _spec(config, "training", "lr_scheduler", "main")
    _, ramp_kwargs = _spec(config, "training", "lr_scheduler", "warmup")
    main_kwargs["T_max"] = num_epochs - train("warmup_epochs")           # cosine over the post-warm-up epochs
    ramp = LinearWarmupScheduler(optimizer, warmup_steps=warmup_steps, start_lr=train("warmup_initial_learning_rate"),
                                 target_lr=train("warmup_final_learning_rate"), **ramp_kwargs)
    return {"main": getattr(lr_scheduler, main_name)(optimizer, **main_kwargs), "warmup": ramp}
