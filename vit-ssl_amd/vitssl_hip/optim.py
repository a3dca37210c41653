"""Flat fused optimizers over the model's flat parameter buffer: FusedAdamW (torch.optim.AdamW semantics; reference builds
AdamW reflectively at utils/train_utils.py:25-29 with configs/base/training.yaml:10-15) and FusedLamb (timm's Lamb
semantics: one trust ratio per parameter).  Both keep their moments as flat buffers beside the store and share, through
FusedOptimizer, the segment-table step, the clip, the param group and the checkpoint layout."""
import torch

from . import ops
from .engine import FlatStore


class FusedOptimizer(torch.optim.Optimizer):
    """What the flat optimizers share: ONE param group over the store's trainable parameters (so the reference's schedulers
    drive its lr), flat exp_avg / exp_avg_sq, the device-resident segment tables (ops.AdamWPlan) keyed by the parameters
    that take part, the step over such a table (grad_sumsq only when clipping, then the subclass's launch), `grad_norm`, and
    state_dict / load_state_dict in torch's per-parameter layout (`step`, `exp_avg`, `exp_avg_sq`).  A subclass supplies
    `_launch_segments`, `step_flat` and `step`."""

    def __init__(self, store: FlatStore, defaults, max_grad_norm, lr_scale, weight_decay_of):
        params = [p for p in store.params if p.requires_grad]
        if max_grad_norm is not None:
            if not float(max_grad_norm) > 0.0:
                raise ValueError(f"max_grad_norm = {max_grad_norm!r} must be positive")
            defaults["max_grad_norm"] = float(max_grad_norm)
        super().__init__(params, defaults)
        self.lr_scale, self.weight_decay_of = lr_scale, weight_decay_of
        self._trainable_names = tuple(n for n, p in zip(store.names, store.params) if p.requires_grad)
        self._index = {n: i for i, n in enumerate(store.names)}
        self._last_plan = None
        self._plans = {}            # (names that take part, group weight decay) -> ops.AdamWPlan
        self._sumsq = None          # sum of squares of the last clipped step's gradient (device) and its gscale
        self._norm_gscale = 1.0
        self.store = store
        self.exp_avg = torch.zeros_like(store.flat)
        self.exp_avg_sq = torch.zeros_like(store.flat)
        self.step_count = 0
        self._all_trainable = len(params) == len(store.params)

    def _hyper(self):
        g = self.param_groups[0]
        return float(g["lr"]), g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]

    @property
    def max_grad_norm(self):
        """The clip's bound, or None: lives in the group dict, so it follows state_dict() / load_state_dict()."""
        return self.param_groups[0].get("max_grad_norm")

    @property
    def grad_norm(self):
        """Pre-clip global norm of the averaged gradient of the last step: a 1-element device tensor (None before the first
        step and without max_grad_norm)."""
        return None if self._sumsq is None else self._sumsq.sqrt() * self._norm_gscale

    def _plan(self, names):
        wd = self.param_groups[0]["weight_decay"]
        last = self._last_plan              # the usual step: the same tuple object and decay as the step before, no hashing
        if last is not None and last[0] is names and last[1] == wd:
            return last[2]
        key = (names, float(wd))
        plan = self._plans.get(key)
        if plan is None:
            st = self.store
            scale = self.lr_scale or (lambda name: 1.0)
            decay = self.weight_decay_of or (lambda name: wd)
            plan = ops.AdamWPlan([(*st.offsets[n], scale(n), decay(n)) for n in names], st.numel, st.flat.device)
            if len(self._plans) >= 8:          # the set changes when a backbone is unfrozen, not every step
                self._plans.clear()
            self._plans[key] = plan
        self._last_plan = (names, wd, plan)
        return plan

    def _launch_segments(self, plan, names, lr, b1, b2, eps, gscale, sumsq, max_norm):
        raise NotImplementedError

    def _step_segments(self, names, gscale):
        """grad_sumsq (when clipping) + the subclass's launch over the parameters `names` of the store"""
        lr, b1, b2, eps, _ = self._hyper()
        self.step_count += 1
        st = self.store
        if names:
            plan = self._plan(names)
            sumsq, max_norm = None, 0.0
            if self.max_grad_norm is not None:
                max_norm = float(self.max_grad_norm)
                sumsq = self._sumsq = ops.grad_sumsq(st.gflat, plan)
                self._norm_gscale = float(gscale)
            self._launch_segments(plan, names, lr, b1, b2, eps, gscale, sumsq, max_norm)
        st.mark_dirty()

    def _step_table(self, gscale, from_flat):
        """torch-style step through the table: gradients that autograd produced as separate tensors are first copied into
        the flat buffer; parameters without a .grad get no table entry"""
        st = self.store
        names, missing = self._trainable_names, False
        if not from_flat:
            for name in names:
                p = st.params[self._index[name]]
                if p.grad is None:
                    missing = True
                    continue
                gslice = st.gview(name)
                if p.grad.data_ptr() != gslice.data_ptr():
                    gslice.copy_(p.grad.reshape(-1))
            if missing:             # a table of its own for the parameters that have a gradient
                names = tuple(n for n in names if st.params[self._index[n]].grad is not None)
        self._step_segments(names, gscale)

    # checkpoint compatibility: torch.optim.AdamW layout (per-parameter state)
    def state_dict(self):
        st = self.store
        state = {}
        trainable = [p for p in self.param_groups[0]["params"]]
        index = {id(p): i for i, p in enumerate(trainable)}
        for name, p in zip(st.names, st.params):
            if id(p) not in index:
                continue
            o, n = st.offsets[name]
            state[index[id(p)]] = {
                "step": torch.tensor(float(self.step_count)),
                "exp_avg": self.exp_avg[o:o + n].view(p.shape).clone(),
                "exp_avg_sq": self.exp_avg_sq[o:o + n].view(p.shape).clone(),
            }
        g = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        g["params"] = list(range(len(trainable)))
        return {"state": state, "param_groups": [g]}

    def load_state_dict(self, sd):
        st = self.store
        trainable = [p for p in self.param_groups[0]["params"]]
        index = {id(p): i for i, p in enumerate(trainable)}
        for k, v in sd["param_groups"][0].items():
            if k != "params":
                self.param_groups[0][k] = v
        for name, p in zip(st.names, st.params):
            i = index.get(id(p))
            if i is None or i not in sd["state"]:
                continue
            o, n = st.offsets[name]
            s = sd["state"][i]
            self.exp_avg[o:o + n].copy_(s["exp_avg"].reshape(-1))
            self.exp_avg_sq[o:o + n].copy_(s["exp_avg_sq"].reshape(-1))
            self.step_count = int(float(s["step"]))


class FusedAdamW(FusedOptimizer):
    """Drop-in for torch.optim.AdamW over a FlatStore.

    * `step_flat(gscale)` -- one kernel over the whole flat buffer; used by the fused
      train step (gradients already live in the flat gradient buffer; `gscale` folds the
      1/world_size of data-parallel averaging).
    * `step()` -- generic torch-style step: gradients that autograd produced as separate
      tensors are first copied into the flat buffer; parameters whose .grad is None are
      skipped, as torch.optim.AdamW does.
    param_groups[0]['lr'] is honoured, so the reference's warm-up / cosine schedulers
    (utils/schedulers.py, torch.optim.lr_scheduler) drive it unchanged.

    Opt-in, keyword only (with all three None every call is what it was):
    * `max_grad_norm` -- clip the global norm of the averaged gradient (torch.nn.utils.clip_grad_norm_'s formula), computed
      and applied on the device with no host read; `grad_norm` then holds the pre-clip norm of the last step as a 1-element
      device tensor (reading it is the caller's synchronisation).  The flat gradient buffer keeps the UNCLIPPED gradient.
    * `lr_scale(name)` -- multiplier of the group's lr for that parameter (layer-wise lr decay);
    * `weight_decay_of(name)` -- that parameter's weight decay (default: the group's).
    param_groups stays ONE group: the multipliers live in the device-resident segment table (ops.AdamWPlan), built once per
    set of parameters that take part, and a step is grad_sumsq (only when clipping) + adamw_segments, also over a store with
    frozen parameters."""

    def __init__(self, store: FlatStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, max_grad_norm=None,
                 lr_scale=None, weight_decay_of=None):
        super().__init__(store, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm, lr_scale, weight_decay_of)

    @property
    def _segmented(self):
        """True when any per-parameter setting or the clip is on (read from the group: a loaded checkpoint may switch the clip on)."""
        return self.lr_scale is not None or self.weight_decay_of is not None or self.max_grad_norm is not None

    def _launch_segments(self, plan, names, lr, b1, b2, eps, gscale, sumsq, max_norm):
        st = self.store
        ops.adamw_segments(st.flat, st.gflat, self.exp_avg, self.exp_avg_sq, plan, lr, b1, b2, eps, self.step_count, gscale, sumsq, max_norm)

    @torch.no_grad()
    def step_flat(self, gscale: float = 1.0):
        if self._segmented:
            return self._step_segments(self._trainable_names, gscale)      # the optimizer's parameters: fixed when it was built
        if not self._all_trainable:
            # frozen parameters in the store: per-parameter launches over the trainable slices.
            # The fused step leaves its gradients in store.gflat only (p.grad stays None).
            return self.step(gscale=gscale, from_flat=True)
        lr, b1, b2, eps, wd = self._hyper()
        self.step_count += 1
        st = self.store
        ops.adamw(st.flat, st.gflat, self.exp_avg, self.exp_avg_sq, lr, b1, b2, eps, wd, self.step_count, gscale)
        st.mark_dirty()

    @torch.no_grad()
    def step(self, closure=None, gscale: float = 1.0, from_flat: bool = False):
        """torch-style step.  `from_flat=True`: the gradients already live in the store's flat
        gradient buffer (fused train_step), so p.grad is not consulted."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._segmented:
            self._step_table(gscale, from_flat)
            return loss
        lr, b1, b2, eps, wd = self._hyper()
        self.step_count += 1
        st = self.store
        trainable = {id(p) for p in self.param_groups[0]["params"]}
        for name, p in zip(st.names, st.params):
            if id(p) not in trainable or (p.grad is None and not from_flat):
                continue
            o, n = st.offsets[name]
            gslice = st.gflat[o:o + n]
            if not from_flat and p.grad.data_ptr() != gslice.data_ptr():
                gslice.copy_(p.grad.reshape(-1))
            ops.adamw(st.flat[o:o + n], gslice, self.exp_avg[o:o + n], self.exp_avg_sq[o:o + n], lr, b1, b2, eps, wd,
                      self.step_count, gscale)
        st.mark_dirty()
        return loss


class FusedLamb(FusedOptimizer):
    """LAMB over a FlatStore, with the surface of FusedAdamW (`step_flat(gscale)`, `step(closure, gscale, from_flat)`,
    `grad_norm`, one param group, torch's checkpoint layout; a FusedAdamW state dict loads).  Semantics are timm's Lamb:
    per parameter, with its lr * lr_scale(name) and its weight decay wd = weight_decay_of(name) (default: the group's),

        r = (m / (1 - b1^step)) / (sqrt(v) / sqrt(1 - b2^step) + eps) + wd * p
        trust = 1 if wd == 0 and not always_adapt, else |p| / |r| (1 when either norm is 0), capped at 1 with trust_clip
        p -= lr * lr_scale * trust * r

    with the 2-norms taken over the whole parameter, on the device (include/vitssl_lamb.h: moment pass, trust ratios, apply
    pass).  A step always goes through the segment table: grad_sumsq only when clipping, then ops.lamb_segments, also over a
    store with frozen parameters.

    Two differences from timm, both about the clip.  It is opt-in here (`max_grad_norm=None`, from `training.clip_grad_norm`),
    where timm's Lamb clips at 1.0 by default; and the coefficient is the project's one formula, clip_grad_norm_'s
    min(1, max_norm / (norm + 1e-6)), where timm divides by max(norm / max_norm, 1) without the 1e-6."""

    def __init__(self, store: FlatStore, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, *, always_adapt=False,
                 trust_clip=False, max_grad_norm=None, lr_scale=None, weight_decay_of=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, always_adapt=bool(always_adapt), trust_clip=bool(trust_clip))
        super().__init__(store, defaults, max_grad_norm, lr_scale, weight_decay_of)
        self._trust = None          # (names, plan) of the last launch

    def _launch_segments(self, plan, names, lr, b1, b2, eps, gscale, sumsq, max_norm):
        st, g = self.store, self.param_groups[0]
        ops.lamb_segments(st.flat, st.gflat, self.exp_avg, self.exp_avg_sq, plan, lr, b1, b2, eps, self.step_count, gscale, sumsq, max_norm,
                          always_adapt=g["always_adapt"], trust_clip=g["trust_clip"])
        self._trust = (names, plan)

    @torch.no_grad()
    def step_flat(self, gscale: float = 1.0):
        self._step_segments(self._trainable_names, gscale)      # the optimizer's parameters: fixed when it was built

    @torch.no_grad()
    def step(self, closure=None, gscale: float = 1.0, from_flat: bool = False):
        """torch-style step.  `from_flat=True`: the gradients already live in the store's flat
        gradient buffer (fused train_step), so p.grad is not consulted."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._step_table(gscale, from_flat)
        return loss

    def trust_ratios(self):
        """{parameter name: trust ratio} of the last step ({} before the first).  For debugging: it copies the ratios to the
        host, which SYNCHRONISES with the device."""
        if self._trust is None:
            return {}
        names, plan = self._trust
        return dict(zip(names, plan.trust.tolist()))
