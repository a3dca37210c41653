"""Plain-torch CPU restatement of the LAMB step of include/vitssl_lamb.h (timm's Lamb; timm is not a dependency, so the
formulas of the header are the specification), shared by the LAMB tests.  The store layout, the case generator and the
gradient scales are those of the segmented-AdamW tests (tests/_optim_cases.py).

Per tensor with its (lr_scale, wd), in float32 or float64:
    gr = g * (gscale * coef);  m = b1 m + (1 - b1) gr;  v = b2 v + (1 - b2) gr^2
    r  = (m / (1 - b1^step)) / (sqrt(v) / sqrt(1 - b2^step) + eps) + wd * p
    trust = 1 if wd == 0 and not always_adapt, else |p| / |r| when both norms are positive, else 1; min(., 1) with trust_clip
    p -= lr * lr_scale * trust * r
"""
import math

import torch

from _optim_cases import BAR_FLOOR, BETAS, COMMON, GRAD_SCALES, LR, MAX_NORM, STEPS, Layout, make_case  # noqa: F401

EPS = 1e-6                                # FusedLamb's default
# the wrong optimizers test_lamb_host.py proves the bar against
VARIANTS = (None, "trust_one", "store_norms", "no_decay_in_update")


def clip_coef(grads, gscale, max_norm, dtype):
    """(coefficient of torch.nn.utils.clip_grad_norm_ over the averaged gradient g * gscale, its pre-clip norm); (1, None)
    without max_norm"""
    if max_norm is None:
        return 1.0, None
    norm = math.sqrt(sum(float(((g.to(dtype) * gscale) ** 2).sum()) for g in grads))
    if dtype == torch.float32:
        norm = float(torch.tensor(norm, dtype=torch.float32))
    return min(1.0, max_norm / (norm + 1e-6)), norm


class LambRef:
    """State of one run: `params` (list of tensors, copied into `dtype`), `rows` = (lr_scale, wd) per tensor."""

    def __init__(self, params, rows, dtype, lr=LR, betas=BETAS, eps=EPS, always_adapt=False, trust_clip=False, variant=None):
        assert dtype in (torch.float32, torch.float64) and variant in VARIANTS
        self.p = [x.detach().to(dtype).clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.rows = [(float(s), float(w)) for s, w in rows]
        self.dtype, self.lr, self.betas, self.eps = dtype, lr, betas, eps
        self.always_adapt, self.trust_clip, self.variant = always_adapt, trust_clip, variant
        self.steps, self.trust = 0, [1.0] * len(self.p)

    def _ratio(self, pn, rn):
        t = pn / rn if pn > 0.0 and rn > 0.0 else 1.0
        return min(t, 1.0) if self.trust_clip else t

    def step(self, grads, gscale=1.0, coef=1.0):
        """one step with the gradients `grads` (one per tensor) scaled by gscale * coef; returns the trust ratios"""
        b1, b2 = self.betas
        self.steps += 1
        bc1, bc2_sqrt = 1.0 - b1 ** self.steps, math.sqrt(1.0 - b2 ** self.steps)
        updates = []
        for i, g in enumerate(grads):
            gr = g.to(self.dtype) * (gscale * coef)
            self.m[i] = self.m[i] * b1 + gr * (1.0 - b1)
            self.v[i] = self.v[i] * b2 + gr * gr * (1.0 - b2)
            r = (self.m[i] / bc1) / (self.v[i].sqrt() / bc2_sqrt + self.eps)
            if self.variant != "no_decay_in_update":
                r = r + self.rows[i][1] * self.p[i]
            updates.append(r)
        norm = lambda ts: math.sqrt(sum(float((t.double() ** 2).sum()) for t in ts))      # noqa: E731
        for i, r in enumerate(updates):
            s, wd = self.rows[i]
            if self.variant == "trust_one" or (wd == 0.0 and not self.always_adapt):
                t = 1.0
            elif self.variant == "store_norms":
                t = self._ratio(norm(self.p), norm(updates))
            else:
                t = self._ratio(norm([self.p[i]]), norm([r]))
            self.trust[i] = t
        for i, r in enumerate(updates):
            self.p[i] = self.p[i] - (self.lr * self.rows[i][0] * self.trust[i]) * r
        return list(self.trust)


def run(params, grads, rows, dtype, max_norm=MAX_NORM, gscale=1.0, **kw):
    """per step of `grads`: (params, exp_avg, exp_avg_sq, trust ratios, pre-clip norm), copies"""
    ref, out = LambRef(params, rows, dtype, **kw), []
    for g in grads:
        coef, norm = clip_coef(g, gscale, max_norm, dtype)
        trust = ref.step(g, gscale, coef)
        out.append(([x.clone() for x in ref.p], [x.clone() for x in ref.m], [x.clone() for x in ref.v], trust, norm))
    return out


def rows_of(layout):
    return [(s, w) for _, _, s, w in layout.rows]


def bar_from(run32, run64):
    """max(4 x max|fp32 run - fp64 run|, 2e-6) over the parameters of every step (the idiom of _optim_cases.bar_from), and the
    distance itself"""
    d = 0.0
    for a, b in zip(run32, run64):
        d = max(d, max(float((x.double() - y).abs().max()) for x, y in zip(a[0], b[0])))
    return max(4.0 * d, BAR_FLOOR), d


def distance(run_a, run_b):
    """max abs distance of two runs' parameters over every step"""
    return max(max(float((x.double() - y.double()).abs().max()) for x, y in zip(a[0], b[0])) for a, b in zip(run_a, run_b))
