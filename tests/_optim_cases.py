"""Shared pieces of the segmented-AdamW tests (include/vitssl_optim.h): the common store layout, the torch reference
(torch.optim.AdamW with one param group per tensor plus torch.nn.utils.clip_grad_norm_, on the CPU in float32 or float64)
and the bar derived from it."""
import torch

ALIGN = 64
SENTINEL = 0x5EAD5EAD                   # int32 pattern of p / m / v pads and frozen slices (a finite float: 2.5e18)
BAR_FLOOR = 2e-6                        # the bar of test_adamw_matches_torch_golden

# (shape, trainable): n = 1, 3, 4, 65, 4097 and 128 x 64, one frozen parameter in the middle without a table entry
COMMON = [((1,), True), ((3,), True), ((2, 2), True), ((200,), False), ((65,), True), ((17, 241), True), ((128, 64), True)]
LR, BETAS, EPS, MAX_NORM, STEPS = 1e-3, (0.9, 0.999), 1e-8, 1.0, 5
GRAD_SCALES = (0.01, 3.0)               # the gradient's global norm on even / odd steps: clip idle / clip active at MAX_NORM


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Layout:
    """Offsets of `shapes` in a flat store (64-float aligned, as engine.FlatStore) and the table rows of the trainable ones:
    lr multiplier 0.65 ** (i % 3) over the trainable index i, weight decay 0 for ndim <= 1, else 0.05."""

    def __init__(self, spec=COMMON):
        self.shapes = [s for s, _ in spec]
        self.trainable = [t for _, t in spec]
        self.offsets, off = [], 0
        for s in self.shapes:
            self.offsets.append(off)
            off = (off + numel(s) + ALIGN - 1) // ALIGN * ALIGN
        self.numel = off
        self.rows, i = [], 0          # (offset, n, lr_scale, weight_decay)
        for s, o, t in zip(self.shapes, self.offsets, self.trainable):
            if t:
                self.rows.append((o, numel(s), 0.65 ** (i % 3), 0.0 if len(s) <= 1 else 0.05))
                i += 1
        self.mask = torch.zeros(off, dtype=torch.bool)       # True on the floats of trainable parameters
        for o, n, _, _ in self.rows:
            self.mask[o:o + n] = True
        self.elements = int(self.mask.sum())

    def gather(self, flat):
        """the trainable parameters' slices of a flat CPU tensor, as a list"""
        return [flat[o:o + n].clone() for o, n, _, _ in self.rows]

    def scatter(self, tensors, fill, dtype=torch.float32):
        flat = torch.full((self.numel,), fill, dtype=dtype)
        for (o, n, _, _), t in zip(self.rows, tensors):
            flat[o:o + n] = t.reshape(-1).to(dtype)
        return flat


def make_case(layout, seed=0):
    """initial parameters and STEPS gradients (lists over the trainable parameters, float32 CPU): the gradient of step k has
    global norm GRAD_SCALES[k % 2]"""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen) for _, n, _, _ in layout.rows]
    grads = []
    for k in range(STEPS):
        g = [torch.randn(n, generator=gen, dtype=torch.float64) for _, n, _, _ in layout.rows]
        norm = torch.sqrt(sum((x * x).sum() for x in g))
        grads.append([(x * (GRAD_SCALES[k % 2] / norm)).float() for x in g])
    return params, grads


def torch_reference(layout, params, grads, dtype, max_norm=MAX_NORM, gscale=1.0, lr=LR):
    """per step: (params, exp_avg, exp_avg_sq, pre-clip norm), each a list of `dtype` tensors"""
    ps = [p.to(dtype).clone().requires_grad_(True) for p in params]
    opt = torch.optim.AdamW([dict(params=[p], lr=lr * s, weight_decay=w) for p, (_, _, s, w) in zip(ps, layout.rows)],
                            lr=lr, betas=BETAS, eps=EPS)
    out = []
    for g in grads:
        for p, x in zip(ps, g):
            p.grad = x.to(dtype) * gscale
        norm = torch.nn.utils.clip_grad_norm_(ps, max_norm) if max_norm is not None else None
        opt.step()
        out.append(([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps],
                    [opt.state[p]["exp_avg_sq"].clone() for p in ps], norm))
    return out


def bar_from(ref32, ref64):
    """4 x the max-abs distance of the float32 and the float64 run of the same torch recipe over the parameters of every step,
    never below BAR_FLOOR"""
    d = 0.0
    for (p32, _, _, _), (p64, _, _, _) in zip(ref32, ref64):
        d = max(d, max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64)))
    return max(4.0 * d, BAR_FLOOR), d
