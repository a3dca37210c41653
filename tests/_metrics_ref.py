"""Restatements in torch of every training metric (the reference's utils/metrics.py and the libraries behind it), used by
the CPU and the GPU tests of the metric kernels.  Everything is computed in `dtype` (fp64 unless a test asks for the fp32
formula to size a tolerance) on the CPU, from the published definitions:

  PSNR   torcheval PeakSignalNoiseRatio(data_range=1.0): 10 log10(1 / (sum((x - y)^2) / count))
  SSIM   ignite SSIM(data_range=1.0, kernel_size=11, sigma=1.5, k1=0.01, k2=0.03): reflect padding by 5, "valid" filtering
         of x, y, x^2, y^2, xy per channel with the outer product of the normalised Gaussian, the index averaged over
         (C, P, P) per patch and over the patches
  DINO   utils/metrics.py:58-156 literally (torch.linalg.norm, flatten().mean / std / var, the broadcast cosine)
  labels utils/metrics.py:198-256 (per-class loops; Precision returns the macro average its loop computes)"""
import math

import torch
import torch.nn.functional as F

K1, K2, WINDOW, SIGMA = 0.01, 0.03, 11, 1.5


def gaussian_window(dtype=torch.float64):
    half = (WINDOW - 1) * 0.5
    g = torch.exp(-0.5 * (torch.linspace(-half, half, steps=WINDOW, dtype=dtype) / SIGMA) ** 2)
    g = (g / g.sum()).unsqueeze(0)
    return g.t() @ g


def recon_sums(pred, target, C, P, dtype=torch.float64):
    """(sum((clamp(pred, 0, 1) - target)^2), sum over patches of the mean SSIM index) of pred / target [n, C*P*P]"""
    x = pred.detach().cpu().float().clamp(0, 1).to(dtype).reshape(-1, C, P, P)
    y = target.detach().cpu().float().to(dtype).reshape(-1, C, P, P)
    n = x.shape[0]
    if n == 0:
        return 0.0, 0.0
    sse = float(((x - y) ** 2).sum())
    pad = (WINDOW - 1) // 2
    xp, yp = F.pad(x, [pad] * 4, mode="reflect"), F.pad(y, [pad] * 4, mode="reflect")
    kernel = gaussian_window(dtype).expand(C, 1, -1, -1)
    out = F.conv2d(torch.cat([xp, yp, xp * xp, yp * yp, xp * yp]), kernel, groups=C)
    mx, my, exx, eyy, exy = (out[i * n:(i + 1) * n] for i in range(5))
    c1, c2 = K1 ** 2, K2 ** 2
    a1, a2 = 2 * mx * my + c1, 2 * (exy - mx * my) + c2
    b1, b2 = mx * mx + my * my + c1, (exx - mx * mx) + (eyy - my * my) + c2
    idx = (a1 * a2) / (b1 * b2)
    return sse, float(idx.mean((1, 2, 3)).to(torch.float64).sum())


def recon_metrics(pred, target, C, P, dtype=torch.float64):
    sse, ssim_sum = recon_sums(pred, target, C, P, dtype)
    n = pred.shape[0]
    return {"PSNR": 10.0 * math.log10(n * C * P * P / sse) if sse > 0 else float("inf"), "SSIM": ssim_sum / n}


def dino_metrics(teacher, student, center, dtype=torch.float64):
    """the eight DINO metrics of teacher [G, B, K], student [V, B, K], center [K] or [1, K]"""
    t, s, c = (v.detach().cpu().float().to(dtype) for v in (teacher, student, center))
    tn, sn = torch.linalg.norm(t, dim=-1).unsqueeze(1), torch.linalg.norm(s, dim=-1).unsqueeze(0)
    dot = (t.unsqueeze(1) * s.unsqueeze(0)).sum(dim=-1)
    cos = dot / (tn * sn + 1e-8)
    tf, sf = t.flatten(), s.flatten()
    return {"CenterNorm": float(torch.linalg.norm(c)), "TeacherMean": float(tf.mean()), "TeacherSTD": float(tf.std()),
            "TeacherVar": float(tf.var()), "StudentMean": float(sf.mean()), "StudentSTD": float(sf.std()), "StudentVar": float(sf.var()),
            "CosineSim": float(cos.mean())}


def naive_fp32_var(x):
    """the formula the statistics kernel must NOT use: (sum(x^2) - n mean^2) / (n - 1) with fp32 sums"""
    x = x.detach().cpu().float().flatten()
    n = x.numel()
    mean = x.sum() / n
    return float(((x * x).sum() - n * mean * mean) / (n - 1))


def label_metrics(y_pred, y_true):
    y_pred, y_true = y_pred.cpu(), y_true.cpu()
    nc = int(y_true.max()) + 1
    ps, rs, fs = [], [], []
    for cls in range(nc):
        tp = int(((y_pred == cls) & (y_true == cls)).sum())
        fp = int(((y_pred == cls) & (y_true != cls)).sum())
        fn = int(((y_pred != cls) & (y_true == cls)).sum())
        p = tp / (tp + fp) if tp + fp > 0 else 0.0
        r = tp / (tp + fn) if tp + fn > 0 else 0.0
        ps.append(p)
        rs.append(r)
        fs.append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    return {"Accuracy": int((y_pred == y_true).sum()) / len(y_true), "F1Score": sum(fs) / nc, "Recall": sum(rs) / nc,
            "Precision": sum(ps) / nc}


# ---- the inputs of the reconstruction-metric tests (CPU and GPU tests must see the very same tensors: the kernel's bar is
# derived from what the fp32 formula loses on them)
RECON_GRID = [(P, C, n) for P in (8, 16, 6) for C in (3, 1) for n in (1, 5, 67, 1000)]
RECON_SPECIAL = [(16, 3, 67, "equal"), (8, 3, 67, "constant"), (6, 1, 5, "constant")]


def recon_inputs(P, C, n, kind="random"):
    """(pred, target) f32 [n, C*P*P].  random: pred ~ N(0.5, 0.5), so the clamp acts on both sides, target uniform in [0, 1];
    equal: pred == target; constant: every patch a constant pair (a, b) in [0, 1]"""
    gen = torch.Generator().manual_seed(1000003 * P + 1009 * C + n + (0 if kind == "random" else 77))
    target = torch.rand(n, C * P * P, generator=gen)
    if kind == "equal":
        return target.clone(), target
    if kind == "constant":
        ab = torch.rand(n, 2, generator=gen)
        return ab[:, :1].expand(n, C * P * P).contiguous(), ab[:, 1:].expand(n, C * P * P).contiguous()
    return 0.5 + 0.5 * torch.randn(n, C * P * P, generator=gen), target


def fp32_formula_deviation():
    """largest relative deviation, over RECON_GRID and RECON_SPECIAL, of the squared-error sum and of the SSIM sum computed
    with the same formula in fp32 torch from the fp64 result"""
    worst = 0.0
    for P, C, n, kind in [(P, C, n, "random") for P, C, n in RECON_GRID] + RECON_SPECIAL:
        pred, target = recon_inputs(P, C, n, kind)
        for lo, hi in zip(recon_sums(pred, target, C, P, torch.float32), recon_sums(pred, target, C, P)):
            if hi != 0:
                worst = max(worst, abs(lo - hi) / abs(hi))
    return worst
