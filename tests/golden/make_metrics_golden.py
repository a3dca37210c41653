#!/usr/bin/env python3
"""Writes tests/golden/metrics.npz: the results of the REFERENCE's own metric classes (utils/metrics.py) on small seeded
inputs, with the inputs.  usage: python tests/golden/make_metrics_golden.py /path/to/reference

utils/metrics.py imports `ignite.metrics.SSIM` and `torcheval.metrics.PeakSignalNoiseRatio` at module level; neither
library is installed where this project is developed, so stub modules stand in for them in sys.modules.  The stubs only
let the import succeed: PSNR and SSIM therefore CANNOT be produced by the reference here and are not in the fixture.  Those
two are held to the fp64 restatement of the published definitions (tests/_metrics_ref.py).

  DINO        CenterNorm, Teacher/Student Mean / STD / Var, CosineSim at G = 2, V = 4, B = 3, K = 256 (fp32, as the trainer
              feeds them)
  supervised  Accuracy, F1Score, Recall on 200 labels of 7 classes; class 5 is never predicted and class 6 never occurs in
              y_true (but is predicted), so max(y_true) + 1 = 6 classes are averaged and zero denominators occur.
              The reference's Precision.compute returns None (no `return`): recorded as such by leaving it out."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch


def main(ref):
    for name, attr in (("ignite", None), ("ignite.metrics", "SSIM"), ("torcheval", None), ("torcheval.metrics", "PeakSignalNoiseRatio")):
        mod = types.ModuleType(name)
        if attr:
            setattr(mod, attr, type(attr, (), {"__init__": lambda self, **kw: None}))
        sys.modules[name] = mod
    # by file: the reference's utils/__init__.py imports torchvision and the rich logger, which metrics.py does not need
    spec = importlib.util.spec_from_file_location("reference_utils_metrics", os.path.join(ref, "utils", "metrics.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)

    gen = torch.Generator().manual_seed(20240607)
    G, V, B, K = 2, 4, 3, 256
    teacher = torch.randn(G, B, K, generator=gen) * 1.5 + 0.3
    student = torch.randn(V, B, K, generator=gen) * 0.7 - 0.2
    student[:G] += 0.5 * teacher                                  # correlated views: the cosine is not ~0
    center = torch.randn(1, K, generator=gen) * 0.1 + 0.05
    names = ["CenterNorm", "TeacherMean", "TeacherSTD", "TeacherVar", "StudentMean", "StudentSTD", "StudentVar", "CosineSim"]
    h = M.MetricHandler({"metrics": names})
    dino = h.calculate_metrics(center=center, teacher_distribution=teacher, student_distribution=student)

    y_true = torch.randint(0, 6, (200,), generator=gen)
    y_pred = torch.where(torch.rand(200, generator=gen) < 0.6, y_true, torch.randint(0, 7, (200,), generator=gen))
    y_pred[y_pred == 5] = 6
    assert int(y_true.max()) == 5 and not (y_pred == 5).any() and (y_pred == 6).any()
    # the classes directly: F1Score / Recall take no **kwargs, so MetricHandler.calculate_metrics cannot feed them `correct`
    sup = {"Accuracy": M.Accuracy().compute(correct=int((y_pred == y_true).sum()), total=200),
           "F1Score": M.F1Score().compute(y_pred=y_pred, y_true=y_true), "Recall": M.Recall().compute(y_pred=y_pred, y_true=y_true)}
    assert M.Precision().compute(y_pred=y_pred, y_true=y_true) is None

    out = {"teacher": teacher.numpy(), "student": student.numpy(), "center": center.numpy(), "y_true": y_true.numpy(),
           "y_pred": y_pred.numpy()}
    out.update({f"dino_{k}": np.float64(float(v)) for k, v in dino.items()})
    out.update({f"sup_{k}": np.float64(float(v)) for k, v in sup.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
