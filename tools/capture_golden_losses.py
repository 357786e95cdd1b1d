#!/usr/bin/env python3
"""Golden vectors for the pixel-space loss terms (tests/golden/pixel_losses.npz), captured from the imported reference (build
container only): the reference's own EdgeLoss and FocalL1Loss classes (MoCE-IR-main/src/utils/loss_utils.py:155-190, :100-136)
run on seeded inputs, values and the gradient with respect to the prediction.  That module imports torchvision,
torchvision.models.vgg19 and pytorch_msssim at module level, none installed here and none touched by the two classes, so the
capture puts the same empty stand-in modules into sys.modules as tools/capture_golden_f3.py.  (SSIMloss calls pytorch_msssim
itself: there is nothing to capture it from.)

Six kinds of term - EdgeLoss with 'l2' and 'l1' at loss_weight 1.0 and 0.05, FocalL1Loss with its defaults and with CG-IR's
gamma=0.5, alpha=1.0 - at three shapes (C = 3) in fp64 and fp32.  To keep the file small the two small shapes run three kinds
in fp64 and the other three in fp32, swapped between them, so that every kind is there in both precisions; the largest shape
adds one fp64 and three fp32 cases.  The inputs of a shape are one fp64 draw rounded to a 2^-8 grid: exact in fp32 and in
bf16, so both precisions - and a GPU test in either dtype - start from the very same numbers, and about one element in 256
is an exact tie.  EdgeLoss keeps its kernel in fp32 whatever the
input; for the fp64 cases the capture casts that attribute to fp64 (its values stay the fp32 products the class built).
For the 'l1' cases the seed is advanced until no element of the Laplacian difference is within 1e-5 of zero, so that sign()
is the same in every precision."""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True
REF = os.environ.get("REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

SHAPES = [(2, 3, 16, 16), (1, 3, 15, 21), (1, 3, 24, 40)]
KINDS = {"edge_l2_w1": ("edge", "l2", 1.0), "edge_l1_w1": ("edge", "l1", 1.0), "edge_l2_w005": ("edge", "l2", 0.05),
         "edge_l1_w005": ("edge", "l1", 0.05), "focal_default": ("focal", 2.0, 1e-6, 0.1), "focal_cgir": ("focal", 0.5, 1e-6, 1.0)}
ROTATION = [(("edge_l2_w1", "edge_l1_w005", "focal_default"), ("edge_l1_w1", "edge_l2_w005", "focal_cgir")),
            (("edge_l1_w1", "edge_l2_w005", "focal_cgir"), ("edge_l2_w1", "edge_l1_w005", "focal_default")),
            (("edge_l1_w1",), ("edge_l2_w005", "edge_l1_w005", "focal_default"))]   # (fp64 kinds, fp32 kinds) per shape


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_module():
    for name in ("torchvision", "torchvision.models", "pytorch_msssim"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision.models"].vgg19 = None
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    return load("MoCE-IR-main/src/utils/loss_utils.py", "ref_loss_utils")


def build(lu, kind, dt):
    k = KINDS[kind]
    if k[0] == "edge":
        m = lu.EdgeLoss(loss_weight=k[2], criterion=k[1])
        m.kernel = m.kernel.to(dt)
        return m
    return lu.FocalL1Loss(gamma=k[1], epsilon=k[2], alpha=k[3])


def draw(shape, seed):
    g = torch.Generator().manual_seed(seed)
    q = lambda t: torch.round(t * 256).clamp_(max=255) / 256
    return q(torch.rand(shape, generator=g, dtype=torch.float64)), q(torch.rand(shape, generator=g, dtype=torch.float64))


def main():
    lu = reference_module()
    out = {}
    for si, shape in enumerate(SHAPES):
        seed = 100 * (si + 1)
        while True:                      # 'l1': keep sign() away from zero
            pred, target = draw(shape, seed)
            lap = lu.EdgeLoss()
            lap.kernel = lap.kernel.double()
            e = lap.laplacian_kernel(pred) - lap.laplacian_kernel(target)
            if float(e.abs().min()) > 1e-5:
                break
            seed += 1
        tag = "x".join(map(str, shape))
        out[f"{tag}/pred"] = pred.float().numpy()
        out[f"{tag}/target"] = target.float().numpy()
        out[f"{tag}/seed"] = np.asarray(seed)
        for dt, kinds in zip((torch.float64, torch.float32), ROTATION[si]):
            for kind in kinds:
                p = pred.to(dt).clone().requires_grad_(True)
                loss = build(lu, kind, dt)(p, target.to(dt))
                loss.backward()
                name = f"{tag}/{'f64' if dt == torch.float64 else 'f32'}/{kind}"
                out[name + "/loss"] = np.asarray(float(loss.detach().double()), dtype=np.float64)
                out[name + "/dpred"] = p.grad.numpy()
                print(name, float(loss.detach()), "min|e| %.2e" % float(e.abs().min()))
    path = os.path.join(OUT, "pixel_losses.npz")
    np.savez_compressed(path, **out)
    print("pixel_losses.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
