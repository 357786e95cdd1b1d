#!/usr/bin/env python3
"""Host-side error table behind the bounds of tests/test_gpu_bn2d.py: for every parity case of tests/bn2d_ref.py, both activation
dtypes and both modes, the error of the DEVICE form of the restatement evaluated on the CPU in the device's storage precision
(float32 throughout, or x, y, f, out, dx, df and the cotangent rounded to bfloat16) against the fp64 formulas, per tensor, as
max |delta| / max |ref|.  The device form is built from elementwise operations and explicit ordered sums only (no matmul, no
library reduction): the table does not depend on the CPU's BLAS.  The GPU test allows 4x these (and never less than 4 x 2^-24).
Writes tests/golden/bn2d_bounds.npz (scalars only).

usage: python tools/bn2d_bounds.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import bn2d_ref as R  # noqa: E402


def main():
    out = {}
    print("| case | dtype | mode | " + " | ".join(R.TENSORS) + " |")
    print("|---|---|---|" + "---|" * len(R.TENSORS))
    for name in R.PARITY_CASES:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            for training, mode in ((True, "train"), (False, "eval")):
                errs, _ = R.host_errors(name, dtype, training)
                for k, v in errs.items():
                    out[f"{name}.{tag}.{mode}.{k}"] = np.float64(v)
                print(f"| {name} | {tag} | {mode} | " + " | ".join(f"{errs[k]:.1e}" for k in R.TENSORS) + " |")
    path = os.path.join(ROOT, "tests", "golden", "bn2d_bounds.npz")
    np.savez_compressed(path, **out)
    print(f"bn2d_bounds: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
