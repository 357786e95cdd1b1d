#!/usr/bin/env python3
"""Host-side error table behind the bounds of tests/test_gpu_sfh_mixer.py: for every parity case of tests/sfh_mixer_ref.py and both
activation dtypes, the error of the DEVICE form of the restatement evaluated on the CPU in the device's storage precision (float32
throughout, or the tensors the kernels store rounded to bfloat16: the list is in the docstring of tests/sfh_mixer_ref.py) against
the fp64 form, per tensor, as max |delta| / max |ref|.  The GPU test allows 4x these (and never less than 4 x 2^-24).  Writes
tests/golden/sfh_mixer_bounds.npz.

usage: python tools/sfh_mixer_bounds.py
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

import sfh_mixer_ref as R  # noqa: E402


def main():
    out = {}
    print("| case | dtype | y | dx | rm | rv | largest parameter-gradient error (tensor) |")
    print("|---|---|---|---|---|---|---|")
    for name in R.PARITY_CASES:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _ = R.host_errors(name, dtype)
            for k, v in errs.items():
                out[f"{name}.{tag}.{k}"] = np.float64(v)
            gk = max((k for k in errs if k.startswith("g.")), key=lambda k: errs[k])
            print(f"| {name} | {tag} | {errs['y']:.2e} | {errs['dx']:.2e} | {errs['rm']:.2e} | {errs['rv']:.2e} | {errs[gk]:.2e} ({gk[2:]}) |")
    path = os.path.join(ROOT, "tests", "golden", "sfh_mixer_bounds.npz")
    np.savez_compressed(path, **out)
    print(f"sfh_mixer_bounds: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
