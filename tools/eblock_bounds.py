#!/usr/bin/env python3
"""Host-side error table behind the bounds of tests/test_gpu_eblock.py: for every parity case of tests/eblock_ref.py, for the
small network and both activation dtypes, the error of the restatement evaluated on the CPU in the device's storage precision
(float32 throughout, or every stored activation and activation gradient rounded to bfloat16; FreMLP in its dense-DFT form) against
its fp64 evaluation with torch.fft, per tensor, as max |delta| / max |ref|.  The GPU test allows 4x these.  Also prints every
case's spectral-floor margin (min |Z| / rms |Z| of the FreMLP inputs; the precondition is >= FLOOR) and checks that the recorded
training seed lets the fp32 host restatement meet the trajectory bars.  Writes tests/golden/eblock_bounds.npz.

usage: python tools/eblock_bounds.py
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

import eblock_ref as E  # noqa: E402


def main():
    out = {}
    print(f"| case | dtype | floor margin (>= {E.FLOOR:g}) | y | dx | largest parameter-gradient error (tensor) |")
    print("|---|---|---|---|---|---|")
    for name in list(E.PARITY_CASES) + ["net"]:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            errs, _, margin = E.net_host_errors(dtype) if name == "net" else E.host_errors(name, dtype)
            assert margin >= E.FLOOR, (name, tag, margin)
            for k, v in errs.items():
                out[f"{name}.{tag}.{k}"] = np.float64(v)
            gk = max((k for k in errs if k.startswith("g.")), key=lambda k: errs[k])
            print(f"| {name} | {tag} | {margin:.1e} | {errs['y']:.2e} | {errs['dx']:.2e} | {errs[gk]:.2e} ({gk[2:]}) |")
    path = os.path.join(ROOT, "tests", "golden", "eblock_bounds.npz")
    np.savez_compressed(path, **out)
    print(f"eblock_bounds: {os.path.getsize(path) / 1024:.1f} KB")
    sd0, x, tgt = E.train_io()
    ref_losses, ref = E.train_reference(sd0, x, tgt)
    losses, got = E.train_reference(sd0, x, tgt, torch.float32, dense=True)
    misses = E.trajectory_misses(losses, got, ref_losses, ref, sd0)
    print(f"training seed {E.TRAIN_SEED}: fp32 host restatement against fp64: {'meets every bar' if not misses else misses}")


if __name__ == "__main__":
    main()
