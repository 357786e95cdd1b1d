#!/usr/bin/env python3
"""Golden vectors for DRSformer's transformer block, captured from the imported reference module (DRSformer_arch.py: TKSA
Attention, MSFN FeedForward, the STB TransformerBlock) in fp64 on the CPU.  Needs torch and einops only.  Parameters come from
the seeded generator of tests/drs_ref.py and inputs / cotangents from oracle.fixtures.seeded_input, so fixtures hold outputs,
input gradients and every parameter gradient only (compacted).  Writes tests/golden/drs_*.npz.

usage: python tools/capture_golden_drs.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import drs_ref as D  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (kind, dim, heads, factor, bias, ln_type, (B, H, W), seed)
CASES = {
    "drs_tksa_c48h1": ("tksa", 48, 1, None, False, None, (2, 16, 16), 11),
    "drs_tksa_c96h2": ("tksa", 96, 2, None, False, None, (2, 12, 12), 12),
    "drs_tksa_c96h1": ("tksa", 96, 1, None, True, None, (2, 9, 11), 13),
    "drs_msfn_c48": ("msfn", 48, 1, 2.66, False, None, (2, 12, 12), 21),
    "drs_msfn_c48_bias": ("msfn", 48, 1, 2.66, True, None, (2, 12, 12), 22),
    "drs_msfn_c32f2": ("msfn", 32, 1, 2.0, False, None, (2, 9, 11), 23),
    "drs_msfn_c32f2_bias": ("msfn", 32, 1, 2.0, True, None, (2, 9, 11), 24),
    "drs_stb_withbias": ("stb", 48, 1, 2.66, False, "WithBias", (2, 16, 16), 31),
    "drs_stb_biasfree": ("stb", 48, 2, 2.66, True, "BiasFree", (2, 12, 12), 32),
}


def case_shapes(kind, dim, heads, factor, bias, ln_type):
    if kind == "tksa":
        return D.tksa_shapes(dim, heads, bias)
    if kind == "msfn":
        return D.msfn_shapes(dim, factor, bias)
    return D.stb_shapes(dim, heads, factor, bias, ln_type)


def case_io(dim, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, dim, H, W), 1000 + seed), seeded_input((B, dim, H, W), 2000 + seed)


def load_reference(ref_root):
    spec = importlib.util.spec_from_file_location("drsformer_arch", os.path.join(ref_root, "DRSformer_arch.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def build_module(R, kind, dim, heads, factor, bias, ln_type):
    if kind == "tksa":
        return R.Attention(dim, heads, bias)
    if kind == "msfn":
        return R.FeedForward(dim, factor, bias)
    return R.TransformerBlock(dim, heads, factor, bias, ln_type)


def save(name, arrays, meta):
    out = {}
    for k, v in arrays.items():
        pack(k, v, out)
    out.update({k: np.asarray(v) for k, v in meta.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    R = load_reference(ref_root)
    torch.manual_seed(0)
    for name, (kind, dim, heads, factor, bias, ln_type, bhw, seed) in CASES.items():
        mod = build_module(R, kind, dim, heads, factor, bias, ln_type).double()
        shapes = case_shapes(kind, dim, heads, factor, bias, ln_type)
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == list(shapes.items()), name
        mod.load_state_dict(D.make_state(shapes, seed))
        x, cot = case_io(dim, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        arrays = {"y": y, "dx": x.grad}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        save(name, arrays, {})
    keys = {}
    for tag, args in (("withbias", (48, 1, 2.66, False, "WithBias")), ("biasfree_bias", (96, 2, 2.66, True, "BiasFree"))):
        sd = R.TransformerBlock(*args).state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(OUT, "drs_stb_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"drs_stb_keys: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
