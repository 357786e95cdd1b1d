#!/usr/bin/env python3
"""Golden vectors for DarkIR's dilated-gate decoder block, captured from the imported reference module
(DarkIR-main/archs/arch_model.py: DBlock) in fp64 on the CPU.  Needs torch only.  Parameters come from the seeded generator of
tests/darkir_ref.py (beta and gamma non-zero) and inputs / cotangents from oracle.fixtures.seeded_input, so fixtures hold
outputs, input gradients and every parameter gradient only (compacted).  Writes tests/golden/darkir_*.npz.

usage: python tools/capture_golden_darkir.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import darkir_ref as D  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (c, dilations, extra_depth_wise, (B, H, W), seed)
CASES = {
    "darkir_dblock_c32": (32, (1, 4, 9), True, (2, 9, 11), 41),
    "darkir_dblock_c64": (64, (1, 4, 9), True, (2, 20, 20), 42),
    "darkir_dblock_c16_plain": (16, (1,), False, (2, 5, 7), 43),
    "darkir_dblock_c12_dil16": (12, (2, 2, 16), True, (2, 12, 12), 44),
}


def case_io(c, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, c, H, W), 1000 + seed), seeded_input((B, c, H, W), 2000 + seed)


def load_reference(ref_root):
    arch = os.path.join(ref_root, "DarkIR-main", "archs")
    sys.path.insert(0, arch)            # arch_model.py falls back to `from arch_util import LayerNorm2d`
    spec = importlib.util.spec_from_file_location("darkir_arch_model", os.path.join(arch, "arch_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def save(name, arrays):
    out = {}
    for k, v in arrays.items():
        pack(k, v, out)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    R = load_reference(ref_root)
    torch.manual_seed(0)
    for name, (c, dil, extra, bhw, seed) in CASES.items():
        mod = R.DBlock(c, dilations=list(dil), extra_depth_wise=extra).double()
        shapes = D.dblock_shapes(c, len(dil), extra)
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == list(shapes.items()), name
        mod.load_state_dict(D.make_state(shapes, seed))
        x, cot = case_io(c, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        arrays = {"y": y, "dx": x.grad}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        save(name, arrays)
    keys = {}
    for tag, args in (("dil149_extra", dict(c=32, dilations=[1, 4, 9], extra_depth_wise=True)),
                      ("dil1_plain", dict(c=16, dilations=[1], extra_depth_wise=False))):
        sd = R.DBlock(**args).state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(OUT, "darkir_dblock_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"darkir_dblock_keys: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
