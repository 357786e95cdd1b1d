#!/usr/bin/env python3
"""Golden vectors for DarkIR's FreMLP, captured from the imported reference module (DarkIR-main/archs/arch_model.py: FreMLP) in
fp64 on the CPU.  Needs torch only.  Parameters come from the seeded generator of tests/darkir_ref.py and inputs / cotangents
from oracle.fixtures.seeded_input, so fixtures hold the output, the input gradient and the four parameter gradients only
(compacted).  Writes tests/golden/darkir_fremlp_*.npz and the reference's state_dict key list, darkir_fremlp_keys.npz.

usage: python tools/capture_golden_fremlp.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import fremlp_ref as R  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (nc, expand, (B, H, W), seed)
CASES = {
    "darkir_fremlp_c32": (32, 2, (2, 9, 11), 61),          # odd H and W
    "darkir_fremlp_c16": (16, 2, (2, 16, 12), 62),         # even H and W: Nyquist row and column
    "darkir_fremlp_c8_e3": (8, 3, (2, 5, 8), 63),
    "darkir_fremlp_c64_e1": (64, 1, (1, 20, 20), 64),
}
# the constructor arguments whose state_dict keys and shapes darkir_fremlp_keys.npz records
KEY_CASES = (("nc32", dict(nc=32)), ("nc8_e3", dict(nc=8, expand=3)))


def case_io(nc, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, nc, H, W), 1000 + seed), seeded_input((B, nc, H, W), 2000 + seed)


def capture(ref_root):
    """Runs the reference's FreMLP (the only place that imports it)."""
    arch = os.path.join(ref_root, "DarkIR-main", "archs")
    sys.path.insert(0, arch)            # arch_model.py falls back to `from arch_util import LayerNorm2d`
    spec = importlib.util.spec_from_file_location("darkir_arch_model", os.path.join(arch, "arch_model.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    for name, (nc, expand, bhw, seed) in CASES.items():
        mod = ref.FreMLP(nc, expand).double()
        shapes = R.fremlp_shapes(nc, expand)
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == list(shapes.items()), name
        mod.load_state_dict(R.make_state(shapes, seed))
        x, cot = case_io(nc, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        arrays = {"y": y, "dx": x.grad}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        out = {}
        for k, v in arrays.items():
            pack(k, v, out)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")
    keys = {}
    for tag, args in KEY_CASES:
        sd = ref.FreMLP(**args).state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    path = os.path.join(OUT, "darkir_fremlp_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"darkir_fremlp_keys: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    capture(ref_root)


if __name__ == "__main__":
    main()
