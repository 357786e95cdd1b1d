#!/usr/bin/env python3
"""Golden vectors for SFHformer's FFN and TokenMixer_For_Local, captured from the imported reference modules (SFHformer.py: FFN,
TokenMixer_For_Local) in fp64 on the CPU.  Needs torch and einops.  Parameters come from the seeded generator of
tests/sfh_ffn_ref.py and inputs / cotangents from oracle.fixtures.seeded_input, so fixtures hold the output, the input gradient and
every parameter gradient only (compacted to sfh_ffn_ref.PACK_ELEMS elements per tensor).  Writes tests/golden/sfh_ffn_*.npz, sfh_local_*.npz and the reference's state_dict key
list, shapes and buffer names, sfh_ffn_keys.npz.

usage: python tools/capture_golden_sfh_ffn.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import sfh_ffn_ref as R  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (kind, dim, (B, H, W), seed)
CASES = {
    "sfh_ffn_d4": ("ffn", 4, (2, 9, 11), 81),               # odd H and W
    "sfh_ffn_d6": ("ffn", 6, (1, 8, 34), 82),               # s = 3: an odd segment width
    "sfh_ffn_d32": ("ffn", 32, (1, 16, 12), 83),
    "sfh_local_d4": ("local", 4, (2, 9, 11), 84),
    "sfh_local_d6": ("local", 6, (1, 5, 34), 85),
}
CLASSES = {"ffn": "FFN", "local": "TokenMixer_For_Local"}
# the constructor arguments whose state_dict keys and shapes sfh_ffn_keys.npz records
KEY_CASES = (("ffn_d8", "ffn", dict(dim=8)), ("ffn_d6", "ffn", dict(dim=6)), ("local_d8", "local", dict(dim=8)),
             ("local_d6", "local", dict(dim=6)))


def case_io(dim, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, dim, H, W), 1000 + seed), seeded_input((B, dim, H, W), 2000 + seed)


def case_state(kind, dim, seed):
    return R.make_state(kind, dim, seed)


def capture(ref_root):
    """Runs the reference's FFN and TokenMixer_For_Local (the only place that imports them)."""
    spec = importlib.util.spec_from_file_location("sfhformer_ref", os.path.join(ref_root, "SFHformer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    for name, (kind, dim, bhw, seed) in CASES.items():
        mod = getattr(ref, CLASSES[kind])(dim).double()
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == R.state_dict_layout(kind, dim), name
        mod.load_state_dict(case_state(kind, dim, seed))
        x, cot = case_io(dim, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        arrays = {"y": y, "dx": x.grad}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        out = {}
        for k, v in arrays.items():
            pack(k, v, out, R.PACK_ELEMS)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")
    keys = {}
    for tag, kind, args in KEY_CASES:
        mod = getattr(ref, CLASSES[kind])(**args)
        sd = mod.state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        keys[tag + ".buffers"] = np.array([k for k, _ in mod.named_buffers()], dtype="<U1")
    path = os.path.join(OUT, "sfh_ffn_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"sfh_ffn_keys: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    capture(ref_root)


if __name__ == "__main__":
    main()
