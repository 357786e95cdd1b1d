#!/usr/bin/env python3
"""Golden vectors for SFHformer's TokenMixer_For_Gloal and Mixer, captured from the imported reference modules (SFHformer.py) in fp64
on the CPU.  Needs torch and einops.  Parameters come from the seeded generator of tests/sfh_mixer_ref.py and inputs / cotangents
from oracle.fixtures.seeded_input, so fixtures hold the output, the input gradient, every parameter gradient and the running
statistics after the call only (compacted to sfh_mixer_ref.PACK_ELEMS elements per tensor).  Writes tests/golden/sfh_mixer_*.npz,
sfh_global_*.npz and the reference's state_dict key list, shapes and buffer names, sfh_mixer_keys.npz.

usage: python tools/capture_golden_sfh_mixer.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import sfh_mixer_ref as R  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (kind, dim, (B, H, W), seed, training)
CASES = {
    "sfh_mixer_d4": ("mixer", 4, (2, 9, 11), 86, True),             # odd H and W
    "sfh_mixer_d6_eval": ("mixer", 6, (2, 8, 10), 87, False),       # segment width 3; seeded running statistics
    "sfh_mixer_d32": ("mixer", 32, (1, 12, 16), 88, True),
    "sfh_global_d3": ("global", 3, (2, 9, 11), 89, True),           # an odd dim
    "sfh_global_d8_eval": ("global", 8, (1, 8, 12), 90, False),
}
CLASSES = {"global": "TokenMixer_For_Gloal", "mixer": "Mixer"}
# the constructor arguments whose state_dict keys and shapes sfh_mixer_keys.npz records
KEY_CASES = (("mixer_d8", "mixer", dict(dim=8)), ("mixer_d6", "mixer", dict(dim=6)), ("global_d8", "global", dict(dim=8)),
             ("global_d3", "global", dict(dim=3)))


def case_io(dim, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, dim, H, W), 1000 + seed), seeded_input((B, dim, H, W), 2000 + seed)


def case_state(kind, dim, seed, training):
    return R.make_state(kind, dim, seed, trivial_stats=training)


def capture(ref_root):
    """Runs the reference's TokenMixer_For_Gloal and Mixer (the only place that imports them)."""
    spec = importlib.util.spec_from_file_location("sfhformer_ref", os.path.join(ref_root, "SFHformer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    for name, (kind, dim, bhw, seed, training) in CASES.items():
        mod = getattr(ref, CLASSES[kind])(dim).double()
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == R.state_dict_layout(kind, dim), name
        mod.load_state_dict(R.module_state(kind, case_state(kind, dim, seed, training)))
        mod.train(training)
        x, cot = case_io(dim, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        sd = mod.state_dict()
        arrays = {"y": y, "dx": x.grad, "rm": sd[R.RM[kind]], "rv": sd[R.RV[kind]]}
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
        keys[tag + ".buffers"] = np.array([k for k, _ in mod.named_buffers()])
    path = os.path.join(OUT, "sfh_mixer_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"sfh_mixer_keys: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    capture(ref_root)


if __name__ == "__main__":
    main()
