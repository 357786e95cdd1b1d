#!/usr/bin/env python3
"""Golden vectors for SFHformer's FourierUnit, captured from the imported reference module (SFHformer.py: FourierUnit) in fp64 on
the CPU.  Needs torch and einops.  Parameters and running statistics come from the seeded generator of tests/sfh_ref.py and inputs /
cotangents from oracle.fixtures.seeded_input, so fixtures hold the output, the input gradient, the eight parameter gradients and
the running statistics after the step only (compacted).  Writes tests/golden/sfh_fu_*.npz and the reference's state_dict key
list, shapes and buffer names, sfh_fu_keys.npz.

usage: python tools/capture_golden_fourier_unit.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import sfh_ref as R  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (c, groups, (B, H, W), seed, training)
CASES = {
    "sfh_fu_c8_g4": (8, 4, (2, 9, 11), 71, True),           # odd H and W
    "sfh_fu_c6_g4": (6, 4, (2, 8, 12), 72, True),           # S = 3: a group boundary splits a complex pair; Nyquist row and column
    "sfh_fu_c16_g2": (16, 2, (1, 16, 12), 73, True),
    "sfh_fu_c8_g4_eval": (8, 4, (2, 6, 8), 74, False),      # eval mode with seeded running statistics
}
# the constructor arguments whose state_dict keys and shapes sfh_fu_keys.npz records
KEY_CASES = (("c8_g4", dict(in_channels=8, out_channels=8)), ("c6_g2", dict(in_channels=6, out_channels=6, groups=2)))


def case_io(c, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, c, H, W), 1000 + seed), seeded_input((B, c, H, W), 2000 + seed)


def case_state(c, G, seed, training):
    return R.make_state(c, G, seed, trivial_stats=training)


def capture(ref_root):
    """Runs the reference's FourierUnit (the only place that imports it)."""
    spec = importlib.util.spec_from_file_location("sfhformer_ref", os.path.join(ref_root, "SFHformer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    for name, (c, G, bhw, seed, training) in CASES.items():
        mod = ref.FourierUnit(c, c, G).double()
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == R.state_dict_layout(c, G), name
        mod.load_state_dict(R.module_state(case_state(c, G, seed, training)))
        mod.train(training)
        x, cot = case_io(c, bhw, seed)
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        assert int(mod.bn.num_batches_tracked) == int(training)
        arrays = {"y": y, "dx": x.grad, "rm": mod.bn.running_mean, "rv": mod.bn.running_var}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        out = {}
        for k, v in arrays.items():
            pack(k, v, out)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")
    keys = {}
    for tag, args in KEY_CASES:
        mod = ref.FourierUnit(**args)
        sd = mod.state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        keys[tag + ".buffers"] = np.array([k for k, _ in mod.named_buffers()])
    path = os.path.join(OUT, "sfh_fu_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"sfh_fu_keys: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    capture(ref_root)


if __name__ == "__main__":
    main()
