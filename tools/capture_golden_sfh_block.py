#!/usr/bin/env python3
"""Golden vectors for SFHformer's Block, Stage and Backbone, captured from the imported reference modules (SFHformer.py) in fp64 on
the CPU.  Needs torch and einops.  Parameters come from the seeded generator of tests/sfh_block_ref.py (beta and gamma of order 1:
the reference's zero initialisation makes a Block the identity) and inputs / cotangents from oracle.fixtures.seeded_input, so
fixtures hold the output, the input gradient, every parameter gradient and every running statistic after the call only (compacted
by oracle.fixtures.pack).  Writes tests/golden/sfh_block_*.npz, sfh_stage_*.npz, sfh_net_*.npz and the reference's state_dict key
list, shapes and buffer names, sfh_block_keys.npz.

Conditioning, asserted per case while capturing (a seed that fails is replaced, never a bar loosened):
 - the same case run in float32 on the CPU stays within FP32_BAR = 1e-4 of the fp64 result in every tensor, in
   oracle.fixtures.check's norm (max |difference| / max |fp64|): a tenth of the 1e-3 the device is held to against the fixture;
 - every BatchNorm input (norm1, norm2 and the FourierUnit's spectral one, of every Block) keeps sfh_ref's VAR_FLOOR: each
   channel's batch variance is 0 or at least VAR_FLOOR x the median channel's.

usage: python tools/capture_golden_sfh_block.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import bn2d_ref as B  # noqa: E402
import sfh_block_ref as R  # noqa: E402
from oracle.fixtures import pack  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FP32_BAR = 1e-4
CASES, KEY_CASES = R.CASES, R.KEY_CASES
CLASSES = {"block": "Block", "stage": "Stage", "net": "Backbone"}


def _run(ref, name, dtype, bn_inputs=None):
    kind, args, _, _, training = CASES[name]
    mod = getattr(ref, CLASSES[kind])(**args).to(dtype)
    assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == R.state_dict_layout(kind, args), name
    mod.load_state_dict(R.module_state(kind, args, R.case_state(name)))
    mod.train(training)
    if bn_inputs is not None:
        for m in mod.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.register_forward_pre_hook(lambda _m, inp: bn_inputs.append(inp[0].detach()))
    x, cot = R.case_io(name)
    x = x.to(dtype).requires_grad_(True)
    y = mod(x)
    y.backward(cot.to(dtype))
    sd = mod.state_dict()
    arrays = {"y": y.detach(), "dx": x.grad}
    arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
    arrays.update({"buf." + k: sd[k] for k in R.buffers_of(kind, args)})
    assert set(arrays) == R.tensors(kind, args) and [k for k, _ in mod.named_parameters()] == R.params_of(kind, args), name
    return arrays


def capture(ref_root):
    """Runs the reference's Block, Stage and Backbone (the only place that imports them)."""
    spec = importlib.util.spec_from_file_location("sfhformer_ref", os.path.join(ref_root, "SFHformer.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(0)
    for name in CASES:
        bn_inputs = []
        arrays = _run(ref, name, torch.float64, bn_inputs)
        assert len(bn_inputs) == 3 * len(R.block_prefixes(*CASES[name][:2])), name
        assert all(B.variances_ok(t) for t in bn_inputs), f"{name}: a BatchNorm input's channel variance is below VAR_FLOOR x the median"
        worst = ("", 0.0)
        for k, v in _run(ref, name, torch.float32).items():
            err = float((v.double() - arrays[k]).abs().max() / arrays[k].abs().max().clamp_min(1e-30))
            worst = max(worst, (k, err), key=lambda t: t[1])
        assert worst[1] <= FP32_BAR, f"{name}: {worst[0]} in float32 is {worst[1]:.2e} from fp64 (bar {FP32_BAR:.0e}): pick another seed"
        assert all(float(v.abs().max()) > 0 for v in arrays.values()), name
        out = {}
        for k, v in arrays.items():
            pack(k, v, out)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB, {len(arrays)} tensors, float32 within {worst[1]:.1e} ({worst[0]})")
    keys = {}
    for tag, kind, args in KEY_CASES:
        mod = getattr(ref, CLASSES[kind])(**args)
        sd = mod.state_dict()
        keys[tag + ".keys"] = np.array(list(sd.keys()))
        keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        keys[tag + ".buffers"] = np.array([k for k, _ in mod.named_buffers()])
    path = os.path.join(OUT, "sfh_block_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"sfh_block_keys: {os.path.getsize(path) / 1024:.1f} KB")


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    capture(ref_root)


if __name__ == "__main__":
    main()
