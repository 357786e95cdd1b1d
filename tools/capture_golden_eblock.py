#!/usr/bin/env python3
"""Golden vectors for DarkIR's encoder block and the whole network, captured from the imported reference modules
(DarkIR-main/archs/arch_model.py: EBlock; archs/DarkIR.py: DarkIR) in fp64 on the CPU.  Needs torch only.  Parameters come from
the seeded generator of tests/darkir_ref.py (beta and gamma non-zero), block inputs / cotangents from
oracle.fixtures.seeded_input and the network's from tests/eblock_ref.py, so fixtures hold outputs, input gradients and every
parameter gradient only (compacted).  Every case is checked for the spectral floor of its FreMLP inputs before it is written.
Writes tests/golden/darkir_eblock_*.npz, darkir_net_w8.npz and darkir_net_keys.npz.

usage: python tools/capture_golden_eblock.py [REFERENCE_ROOT]   (default: $REFERENCE_ROOT)
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

import eblock_ref as E  # noqa: E402
from oracle.fixtures import pack, seeded_input  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F64 = torch.float64

# name -> (c, dilations, extra_depth_wise, (B, H, W), seed)
CASES = {
    "darkir_eblock_c32": (32, (1,), True, (2, 9, 11), 61),
    "darkir_eblock_c64": (64, (1,), True, (2, 16, 16), 62),
    "darkir_eblock_c16_plain": (16, (1,), False, (2, 5, 7), 63),
    "darkir_eblock_c12_dil149": (12, (1, 4, 9), True, (2, 12, 12), 64),
}
NET_CASE = "darkir_net_w8"


def case_io(c, bhw, seed):
    B, H, W = bhw
    return seeded_input((B, c, H, W), 1000 + seed), seeded_input((B, c, H, W), 2000 + seed)


def load_reference(ref_root):
    arch = os.path.join(ref_root, "DarkIR-main", "archs")
    sys.path.insert(0, arch)            # the modules fall back to `from arch_util import ...`
    mods = []
    for name in ("arch_model", "DarkIR"):
        spec = importlib.util.spec_from_file_location("darkir_" + name, os.path.join(arch, name + ".py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


def save(name, arrays, keep_sum=True):
    out = {}
    for k, v in arrays.items():
        pack(k, v, out)
    if not keep_sum:        # oracle.fixtures.check reads the subset and the L2 digest only; ~190 tensors x one archive member each
        out = {k: v for k, v in out.items() if not k.endswith(".sum")}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB")


def key_lists(sd, tag, keys):
    keys[tag + ".keys"] = np.array(list(sd.keys()))
    keys[tag + ".shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REFERENCE_ROOT")
    if not ref_root:
        raise SystemExit("give the reference root (argument or $REFERENCE_ROOT)")
    A, N = load_reference(ref_root)
    torch.manual_seed(0)
    for name, (c, dil, extra, bhw, seed) in CASES.items():
        mod = A.EBlock(c, dilations=list(dil), extra_depth_wise=extra).double()
        shapes = E.eblock_shapes(c, len(dil), extra)
        assert [(k, tuple(v.shape)) for k, v in mod.state_dict().items()] == list(shapes.items()), name
        sd = E.make_state(shapes, seed)
        mod.load_state_dict(sd)
        x, cot = case_io(c, bhw, seed)
        probe = []
        E.run(x, cot, sd, dil, probe=probe)
        assert E.floor_margin(probe) >= E.FLOOR, (name, E.floor_margin(probe))
        x = x.to(F64).requires_grad_(True)
        y = mod(x)
        y.backward(cot.to(F64))
        arrays = {"y": y, "dx": x.grad}
        arrays.update({"g." + k: p.grad for k, p in mod.named_parameters()})
        save(name, arrays)
    # the small network, side_loss=True, on an input that needs padding in both directions
    cfg = E.SMALL_NET
    net = N.DarkIR(**cfg).double()
    shapes = E.net_shapes(cfg)
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == list(shapes.items())
    sd, x, cots = E.net_io()
    net.load_state_dict(sd)
    probe = []
    E.run_net(x, cots, sd, cfg, probe=probe)
    assert E.floor_margin(probe) >= E.FLOOR, E.floor_margin(probe)
    x = x.to(F64).requires_grad_(True)
    side, y = net(x, side_loss=True)
    torch.autograd.backward([side, y], [cots[0].to(F64), cots[1].to(F64)])
    arrays = {"side": side, "y": y, "dx": x.grad}
    arrays.update({"g." + k: p.grad for k, p in net.named_parameters()})
    save(NET_CASE, arrays, keep_sum=False)
    keys = {}
    for tag, args in (("eblock_extra", dict(c=32, extra_depth_wise=True)), ("eblock_dil149_plain", dict(c=16, dilations=[1, 4, 9]))):
        key_lists(A.EBlock(**args).state_dict(), tag, keys)
    key_lists(N.DarkIR().state_dict(), "darkir_m", keys)
    assert list(E.net_shapes(E.net_config()).items()) == [(k, tuple(v.shape)) for k, v in N.DarkIR().state_dict().items()]
    path = os.path.join(OUT, "darkir_net_keys.npz")
    np.savez_compressed(path, **keys)
    print(f"darkir_net_keys: {os.path.getsize(path) / 1024:.1f} KB")


if __name__ == "__main__":
    main()
