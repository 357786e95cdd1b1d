#!/usr/bin/env python3
"""Times DarkIR's dilated-gate decoder block on the MI355X at its four decoder shapes (bs 8, bf16, dilations [1, 4, 9],
extra_depth_wise): the dilated-gate kernel forward and backward on its own, and the whole DBlock forward and forward + backward,
beside the same block in PyTorch-ROCm eager on the same device (a comparison inside this tool only: never on the product path)
and beside the rate of the sibling streaming kernels (dwconv_gate_fwd / dwconv_gate_bwd_data in profiles/r04_z_shape_table.txt).

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows.
Algorithmic bytes: the forward of the dilated gate reads 2c planes and writes c: 3 c N 2 B per image; its backward reads dg
(c) and x (2c) and writes dx (2c): 5 c N 2 B per image (its fp32 dz scratch between the two passes is extra traffic the figure
does not credit).

usage: python tools/bench_darkir.py [--bs 8] [--iters 20] [--repeats 7] [--warmup 5]
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

SHAPES = ((32, 256), (64, 128), (128, 64), (256, 32))   # (c, H = W) of DarkIR's decoder levels at a 256 x 256 input
DIL = (1, 4, 9)


def sibling_rates():
    """(min, max) GB/s of the sibling streaming kernels over the shapes of profiles/r04_z_shape_table.txt."""
    out = {}
    path = os.path.join(ROOT, "profiles", "r04_z_shape_table.txt")
    for line in open(path):
        m = re.match(r"(dwconv_gate_fwd|dwconv_gate_bwd_data)\s.*?(\d+) GB/s", line)
        if m:
            out.setdefault(m.group(1), []).append(int(m.group(2)))
    return {k: (min(v), max(v)) for k, v in out.items()}


def timed(fn, warmup, iters, repeats):
    """Median over `repeats` windows of the mean time of one call (us), device events around `iters` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / iters)
    return statistics.median(ts), min(ts), max(ts)


class EagerDBlock(torch.nn.Module):
    """The same block in plain PyTorch ops (the formulas of tests/darkir_ref.py as a module), bf16 parameters and activations."""

    def __init__(self, sd, dil):
        super().__init__()
        self.p = torch.nn.ParameterDict({k.replace(".", "_"): torch.nn.Parameter(v.clone()) for k, v in sd.items()})
        self.dil = dil

    def forward(self, x):
        import darkir_ref as D
        return D.dblock(x, {k: self.p[k.replace(".", "_")] for k in self._keys()}, self.dil)

    def _keys(self):
        import darkir_ref as D
        c = self.p["beta"].shape[1]
        return list(D.dblock_shapes(c, len(self.dil), True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_darkir: needs the MI355X (no CPU timing)")
    import darkir_ref as D
    from image_restoration_amd import darkir, ops
    dev = torch.device("cuda:0")
    sib = sibling_rates()
    print(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}, bf16, dilations {list(DIL)}, extra_depth_wise; "
          f"median of {a.repeats} windows of {a.iters} calls (min..max in brackets)")
    print(f"yardstick, sibling streaming kernels (profiles/r04_z_shape_table.txt): dwconv_gate_fwd {sib['dwconv_gate_fwd'][0]}.."
          f"{sib['dwconv_gate_fwd'][1]} GB/s, dwconv_gate_bwd_data {sib['dwconv_gate_bwd_data'][0]}..{sib['dwconv_gate_bwd_data'][1]} GB/s")
    t = lambda fn: timed(fn, a.warmup, a.iters, a.repeats)   # noqa: E731
    for c, hw in SHAPES:
        B, N = a.bs, hw * hw
        sd = D.make_state(D.dblock_shapes(c, len(DIL), True), 3)
        g = torch.Generator().manual_seed(c)
        # ---- the dilated-gate kernel alone
        x2 = torch.randn(B, 2 * c, hw, hw, generator=g).to(dev).to(torch.bfloat16)
        dg = torch.randn(B, c, hw, hw, generator=g).to(dev).to(torch.bfloat16)
        add = torch.randn(B, c, generator=g).to(dev)
        ws = [sd[f"branches.{i}.branch.0.weight"].to(dev) for i in range(len(DIL))]
        bs = [sd[f"branches.{i}.branch.0.bias"].to(dev) for i in range(len(DIL))]
        gw, gb = [torch.zeros_like(w) for w in ws], [torch.zeros_like(b) for b in bs]
        fwd = t(lambda: ops.dilgate_fwd(x2, ws, bs, DIL))
        bwd = t(lambda: ops.dilgate_bwd(dg, add, x2, ws, bs, DIL, gw, gb, False))
        fb, bb = 3.0 * c * N * 2 * B, 5.0 * c * N * 2 * B
        plan = ops.dilgate_plan(B, c, hw, hw, torch.bfloat16, DIL)
        print(f"c={c:3d} {hw}x{hw}  dilgate fwd {fwd[0]:8.1f} us [{fwd[1]:.1f}..{fwd[2]:.1f}]  {fb / fwd[0] / 1e3:6.0f} GB/s algorithmic"
              f" ({fb / 1e6:.1f} MB; {plan['grid_x'] * plan['grid_y'] * plan['grid_z']} workgroups, {plan['lds_bytes']} B LDS)")
        print(f"c={c:3d} {hw}x{hw}  dilgate bwd {bwd[0]:8.1f} us [{bwd[1]:.1f}..{bwd[2]:.1f}]  {bb / bwd[0] / 1e3:6.0f} GB/s algorithmic"
              f" ({bb / 1e6:.1f} MB; three launches and {2 * len(DIL)} gradient sums)")
        # ---- the whole block, native and eager
        blk = darkir.DBlock(c, dilations=list(DIL), extra_depth_wise=True)
        blk.load_state_dict(sd)
        blk = blk.to(dev)
        eager = EagerDBlock({k: v.to(torch.bfloat16) for k, v in sd.items()}, DIL).to(dev)
        x = torch.randn(B, c, hw, hw, generator=g).to(dev).to(torch.bfloat16)
        cot = torch.randn(B, c, hw, hw, generator=g).to(dev).to(torch.bfloat16)

        def fwd_only(m):
            with torch.no_grad():
                m(x)

        def fwd_bwd(m):
            xg = x.detach().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            m(xg).backward(cot)

        for name, m in (("native", blk), ("eager ", eager)):
            f, fbk = t(lambda m=m: fwd_only(m)), t(lambda m=m: fwd_bwd(m))
            print(f"c={c:3d} {hw}x{hw}  DBlock {name} fwd {f[0]:8.1f} us [{f[1]:.1f}..{f[2]:.1f}]   fwd+bwd {fbk[0]:8.1f} us "
                  f"[{fbk[1]:.1f}..{fbk[2]:.1f}]")
        del blk, eager, x, cot, x2, dg
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
