#!/usr/bin/env python3
"""Times DarkIR's FreMLP on the MI355X at the four EBlock shapes of DarkIR width 32 on 256 x 256 crops (bs 8, bf16 activations,
expand 2): the native module forward and forward + backward beside the eager formulation on the same device (torch.fft, i.e.
rocFFT, plus elementwise passes over complex tensors and autograd: restated here, a comparison inside this tool only, never on the
product path), and the two transforms on their own with the achieved fp32-MFMA rate of their dense-DFT stages.

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
native and the eager windows alternate.  Flops of the DFT stages (K = W/2 + 1, P = B nc planes): r2c = 4 P H W K (real x complex)
+ 8 P H H K (complex x complex); c2r = 8 P H H K + 4 P H K W (real part only).  The forward runs one of each, the backward one of
each again (their adjoints), so a forward + backward runs four times the r2c + c2r pair's flops / 2.

usage: python tools/bench_fremlp.py [--bs 8] [--iters 10] [--repeats 7] [--warmup 3] [--log profiles/fremlp_bench.log]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

SHAPES = ((32, 256), (64, 128), (128, 64), (256, 32))   # (nc, H = W) of DarkIR's encoder levels at a 256 x 256 input
EXPAND = 2


class EagerFreMLP(torch.nn.Module):
    """The reference formulation in plain PyTorch ops: fp32 spectra and parameters around bf16 activations."""

    def __init__(self, nc, expand):
        super().__init__()
        self.process1 = torch.nn.Sequential(torch.nn.Conv2d(nc, expand * nc, 1, 1, 0), torch.nn.LeakyReLU(0.1, inplace=True),
                                            torch.nn.Conv2d(expand * nc, nc, 1, 1, 0))

    def forward(self, x):
        H, W = x.shape[-2:]
        z = torch.fft.rfft2(x.float(), norm="backward")
        mag, pha = torch.abs(z), torch.angle(z)
        mag = self.process1(mag)
        out = torch.fft.irfft2(torch.complex(mag * torch.cos(pha), mag * torch.sin(pha)), s=(H, W), norm="backward")
        return out.to(x.dtype)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed(fns, warmup, iters, repeats):
    """Median (min, max) over `repeats` windows of the mean time of one call (us), for each of `fns`; their windows alternate."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ts[i].append(window(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fremlp: needs the MI355X (no CPU timing)")
    import fremlp_ref as R
    from image_restoration_amd import darkir, ops
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}, bf16 activations, expand {EXPAND}; median of {a.repeats} windows of "
        f"{a.iters} calls [min..max], native and eager windows alternating")
    for nc, hw in SHAPES:
        B, H, W, K = a.bs, hw, hw, hw // 2 + 1
        P = B * nc
        sd = R.make_state(R.fremlp_shapes(nc, EXPAND), 3)
        native = darkir.FreMLP(nc, EXPAND)
        native.load_state_dict(sd)
        native = native.to(dev)
        eager = EagerFreMLP(nc, EXPAND)
        eager.load_state_dict(sd)
        eager = eager.to(dev)
        g = torch.Generator().manual_seed(nc)
        x = torch.randn(B, nc, H, W, generator=g).to(dev).to(torch.bfloat16)
        cot = torch.randn(B, nc, H, W, generator=g).to(dev).to(torch.bfloat16)

        def fwd_only(m):
            with torch.no_grad():
                m(x)

        def fwd_bwd(m):
            xg = x.detach().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            m(xg).backward(cot)

        (nf, ef) = timed([lambda: fwd_only(native), lambda: fwd_only(eager)], a.warmup, a.iters, a.repeats)
        (nb, eb) = timed([lambda: fwd_bwd(native), lambda: fwd_bwd(eager)], a.warmup, a.iters, a.repeats)
        zre, zim = ops.dft2_r2c(x)
        (tr, tc) = timed([lambda: ops.dft2_r2c(x), lambda: ops.dft2_c2r(zre, zim, W, torch.bfloat16)], a.warmup, a.iters, a.repeats)
        f_r2c = 4.0 * P * H * W * K + 8.0 * P * H * H * K
        f_c2r = 8.0 * P * H * H * K + 4.0 * P * H * K * W
        plan = ops.fremlp_plan(B, nc, EXPAND, H, W, torch.bfloat16)
        tag = f"nc={nc:3d} {hw}x{hw}"
        say(f"{tag}  fwd      native {nf[0]:9.1f} us [{nf[1]:.1f}..{nf[2]:.1f}]   eager {ef[0]:9.1f} us [{ef[1]:.1f}..{ef[2]:.1f}]   "
            f"native/eager {nf[0] / ef[0]:.2f}")
        say(f"{tag}  fwd+bwd  native {nb[0]:9.1f} us [{nb[1]:.1f}..{nb[2]:.1f}]   eager {eb[0]:9.1f} us [{eb[1]:.1f}..{eb[2]:.1f}]   "
            f"native/eager {nb[0] / eb[0]:.2f}")
        say(f"{tag}  r2c alone (tables + stages 1, 2) {tr[0]:8.1f} us  {f_r2c / tr[0] / 1e6:6.1f} TFLOP/s fp32 MFMA;  "
            f"c2r alone (tables + stages 3, 4) {tc[0]:8.1f} us  {f_c2r / tc[0] / 1e6:6.1f} TFLOP/s;  "
            f"the rest of the forward (|Z|, two 1x1 products, LeakyReLU, mag' u) {nf[0] - tr[0] - tc[0]:8.1f} us")
        say(f"{tag}  saved {plan['saved_bytes'] / 2**20:.1f} MiB, workspace {plan['workspace'] / 2**20:.1f} MiB, "
            f"grids {plan['grid_rows_k']} / {plan['grid_planes']} / {plan['grid_rows_w']} workgroups")
        del native, eager, x, cot, zre, zim
        torch.cuda.empty_cache()
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
