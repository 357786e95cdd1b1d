#!/usr/bin/env python3
"""Times the SFHformer Block's BatchNorm2d and scaled residual on the MI355X at the three levels of SFHformer width 32 on a 256 x 256
crop (C 32 at 256^2, 64 at 128^2, 128 at 64^2; bs 8), fp32 and bf16 activations, forward (no_grad) and forward + backward, all in
this one process:

  (a) native BN   image_restoration_amd.sfhformer.BatchNorm2d in training mode (one autograd node over mi_bn2d_*)
  (b) torch BN    torch.nn.BatchNorm2d on the same device in the same dtype (a comparison inside this tool only)
  (c) native res  image_restoration_amd.sfhformer.scaled_residual (one autograd node over mi_scale_res_*)
  (d) eager res   f * s + x in plain PyTorch ops
  (e) scale_add   mi_scale_add_* with p2 = 1 (AdaIR's out * p1 + y * p2), the only a p[c] + y the library had, under an autograd
                  node of this tool

and, from a torch.profiler pass, each streaming kernel of csrc/bn2d.hip on its own with the bytes the algorithm needs over its time,
beside 6.29 TB/s, the rate a plain device copy has been measured at on the MI355X: the statistics pass reads 1 plane of [B, C, N],
the apply pass moves 2, the backward's sum pass 2, its dx pass 3 (4 with dres), the residual's forward and backward 3 each; the
per-channel finish kernels are listed with their time only.

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
windows of the variants alternate.

usage: python tools/bench_bn2d.py [--bs 8] [--iters 20] [--repeats 7] [--warmup 3] [--log profiles/bn2d_bench.log]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

from bench_fremlp import timed  # noqa: E402
from bench_sfh_mixer import COPY_TBS, SHAPES, kernel_times  # noqa: E402

# kernel -> planes of [B, C, N] the algorithm moves
STREAMS = (("bn_stats_kernel", 1), ("bn_apply_kernel", 2), ("bn_bwd_sums_kernel", 2), ("bn_bwd_dx_kernel", 3), ("sr_fwd_kernel", 3),
           ("sr_bwd_kernel", 3))
FINISH = ("bn_finish_kernel", "bn_bwd_finish_kernel", "sr_finish_kernel")


def make_scale_add(ops):
    class ScaleAdd(torch.autograd.Function):
        """f * p1 + x * p2 through mi_scale_add_*; p2 is a constant 1 whose gradient is computed and dropped."""

        @staticmethod
        def forward(ctx, f, x, p1, p2):
            ctx.save_for_backward(f, x, p1, p2)
            return ops.scale_add_fwd(f, x, p1, p2)

        @staticmethod
        def backward(ctx, dout):
            f, x, p1, p2 = ctx.saved_tensors
            dp1, dp2 = torch.empty_like(p1), torch.empty_like(p2)
            df, dx = ops.scale_add_bwd(f, x, p1, p2, dout.contiguous(), dp1, dp2, False)
            return df, dx, dp1, None

    return ScaleAdd.apply


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bn2d: needs the MI355X (no CPU timing)")
    from image_restoration_amd import ops, sfhformer
    dev = torch.device("cuda:0")
    scale_add = make_scale_add(ops)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}; median of {a.repeats} windows of {a.iters} calls (us), the variants' "
        f"windows alternating; TB/s: a kernel's algorithmic bytes over its time, beside the {COPY_TBS} TB/s copy ceiling")
    say("| C | plane | dtype | pass | (a) native BN | (b) torch BN | a/b | (c) native res | (d) eager res | (e) scale_add | c/d | c/e |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    kernel_rows = []
    for Cn, hw in SHAPES:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            B, el = a.bs, 4 if dtype == torch.float32 else 2
            g = torch.Generator().manual_seed(Cn)
            x, f, cot = (torch.randn(B, Cn, hw, hw, generator=g).to(dev).to(dtype) for _ in range(3))
            native, eager = sfhformer.BatchNorm2d(Cn).to(dev).train(), torch.nn.BatchNorm2d(Cn).to(dev).train()
            w0, b0 = 1.0 + 0.3 * torch.randn(Cn, generator=g), 0.1 * torch.randn(Cn, generator=g)
            with torch.no_grad():
                for m in (native, eager):
                    m.weight.copy_(w0)
                    m.bias.copy_(b0)
            s = torch.nn.Parameter((0.5 * torch.randn(1, Cn, 1, 1, generator=g)).to(dev))
            ones = torch.ones(Cn, device=dev)
            with torch.no_grad():
                ye = eager(x).float()
                d = float((native(x).float() - ye).abs().max() / ye.abs().max())
                oe = (f * s.to(dtype) + x).float()
                d2 = float((sfhformer.scaled_residual(f, x, s).float() - oe).abs().max() / oe.abs().max())
                d3 = float((scale_add(f, x, s.view(-1), ones).float() - oe).abs().max() / oe.abs().max())
            tol = 1e-5 if dtype == torch.float32 else 2e-2
            assert d < tol and d2 < tol and d3 < tol, (d, d2, d3)

            def bn_fwd(m):
                with torch.no_grad():
                    m(x)

            def bn_fwd_bwd(m):
                xg = x.detach().requires_grad_(True)
                m.zero_grad(set_to_none=True)
                m(xg).backward(cot)

            def res(kind, fg, xg):
                if kind == "native":
                    return sfhformer.scaled_residual(fg, xg, s)
                if kind == "eager":
                    return fg * s.to(dtype) + xg
                return scale_add(fg, xg, s.view(-1), ones)

            def res_fwd(kind):
                with torch.no_grad():
                    res(kind, f, x)

            def res_fwd_bwd(kind):
                fg, xg = f.detach().requires_grad_(True), x.detach().requires_grad_(True)
                s.grad = None
                res(kind, fg, xg).backward(cot)

            kinds = ("native", "eager", "scale_add")
            tf = timed([lambda: bn_fwd(native), lambda: bn_fwd(eager)] + [lambda k=k: res_fwd(k) for k in kinds], a.warmup, a.iters, a.repeats)
            tb = timed([lambda: bn_fwd_bwd(native), lambda: bn_fwd_bwd(eager)] + [lambda k=k: res_fwd_bwd(k) for k in kinds], a.warmup,
                       a.iters, a.repeats)
            for what, t in (("fwd", tf), ("fwd+bwd", tb)):
                na, to, rn, re_, rs = (t[i][0] for i in range(5))
                say(f"| {Cn} | {hw}x{hw} | {tag} | {what} | {na:.1f} | {to:.1f} | {na / to:.2f} | {rn:.1f} | {re_:.1f} | {rs:.1f} | {rn / re_:.2f} | "
                    f"{rn / rs:.2f} |")

            # per kernel: one profiler pass over both native nodes, one over the backward with dres
            def both():
                bn_fwd_bwd(native)
                res_fwd_bwd("native")

            kt = kernel_times(both, [n for n, _ in STREAMS] + list(FINISH))
            w, rm, rv = native.weight.detach(), native.running_mean.clone(), native.running_var.clone()
            _, stat = ops.bn2d_fwd(x, w, native.bias.detach(), rm, rv, True, True)
            grads = (torch.empty_like(w), torch.empty_like(w))
            kd = kernel_times(lambda: ops.bn2d_bwd(x, cot, w, stat, grads, False, True, dres=f), ["bn_bwd_dx_kernel"])
            plane = B * Cn * hw * hw * el
            row = [f"{Cn}", f"{hw}x{hw}", tag]
            for n, planes in STREAMS + (("dres", 4),):
                us = kd["bn_bwd_dx_kernel"][0] if n == "dres" else kt[n][0]
                row += [f"{us:.1f}", f"{planes * plane / us / 1e6:.2f}"]
            row += [f"{kt[n][0]:.1f}" for n in FINISH]
            kernel_rows.append("| " + " | ".join(row) + " |")
            del native, eager, x, f, cot
            torch.cuda.empty_cache()
    say("")
    say("| C | plane | dtype | stats us | TB/s | apply us | TB/s | bwd sums us | TB/s | bwd dx us | TB/s | res fwd us | TB/s | res bwd us | TB/s | "
        "bwd dx + dres us | TB/s | bn finish us | bn bwd finish us | res finish us |")
    say("|" + "---|" * 20)
    for r in kernel_rows:
        say(r)
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
