#!/usr/bin/env python3
"""Times SFHformer's Stage node against the chain of public modules it replaces, on the MI355X, at the three levels of SFHformer
width 32 on a 256 x 256 crop (dim 32 at 256^2, 64 at 128^2, 128 at 64^2; bs 8), fp32 and bf16 activations, forward (no_grad) and
forward + backward, all in this one process:

  (a) node    image_restoration_amd.sfhformer.Stage(depth, dim): ONE autograd node over mi_sfh_block_* for the whole run of Blocks
  (b) chain   the same module's parameters through BatchNorm2d -> Mixer -> scaled_residual -> BatchNorm2d -> FFN -> scaled_residual
              per Block: six autograd nodes and six module-op paths per Block, one statistics pass more per BatchNorm

then one SFHformer_s training step (forward, L1 loss, backward) at bs x 3 x 256^2 in both dtypes, the network as it is against the
same glue with every Stage run as chain (b).  Both contenders run the same kernels on the same parameters; before timing their
outputs are held equal bit for bit.

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows with the
fastest and slowest window beside it (the run-to-run spread); the windows of the contenders alternate.

usage: python tools/bench_sfh_block.py [--bs 8] [--depth 2] [--iters 10] [--repeats 7] [--warmup 3] [--skip-net]
                                       [--log profiles/sfh_block_bench.log]
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
from bench_sfh_mixer import SHAPES  # noqa: E402


def chain_stage(N, stage, x):
    for blk in stage.blocks:
        x1 = N.scaled_residual(blk.mixer(blk.norm1(x)), x, blk.beta)
        x = N.scaled_residual(blk.ffn(blk.norm2(x1)), x1, blk.gamma)
    return x


def chain_net(N, net, x):
    copy0 = x
    copy1 = x = chain_stage(N, net.layer1, net.patch_embed(x))
    copy2 = x = chain_stage(N, net.layer2, net.downsample1(x))
    x = chain_stage(N, net.layer3, net.downsample2(x))
    x = chain_stage(N, net.layer8, N._up_skip(net.upsample3, x, copy2, net.skip2))
    x = chain_stage(N, net.layer9, N._up_skip(net.upsample4, x, copy1, net.skip1))
    return net.patch_unembed(x, copy0)


def seed_scales(mod, g):
    """beta and gamma of order 1 (the reference initialises them to 0, which makes a Block the identity)."""
    with torch.no_grad():
        for k, p in mod.named_parameters():
            if k.rsplit(".", 1)[-1] in ("beta", "gamma"):
                p.copy_((0.5 + torch.rand(p.shape, generator=g)).to(p.device))


def row(t):
    med, lo, hi = t
    return f"{med:.0f} ({lo:.0f}..{hi:.0f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sfh_block: needs the MI355X (no CPU timing)")
    from image_restoration_amd import sfhformer as N
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}; Stage depth {a.depth}; median (fastest..slowest) of {a.repeats} windows of "
        f"{a.iters} calls, us per call, the contenders' windows alternating")
    say("| dim | plane | dtype | pass | (a) node | (b) chain | a/b |")
    say("|---|---|---|---|---|---|---|")
    for dim, hw in SHAPES:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            g = torch.Generator().manual_seed(dim)
            stage = N.Stage(a.depth, dim).to(dev).train()
            seed_scales(stage, g)
            x, cot = (torch.randn(a.bs, dim, hw, hw, generator=g).to(dev).to(dtype) for _ in range(2))
            with torch.no_grad():
                assert torch.equal(stage(x), chain_stage(N, stage, x))

            def fwd(f):
                with torch.no_grad():
                    f(x)

            def fwd_bwd(f):
                xg = x.detach().requires_grad_(True)
                stage.zero_grad(set_to_none=True)
                f(xg).backward(cot)

            fns = (stage, lambda t: chain_stage(N, stage, t))
            for what, run in (("fwd", fwd), ("fwd+bwd", fwd_bwd)):
                ta, tb = timed([lambda f=f: run(f) for f in fns], a.warmup, a.iters, a.repeats)
                say(f"| {dim} | {hw}x{hw} | {tag} | {what} | {row(ta)} | {row(tb)} | {ta[0] / tb[0]:.3f} |")
            del stage, x, cot
            torch.cuda.empty_cache()
    if not a.skip_net:
        say("")
        say(f"SFHformer_s, one training step (forward, L1 loss, backward) at {a.bs} x 3 x 256 x 256, ms per step")
        say("| dtype | (a) Stage nodes | (b) module chains | a/b |")
        say("|---|---|---|---|")
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            g = torch.Generator().manual_seed(7)
            net = N.SFHformer_s().to(dev).train()
            seed_scales(net, g)
            x, tgt = (torch.rand(a.bs, 3, 256, 256, generator=g).to(dev).to(dtype) for _ in range(2))
            with torch.no_grad():
                assert torch.equal(net(x), chain_net(N, net, x))

            def step(f):
                net.zero_grad(set_to_none=True)
                (f(x) - tgt).abs().mean().backward()

            ta, tb = timed([lambda: step(net), lambda: step(lambda t: chain_net(N, net, t))], a.warmup, max(a.iters // 2, 2), a.repeats)
            ms = lambda t: f"{t[0] / 1e3:.2f} ({t[1] / 1e3:.2f}..{t[2] / 1e3:.2f})"   # noqa: E731
            say(f"| {tag} | {ms(ta)} | {ms(tb)} | {ta[0] / tb[0]:.3f} |")
            del net, x, tgt
            torch.cuda.empty_cache()
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
