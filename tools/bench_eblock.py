#!/usr/bin/env python3
"""Times DarkIR's EBlock, its tail kernels and the DarkIR-m network on the MI355X (bs 8, bf16 activations), at the four encoder
shapes of width 32 on 256 x 256 crops:

  tail     mi_fregate_fwd / mi_fregate_bwd beside mi_ewise_fwd / mi_ewise_bwd (op 0, a * b) on the same planes: the sibling that
           moves almost the same bytes (forward 3 planes either way; backward 5 planes either way, fregate also writes its
           per-workgroup partial rows and runs their row sum).  GB/s are algorithmic bytes over the time.
  block    EBlock forward (no_grad) and forward + backward, native beside eager: the reference formulation restated here in
           plain PyTorch ops (torch.fft, vendor convolutions, autograd) - a comparison inside this tool only, never on the
           product path.
  network  one DarkIR-m training step (forward with side_loss, L1 on both outputs, backward) at 256 x 256, native beside eager.
  saved    the saved-blob sections and the workspace of the block (mi_eblock_plan).

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
native and the eager windows alternate.

usage: python tools/bench_eblock.py [--bs 8] [--iters 10] [--repeats 7] [--warmup 3] [--skip-net] [--log profiles/eblock_bench.log]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

from bench_fremlp import EagerFreMLP, timed  # noqa: E402

SHAPES = ((32, 256), (64, 128), (128, 64), (256, 32))   # (c, H = W) of DarkIR's encoder levels at a 256 x 256 input


class EagerLN2d(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(c)), nn.Parameter(torch.zeros(c))

    def forward(self, x):
        xf = x.float()
        mu = xf.mean(1, keepdim=True)
        var = (xf - mu).pow(2).mean(1, keepdim=True)
        return ((xf - mu) / (var + 1e-6).sqrt() * self.weight.view(1, -1, 1, 1) + self.bias.view(1, -1, 1, 1)).to(x.dtype)


class EagerBranch(nn.Module):
    def __init__(self, c, d):
        super().__init__()
        self.branch = nn.Sequential(nn.Conv2d(c, c, 3, padding=d, groups=c, dilation=d))

    def forward(self, x):
        return self.branch(x)


def _gate(x):
    a, b = x.chunk(2, dim=1)
    return a * b


class EagerEBlock(nn.Module):
    """arch_model.py:141-204 in plain PyTorch ops, parameters cast to the activation dtype per call (autocast-free)."""

    def __init__(self, c, dilations=(1,), extra_depth_wise=False):
        super().__init__()
        self.extra_conv = nn.Conv2d(c, c, 3, padding=1, groups=c) if extra_depth_wise else nn.Identity()
        self.conv1 = nn.Conv2d(c, 2 * c, 1)
        self.branches = nn.ModuleList([EagerBranch(2 * c, d) for d in dilations])
        self.sca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(c, c, 1))
        self.conv3 = nn.Conv2d(c, c, 1)
        self.norm1, self.norm2 = EagerLN2d(c), EagerLN2d(c)
        self.freq = EagerFreMLP(c, 2)
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)))
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)))

    def forward(self, inp):
        with torch.autocast("cuda", dtype=inp.dtype, enabled=inp.dtype != torch.float32):
            x = self.conv1(self.extra_conv(self.norm1(inp)))
            z = 0
            for b in self.branches:
                z = z + b(x)
            z = _gate(z)
            y = inp + self.beta.to(inp.dtype) * self.conv3(self.sca(z) * z)
        f = self.freq(self.norm2(y))
        return y + (y * f) * self.gamma.to(inp.dtype)


class EagerDBlock(nn.Module):
    def __init__(self, c, dilations=(1, 4, 9), extra_depth_wise=True):
        super().__init__()
        self.conv1 = nn.Conv2d(c, 2 * c, 1)
        self.extra_conv = nn.Conv2d(2 * c, 2 * c, 3, padding=1, groups=c) if extra_depth_wise else nn.Identity()
        self.branches = nn.ModuleList([EagerBranch(2 * c, d) for d in dilations])
        self.sca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(c, c, 1))
        self.conv3 = nn.Conv2d(c, c, 1)
        self.conv4 = nn.Conv2d(c, 2 * c, 1)
        self.conv5 = nn.Conv2d(c, c, 1)
        self.norm1, self.norm2 = EagerLN2d(c), EagerLN2d(c)
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)))
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)))

    def forward(self, inp):
        with torch.autocast("cuda", dtype=inp.dtype, enabled=inp.dtype != torch.float32):
            x = self.extra_conv(self.conv1(self.norm1(inp)))
            z = 0
            for b in self.branches:
                z = z + b(x)
            z = _gate(z)
            y = inp + self.beta.to(inp.dtype) * self.conv3(self.sca(z) * z)
            x = self.conv5(_gate(self.conv4(self.norm2(y))))
            return y + x * self.gamma.to(inp.dtype)


class EagerSeq(nn.Module):
    def __init__(self, *mods):
        super().__init__()
        self.modules_list = nn.ModuleList(mods)

    def forward(self, x):
        for m in self.modules_list:
            x = m(x)
        return x


class EagerDarkIR(nn.Module):
    """archs/DarkIR.py with the eager blocks above; the same state_dict as the native network."""

    def __init__(self, img_channel=3, width=32, middle_blk_num_enc=2, middle_blk_num_dec=2, enc_blk_nums=(1, 2, 3),
                 dec_blk_nums=(3, 1, 1), dilations=(1, 4, 9), extra_depth_wise=True):
        super().__init__()
        self.intro = nn.Conv2d(img_channel, width, 3, padding=1)
        self.ending = nn.Conv2d(width, img_channel, 3, padding=1)
        self.encoders, self.decoders, self.ups, self.downs = nn.ModuleList(), nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        chan = width
        for num in enc_blk_nums:
            self.encoders.append(EagerSeq(*[EagerEBlock(chan, extra_depth_wise=extra_depth_wise) for _ in range(num)]))
            self.downs.append(nn.Conv2d(chan, 2 * chan, 2, 2))
            chan *= 2
        self.middle_blks_enc = EagerSeq(*[EagerEBlock(chan, extra_depth_wise=extra_depth_wise) for _ in range(middle_blk_num_enc)])
        self.middle_blks_dec = EagerSeq(*[EagerDBlock(chan, dilations, extra_depth_wise) for _ in range(middle_blk_num_dec)])
        for num in dec_blk_nums:
            self.ups.append(nn.Sequential(nn.Conv2d(chan, chan * 2, 1, bias=False), nn.PixelShuffle(2)))
            chan //= 2
            self.decoders.append(EagerSeq(*[EagerDBlock(chan, dilations, extra_depth_wise) for _ in range(num)]))
        self.side_out = nn.Conv2d(width * 2 ** len(enc_blk_nums), img_channel, 3, padding=1)

    def forward(self, inp, side_loss=False):
        with torch.autocast("cuda", dtype=inp.dtype, enabled=inp.dtype != torch.float32):
            x = self.intro(inp)
            skips = []
            for enc, down in zip(self.encoders, self.downs):
                x = enc(x)
                skips.append(x)
                x = down(x)
            x_light = self.middle_blks_enc(x)
            out_side = self.side_out(x_light) if side_loss else None
            x = self.middle_blks_dec(x_light) + x_light
            for dec, up, skip in zip(self.decoders, self.ups, skips[::-1]):
                x = dec(up(x) + skip)
            out = self.ending(x) + inp
        return (out_side, out) if side_loss else out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-net", action="store_true")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eblock: needs the MI355X (no CPU timing)")
    import eblock_ref as E
    from image_restoration_amd import darkir, ops
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def fmt(t):
        return f"{t[0]:9.1f} us [{t[1]:.1f}..{t[2]:.1f}]"

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}, bf16 activations; median of {a.repeats} windows of {a.iters} calls "
        f"[min..max], native and eager (or sibling) windows alternating")
    for c, hw in SHAPES:
        B, H, W = a.bs, hw, hw
        tag = f"c={c:3d} {hw}x{hw}"
        g = torch.Generator().manual_seed(c)
        x, cot, f = (torch.randn(B, c, H, W, generator=g).to(dev).to(bf) for _ in range(3))
        gamma = torch.randn(c, generator=g).to(dev)
        dgam = torch.empty_like(gamma)
        n_bytes = B * c * H * W * 2
        (tf, ef) = timed([lambda: ops.fregate_fwd(x, f, gamma), lambda: ops.ewise_fwd(x, f, 0)], a.warmup, a.iters, a.repeats)
        (tb, eb) = timed([lambda: ops.fregate_bwd(cot, x, f, gamma, dgam, False), lambda: ops.ewise_bwd(x, f, cot, 0)], a.warmup, a.iters,
                         a.repeats)
        say(f"{tag}  tail fwd  fregate {fmt(tf)} {3 * n_bytes / tf[0] / 1e3:7.1f} GB/s   ewise {fmt(ef)} {3 * n_bytes / ef[0] / 1e3:7.1f} GB/s   "
            f"fregate/ewise {tf[0] / ef[0]:.2f}")
        say(f"{tag}  tail bwd  fregate {fmt(tb)} {5 * n_bytes / tb[0] / 1e3:7.1f} GB/s   ewise {fmt(eb)} {5 * n_bytes / eb[0] / 1e3:7.1f} GB/s   "
            f"fregate/ewise {tb[0] / eb[0]:.2f}   (fregate: kernel + the row sum of its partials)")
        sd = E.make_state(E.eblock_shapes(c, 1, True), 3)
        native = darkir.EBlock(c, extra_depth_wise=True)
        native.load_state_dict(sd)
        native = native.to(dev)
        eager = EagerEBlock(c, (1,), True)
        eager.load_state_dict(sd)
        eager = eager.to(dev)

        def fwd_only(m):
            with torch.no_grad():
                m(x)

        def fwd_bwd(m):
            xg = x.detach().requires_grad_(True)
            m.zero_grad(set_to_none=True)
            m(xg).backward(cot)

        (nf, ef) = timed([lambda: fwd_only(native), lambda: fwd_only(eager)], a.warmup, a.iters, a.repeats)
        (nb, eb) = timed([lambda: fwd_bwd(native), lambda: fwd_bwd(eager)], a.warmup, a.iters, a.repeats)
        say(f"{tag}  block fwd      native {fmt(nf)}   eager {fmt(ef)}   native/eager {nf[0] / ef[0]:.2f}")
        say(f"{tag}  block fwd+bwd  native {fmt(nb)}   eager {fmt(eb)}   native/eager {nb[0] / eb[0]:.2f}")
        p = ops.eblock_plan(B, c, H, W, bf, (1,), True)
        mib = 2.0 ** 20
        say(f"{tag}  saved {p['saved_bytes'] / mib:.1f} MiB = planes x0 {p['x0_bytes'] / mib:.1f} + xe {p['xe_bytes'] / mib:.1f} + x1 "
            f"{p['x1_bytes'] / mib:.1f} + g {p['g_bytes'] / mib:.1f} + y {p['y_bytes'] / mib:.1f} + f {p['f_bytes'] / mib:.1f}, statistics "
            f"{p['stats_bytes'] / mib:.1f}, small {p['small_bytes'] / mib:.1f}, FreMLP blob {p['fremlp_blob_bytes'] / mib:.1f} "
            f"({p['fremlp_blob_bytes'] / p['x0_bytes']:.2f} x the input); workspace {p['workspace'] / mib:.1f} MiB; calls "
            f"{p['calls_fwd']} fwd / {p['calls_bwd']} bwd")
        del native, eager, x, cot, f
        torch.cuda.empty_cache()
    if not a.skip_net:
        sd = E.make_state(E.net_shapes(E.net_config()), 5)
        native = darkir.DarkIR()
        native.load_state_dict(sd)
        native = native.to(dev).train()
        eager = EagerDarkIR()
        eager.load_state_dict(sd, strict=True)
        eager = eager.to(dev).train()
        g = torch.Generator().manual_seed(1)
        x = torch.rand(a.bs, 3, 256, 256, generator=g).to(dev).to(bf)
        tgt = torch.rand(a.bs, 3, 256, 256, generator=g).to(dev).to(bf)
        tgt_side = F.avg_pool2d(tgt.float(), 8).to(bf)

        def step(m):
            m.zero_grad(set_to_none=True)
            side, out = m(x, side_loss=True)
            ((out - tgt).abs().mean() + (side - tgt_side).abs().mean()).backward()

        (tn, te) = timed([lambda: step(native), lambda: step(eager)], max(a.warmup - 1, 1), max(a.iters // 2, 1), a.repeats)
        say(f"DarkIR-m 256x256 training step (fwd with side_loss + L1 + bwd)  native {tn[0] / 1e3:8.2f} ms [{tn[1] / 1e3:.2f}..{tn[2] / 1e3:.2f}]   "
            f"eager {te[0] / 1e3:8.2f} ms [{te[1] / 1e3:.2f}..{te[2] / 1e3:.2f}]   native/eager {tn[0] / te[0]:.2f}")
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
