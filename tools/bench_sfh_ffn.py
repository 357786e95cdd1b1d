#!/usr/bin/env python3
"""Times SFHformer's FFN and TokenMixer_For_Local on the MI355X at the three levels of SFHformer width 32 on a 256 x 256 crop
(dim 32 at 256^2, 64 at 128^2, 128 at 64^2; bs 8), fp32 and bf16 activations, forward and forward + backward:

  native    the modules of image_restoration_amd.sfhformer (one segmented stencil kernel per direction between the 1x1 products)
  eager     the reference classes restated here in plain PyTorch ops, run by PyTorch on the same device in the same dtype
            (a comparison inside this tool only, never on the product path)
  composed  (FFN only) the same mathematics out of ops that exist without the segmented kernels: ops.conv1x1, three contiguous
            slice copies, ops.dwconv_fwd / ops.dwconv_bwd per segment, torch cat and GELU, ops.gram and ops.chan_sum for the 1x1
            gradients.  The depthwise ops have no dilation, so the local mixer has no such composition.

and the two stencil kernels on their own (through the local mixer, which is nothing else, and for the FFN as native minus its 1x1
products timed alone), with the bytes they move over the time beside 6.29 TB/s, the rate a plain device copy has been measured at on the MI355X.

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
windows of the variants alternate.

usage: python tools/bench_sfh_ffn.py [--bs 8] [--iters 10] [--repeats 7] [--warmup 3] [--log profiles/sfh_ffn_bench.log]
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

from bench_fremlp import timed  # noqa: E402

SHAPES = ((32, 256), (64, 128), (128, 64))   # (dim, H = W) of SFHformer's three levels at a 256 x 256 input
COPY_TBS = 6.29                              # a plain device copy, measured on the MI355X


class EagerFFN(nn.Module):
    def __init__(self, dim):
        super().__init__()
        sp = self.dim_sp = dim // 2
        self.conv_init = nn.Sequential(nn.Conv2d(dim, dim * 2, 1))
        self.conv1_1 = nn.Sequential(nn.Conv2d(sp, sp, 3, padding=1, groups=sp))
        self.conv1_2 = nn.Sequential(nn.Conv2d(sp, sp, 5, padding=2, groups=sp))
        self.conv1_3 = nn.Sequential(nn.Conv2d(sp, sp, 7, padding=3, groups=sp))
        self.conv_fina = nn.Sequential(nn.Conv2d(dim * 2, dim, 1))

    def forward(self, x):
        x = list(torch.split(self.conv_init(x), self.dim_sp, dim=1))
        x[1], x[2], x[3] = self.conv1_1(x[1]), self.conv1_2(x[2]), self.conv1_3(x[3])
        return self.conv_fina(F.gelu(torch.cat(x, dim=1)))


class EagerLocal(nn.Module):
    def __init__(self, dim):
        super().__init__()
        sp = dim // 2
        self.CDilated_1 = nn.Conv2d(sp, sp, 3, stride=1, padding=1, dilation=1, groups=sp)
        self.CDilated_2 = nn.Conv2d(sp, sp, 3, stride=1, padding=2, dilation=2, groups=sp)

    def forward(self, x):
        x1, x2 = x.chunk(2, dim=1)
        return torch.cat([self.CDilated_1(x1), self.CDilated_2(x2)], dim=1)


class Composed:
    """The FFN out of the ops that exist without the segmented kernels; backward written out by hand over the same ops."""

    def __init__(self, ops, mod):
        self.ops, self.m = ops, mod

    def forward(self, x, keep):
        ops, m, s = self.ops, self.m, self.m.dim_sp
        h = ops.conv1x1(x, m.conv_init[0].weight, m.conv_init[0].bias)
        segs = [h[:, k * s:(k + 1) * s].contiguous() for k in (1, 2, 3)]
        outs = [ops.dwconv_fwd(t, c[0].weight, c[0].bias) for t, c in zip(segs, (m.conv1_1, m.conv1_2, m.conv1_3))]
        u = torch.cat([h[:, :s]] + outs, dim=1)
        g = F.gelu(u)
        out = ops.conv1x1(g, m.conv_fina[0].weight, m.conv_fina[0].bias)
        return (out, (x, segs, u, g)) if keep else (out, None)

    def backward(self, dout, kept):
        ops, m, s = self.ops, self.m, self.m.dim_sp
        x, segs, u, g = kept
        ops.chan_sum(dout)
        ops.gram(dout, g, sum_batch=True)
        dg = ops.conv1x1(dout, m.conv_fina[0].weight, transposed=True)
        du = torch.ops.aten.gelu_backward(dg, u)
        dh = [du[:, :s]]
        for k, (t, c) in enumerate(zip(segs, (m.conv1_1, m.conv1_2, m.conv1_3)), start=1):
            dh.append(ops.dwconv_bwd(du[:, k * s:(k + 1) * s].contiguous(), t, c[0].weight, True)[0])
        dh = torch.cat(dh, dim=1)
        ops.chan_sum(dh)
        ops.gram(dh, x, sum_batch=True)
        return ops.conv1x1(dh, m.conv_init[0].weight, transposed=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sfh_ffn: needs the MI355X (no CPU timing)")
    import sfh_ffn_ref as R
    from image_restoration_amd import ops, sfhformer
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}; median of {a.repeats} windows of {a.iters} calls (us), the variants' "
        f"windows alternating; TB/s: the stencil kernel's bytes over its time, beside the {COPY_TBS} TB/s copy ceiling")
    say("| module | dim | plane | dtype | pass | native | eager | composed | native/eager | native/composed | stencil kernel us | TB/s |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for dim, hw in SHAPES:
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            B, el = a.bs, 4 if dtype == torch.float32 else 2
            g = torch.Generator().manual_seed(dim)
            x = torch.randn(B, dim, hw, hw, generator=g).to(dev).to(dtype)
            cot = torch.randn(B, dim, hw, hw, generator=g).to(dev).to(dtype)
            for kind, Native, Eager in (("ffn", sfhformer.FFN, EagerFFN), ("local", sfhformer.TokenMixer_For_Local, EagerLocal)):
                sd = R.make_state(kind, dim, 3)
                native, eager = Native(dim), Eager(dim)
                native.load_state_dict(sd)
                eager.load_state_dict(sd)
                native, eager = native.to(dev), eager.to(dev).to(dtype)
                comp = Composed(ops, native) if kind == "ffn" else None
                with torch.no_grad():
                    ye = eager(x).float()
                    d = float((native(x).float() - ye).abs().max() / ye.abs().max())
                    dc = float((comp.forward(x, False)[0].float() - ye).abs().max() / ye.abs().max()) if comp else 0.0
                assert d < (1e-4 if dtype == torch.float32 else 5e-2) and dc < (1e-4 if dtype == torch.float32 else 5e-2), (d, dc)

                def fwd_only(m):
                    with torch.no_grad():
                        m(x)

                def fwd_bwd(m):
                    xg = x.detach().requires_grad_(True)
                    m.zero_grad(set_to_none=True)
                    m(xg).backward(cot)

                def comp_fwd():
                    with torch.no_grad():
                        comp.forward(x, False)

                def comp_fwd_bwd():
                    with torch.no_grad():
                        _, kept = comp.forward(x, True)
                        comp.backward(cot, kept)

                fns_f = [lambda: fwd_only(native), lambda: fwd_only(eager)] + ([comp_fwd] if comp else [])
                fns_b = [lambda: fwd_bwd(native), lambda: fwd_bwd(eager)] + ([comp_fwd_bwd] if comp else [])
                plane = B * (2 * dim if kind == "ffn" else dim) * hw * hw * el
                if kind == "ffn":
                    # the 1x1 products and their gradients alone, on tensors of the same shapes: native minus these is the stencil kernel
                    cf, ci = native.conv_fina[0], native.conv_init[0]
                    with torch.no_grad():
                        hh = ops.conv1x1(x, ci.weight, ci.bias)

                    def pw_fwd():
                        with torch.no_grad():
                            ops.conv1x1(x, ci.weight, ci.bias)
                            ops.conv1x1(hh, cf.weight, cf.bias)

                    def pw_bwd():
                        with torch.no_grad():
                            ops.chan_sum(cot); ops.conv1x1(cot, cf.weight, transposed=True); ops.gram(cot, hh, sum_batch=True)
                            ops.chan_sum(hh); ops.gram(hh, x, sum_batch=True); ops.conv1x1(hh, ci.weight, transposed=True)

                    fns_f.append(pw_fwd)
                    fns_b.append(lambda: (pw_fwd(), pw_bwd()))
                tf = timed(fns_f, a.warmup, a.iters, a.repeats)
                tb = timed(fns_b, a.warmup, a.iters, a.repeats)
                for what, t, passes in (("fwd", tf, 2), ("fwd+bwd", tb, 5 if kind == "local" else 8)):
                    # planes the stencil kernels move: local fwd reads x, writes out (2); bwd reads dout and x, writes dx (3);
                    # FFN inference fwd reads h, writes g (2); training fwd also writes u (3), bwd reads dg, u, h, writes g, dh (5)
                    nat, eag = t[0][0], t[1][0]
                    cmp_ = t[2][0] if comp else float("nan")
                    kern = nat - t[-1][0] if kind == "ffn" else nat
                    say(f"| {kind} | {dim} | {hw}x{hw} | {tag} | {what} | {nat:.1f} | {eag:.1f} | {cmp_:.1f} | {nat / eag:.2f} | "
                        f"{nat / cmp_:.2f} | {kern:.1f} | {passes * plane / max(kern, 1e-9) / 1e6:.2f} |")
                del native, eager, comp
            del x, cot
            torch.cuda.empty_cache()
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
