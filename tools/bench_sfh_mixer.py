#!/usr/bin/env python3
"""Times SFHformer's Mixer on the MI355X at the three levels of SFHformer width 32 on a 256 x 256 crop (dim 32 at 256^2, 64 at
128^2, 128 at 64^2; bs 8), fp32 and bf16 activations, forward and forward + backward:

  native    image_restoration_amd.sfhformer.Mixer (one autograd node over mi_sfh_mixer_*)
  eager     the reference classes restated here in plain PyTorch ops (torch.fft, nn.Conv2d, nn.BatchNorm2d), run by PyTorch on the
            same device in the same dtype (a comparison inside this tool only, never on the product path)
  composed  the reference's Mixer wiring out of what the package had before mi_sfh_mixer_*: its FourierUnit and
            TokenMixer_For_Local modules, ops.conv1x1 (with ops.gram / ops.chan_sum for its gradients) for every 1x1 conv over
            the plane, and torch for the rest (split, cat, GELU, the residual add, the pool, the gate and the full-plane multiply).
            This is the yardstick: what a user could run before.

beside them the FourierUnit inside the module timed alone on an input of its shape (native and composed run it through the same
kernels), and, from a torch.profiler pass over the native module, the tail's two streaming kernels on their own with the bytes they move
over their time beside 6.29 TB/s, the rate a plain device copy has been measured at on the MI355X: the tail-in pass (reads l and
u2, writes g: 4 planes of [B, dim, N]; the mean over its two launches per forward + backward, the forward's and the backward's
recomputation of g) and the tail's backward pass (reads e, l and u2, writes dl and du2: 6 planes).

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
windows of the variants alternate.

usage: python tools/bench_sfh_mixer.py [--bs 8] [--iters 10] [--repeats 7] [--warmup 3] [--log profiles/sfh_mixer_bench.log]
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
from bench_sfh_ffn import EagerLocal  # noqa: E402

SHAPES = ((32, 256), (64, 128), (128, 64))   # (dim, H = W) of SFHformer's three levels at a 256 x 256 input
COPY_TBS = 6.29                              # a plain device copy, measured on the MI355X


class EagerFourierUnit(nn.Module):
    def __init__(self, c, groups=4):
        super().__init__()
        self.groups = groups
        self.bn = nn.BatchNorm2d(c * 2)
        self.fdc = nn.Conv2d(c * 2, c * 2 * groups, 1, groups=groups)
        self.weight = nn.Sequential(nn.Conv2d(c * 2, groups, 1), nn.Softmax(dim=1))
        self.fpe = nn.Conv2d(c * 2, c * 2, 3, padding=1, groups=c * 2)

    def forward(self, x):
        B, c, H, W = x.shape
        z = torch.fft.rfft2(x.float(), norm="ortho")
        t = torch.stack([z.real, z.imag], dim=2).reshape(B, 2 * c, H, -1).to(x.dtype)
        t = self.bn(t)
        t = self.fpe(t) + t
        s = self.weight(t)
        u = self.fdc(t).view(B, self.groups, 2 * c, H, -1)
        o = F.gelu(torch.einsum("ijkml,ijml->ikml", u, s)).view(B, c, 2, H, -1).float()
        return torch.fft.irfft2(torch.complex(o[:, :, 0], o[:, :, 1]), s=(H, W), norm="ortho").to(x.dtype)


class EagerGloal(nn.Module):
    def __init__(self, dim, ffc=None):
        super().__init__()
        self.conv_init = nn.Sequential(nn.Conv2d(dim, dim * 2, 1), nn.GELU())
        self.conv_fina = nn.Sequential(nn.Conv2d(dim * 2, dim, 1), nn.GELU())
        self.FFC = ffc if ffc is not None else EagerFourierUnit(dim * 2)

    def forward(self, x):
        x = self.conv_init(x)
        return self.conv_fina(self.FFC(x) + x)


class EagerMixer(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.mixer_local = EagerLocal(dim)
        self.mixer_gloal = EagerGloal(dim)
        self.ca_conv = nn.Sequential(nn.Conv2d(2 * dim, dim, 1))
        self.ca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(2 * dim, dim, 1), nn.ReLU(inplace=True), nn.Conv2d(dim, 2 * dim, 1),
                                nn.Sigmoid())
        self.conv_init = nn.Sequential(nn.Conv2d(dim, 2 * dim, 1))

    def forward(self, x):
        x = list(torch.split(self.conv_init(x), self.dim, dim=1))
        x = F.gelu(torch.cat([self.mixer_local(x[0]), self.mixer_gloal(x[1])], dim=1))
        return self.ca_conv(self.ca(x) * x)


def make_conv1x1(ops):
    class Conv1x1(torch.autograd.Function):
        """ops.conv1x1 with its gradients out of ops.gram, ops.chan_sum and the transposed product."""

        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return ops.conv1x1(x, w, b)

        @staticmethod
        def backward(ctx, dy):
            x, w = ctx.saved_tensors
            dy = dy.contiguous()
            dw = ops.gram(dy, x, sum_batch=True).view_as(w)
            return ops.conv1x1(dy, w, transposed=True), dw, ops.chan_sum(dy)

    return Conv1x1.apply


class ComposedMixer(nn.Module):
    """The reference's wiring over the package's FourierUnit and TokenMixer_For_Local modules and ops.conv1x1; parameters are those
    of a native Mixer (shared, not copied)."""

    def __init__(self, ops, sfhformer, native):
        super().__init__()
        self.n, self.dim, self.conv = native, native.dim, make_conv1x1(ops)
        self.local = sfhformer.TokenMixer_For_Local(native.dim)
        self.local.CDilated_1, self.local.CDilated_2 = native.mixer_local.CDilated_1, native.mixer_local.CDilated_2
        self.ffc = native.mixer_gloal.FFC

    def forward(self, x):
        n, g, dim = self.n, self.n.mixer_gloal, self.dim
        h = self.conv(x, n.conv_init[0].weight, n.conv_init[0].bias)
        a, b = h[:, :dim].contiguous(), h[:, dim:].contiguous()
        p = F.gelu(self.conv(b, g.conv_init[0].weight, g.conv_init[0].bias))
        r = self.ffc(p) + p
        q = F.gelu(self.conv(r, g.conv_fina[0].weight, g.conv_fina[0].bias))
        t = F.gelu(torch.cat([self.local(a), q], dim=1))
        return self.conv((n.ca(t.float()).to(t.dtype) * t), n.ca_conv[0].weight, n.ca_conv[0].bias)


def kernel_times(fn, names, iters=5):
    """{name: (mean device time in us of the kernels whose name contains it, their launches per call of fn)} over `iters` calls of
    fn, from a torch.profiler pass.  A name that matches no kernel is an error: the figures quoted from this tool must not go
    silently empty when a kernel is renamed."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = {}
    for n in names:
        dur = [e.device_time for e in prof.events() if n in e.name]
        if not dur or len(dur) % iters:
            raise SystemExit(f"bench_sfh_mixer: {len(dur)} launches of a kernel named *{n}* in {iters} calls")
        out[n] = (sum(dur) / len(dur), len(dur) // iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dims", default="32,64,128")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sfh_mixer: needs the MI355X (no CPU timing)")
    import sfh_mixer_ref as R
    from image_restoration_amd import ops, sfhformer
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}; median of {a.repeats} windows of {a.iters} calls (us), the variants' "
        f"windows alternating; TB/s: a kernel's bytes over its time, beside the {COPY_TBS} TB/s copy ceiling")
    say("| dim | plane | dtype | pass | native | eager | composed | native/eager | native/composed | FourierUnit alone | tail-in us | TB/s | "
        "tail-back us | TB/s |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    dims = {int(d) for d in a.dims.split(",")}
    for dim, hw in SHAPES:
        if dim not in dims:
            continue
        for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
            B, el = a.bs, 4 if dtype == torch.float32 else 2
            g = torch.Generator().manual_seed(dim)
            x = torch.randn(B, dim, hw, hw, generator=g).to(dev).to(dtype)
            cot = torch.randn(B, dim, hw, hw, generator=g).to(dev).to(dtype)
            sd = R.module_state("mixer", R.make_state("mixer", dim, 3))
            native, eager = sfhformer.Mixer(dim), EagerMixer(dim)
            native.load_state_dict(sd)
            eager.load_state_dict(sd)
            native, eager = native.to(dev), eager.to(dev).to(dtype)
            comp = ComposedMixer(ops, sfhformer, native)
            with torch.no_grad():
                ye = eager(x).float()
                d = float((native(x).float() - ye).abs().max() / ye.abs().max())
                dc = float((comp(x).float() - ye).abs().max() / ye.abs().max())
            tol = 1e-4 if dtype == torch.float32 else 5e-2
            assert d < tol and dc < tol, (d, dc)

            def fwd_only(m):
                with torch.no_grad():
                    m(x)

            def fwd_bwd(m):
                xg = x.detach().requires_grad_(True)
                m.zero_grad(set_to_none=True)
                m(xg).backward(cot)

            # the FourierUnit inside, alone, on an input of p's shape: the part native and composed run through the same kernels
            fu = native.mixer_gloal.FFC
            xp = torch.randn(B, 2 * dim, hw, hw, generator=g).to(dev).to(dtype)

            def fu_fwd():
                with torch.no_grad():
                    fu(xp)

            def fu_fwd_bwd():
                xg = xp.detach().requires_grad_(True)
                fu.zero_grad(set_to_none=True)
                fu(xg).backward(xp)

            tf = timed([lambda: fwd_only(native), lambda: fwd_only(eager), lambda: fwd_only(comp), fu_fwd], a.warmup, a.iters, a.repeats)
            tb = timed([lambda: fwd_bwd(native), lambda: fwd_bwd(eager), lambda: fwd_bwd(comp), fu_fwd_bwd], a.warmup, a.iters, a.repeats)
            kt = kernel_times(lambda: fwd_bwd(native), ("sm_tail_in", "sm_tail_back"))
            plane = B * dim * hw * hw * el

            def rate(k, planes):
                return f"{kt[k][0]:.1f}", f"{planes * plane / kt[k][0] / 1e6:.2f}"

            for what, t in (("fwd", tf), ("fwd+bwd", tb)):
                nat, eag, cmp_ = t[0][0], t[1][0], t[2][0]
                ti, tbk = rate("sm_tail_in", 4), rate("sm_tail_back", 6)
                say(f"| {dim} | {hw}x{hw} | {tag} | {what} | {nat:.1f} | {eag:.1f} | {cmp_:.1f} | {nat / eag:.2f} | {nat / cmp_:.2f} | "
                    f"{t[3][0]:.1f} | {ti[0]} | {ti[1]} | {tbk[0]} | {tbk[1]} |")
            del native, eager, comp, fu, x, cot, xp
            torch.cuda.empty_cache()
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
