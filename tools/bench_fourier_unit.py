#!/usr/bin/env python3
"""Times SFHformer's FourierUnit on the MI355X at the three levels of SFHformer width 32 on a 256 x 256 crop (bs 8, bf16
activations, groups 4): the native module forward and forward + backward beside an eager module of the same mathematics on the
same device (torch.fft, i.e. rocFFT, in fp32, nn.BatchNorm2d, the depthwise and the grouped conv with its [B, G 2c, H, K] output
materialised, as the reference does: restated here, a comparison inside this tool only, never on the product path), and the two
transforms on their own, so that the middle section's share of the native forward can be read off.

Times are device events around `--iters` back-to-back calls after `--warmup` calls, the median of `--repeats` such windows; the
native and the eager windows alternate.  Both modules run in training mode (batch statistics, running statistics updated).

usage: python tools/bench_fourier_unit.py [--bs 8] [--iters 10] [--repeats 7] [--warmup 3] [--log profiles/fourier_unit_bench.log]
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.dont_write_bytecode = True

from bench_fremlp import timed  # noqa: E402

SHAPES = ((64, 256), (128, 128), (256, 64))   # (c, H = W) of the FourierUnits of SFHformer's three levels at a 256 x 256 input
GROUPS = 4
# what the middle of the native forward moves, in fp32 spectra [B, 2c, H, K]: the statistics read Z (1; the second read of each
# 8 KiB chunk comes from cache), t = fpe(bn(Z)) + bn(Z) reads and writes (2), the gate reads t twice and writes the scaled input
# (3), the folded product reads and writes (2), GELU reads and writes (2)
MIDDLE_PASSES = 10


class EagerFourierUnit(torch.nn.Module):
    """The reference formulation in plain PyTorch ops: fp32 spectra and parameters around bf16 activations."""

    def __init__(self, c, groups):
        super().__init__()
        self.groups = groups
        self.bn = torch.nn.BatchNorm2d(2 * c)
        self.fdc = torch.nn.Conv2d(2 * c, 2 * c * groups, 1, 1, 0, groups=groups, bias=True)
        self.weight = torch.nn.Sequential(torch.nn.Conv2d(2 * c, groups, 1, 1, 0), torch.nn.Softmax(dim=1))
        self.fpe = torch.nn.Conv2d(2 * c, 2 * c, 3, 1, 1, groups=2 * c, bias=True)

    def forward(self, x):
        B, c, H, W = x.shape
        z = torch.fft.rfft2(x.float(), norm="ortho")
        t = torch.stack([z.real, z.imag], dim=2).reshape(B, 2 * c, H, -1)
        t = self.bn(t)
        t = self.fpe(t) + t
        s = self.weight(t)
        u = self.fdc(t).view(B, self.groups, 2 * c, H, -1)
        o = F.gelu(torch.einsum("ijkml,ijml->ikml", u, s)).view(B, c, 2, H, -1)
        out = torch.fft.irfft2(torch.complex(o[:, :, 0], o[:, :, 1]), s=(H, W), norm="ortho")
        return out.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fourier_unit: needs the MI355X (no CPU timing)")
    import sfh_ref as R
    from image_restoration_amd import ops, sfhformer
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name(0)}; bs {a.bs}, bf16 activations, groups {GROUPS}, training mode; median of {a.repeats} "
        f"windows of {a.iters} calls [min..max], native and eager windows alternating")
    for c, hw in SHAPES:
        B, H, W, K = a.bs, hw, hw, hw // 2 + 1
        sd = R.module_state(R.make_state(c, GROUPS, 3))
        native = sfhformer.FourierUnit(c, c, GROUPS)
        native.load_state_dict(sd)
        native = native.to(dev).train()
        eager = EagerFourierUnit(c, GROUPS)
        eager.load_state_dict(sd)
        eager = eager.to(dev).train()
        g = torch.Generator().manual_seed(c)
        x = torch.randn(B, c, H, W, generator=g).to(dev).to(torch.bfloat16)
        cot = torch.randn(B, c, H, W, generator=g).to(dev).to(torch.bfloat16)
        with torch.no_grad():
            d = (native(x).float() - eager(x).float()).abs().max() / eager(x).float().abs().max()
        say(f"c={c:3d} {hw}x{hw}  native vs eager output, max |delta| / max |eager| = {float(d):.2e} (bf16 storage)")

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
        plan = ops.fourier_unit_plan(B, c, GROUPS, H, W, torch.bfloat16)
        spectrum = 8 * B * c * H * K
        tag = f"c={c:3d} {hw}x{hw}"
        say(f"{tag}  fwd      native {nf[0]:9.1f} us [{nf[1]:.1f}..{nf[2]:.1f}]   eager {ef[0]:9.1f} us [{ef[1]:.1f}..{ef[2]:.1f}]   "
            f"native/eager {nf[0] / ef[0]:.2f}")
        say(f"{tag}  fwd+bwd  native {nb[0]:9.1f} us [{nb[1]:.1f}..{nb[2]:.1f}]   eager {eb[0]:9.1f} us [{eb[1]:.1f}..{eb[2]:.1f}]   "
            f"native/eager {nb[0] / eb[0]:.2f}")
        mid = max(nf[0] - tr[0] - tc[0], 1e-9)
        say(f"{tag}  r2c alone {tr[0]:8.1f} us;  c2r alone {tc[0]:8.1f} us;  the middle of the native forward (BatchNorm, fpe, gate, "
            f"the folded product, GELU) {mid:8.1f} us: {MIDDLE_PASSES} spectrum-sized reads or writes of {spectrum / 2**20:.1f} MiB "
            f"each = {MIDDLE_PASSES * spectrum / mid / 1e6:.2f} TB/s")
        say(f"{tag}  saved {plan['saved_bytes'] / 2**20:.1f} MiB, workspace {plan['workspace'] / 2**20:.1f} MiB, launches "
            f"{plan['kernels_fwd']} + {plan['lib_calls_fwd']} forward, {plan['kernels_bwd']} + {plan['lib_calls_bwd']} backward")
        del native, eager, x, cot, zre, zim
        torch.cuda.empty_cache()
    if a.log:
        with open(os.path.join(ROOT, a.log) if not os.path.isabs(a.log) else a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
