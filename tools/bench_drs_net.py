#!/usr/bin/env python3
"""DRSformer base training step on the native kernels (image_restoration_amd.drsformer.DRSformer): bf16 activations, FlatTrainer
(main_grad accumulation, fused AdamW), L1 loss, --bs images of --hw^2.  Reports ms per step and Mpix/s, then the two MEFCs
(encoder_level0 at dim, refinement at 2 dim) alone, forward + backward at their planes inside that step, as a share of the step.
Last, one MEFC layer pair with a single step (routing head, preprocess and one OperationLayer) forward + backward, native against
an eager torch form of the same computation (tests/drs_net_ref.py: F.conv2d, avg_pool2d, torch.cat, autograd) on the same GPU,
fp32 and bf16.  Median of --iters timed iterations after --warmup, HIP events.

usage: python tools/bench_drs_net.py [--iters 10] [--warmup 3] [--bs 8] [--hw 256] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import drs_net_ref as R  # noqa: E402
import drs_ref as D  # noqa: E402
from image_restoration_amd import configs  # noqa: E402
from image_restoration_amd import drsformer as N  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def bench_step(bs, hw, iters, warmup):
    from image_restoration_amd.trainer import FlatTrainer
    torch.manual_seed(0)
    net = N.DRSformer(**configs.DRSFORMER_BASE).to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(bs, 3, hw, hw, device=DEV, generator=g).to(torch.bfloat16)
    t = torch.randn(bs, 3, hw, hw, device=DEV, generator=g).to(torch.bfloat16)
    tr = FlatTrainer(net, lr=2e-4)
    try:
        def step():
            tr.zero_grad()
            loss = (net(x).float() - t.float()).abs().mean()
            loss.backward()
            tr.reduce_gradients()
            tr.optimizer_step()
        ms = timed(step, iters, warmup)
        out = {"step_ms": ms, "mpix_s": bs * hw * hw / (ms * 1e3)}
        dim = configs.DRSFORMER_BASE["dim"]
        for name, c in (("encoder_level0", dim), ("refinement", 2 * dim)):
            mod = getattr(net, name)
            h = torch.randn(bs, c, hw, hw, device=DEV, generator=g).to(torch.bfloat16).requires_grad_(True)
            cot = torch.randn(bs, c, hw, hw, device=DEV, generator=g).to(torch.bfloat16)
            out[name + "_ms"] = timed(lambda: mod(h).backward(cot), iters, warmup)
            del h, cot
        out["mefc_share"] = (out["encoder_level0_ms"] + out["refinement_ms"]) / ms
    finally:
        tr.close()
    return out


def bench_pair(dim, bs, hw, dtype, iters, warmup):
    sd = D.make_state(R.subnet_shapes(dim, 1, 1), seed=dim)
    mod = N.subnet(dim, 1, 1)
    mod.load_state_dict(sd)
    mod = mod.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(bs, dim, hw, hw, device=DEV, generator=g).to(dtype).requires_grad_(True)
    cot = torch.randn(bs, dim, hw, hw, device=DEV, generator=g).to(dtype)
    ps = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items()}

    def eager():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            y, _ = R.subnet(x, ps, 1, 1)
        y.backward(cot)

    out = {"native_ms": timed(lambda: mod(x).backward(cot), iters, warmup), "eager_ms": timed(eager, iters, warmup)}
    out["speedup"] = out["eager_ms"] / out["native_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bs", type=int, default=8)
    ap.add_argument("--hw", type=int, default=256)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"step": bench_step(a.bs, a.hw, a.iters, a.warmup), "pair": []}
    s = res["step"]
    print(f"DRSformer base training step bf16 bs {a.bs} {a.hw}^2: {s['step_ms']:.1f} ms, {s['mpix_s']:.2f} Mpix/s; MEFC fwd+bwd "
          f"encoder_level0 {s['encoder_level0_ms']:.1f} ms, refinement {s['refinement_ms']:.1f} ms ({100 * s['mefc_share']:.1f} % "
          f"of the step)", flush=True)
    torch.cuda.empty_cache()
    dim = configs.DRSFORMER_BASE["dim"]
    for dtype in (torch.float32, torch.bfloat16):
        for c in (dim, 2 * dim):
            r = bench_pair(c, a.bs, a.hw, dtype, a.iters, a.warmup)
            r.update(dim=c, dtype=str(dtype).replace("torch.", ""))
            res["pair"].append(r)
            print(f"{r['dtype']:8s} MEFC pair, one step, C {c:3d}: native {r['native_ms']:8.2f} ms  eager {r['eager_ms']:8.2f} ms  "
                  f"x{r['speedup']:.2f}", flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
