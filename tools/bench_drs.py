#!/usr/bin/env python3
"""Forward + backward time of DRSformer's Sparse Transformer Block (STB): the native block (image_restoration_amd.drsformer)
against an eager torch form of the same block (tests/drs_ref.py's functional statement: F.conv2d, matmuls, a sort for the
top-k masks, torch.where + softmax, autograd) on the same GPU, fp32 and bf16, at the per-level shapes of DRSformer base
(dim 48, heads 1/2/4/8, ffn_expansion_factor 2.66, bias False, WithBias) for bs 8 at 256^2, plus decoder level 1 (dim 96, one
head).  Also the native TKSA and MSFN halves alone.  Median of --iters timed iterations after --warmup, HIP events.

usage: python tools/bench_drs.py [--iters 10] [--warmup 3] [--bs 8] [--hw 256] [--json out.json]
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

import drs_ref as D  # noqa: E402
from image_restoration_amd import drsformer as N  # noqa: E402

DEV = torch.device("cuda:0")
# (label, dim, heads, plane divisor)
LEVELS = [("L1", 48, 1, 1), ("L2", 96, 2, 2), ("L3", 192, 4, 4), ("L4", 384, 8, 8), ("dec-L1", 96, 1, 1)]


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


def bench_level(dim, heads, shape, dtype, iters, warmup):
    sd = D.make_state(D.stb_shapes(dim, heads, 2.66, False, "WithBias"), seed=dim + heads)
    blk = N.TransformerBlock(dim, heads, 2.66, False, "WithBias")
    blk.load_state_dict(sd)
    blk = blk.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(shape, device=DEV, generator=g).to(dtype).requires_grad_(True)
    cot = torch.randn(shape, device=DEV, generator=g).to(dtype)

    def native():
        blk(x).backward(cot)

    def half(mod):
        def run():
            mod(x).backward(cot)
        return run

    ps = {k: v.to(DEV).requires_grad_(True) for k, v in sd.items()}

    def eager():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            y, _ = D.stb(x, ps, heads)
        y.backward(cot)

    out = {"native_ms": timed(native, iters, warmup),
           "tksa_ms": timed(half(blk.attn), iters, warmup),
           "msfn_ms": timed(half(blk.ffn), iters, warmup)}
    out["eager_ms"] = timed(eager, iters, warmup)
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
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for label, dim, heads, div in LEVELS:
            shape = (a.bs, dim, a.hw // div, a.hw // div)
            r = bench_level(dim, heads, shape, dtype, a.iters, a.warmup)
            r.update(level=label, dim=dim, heads=heads, shape=list(shape), dtype=str(dtype).replace("torch.", ""))
            rows.append(r)
            print(f"{r['dtype']:8s} {label:6s} {str(tuple(shape)):22s} native STB {r['native_ms']:8.2f} ms "
                  f"(TKSA {r['tksa_ms']:7.2f}, MSFN {r['msfn_ms']:7.2f})  eager {r['eager_ms']:8.2f} ms  x{r['speedup']:.2f}",
                  flush=True)
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
