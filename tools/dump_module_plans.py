#!/usr/bin/env python3
"""Dumps what the section modules plan, one JSON line per query, host only (no GPU is touched).

For FreMLP, FourierUnit, the SFHformer FFN, local mixer, global mixer and Mixer, BatchNorm2d and the scaled residual: the raw
out[64] of the C plan call, the two sizing calls, and the dict the ``ops.*_plan`` wrapper decodes; for EBlock and DBlock: the
sizing calls (and mi_eblock_plan).  The sweep is fixed: B in {1, 3}; the smallest, an odd (where the module takes one) and the
largest channel width; planes 2x2, 5x7, 64x64, 130x66, 256x256; fp32 and bf16; training on and off where the shape has it; then
each module's refusals with the return code and the mi_last_error text.

Two runs, before and after a change of the host code under the plans, must print the same bytes:

    python tools/dump_module_plans.py > after.jsonl
    python tools/dump_module_plans.py --lib /path/to/the/other/libmi_restore.so > before.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from image_restoration_amd import _lib as L  # noqa: E402

BATCHES = (1, 3)
PLANES = ((2, 2), (5, 7), (64, 64), (130, 66), (256, 256))
DTYPES = ((L.MI_F32, torch.float32), (L.MI_BF16, torch.bfloat16))


def emit(q, args, **fields):
    print(json.dumps({"q": q, "args": args, **fields}))


def err(handle):
    return handle.mi_last_error().decode("utf-8", "replace")


def raw(handle, q, shape, args, plan=None, saved=None, ws=None, slots=64):
    """The C calls of one shape: rc and out[] of the plan call, the sizing calls; the error text wherever one refuses."""
    fields = {}
    if plan is not None:
        out = (L.c_i64 * slots)()
        rc = getattr(handle, plan)(C.byref(shape), out)
        fields.update(rc=rc, out=list(out) if rc == 0 else None, plan_error="" if rc == 0 else err(handle))
    for key, fn in (("saved_bytes", saved), ("workspace", ws)):
        if fn is not None:
            n = int(getattr(handle, fn)(C.byref(shape)))
            fields[key] = n
            if n == 0:
                fields[key + "_error"] = err(handle)
    emit(q, args, **fields)


def decoded(q, fn, *args):
    try:
        emit(q, [str(a) for a in args], plan=fn(*args))
    except (RuntimeError, NotImplementedError, ValueError, TypeError) as e:
        emit(q, [str(a) for a in args], raised=type(e).__name__, text=str(e))


def block_shape(cls, B, c, H, W, dt, dil, extra):
    s = cls(B, c, H, W, dt, len(dil))
    for i, d in enumerate(dil[:4]):
        s.dil[i] = int(d)
    s.extra = int(extra)
    return s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the libmi_restore.so to query (default: the one built in this tree)")
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = os.path.abspath(a.lib)
    h = L.lib()
    from image_restoration_amd import ops

    fre = dict(plan="mi_fremlp_plan", saved="mi_fremlp_saved_bytes", ws="mi_fremlp_workspace")
    fu = dict(plan="mi_fourier_unit_plan", saved="mi_fourier_unit_saved_bytes", ws="mi_fourier_unit_workspace")
    ffn = dict(plan="mi_sfh_ffn_plan", saved="mi_sfh_ffn_saved_bytes", ws="mi_sfh_ffn_workspace")
    loc = dict(plan="mi_sfh_local_plan", ws="mi_sfh_local_workspace")
    glo = dict(plan="mi_sfh_global_plan", saved="mi_sfh_global_saved_bytes", ws="mi_sfh_global_workspace")
    mix = dict(plan="mi_sfh_mixer_plan", saved="mi_sfh_mixer_saved_bytes", ws="mi_sfh_mixer_workspace")
    bn = dict(plan="mi_bn2d_plan", ws="mi_bn2d_workspace")
    sr = dict(plan="mi_scale_res_plan", ws="mi_scale_res_workspace")
    eb = dict(plan="mi_eblock_plan", saved="mi_eblock_saved_bytes", ws="mi_eblock_workspace", slots=16)
    db = dict(saved="mi_dblock_saved_bytes", ws="mi_dblock_workspace")

    for B in BATCHES:
        for H, W in PLANES:
            for dt, td in DTYPES:
                for nc, expand in ((1, 1), (5, 2), (256, 2), (1, 512)):
                    raw(h, "fremlp", L.FremlpShape(B, nc, expand, H, W, dt), [B, nc, expand, H, W, dt], **fre)
                    decoded("ops.fremlp_plan", ops.fremlp_plan, B, nc, expand, H, W, td)
                for c, G in ((1, 1), (1, 2), (5, 2), (256, 4), (256, 8)):
                    for tr in (1, 0):
                        raw(h, "fourier_unit", L.FourierUnitShape(B, c, G, H, W, dt, tr, 1e-5, 0.1), [B, c, G, H, W, dt, tr], **fu)
                    decoded("ops.fourier_unit_plan", ops.fourier_unit_plan, B, c, G, H, W, td)
                for dim in (2, 6, 256):
                    raw(h, "sfh_ffn", L.SfhFfnShape(B, dim, H, W, dt), [B, dim, H, W, dt], **ffn)
                    raw(h, "sfh_local", L.SfhLocalShape(B, dim, H, W, dt), [B, dim, H, W, dt], **loc)
                    decoded("ops.sfh_ffn_plan", ops.sfh_ffn_plan, B, dim, H, W, td)
                    decoded("ops.sfh_local_plan", ops.sfh_local_plan, B, dim, H, W, td)
                for dim in (1, 2, 5, 6, 128):
                    for tr in (1, 0):
                        s = L.SfhMixerShape(B, dim, H, W, dt, tr, 1e-5, 0.1)
                        raw(h, "sfh_global", s, [B, dim, H, W, dt, tr], **glo)
                        raw(h, "sfh_mixer", s, [B, dim, H, W, dt, tr], **mix)        # (dim 1 and 5: the Mixer's odd-width refusal)
                    decoded("ops.sfh_global_plan", ops.sfh_global_plan, B, dim, H, W, td)
                    decoded("ops.sfh_mixer_plan", ops.sfh_mixer_plan, B, dim, H, W, td)
                for Cn in (1, 5, 4096):
                    for tr in (1, 0):
                        raw(h, "bn2d", L.Bn2dShape(B, Cn, H, W, dt, tr, 1e-5, 0.1), [B, Cn, H, W, dt, tr], **bn)
                        decoded("ops.bn2d_plan", ops.bn2d_plan, B, Cn, H, W, td, bool(tr))
                    raw(h, "scale_res", L.Bn2dShape(B, Cn, H, W, dt, 1, 1e-5, 0.1), [B, Cn, H, W, dt], **sr)
                    decoded("ops.scale_res_plan", ops.scale_res_plan, B, Cn, H, W, td)
                for c in (1, 5, 256):
                    for dil, extra in (((1,), True), ((1, 4, 9), False)):
                        args = [B, c, H, W, dt, list(dil), int(extra)]
                        raw(h, "eblock", block_shape(L.EblockShape, B, c, H, W, dt, dil, extra), args, **eb)
                        raw(h, "dblock", block_shape(L.DblockShape, B, c, H, W, dt, dil, extra), args, **db)
                        emit("ops.eblock_sizes", args, sizes=ops.eblock_sizes(B, c, H, W, td, dil, extra))
                        emit("ops.dblock_sizes", args, sizes=ops.dblock_sizes(B, c, H, W, td, dil, extra))

    # ---- the refusals of the modules' host tests: bad dtype, B = 0, a width and a plane one past the limit, the 2^31 overflow
    def refusals(q, cls, ok, bad, calls):
        for kw in bad:
            args = dict(ok, **kw)
            raw(h, q + ":refused", cls(*args.values()), args, **calls)

    refusals("fremlp", L.FremlpShape, dict(B=2, nc=8, expand=2, H=8, W=8, dtype=0),
             [dict(H=1), dict(W=1), dict(H=513), dict(W=513), dict(nc=0), dict(nc=257, expand=1), dict(nc=171, expand=3),
              dict(nc=1, expand=513), dict(expand=0), dict(B=0), dict(dtype=7), dict(B=64, nc=256, H=512, W=512)], fre)
    refusals("fourier_unit", L.FourierUnitShape, dict(B=2, c=8, groups=4, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1),
             [dict(c=5, groups=4), dict(groups=9, c=9), dict(groups=0), dict(c=257, groups=2), dict(c=0), dict(H=1), dict(W=1),
              dict(H=513), dict(W=513), dict(dtype=7), dict(B=0), dict(eps=0.0), dict(momentum=1.5), dict(B=300, c=256, H=512, W=512)], fu)
    sf_bad = [dict(dim=5), dict(dim=0), dict(dim=258), dict(H=0), dict(W=0), dict(dtype=7), dict(B=0), dict(dim=-2),
              dict(B=1024, dim=256, H=4096, W=4096)]
    refusals("sfh_ffn", L.SfhFfnShape, dict(B=2, dim=8, H=8, W=8, dtype=0), sf_bad, ffn)
    refusals("sfh_local", L.SfhLocalShape, dict(B=2, dim=8, H=8, W=8, dtype=0), sf_bad, loc)
    sm_ok = dict(B=2, dim=8, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1)
    sm_bad = [dict(dim=0), dict(dim=129), dict(dim=130), dict(dim=-2), dict(H=1), dict(H=513), dict(W=1), dict(W=514), dict(dtype=7), dict(B=0),
              dict(B=65536), dict(B=1024, dim=128, H=512, W=512), dict(eps=0.0), dict(momentum=1.5)]
    refusals("sfh_global", L.SfhMixerShape, sm_ok, sm_bad, glo)
    refusals("sfh_mixer", L.SfhMixerShape, sm_ok, sm_bad + [dict(dim=5), dict(dim=1)], mix)
    bn_ok = dict(B=2, C=8, H=8, W=8, dtype=0, training=1, eps=1e-5, momentum=0.1)
    bn_bad = [dict(C=0), dict(C=4097), dict(C=-2), dict(H=0), dict(W=0), dict(W=-3), dict(B=0), dict(dtype=7), dict(B=64, C=4096, H=128, W=64),
              dict(B=1 << 20, C=1 << 11, H=1, W=1)]
    refusals("bn2d", L.Bn2dShape, bn_ok, bn_bad + [dict(eps=0.0), dict(eps=-1e-5), dict(momentum=1.5), dict(momentum=-0.1),
                                                  dict(B=1, H=1, W=1), dict(B=1, C=4096, H=1, W=1)], bn)
    refusals("scale_res", L.Bn2dShape, bn_ok, bn_bad, sr)
    blk_ok = dict(B=2, c=32, H=20, W=24, dt=0, dil=(1,), extra=True)
    for kw in (dict(c=257), dict(c=0), dict(B=0), dict(H=1), dict(W=1), dict(H=513), dict(W=513), dict(dil=(1, 17)), dict(dil=(0,)),
               dict(dil=()), dict(dil=(1, 2, 3, 4, 5)), dict(dt=7), dict(B=64, c=256, H=512, W=256, dt=1)):
        args = dict(blk_ok, **kw)
        raw(h, "eblock:refused", block_shape(L.EblockShape, **args), {k: list(v) if isinstance(v, tuple) else v for k, v in args.items()}, **eb)
        raw(h, "dblock:refused", block_shape(L.DblockShape, **args), {k: list(v) if isinstance(v, tuple) else v for k, v in args.items()}, **db)


if __name__ == "__main__":
    main()
