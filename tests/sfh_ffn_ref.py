"""fp64-capable CPU restatement of SFHformer's FFN and TokenMixer_For_Local (TEST INFRASTRUCTURE), in plain torch so that autograd
supplies the backward.  s = dim / 2 is the segment width.

    FFN    h = W1 x + b1  [B, 2 dim, H, W]                       conv_init.0: biased 1x1
           u = cat(h[:, :s], dw3(h[:, s:2s]), dw5(h[:, 2s:3s]), dw7(h[:, 3s:]))    depthwise k x k, zero padding (k - 1) / 2, biased
           g = gelu(u)  (erf form);  out = W2 g + b2             conv_fina.0: biased 1x1
    local  out = cat(dw3(x[:, :s]), dw3 at dilation 2 (x[:, s:])), zero padding 1 and 2, biased; no activation

Two forms of the same functions:

``ffn`` / ``local``                written from the formulas with ``F.conv2d``: the reference of every comparison.
``ffn_device`` / ``local_device``  the way the device computes them: one segmented tensor, every stencil as a sum of shifted copies
                                   of the zero-padded plane, one tap after the other in the kernels' order (rows, then columns).
                                   ``rnd=`` (identity, or ``round_bf16``) is applied exactly where the kernels store a tensor in the
                                   activation dtype: in the forward x, h, u, g and out (FFN), x and out (local); in the backward
                                   the cotangent, dg (the gradient arriving at g), dh (at h) and dx (at x) (FFN), the cotangent and dx
                                   (local).  u is rounded in the forward only: the gradient at u, dg gelu'(u), lives in fp32 in
                                   the kernels' LDS and is never stored.  gelu and gelu' see u as stored.  The two 1x1 products
                                   read their weight matrices from the packed image the matrix-core path keeps in the activation
                                   dtype, forward and transposed (the weight GRADIENTS are fp32 sums over stored activations);
                                   biases, stencil weights and every accumulation are fp32.  Evaluated in float32 this form is
                                   the host-side error model of the kernels.

State dicts carry the reference's keys in its order.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from darkir_ref import _id, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)
from oracle.fixtures import compact

PACK_ELEMS = 1536     # elements kept per tensor in the captured fixtures (oracle.fixtures.pack's max_elems)

FFN_PARAMS = ("conv_init.0.weight", "conv_init.0.bias", "conv1_1.0.weight", "conv1_1.0.bias", "conv1_2.0.weight", "conv1_2.0.bias",
              "conv1_3.0.weight", "conv1_3.0.bias", "conv_fina.0.weight", "conv_fina.0.bias")
LOCAL_PARAMS = ("CDilated_1.weight", "CDilated_1.bias", "CDilated_2.weight", "CDilated_2.bias")
PARAMS = {"ffn": FFN_PARAMS, "local": LOCAL_PARAMS}
# (kernel size, dilation) per segment; kernel size 1: identity
FFN_TAPS = ((1, 1), (3, 1), (5, 1), (7, 1))
LOCAL_TAPS = ((3, 1), (3, 2))


def shapes(kind, dim):
    s, out = dim // 2, OrderedDict()
    if kind == "ffn":
        out["conv_init.0.weight"], out["conv_init.0.bias"] = (2 * dim, dim, 1, 1), (2 * dim,)
        for i, k in ((1, 3), (2, 5), (3, 7)):
            out[f"conv1_{i}.0.weight"], out[f"conv1_{i}.0.bias"] = (s, 1, k, k), (s,)
        out["conv_fina.0.weight"], out["conv_fina.0.bias"] = (dim, 2 * dim, 1, 1), (dim,)
    else:
        for i in (1, 2):
            out[f"CDilated_{i}.weight"], out[f"CDilated_{i}.bias"] = (s, 1, 3, 3), (s,)
    return out


def state_dict_layout(kind, dim):
    """(key, shape) in the reference's state_dict order (neither module has buffers)."""
    return list(shapes(kind, dim).items())


def make_state(kind, dim, seed):
    """Seeded float32 parameters: weights N(0,1) / sqrt(fan-in), biases 0.1 N(0,1)."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shape in shapes(kind, dim).items():
        z = rng.standard_normal(shape)
        v = 0.1 * z if k.endswith("bias") else z / math.sqrt(int(np.prod(shape[1:])))
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


# ---------------------------------------------------------------- the formulas
def ffn(x, sd):
    s = x.shape[1] // 2
    h = list(torch.split(F.conv2d(x, sd["conv_init.0.weight"], sd["conv_init.0.bias"]), s, dim=1))
    for i, k in ((1, 3), (2, 5), (3, 7)):
        h[i] = F.conv2d(h[i], sd[f"conv1_{i}.0.weight"], sd[f"conv1_{i}.0.bias"], padding=k // 2, groups=s)
    return F.conv2d(F.gelu(torch.cat(h, dim=1)), sd["conv_fina.0.weight"], sd["conv_fina.0.bias"])


def local(x, sd):
    s = x.shape[1] // 2
    a = F.conv2d(x[:, :s], sd["CDilated_1.weight"], sd["CDilated_1.bias"], padding=1, dilation=1, groups=s)
    b = F.conv2d(x[:, s:], sd["CDilated_2.weight"], sd["CDilated_2.bias"], padding=2, dilation=2, groups=s)
    return torch.cat([a, b], dim=1)


# ---------------------------------------------------------------- the device's formulation
class _RoundFwd(torch.autograd.Function):
    """``rnd`` in the forward, the identity in the backward: a tensor that is stored whose gradient is not."""

    @staticmethod
    def forward(ctx, t, rnd):
        return rnd(t.detach())

    @staticmethod
    def backward(ctx, g):
        return g, None


def stencil(p, w, b, ks, dil):
    """Depthwise ks x ks at dilation dil over p [B, s, H, W] as the kernels sum it: bias first, then one tap after the other."""
    if ks == 1:
        return p
    r = dil * (ks - 1) // 2
    H, W = p.shape[-2:]
    q = F.pad(p, (r, r, r, r))
    acc = b.view(1, -1, 1, 1).expand_as(p)
    for dy in range(ks):
        for dx in range(ks):
            acc = acc + w[:, 0, dy, dx].view(1, -1, 1, 1) * q[:, :, dy * dil:dy * dil + H, dx * dil:dx * dil + W]
    return acc


def segmented(t, taps, weights):
    s = t.shape[1] // len(taps)
    return torch.cat([stencil(t[:, k * s:(k + 1) * s], *weights[k], ks, dil) for k, (ks, dil) in enumerate(taps)], dim=1)


def _pw(x, w, b, rnd):
    """A 1x1 product as the matrix-core path runs it: it reads its weight matrix from a packed image in the activation dtype (in
    the transposed product of the backward too); the bias and the accumulation stay fp32."""
    return torch.einsum("mk,bkhw->bmhw", _RoundFwd.apply(w[:, :, 0, 0], rnd), x) + b.view(1, -1, 1, 1)


def ffn_device(x, sd, rnd=_id):
    x = rnd(x)
    h = rnd(_pw(x, sd["conv_init.0.weight"], sd["conv_init.0.bias"], rnd))
    weights = [(None, None)] + [(sd[f"conv1_{i}.0.weight"], sd[f"conv1_{i}.0.bias"]) for i in (1, 2, 3)]
    u = _RoundFwd.apply(segmented(h, FFN_TAPS, weights), rnd)
    g = rnd(F.gelu(u))
    return rnd(_pw(g, sd["conv_fina.0.weight"], sd["conv_fina.0.bias"], rnd))


def local_device(x, sd, rnd=_id):
    weights = [(sd[f"CDilated_{i}.weight"], sd[f"CDilated_{i}.bias"]) for i in (1, 2)]
    return rnd(segmented(rnd(x), LOCAL_TAPS, weights))


FORMS = {("ffn", False): lambda x, p, rnd: ffn(x, p), ("local", False): lambda x, p, rnd: local(x, p),
         ("ffn", True): ffn_device, ("local", True): local_device}


def run(kind, x, cot, sd, dtype=torch.float64, rnd=_id, device=False):
    """Forward and backward in ``dtype``: -> {"y", "dx", "g.<key>"...} (detached)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = x.detach().to(dtype).requires_grad_(True)
    y = FORMS[(kind, device)](xr, p, rnd)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad}
    out.update({"g." + k: p[k].grad for k in PARAMS[kind]})
    return out


def check(prefix, got, gold, rtol, what=""):
    """oracle.fixtures.check for fixtures packed with PACK_ELEMS: the strided subset within rtol x max |gold|, and the L2 digest."""
    c = compact(got, PACK_ELEMS)
    ref_sub = np.asarray(gold[f"{prefix}.sub"], dtype=np.float64)
    assert c["sub"].shape == ref_sub.shape, f"{what}{prefix}: {c['sub'].shape} vs {ref_sub.shape}"
    scale = max(float(np.abs(ref_sub).max()), 1e-30)
    err = float(np.abs(c["sub"].astype(np.float64) - ref_sub).max()) / scale
    assert err <= rtol, f"{what}{prefix}: max rel err {err:.3e} > {rtol:.1e}"
    l2 = float(gold[f"{prefix}.l2"])
    assert abs(c["l2"] - l2) <= 10 * rtol * max(l2, 1e-30), f"{what}{prefix}: l2 {c['l2']:.6e} vs {l2:.6e}"
    return err


def tensors(kind):
    return {"y", "dx"} | {"g." + k for k in PARAMS[kind]}


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_sfh_ffn.py
# name -> (kind, (B, dim, H, W), seed).  Stated against the tile the kernels were built with, 64 wide x 16 high (four pixels of a row
# per thread), 16 backward splits; rows are handled 4 wide where W % 4 == 0 and element by element otherwise, so both kinds of W occur.
PARITY_CASES = OrderedDict([
    ("tile", ("ffn", (1, 4, 16, 64), 6100)),            # the plane is exactly one tile; 4-wide rows
    ("tile_plus_1", ("ffn", (1, 4, 17, 65), 6101)),     # one row and one column past it: 2 x 2 tiles, three of them slivers
    ("ragged", ("ffn", (1, 4, 83, 136), 6102)),         # 3 ragged tiles across, 6 down: 18 tiles, more than the 16 splits; 4-wide rows
    ("ragged_odd", ("ffn", (1, 4, 40, 70), 6103)),      # the plane the issue names for a 32 x 8 tile: 2 x 3 tiles here, W % 4 != 0
    ("tiny", ("ffn", (1, 4, 2, 2), 6104)),              # smaller than every halo
    ("row", ("ffn", (1, 4, 1, 5), 6105)),               # one row: every vertical tap but the centre is padding
    ("k7", ("ffn", (1, 4, 7, 7), 6106)),                # the plane equals the largest kernel
    ("dim2", ("ffn", (2, 2, 9, 12), 6107)),             # s = 1; a 4-wide row shorter than the tile
    ("dim6", ("ffn", (1, 6, 8, 34), 6108)),             # s = 3: an odd segment width
    ("wide", ("ffn", (1, 64, 8, 8), 6109)),             # the 1x1 plans at SFHformer's width
    ("b3", ("ffn", (3, 4, 9, 33), 6110)),               # three images; the issue's "one past a 32 x 8 tile" plane
    ("loc_tiny", ("local", (1, 4, 2, 2), 6111)),        # dilation 2 leaves only the centre tap inside
    ("loc_3x3", ("local", (1, 4, 3, 3), 6112)),         # dilation 2: the centre and, from the corners, the opposite corners
    ("loc_b3", ("local", (3, 6, 9, 33), 6113)),         # s = 3, three images
    ("loc_tile_plus_1", ("local", (1, 4, 17, 65), 6114)),
    ("loc_ragged_odd", ("local", (1, 4, 40, 70), 6115)),
    ("loc_ragged", ("local", (2, 2, 83, 134), 6116)),   # 18 tiles over 16 splits, element-wise rows, s = 1
    ("loc_vec", ("local", (1, 8, 20, 72), 6117)),       # 4-wide rows over 2 x 2 tiles
])


def parity_io(name):
    """-> (kind, state, input, cotangent) of a parity case, float32."""
    kind, (B, dim, H, W), seed = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, dim, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, dim, H, W))).float()
    return kind, make_state(kind, dim, seed + 50), x, cot


def host_errors(name, dtype):
    """Error of the DEVICE form evaluated on the host in the device's storage precision (float32 throughout, or float32 with the
    tensors listed in the module docstring rounded to bfloat16) against the fp64 form, per tensor, in the parity metric.
    -> ({tensor: error}, the fp64 results)."""
    kind, sd, x, cot = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    ref = run(kind, x, cot, sd)
    got = run(kind, x, cot, sd, torch.float32, _id if dtype == torch.float32 else round_bf16, device=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
