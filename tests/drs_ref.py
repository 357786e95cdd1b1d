"""fp64 CPU restatement of DRSformer's transformer block (TEST INFRASTRUCTURE).

Written from the block's semantics (the STB of DRSformer_arch.py:174-187 with its TKSA attention and MSFN feed-forward), in
plain torch so that autograd supplies the backward.  Every function takes a flat ``{name: tensor}`` parameter dict with the
reference's state_dict keys (without the module prefix for ``tksa`` / ``msfn``).

``masks=``: the four boolean top-k masks [B, heads, c, c] to use instead of ranking S here.  Top-k is discontinuous: where S has
a near-tie at a top-k boundary the device's fp32 S and this fp64 S may keep different entries, so the GPU parity tests rank the
device's own scores (``topk_masks``) and hand the masks in.  ``relu_masks=`` (a > 0, b > 0, y > 0 of the MSFN) does the same for
the feed-forward's ReLUs, which flip where a pre-activation sits within rounding of 0.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-5


def topk_sizes(c: int):
    return int(c / 2), int(c * 2 / 3), int(c * 3 / 4), int(c * 4 / 5)


def topk_masks(S: torch.Tensor, ks=None):
    """Boolean masks of the k largest entries of each row of S (ties: lower column index first)."""
    S = S.detach()
    c = S.shape[-1]
    ks = topk_sizes(c) if ks is None else ks
    order = torch.sort(S, dim=-1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(-1, order, torch.arange(c, device=S.device).expand_as(order).contiguous())
    return [rank < k for k in ks]


def layer_norm(x, w, b=None):
    """Per-pixel LayerNorm over channels; b None: the bias-free form (scaled by the std, mean not removed)."""
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    wv = w.view(1, -1, 1, 1)
    if b is None:
        return x / torch.sqrt(var + LN_EPS) * wv
    return (x - mu) / torch.sqrt(var + LN_EPS) * wv + b.view(1, -1, 1, 1)


def tksa(x, p, heads, masks=None):
    """-> (out, S).  S = temperature * cos(q, k) per head; out = project_out(sum_m attn_m softmax_masked_m(S) v)."""
    B, C, H, W = x.shape
    c = C // heads
    qkv = F.conv2d(x, p["qkv.weight"], p.get("qkv.bias"))
    qkv = F.conv2d(qkv, p["qkv_dwconv.weight"], p.get("qkv_dwconv.bias"), padding=1, groups=3 * C)
    q, k, v = (t.reshape(B, heads, c, H * W) for t in qkv.chunk(3, dim=1))
    q = F.normalize(q, dim=-1)
    k = F.normalize(k, dim=-1)
    S = (q @ k.transpose(-2, -1)) * p["temperature"]
    if masks is None:
        masks = topk_masks(S)
    out = 0
    for m, mask in enumerate(masks):
        P = torch.where(mask, S, torch.full_like(S, float("-inf"))).softmax(dim=-1)
        out = out + (P @ v) * p[f"attn{m + 1}"]
    out = F.conv2d(out.reshape(B, C, H, W), p["project_out.weight"], p.get("project_out.bias"))
    return out, S


def _relu(z, mask):
    return F.relu(z) if mask is None else z * mask.to(z.dtype)


def msfn(x, p, relu_masks=None):
    ma, mb, my = relu_masks if relu_masks is not None else (None, None, None)
    h0 = F.conv2d(x, p["project_in.weight"], p.get("project_in.bias"))
    h2 = h0.shape[1]
    h = h2 // 2
    a = _relu(F.conv2d(h0, p["dwconv3x3.weight"], p.get("dwconv3x3.bias"), padding=1, groups=h2), ma)
    b = _relu(F.conv2d(h0, p["dwconv5x5.weight"], p.get("dwconv5x5.bias"), padding=2, groups=h2), mb)
    x1 = torch.cat([a[:, :h], b[:, :h]], dim=1)
    x2 = torch.cat([a[:, h:], b[:, h:]], dim=1)
    y1 = F.conv2d(x1, p["dwconv3x3_1.weight"], p.get("dwconv3x3_1.bias"), padding=1, groups=h)
    y2 = F.conv2d(x2, p["dwconv5x5_1.weight"], p.get("dwconv5x5_1.bias"), padding=2, groups=h)
    y = _relu(torch.cat([y1, y2], dim=1), my)
    return F.conv2d(y, p["project_out.weight"], p.get("project_out.bias"))


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def stb(x, sd, heads, masks=None, relu_masks=None):
    """-> (out, S) of the Sparse Transformer Block; the LayerNorm flavour follows the presence of norm1.body.bias."""
    xn = layer_norm(x, sd["norm1.body.weight"], sd.get("norm1.body.bias"))
    a, S = tksa(xn, sub(sd, "attn."), heads, masks)
    y = x + a
    yn = layer_norm(y, sd["norm2.body.weight"], sd.get("norm2.body.bias"))
    return y + msfn(yn, sub(sd, "ffn."), relu_masks), S


# ---------------------------------------------------------------- parameter shapes (reference state_dict order) and values
def tksa_shapes(dim, heads, bias):
    s = OrderedDict()
    s["temperature"] = (heads, 1, 1)
    for m in range(1, 5):
        s[f"attn{m}"] = (1,)
    s["qkv.weight"] = (3 * dim, dim, 1, 1)
    if bias:
        s["qkv.bias"] = (3 * dim,)
    s["qkv_dwconv.weight"] = (3 * dim, 1, 3, 3)
    if bias:
        s["qkv_dwconv.bias"] = (3 * dim,)
    s["project_out.weight"] = (dim, dim, 1, 1)
    if bias:
        s["project_out.bias"] = (dim,)
    return s


def msfn_shapes(dim, factor, bias):
    h = int(dim * factor)
    s = OrderedDict()
    for name, shape in (("project_in", (2 * h, dim, 1, 1)), ("dwconv3x3", (2 * h, 1, 3, 3)), ("dwconv5x5", (2 * h, 1, 5, 5)),
                        ("dwconv3x3_1", (h, 2, 3, 3)), ("dwconv5x5_1", (h, 2, 5, 5)), ("project_out", (dim, 2 * h, 1, 1))):
        s[name + ".weight"] = shape
        if bias:
            s[name + ".bias"] = (shape[0],)
    return s


def stb_shapes(dim, heads, factor, bias, ln_type):
    s = OrderedDict()
    for norm, part in (("norm1", tksa_shapes(dim, heads, bias)), ("norm2", msfn_shapes(dim, factor, bias))):
        s[norm + ".body.weight"] = (dim,)
        if ln_type != "BiasFree":
            s[norm + ".body.bias"] = (dim,)
        pre = "attn." if norm == "norm1" else "ffn."
        for k, v in part.items():
            s[pre + k] = v
    return s


def make_state(shapes, seed):
    """Seeded float32 values for the given shapes: convs scaled by 1/sqrt(fan-in), LayerNorm weights near 1, temperatures
    near 1, attn1..4 spread around the reference's 0.2."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shape in shapes.items():
        z = rng.standard_normal(shape)
        if k.endswith("temperature"):
            v = 1.0 + 0.3 * z
        elif k.split(".")[-1].startswith("attn") and shape == (1,):
            v = 0.2 + 0.1 * z
        elif ".body." in k:
            v = (1.0 + 0.1 * z) if k.endswith("weight") else 0.1 * z
        elif k.endswith("bias"):
            v = 0.1 * z
        else:
            fan_in = int(np.prod(shape[1:]))
            v = z / np.sqrt(fan_in)
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd
