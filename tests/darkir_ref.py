"""fp64 CPU restatement of DarkIR's dilated-gate decoder block, DBlock (TEST INFRASTRUCTURE).

Written from the block's formulas, in plain torch so that autograd supplies the backward:

    x0 = LN2d(inp; norm1, eps 1e-6)            channel LayerNorm with bias, biased variance
    x1 = conv1(x0)                             1x1, c -> 2c
    x2 = extra_conv(x1)                        3x3 pad 1, groups = c on 2c channels (when the state has extra_conv.weight)
    z  = sum_i dw3x3(x2; dilation d_i, pad d_i) + b_i
    g  = z[:, :c] * z[:, c:]
    s  = W_sca . mean_hw(g) + b_sca
    y  = inp + beta * conv3(s * g)
    u  = conv4(LN2d(y; norm2))
    out = y + gamma * conv5(u[:, :c] * u[:, c:])

Every function takes a flat ``{name: tensor}`` dict with the reference's state_dict keys.  ``rnd=``: a function applied to every
activation tensor the device stores (identity: exact arithmetic in the tensors' dtype; ``round_bf16``: storage in bfloat16), so
that the same code gives the host-side error of a storage precision against fp64 - the source of the GPU tests' bounds.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-6


class _RoundBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.to(torch.bfloat16).to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def round_bf16(t):
    """A tensor as the device stores it in bfloat16 (round to nearest even); the gradient arriving at it is stored the same way."""
    return _RoundBf16.apply(t)


def _id(t):
    return t


def layer_norm2d(x, w, b, eps=LN_EPS):
    mu = x.mean(1, keepdim=True)
    var = ((x - mu) ** 2).mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def n_branches(sd):
    n = 0
    while f"branches.{n}.branch.0.weight" in sd:
        n += 1
    return n


def pairconv(x, w, b):
    """extra_conv: groups = c on 2c channels."""
    return F.conv2d(x, w, b, padding=1, groups=x.shape[1] // 2)


def dilated_sum(x, sd, dilations):
    z = 0
    for i, d in enumerate(dilations):
        z = z + F.conv2d(x, sd[f"branches.{i}.branch.0.weight"], sd[f"branches.{i}.branch.0.bias"], padding=d, dilation=d,
                         groups=x.shape[1])
    return z


def simple_gate(z):
    c = z.shape[1] // 2
    return z[:, :c] * z[:, c:]


def dilgate(x, sd, dilations):
    """-> (g, pool sums [B, c]) of the hot kernel."""
    g = simple_gate(dilated_sum(x, sd, dilations))
    return g, g.sum(dim=(2, 3))


def dblock(inp, sd, dilations, rnd=_id):
    c = inp.shape[1]
    x0 = rnd(layer_norm2d(inp, sd["norm1.weight"], sd["norm1.bias"]))
    x = rnd(F.conv2d(x0, sd["conv1.weight"], sd["conv1.bias"]))
    if "extra_conv.weight" in sd:
        x = rnd(pairconv(x, sd["extra_conv.weight"], sd["extra_conv.bias"]))
    g = simple_gate(dilated_sum(x, sd, dilations))
    s = F.conv2d(g.mean(dim=(2, 3), keepdim=True), sd["sca.1.weight"], sd["sca.1.bias"])
    g = rnd(g)
    y = rnd(inp + sd["beta"] * F.conv2d(s * g, sd["conv3.weight"], sd["conv3.bias"]))
    u = rnd(F.conv2d(rnd(layer_norm2d(y, sd["norm2.weight"], sd["norm2.bias"])), sd["conv4.weight"], sd["conv4.bias"]))
    h = rnd(u[:, :c] * u[:, c:])
    return rnd(y + sd["gamma"] * F.conv2d(h, sd["conv5.weight"], sd["conv5.bias"]))


def dblock_stack(inp, sds, dilations, rnd=_id):
    for sd in sds:
        inp = dblock(inp, sd, dilations, rnd)
    return inp


# ---------------------------------------------------------------- parameter shapes (reference state_dict order) and values
def dblock_shapes(c, n_dil, extra_depth_wise):
    s = OrderedDict()
    s["gamma"] = (1, c, 1, 1)
    s["beta"] = (1, c, 1, 1)
    s["conv1.weight"] = (2 * c, c, 1, 1)
    s["conv1.bias"] = (2 * c,)
    if extra_depth_wise:
        s["extra_conv.weight"] = (2 * c, 2, 3, 3)
        s["extra_conv.bias"] = (2 * c,)
    for i in range(n_dil):
        s[f"branches.{i}.branch.0.weight"] = (2 * c, 1, 3, 3)
        s[f"branches.{i}.branch.0.bias"] = (2 * c,)
    s["sca.1.weight"] = (c, c, 1, 1)
    s["sca.1.bias"] = (c,)
    s["conv3.weight"] = (c, c, 1, 1)
    s["conv3.bias"] = (c,)
    s["conv4.weight"] = (2 * c, c, 1, 1)
    s["conv4.bias"] = (2 * c,)
    s["conv5.weight"] = (c, c, 1, 1)
    s["conv5.bias"] = (c,)
    for n in ("norm1", "norm2"):
        s[n + ".weight"] = (c,)
        s[n + ".bias"] = (c,)
    return s


def make_state(shapes, seed):
    """Seeded float32 values (keys may carry a module prefix, as in a stack of blocks): convs scaled by 1/sqrt(fan-in), LayerNorm weights near 1, biases 0.1 N(0,1); beta and gamma NON-ZERO
    (0.5 + 0.2 N(0,1) in magnitude, random sign): the reference's zero initialisation would hide both halves of the block."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shape in shapes.items():
        z = rng.standard_normal(shape)
        if k.split(".")[-1] in ("beta", "gamma"):
            v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * (0.5 + 0.2 * np.abs(z))
        elif k.split(".")[-2].startswith("norm"):
            v = (1.0 + 0.1 * z) if k.endswith("weight") else 0.1 * z
        elif k.endswith("bias"):
            v = 0.1 * z
        else:
            v = z / np.sqrt(int(np.prod(shape[1:])))
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


def run(inp, cot, sd, dilations, dtype=torch.float64, rnd=_id):
    """Forward and backward of the restatement in ``dtype``: -> {"y", "dx", "g.<key>"...} (detached, in ``dtype``)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = inp.detach().to(dtype).requires_grad_(True)
    y = dblock(rnd(x), p, dilations, rnd)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"g." + k: v.grad for k, v in p.items()})
    return out


def rel_err(got, ref):
    """The per-tensor metric of the GPU parity tests: max |got - ref| / max |ref|."""
    ref = ref.double()
    return float((got.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_darkir.py
# (B, c, H, W), dilations, extra_depth_wise: chosen for where the stencil can go wrong
PARITY_CASES = OrderedDict([
    ("sub_halo", ((2, 32, 5, 7), (1, 4, 9), True)),          # a plane smaller than every halo
    ("row", ((2, 32, 1, 70), (1, 4, 9), True)),              # one-pixel planes
    ("column", ((2, 32, 70, 1), (1, 4, 9), True)),
    ("seams_b3", ((3, 32, 37, 100), (1, 4, 9), True)),       # tile seams, ragged last tiles in both directions, B = 3
    ("seams_c64", ((2, 64, 72, 65), (1, 4, 9), True)),
    ("odd_n", ((2, 32, 9, 11), (1, 4, 9), True)),            # planes not 16-byte aligned
    ("c12", ((2, 12, 12, 20), (1, 4, 9), True)),             # c no multiple of 16
    ("c256", ((1, 256, 8, 8), (1, 4, 9), True)),
    ("max_dil", ((2, 16, 40, 40), (16, 16, 2, 1), True)),    # the maximum dilation, repeated dilations
    ("one_branch", ((2, 16, 20, 20), (1,), False)),          # a single branch without extra_conv
    ("real_plane", ((1, 32, 256, 256), (1, 4, 9), True)),    # one real plane
])


def parity_io(name):
    """-> (state, input, cotangent, dilations) of a parity case, float32."""
    idx = list(PARITY_CASES).index(name)
    (B, c, H, W), dil, extra = PARITY_CASES[name]
    rng = np.random.default_rng(3000 + idx)
    x = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    return make_state(dblock_shapes(c, len(dil), extra), 50 + idx), x, cot, dil


def storage_io(x, cot, dtype):
    """The input and cotangent as a run in ``dtype`` sees them (bf16: rounded once; the fp64 restatement gets the same values)."""
    return x.to(dtype).float(), cot.to(dtype).float()


def host_errors(name, dtype):
    """Error of the restatement evaluated on the host in the device's storage precision (float32 throughout, or float32 with
    every stored activation and activation gradient rounded to bfloat16) against fp64, per tensor, in the parity metric.
    -> ({tensor: error}, the fp64 results)."""
    sd, x, cot, dil = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    ref = run(x, cot, sd, dil)
    got = run(x, cot, sd, dil, torch.float32, _id if dtype == torch.float32 else round_bf16)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
