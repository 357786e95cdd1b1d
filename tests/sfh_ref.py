"""fp64-capable CPU restatement of SFHformer's FourierUnit (TEST INFRASTRUCTURE), in plain torch so that autograd supplies the
backward.  c = in_channels = out_channels, C2 = 2c, K = W/2 + 1, G groups, S = C2 / G.

    Z = rfft2(x, norm='ortho');  t0[:, 2i + d] = Re Z_i (d = 0) / Im Z_i (d = 1)
    t1 = BatchNorm(t0)   training: batch mean and biased variance over the B H K bins of a channel; running_mean <- 0.9 rm + 0.1 mean,
                         running_var <- 0.9 rv + 0.1 var n / (n - 1).  eval: the running statistics, nothing updated
    t  = fpe(t1) + t1    depthwise 3x3, zero padding 1, bias
    s  = softmax_g(Ww t + bw);  u = fdc(t) (grouped 1x1, G groups, C2 outputs each);  pre[k] = sum_g s_g u[g, k]
    out = irfft2(gelu(pre) de-interleaved, s=(H, W), norm='ortho')

Two forms of the same function:

``fourier_unit``        written from the formulas with ``torch.fft`` and the grouped conv materialised: the reference of every
                        comparison.
``fourier_unit_dense``  the way the device computes it: the dense cos / sin DFT matrices of ``fremlp_ref``, channels in planar order
                        (all Re, then all Im) with every parameter read through the permutation, the statistics of the UNSCALED
                        spectrum with the ortho scale folded into the reciprocal deviation, the grouped conv and the gate folded
                        into one dense C2 x C2 product on the gate-scaled input plus a C2 x G product on s.  ``rnd=`` is applied to x
                        and out (identity, or ``round_bf16``).  Evaluated in float32 it is the host-side error model of the kernels.

State dicts carry the reference's keys: the eight parameters, then ``bn.running_mean`` / ``bn.running_var``.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from darkir_ref import _id, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)
from fremlp_ref import PARITY_CASES as FRE_CASES, c2r_dense, r2c_dense

EPS, MOMENTUM = 1e-5, 0.1
VAR_FLOOR = 1e-3      # the parity cases' precondition: every channel's batch variance is 0 or >= VAR_FLOOR x the median channel's
PARAMS = ("bn.weight", "bn.bias", "fdc.weight", "fdc.bias", "weight.0.weight", "weight.0.bias", "fpe.weight", "fpe.bias")


def fu_shapes(c, G):
    s = OrderedDict()
    s["bn.weight"] = (2 * c,)
    s["bn.bias"] = (2 * c,)
    s["fdc.weight"] = (2 * c * G, 2 * c // G, 1, 1)
    s["fdc.bias"] = (2 * c * G,)
    s["weight.0.weight"] = (G, 2 * c, 1, 1)
    s["weight.0.bias"] = (G,)
    s["fpe.weight"] = (2 * c, 1, 3, 3)
    s["fpe.bias"] = (2 * c,)
    return s


def state_dict_layout(c, G):
    """(key, shape) in the reference's state_dict order (buffers sit behind their module's parameters)."""
    s = fu_shapes(c, G)
    out = [("bn.weight", s["bn.weight"]), ("bn.bias", s["bn.bias"]), ("bn.running_mean", (2 * c,)), ("bn.running_var", (2 * c,)),
           ("bn.num_batches_tracked", ())]
    return out + [(k, s[k]) for k in PARAMS[2:]]


def make_state(c, G, seed, trivial_stats=True):
    """Seeded float32 parameters (convs scaled by 1/sqrt(fan-in), gamma near 1 with either sign possible only through its spread,
    biases 0.1 N(0,1)) and running statistics: 0 / 1 as a fresh module has them, or seeded non-trivial ones."""
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shape in fu_shapes(c, G).items():
        z = rng.standard_normal(shape)
        if k == "bn.weight":
            v = 1.0 + 0.3 * z
        elif k.endswith("bias"):
            v = 0.1 * z
        else:
            v = z / math.sqrt(int(np.prod(shape[1:])))
        sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    zm, zv = rng.standard_normal(2 * c), rng.standard_normal(2 * c)
    sd["bn.running_mean"] = torch.zeros(2 * c) if trivial_stats else torch.from_numpy((0.2 * zm).astype(np.float32))
    sd["bn.running_var"] = torch.ones(2 * c) if trivial_stats else torch.from_numpy((0.3 + 0.4 * np.abs(zv)).astype(np.float32))
    return sd


def module_state(sd, steps=0):
    """The dict ``load_state_dict(strict=True)`` takes: ``sd`` plus num_batches_tracked."""
    out = OrderedDict(sd)
    out["bn.num_batches_tracked"] = torch.tensor(steps, dtype=torch.long)
    return out


def batch_norm(t0, w, b, rm, rv, training):
    """-> (t1, running_mean after, running_var after)"""
    if training:
        n = t0.numel() // t0.shape[1]
        mean = t0.mean(dim=(0, 2, 3))
        var = ((t0 - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        new_rm = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
        new_rv = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * n / (n - 1)
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    xhat = (t0 - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS)
    return xhat * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1), new_rm, new_rv


def fourier_unit(x, sd, G, training=True):
    B, c, H, W = x.shape
    z = torch.fft.rfft2(x, norm="ortho")
    t0 = torch.stack([z.real, z.imag], dim=2).reshape(B, 2 * c, H, -1)
    t1, rm, rv = batch_norm(t0, sd["bn.weight"], sd["bn.bias"], sd["bn.running_mean"], sd["bn.running_var"], training)
    t = F.conv2d(t1, sd["fpe.weight"], sd["fpe.bias"], padding=1, groups=2 * c) + t1
    s = torch.softmax(F.conv2d(t, sd["weight.0.weight"], sd["weight.0.bias"]), dim=1)
    u = F.conv2d(t, sd["fdc.weight"], sd["fdc.bias"], groups=G).view(B, G, 2 * c, H, -1)
    o = F.gelu((u * s.unsqueeze(2)).sum(dim=1)).view(B, c, 2, H, -1)
    return torch.fft.irfft2(torch.complex(o[:, :, 0], o[:, :, 1]), s=(H, W), norm="ortho"), rm, rv


def planar_perm(c):
    """j(p): the interleaved channel that planar channel p = d c + i holds."""
    p = torch.arange(2 * c)
    return 2 * (p % c) + p // c


def fold(sd, c, G):
    """-> (W' [C2, C2] with W'[k, g S + jl] = fdc.weight[g C2 + k, jl], the bias matrix [C2, G] with column g = fdc.bias[g C2 : (g+1) C2])"""
    C2, S = 2 * c, 2 * c // G
    w = sd["fdc.weight"].view(G, C2, S).permute(1, 0, 2).reshape(C2, C2)
    return w, sd["fdc.bias"].view(G, C2).t()


def fourier_unit_dense(x, sd, G, training=True, rnd=_id):
    x = rnd(x)
    B, c, H, W = x.shape
    C2, S = 2 * c, 2 * c // G
    j = planar_perm(c)
    alpha = 1.0 / math.sqrt(H * W)
    zre, zim = r2c_dense(x)
    z = torch.cat([zre, zim], dim=1)                                 # unscaled, planar order
    rm0, rv0 = sd["bn.running_mean"], sd["bn.running_var"]
    if training:
        n = B * z.shape[-2] * z.shape[-1]
        mu = z.mean(dim=(0, 2, 3))
        var = ((z - mu.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        r = alpha / torch.sqrt(alpha * alpha * var + EPS)
        rm, rv = rm0.clone(), rv0.clone()
        rm[j] = ((1 - MOMENTUM) * rm0[j] + MOMENTUM * (alpha * mu.detach())).to(rm0.dtype)
        rv[j] = ((1 - MOMENTUM) * rv0[j] + MOMENTUM * (alpha * alpha * var.detach() * n / (n - 1))).to(rv0.dtype)
    else:
        mu, r, rm, rv = rm0[j] / alpha, alpha / torch.sqrt(rv0[j] + EPS), rm0, rv0
    t1 = sd["bn.weight"][j].view(1, -1, 1, 1) * ((z - mu.view(1, -1, 1, 1)) * r.view(1, -1, 1, 1)) + sd["bn.bias"][j].view(1, -1, 1, 1)
    t = F.conv2d(t1, sd["fpe.weight"][j], sd["fpe.bias"][j], padding=1, groups=C2) + t1
    ww = sd["weight.0.weight"].view(G, C2)[:, j]
    s = torch.softmax(torch.einsum("gp,bphl->bghl", ww, t) + sd["weight.0.bias"].view(1, -1, 1, 1), dim=1)
    wf, bf = fold(sd, c, G)
    ts = s[:, j // S] * t                                            # s_{g(j)} t[j]
    pre = torch.einsum("kp,bphl->bkhl", wf[j][:, j], ts) + torch.einsum("kg,bghl->bkhl", bf[j], s)
    o = F.gelu(pre) * math.sqrt(H * W)
    return rnd(c2r_dense(o[:, :c], o[:, c:], W)), rm, rv


def run(x, cot, sd, G, training=True, dtype=torch.float64, rnd=_id, dense=False):
    """Forward and backward in ``dtype``: -> {"y", "dx", "g.<key>"..., "rm", "rv"} (detached; rm / rv: the running statistics after
    the call)."""
    p = {k: v.detach().to(dtype).requires_grad_(k in PARAMS) for k, v in sd.items()}
    xr = x.detach().to(dtype).requires_grad_(True)
    if dense:
        y, rm, rv = fourier_unit_dense(xr, p, G, training, rnd)
    else:
        y, rm, rv = fourier_unit(xr, p, G, training)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad, "rm": rm.detach(), "rv": rv.detach()}
    out.update({"g." + k: p[k].grad for k in PARAMS})
    return out


def channel_variances(x):
    """fp64 batch variance of every spectral channel (ortho scale), interleaved order."""
    z = torch.fft.rfft2(x.double(), norm="ortho")
    B, c = x.shape[:2]
    t0 = torch.stack([z.real, z.imag], dim=2).reshape(B, 2 * c, -1)
    mean = t0.mean(dim=(0, 2), keepdim=True)
    return ((t0 - mean) ** 2).mean(dim=(0, 2))


def variances_ok(x):
    v = channel_variances(x)
    return bool(((v == 0) | (v >= VAR_FLOOR * v.median())).all())


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_sfh_fu.py
# (B, c, H, W), G, seed, kind.  kind: "train", "eval" (seeded running statistics), "dc" (input = seeded + 4.0), "zero" (input
# channel 1 all zero).  With the recorded seeds every case keeps the variance precondition in both storage precisions.
_SEAMS_HW = FRE_CASES["seams"][0][2:]
PARITY_CASES = OrderedDict([
    ("odd", ((2, 6, 5, 7), 4, 5100, "train")),          # no Nyquist column; S = 3 splits a complex pair
    ("even", ((2, 8, 8, 12), 4, 5101, "train")),        # Nyquist row and column, which c2r must drop
    ("g1", ((1, 4, 4, 4), 1, 5102, "train")),           # softmax of one logit is exactly 1; 12 bins per channel
    ("g2", ((2, 4, 6, 10), 2, 5103, "train")),
    ("seams", ((3, 10) + tuple(_SEAMS_HW), 4, 5104, "train")),   # 19800 bins (no multiple of 256), 6600 per plane (ragged 2048-bin chunks), 2c = 20
    ("wide", ((1, 256, 4, 6), 4, 5105, "train")),       # 2c = 512, the channel limit
    ("dc", ((2, 8, 16, 16), 4, 5106, "dc")),            # a DC bin 80x the other bins in every Re plane
    ("zero", ((2, 8, 6, 8), 4, 5107, "zero")),          # batch variance exactly 0, xhat = 0
    ("eval", ((2, 8, 6, 8), 4, 5108, "eval")),          # running statistics, nothing updated
])


def parity_io(name):
    """-> (state, input, cotangent, G, training) of a parity case, float32."""
    (B, c, H, W), G, seed, kind = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    if kind == "dc":
        x = x + 4.0
    if kind == "zero":
        x[:, 1] = 0
    return make_state(c, G, seed + 50, trivial_stats=kind != "eval"), x, cot, G, kind != "eval"


def host_errors(name, dtype):
    """Error of the DENSE form evaluated on the host in the device's storage precision (float32 throughout, or float32 with x, out,
    the cotangent and dx rounded to bfloat16) against the fp64 torch.fft form, per tensor, in the parity metric.
    -> ({tensor: error}, the fp64 results)."""
    sd, x, cot, G, training = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    ref = run(x, cot, sd, G, training)
    got = run(x, cot, sd, G, training, torch.float32, _id if dtype == torch.float32 else round_bf16, dense=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
