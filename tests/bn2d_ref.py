"""fp64-capable CPU restatement of the SFHformer Block's BatchNorm2d and scaled residual (TEST INFRASTRUCTURE; SFHformer.py:254-282).

    batch_norm       training: mu, var = the batch mean and BIASED variance of each channel over its n = B H W values;
                     y = w (x - mu) / sqrt(var + eps) + b;  running_mean <- (1 - m) running_mean + m mu,
                     running_var <- (1 - m) running_var + m var n / (n - 1).   eval: mu, var = the running statistics, nothing moves.
    scaled_residual  out = f * scale + x, scale [1, C, 1, 1]

Two forms of the same functions:

``batch_norm`` / ``scaled_residual``                written from the formulas in plain torch, autograd supplies the backward: the
                                                    reference of every comparison.
``batch_norm_device`` / ``scaled_residual_device``  the way csrc/bn2d.hip computes them, forward and backward, operation by operation
                                                    in the working dtype (float32: the host-side error model of the kernels).  A plane is
                                                    cut into chunks of CHUNK elements; thread t of 256 holds SLOTS elements of its chunk
                                                    (slot i = element ((i / V) 256 + t) V + i % V, V = 4 in fp32 and 8 in bf16), adds them in
                                                    slot order, and the 256 threads are summed by a pairwise tree over adjacent
                                                    threads; a chunk gives (mean, M2 about that mean), one channel's B nchunk pairs are
                                                    merged image by image and chunk by chunk (Chan's update); the backward's sums of dy,
                                                    dy xhat and f dout take the same route and are added up in the same order.  Every
                                                    sum here is an explicit ordered sum of elementwise operations (no matmul, no
                                                    library reduction), so the result does not depend on the CPU or its BLAS.
                                                    ``rnd=`` (identity, or ``round_bf16``, which rounds a tensor and the gradient arriving
                                                    at it) is applied exactly where the kernels store in the activation dtype: x, y, f,
                                                    out and the gradients dx, df; statistics, parameters and their gradients are fp32.

PARITY_CASES is built under the precondition of sfh_ref.VAR_FLOOR as it stands: every channel's batch variance of the input as stored
(fp32 and bf16) is 0 or >= VAR_FLOOR x the median channel's.  The seeds are recorded; no case is dropped for it.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch

from darkir_ref import _id, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)
from sfh_ref import VAR_FLOOR

CHUNK, THREADS, SLOTS = 4096, 256, 16
EPS, MOMENTUM = 1e-5, 0.1
TENSORS = ("y", "dx", "dw", "db", "rm", "rv", "out", "df", "ds")


def vec_width(dtype):
    """Elements of one 16-byte access: the V of the kernels' assignment of elements to threads."""
    return 8 if dtype == torch.bfloat16 else 4


# ---------------------------------------------------------------- the formulas
def batch_norm(x, w, b, rm, rv, training, eps=EPS, momentum=MOMENTUM):
    """-> (y, running_mean, running_var after the call)"""
    if training:
        n = x.numel() // x.shape[1]
        mu = x.mean(dim=(0, 2, 3))
        var = ((x - mu.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        rm = (1 - momentum) * rm + momentum * mu.detach()
        rv = (1 - momentum) * rv + momentum * var.detach() * n / (n - 1)
    else:
        mu, var = rm, rv
    y = w.view(1, -1, 1, 1) * (x - mu.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + eps) + b.view(1, -1, 1, 1)
    return y, rm, rv


def scaled_residual(f, x, scale):
    return f * scale.view(1, -1, 1, 1) + x


# ---------------------------------------------------------------- the device's order of summation
def _chunks(t, V):
    """t [B, C, N] -> [B, C, nchunk, T, S]: chunk, thread, slot, zero where the plane has ended.  A plane shorter than a chunk uses
    its first threads and slots only; the rest hold zeros on the device, and adding a zero changes no sum, so T is the next power of
    two that holds the plane (the pairwise tree over 256 threads of which the upper ones are zero is the tree over the lower ones)."""
    B, C, N = t.shape
    nchunk = -(-N // CHUNK)
    A = SLOTS // V
    if nchunk > 1 or N > THREADS * V:
        T, a = THREADS, A
    else:
        T, a = 1, 1
        while T * V < N:
            T *= 2
    size = a * T * V
    pad = torch.zeros(B, C, nchunk * CHUNK if size == CHUNK else size, dtype=t.dtype)
    pad[:, :, :N] = t
    if size == CHUNK:
        v = pad.view(B, C, nchunk, A, THREADS, V)
    else:
        v = pad.view(B, C, 1, a, T, V)
    return v.permute(0, 1, 2, 4, 3, 5).reshape(B, C, nchunk, T, -1)


def _block_sum(v):
    """[.., T, S] -> [..]: each thread adds its slots in order, then the pairwise tree over adjacent threads."""
    acc = v[..., 0]
    for i in range(1, v.shape[-1]):
        acc = acc + v[..., i]
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def _counts(N):
    nchunk = -(-N // CHUNK)
    return [min(N - k * CHUNK, CHUNK) for k in range(nchunk)], nchunk


def chunk_pairs(x, V):
    """The kernels' (mean, M2) pairs of x [B, C, H, W] -> two [B, C, nchunk] tensors."""
    B, C = x.shape[:2]
    v = _chunks(x.reshape(B, C, -1), V)
    N = x.shape[2] * x.shape[3]
    ok = _chunks(torch.ones(1, 1, N, dtype=x.dtype), V) > 0
    cnt, _ = _counts(N)
    mean = _block_sum(v) / torch.tensor([float(c) for c in cnt], dtype=x.dtype)
    d = torch.where(ok, v - mean[..., None, None], torch.zeros((), dtype=x.dtype))
    return mean, _block_sum(d * d)


def merge_pairs(mean_k, m2_k, N):
    """Chan's update over a channel's pairs, image by image and chunk by chunk -> (mean [C], M2 [C], count)."""
    B, C, nchunk = mean_k.shape
    dt = mean_k.dtype
    cnts, _ = _counts(N)
    cnt, mean, m2 = 0, torch.zeros(C, dtype=dt), torch.zeros(C, dtype=dt)
    for b in range(B):
        for k in range(nchunk):
            nb, tot = cnts[k], cnt + cnts[k]
            d = mean_k[b, :, k] - mean
            w = torch.tensor(float(nb), dtype=dt) / torch.tensor(float(tot), dtype=dt)
            mean = mean + d * w
            m2 = (m2 + m2_k[b, :, k]) + (d * d) * (torch.tensor(float(cnt), dtype=dt) * w)
            cnt = tot
    return mean, m2, cnt


def _ordered(part):
    """[B, C, nchunk] -> [C]: one after the other, image by image and chunk by chunk."""
    B, C, nchunk = part.shape
    acc = torch.zeros(C, dtype=part.dtype)
    for b in range(B):
        for k in range(nchunk):
            acc = acc + part[b, :, k]
    return acc


def _c(t):
    return t.view(1, -1, 1, 1)


class _BnDevice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, rm, rv, training, eps, momentum, V, side):
        dt = x.dtype
        N = x.shape[2] * x.shape[3]
        eps_t, mom = torch.tensor(eps, dtype=dt), torch.tensor(momentum, dtype=dt)
        one = torch.tensor(1.0, dtype=dt)
        if training:
            mu, m2, cnt = merge_pairs(*chunk_pairs(x, V), N)
            n = torch.tensor(float(cnt), dtype=dt)
            var = m2 / n
            r = one / torch.sqrt(var + eps_t)
            side["rm"] = (one - mom) * rm + mom * mu
            side["rv"] = (one - mom) * rv + mom * (var * (n / torch.tensor(float(cnt - 1), dtype=dt)))
        else:
            mu, r = rm.clone(), one / torch.sqrt(rv + eps_t)
            side["rm"], side["rv"] = rm.clone(), rv.clone()
        side["mu"], side["r"] = mu, r
        ctx.save_for_backward(x, w, mu, r)
        ctx.training, ctx.V = training, V
        return (x - _c(mu)) * _c(w * r) + _c(b)

    @staticmethod
    def backward(ctx, dy):
        x, w, mu, r = ctx.saved_tensors
        dt, V = x.dtype, ctx.V
        B, C = x.shape[:2]
        xhat = (x - _c(mu)) * _c(r)
        s1 = _ordered(_block_sum(_chunks(dy.reshape(B, C, -1), V)))
        s2 = _ordered(_block_sum(_chunks(dy.reshape(B, C, -1), V) * _chunks(xhat.reshape(B, C, -1), V)))
        g = w * r
        if ctx.training:
            inv_n = torch.tensor(1.0, dtype=dt) / torch.tensor(float(x.numel() // C), dtype=dt)
            dx = _c(g) * ((dy - _c(s1 * inv_n)) - xhat * _c(s2 * inv_n))
        else:
            dx = _c(g) * dy
        return dx, s2, s1, None, None, None, None, None, None, None


class _ResDevice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, x, scale, V):
        ctx.save_for_backward(f, scale)
        ctx.V = V
        return f * _c(scale) + x

    @staticmethod
    def backward(ctx, dout):
        f, scale = ctx.saved_tensors
        B, C = f.shape[:2]
        ds = _ordered(_block_sum(_chunks(f.reshape(B, C, -1), ctx.V) * _chunks(dout.reshape(B, C, -1), ctx.V)))
        return dout * _c(scale), dout, ds.view(scale.shape), None


def batch_norm_device(x, w, b, rm, rv, training, rnd=_id, V=4, eps=EPS, momentum=MOMENTUM, side=None):
    """x as the caller holds it -> (y as stored, running_mean, running_var after the call); ``side`` also receives mu and r."""
    side = {} if side is None else side
    y = rnd(_BnDevice.apply(rnd(x), w, b, rm, rv, training, eps, momentum, V, side))
    return y, side["rm"], side["rv"]


def scaled_residual_device(f, x, scale, rnd=_id, V=4):
    return rnd(_ResDevice.apply(rnd(f), rnd(x), scale.reshape(-1), V))


def run(io, training, dtype=torch.float64, rnd=_id, device=False, V=4):
    """Both functions, forward and backward, on one case's tensors in ``dtype``: -> {name: tensor} over TENSORS (detached; rm / rv:
    the running statistics after the call; dx: BatchNorm's input gradient; out, df, ds: the scaled residual's)."""
    t = {k: v.detach().to(dtype) for k, v in io.items()}
    x, f, xr = (t[k].clone().requires_grad_(True) for k in ("x", "f", "x"))
    w, b, s = (t[k].clone().requires_grad_(True) for k in ("w", "b", "scale"))
    if device:
        y, rm, rv = batch_norm_device(x, w, b, t["rm"], t["rv"], training, rnd, V)
        out = scaled_residual_device(f, xr, s, rnd, V)
    else:
        y, rm, rv = batch_norm(x, w, b, t["rm"], t["rv"], training)
        out = scaled_residual(f, xr, s)
    y.backward(t["cot"])
    out.backward(t["cot"])
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad, "db": b.grad, "rm": rm.detach(), "rv": rv.detach(), "out": out.detach(),
            "df": f.grad, "ds": s.grad.reshape(-1)}


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_bn2d.py
# name -> ((B, C, H, W), seed, kind).  CHUNK = 4096 is the plan's chunk size (tests/test_bn2d_cabi.py holds the two together).
# kind "dc": the input of "ragged" plus 128 standard deviations; "const": channel 1 equal to 2.0 everywhere (batch variance exactly 0).
PARITY_CASES = OrderedDict([
    ("n2", ((2, 3, 1, 1), 8100, "plain")),          # n = 2, the minimum count: n / (n - 1) = 2
    ("odd", ((2, 3, 5, 7), 8101, "plain")),         # N = 35: plane bases off 16 bytes, the element-by-element form
    ("ch_m1", ((1, 2, 63, 65), 8102, "plain")),     # N = CHUNK - 1 (odd: the narrow form)
    ("ch", ((1, 2, 64, 64), 8103, "plain")),        # N = CHUNK: one full chunk
    ("ch_p1", ((1, 2, 17, 241), 8104, "plain")),    # N = CHUNK + 1: a second chunk of ONE element
    ("ragged", ((3, 5, 82, 100), 8105, "plain")),   # N = 2 CHUNK + 8: nine partials per channel, counts 4096, 4096, 8
    ("c1", ((2, 1, 4, 4), 8106, "plain")),          # C = 1
    ("c257", ((2, 257, 2, 2), 8107, "plain")),      # C one past a finish workgroup's 256 threads
    ("dc", ((3, 5, 82, 100), 8105, "dc")),          # a sum x^2 - (sum x)^2 form loses the variance here
    ("const", ((2, 4, 6, 10), 8108, "const")),      # N = 60: 16-byte rows in fp32, not in bf16
    ("grid", ((257, 4096, 1, 1), 8109, "plain")),   # 1 052 672 chunks of one element: past the 2^20 workgroups of one launch
])
DC_OFFSET = 128.0


def parity_io(name):
    """-> {x, f, cot, w, b, scale, rm, rv} of a parity case, float32; the running statistics are seeded and non-trivial."""
    (B, C, H, W), seed, kind = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    x, f, cot = (torch.from_numpy(rng.standard_normal((B, C, H, W))).float() for _ in range(3))
    if kind == "dc":
        x = x + DC_OFFSET
    if kind == "const":
        x[:, 1] = 2.0
    vec = lambda scale, shift: torch.from_numpy(shift + scale * rng.standard_normal(C)).float()   # noqa: E731
    return {"x": x, "f": f, "cot": cot, "w": vec(0.3, 1.0), "b": vec(0.1, 0.0), "scale": vec(0.5, 0.0), "rm": vec(0.2, 0.0),
            "rv": torch.from_numpy(0.5 + rng.random(C)).float()}


def channel_variances(x):
    """fp64 batch variance of every channel."""
    x = x.double()
    return ((x - x.mean(dim=(0, 2, 3), keepdim=True)) ** 2).mean(dim=(0, 2, 3))


def variances_ok(x):
    v = channel_variances(x)
    return bool(((v == 0) | (v >= VAR_FLOOR * v.median())).all())


def _checked(cases):
    for name in cases:
        x = parity_io(name)["x"]
        for dtype in (torch.float32, torch.bfloat16):
            assert variances_ok(x.to(dtype).float()), f"{name}: a channel's variance is below VAR_FLOOR x the median (pick another seed)"
    return cases


PARITY_CASES = _checked(PARITY_CASES)


def stored(io, dtype):
    """The case as a run in ``dtype`` sees it: activations and cotangent rounded once, parameters and statistics untouched."""
    return {k: (v.to(dtype).float() if k in ("x", "f", "cot") else v) for k, v in io.items()}


def host_errors(name, dtype, training):
    """Error of the DEVICE form evaluated on the host in the device's storage precision against the fp64 formulas, per tensor, in
    the parity metric (max |delta| / max |ref|).  -> ({tensor: error}, the fp64 results)."""
    io = stored(parity_io(name), dtype)
    ref = run(io, training)
    got = run(io, training, torch.float32, _id if dtype == torch.float32 else round_bf16, device=True, V=vec_width(dtype))
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
