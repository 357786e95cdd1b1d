"""fp64-capable CPU restatement of DarkIR's FreMLP (TEST INFRASTRUCTURE), in plain torch so that autograd supplies the backward.

    Z = rfft2(x);  mag = |Z|;  pha = angle(Z)
    mag' = conv1x1(LeakyReLU_0.1(conv1x1(mag)))            nc -> expand nc -> nc, both with bias
    out = irfft2(mag' cos pha + i mag' sin pha, s=(H, W))

Two forms of the same function:

``fremlp``        written from the formulas with ``torch.fft``: the reference of every comparison.
``fremlp_dense``  the way the device computes it: explicit cos / sin DFT matrices (two real matrix products per stage), the polar
                  form as mag = sqrt(Re^2 + Im^2) and u = Z / mag with u = (1, 0) and zero gradient where mag == 0, the inverse as
                  out[y,x] = 1/(HW) sum_l w_l Re(e^{+2 pi i l x / W} sum_k e^{+2 pi i k y / H} Y[k,l]), w_l = 1 at l = 0 and (even
                  W) l = W/2, else 2.  ``rnd=`` is applied to x and out (and through them to the cotangent and dx): identity, or
                  ``round_bf16`` for bfloat16 storage.  Evaluated in float32 it is the host-side error model of the kernels: a
                  dense DFT in fp32 carries 1-4x the error of an FFT, so the GPU bounds come from this form, not from torch.fft.

Every function takes a flat ``{name: tensor}`` dict with the reference's state_dict keys (``process1.0.weight`` ...).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from darkir_ref import _id, make_state, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)

SLOPE = 0.1
FLOOR = 2e-4          # the parity cases' precondition: min |Z| >= FLOOR * rms |Z| (the phase gradient divides by |Z|)


def mlp(mag, sd):
    h = F.leaky_relu(F.conv2d(mag, sd["process1.0.weight"], sd["process1.0.bias"]), SLOPE)
    return F.conv2d(h, sd["process1.2.weight"], sd["process1.2.bias"])


def fremlp(x, sd):
    H, W = x.shape[-2:]
    z = torch.fft.rfft2(x, norm="backward")
    mag, pha = torch.abs(z), torch.angle(z)
    mag = mlp(mag, sd)
    return torch.fft.irfft2(torch.complex(mag * torch.cos(pha), mag * torch.sin(pha)), s=(H, W), norm="backward")


def dft_tables(n, cols, dtype):
    """cos and sin of 2 pi ((a b) mod n) / n for a < n, b < cols, formed in fp64 from the integer-reduced angle, then cast."""
    r = (torch.arange(n).view(-1, 1) * torch.arange(cols).view(1, -1)) % n
    ang = 2.0 * math.pi * r.double() / n
    c, s = torch.cos(ang), torch.sin(ang)
    # exact at every multiple of a quarter turn, as the device's tables are
    c = torch.where((4 * r) % n == 0, torch.round(c), c)
    s = torch.where((4 * r) % n == 0, torch.round(s), s)
    return c.to(dtype), s.to(dtype)


def col_weights(W, dtype):
    K = W // 2 + 1
    w = torch.full((K,), 2.0, dtype=dtype)
    w[0] = 1.0
    if W % 2 == 0:
        w[W // 2] = 1.0
    return w


def r2c_dense(x):
    """-> (Re Z, Im Z) of rfft2(x), [..., H, K]."""
    H, W = x.shape[-2:]
    K = W // 2 + 1
    cw, sw = dft_tables(W, K, x.dtype)
    ch, sh = dft_tables(H, H, x.dtype)
    tre, tim = x @ cw, -(x @ sw)                          # T = x . E_W
    return ch @ tre + sh @ tim, ch @ tim - sh @ tre       # Z = E_H . T


def c2r_dense(yre, yim, W):
    """irfft2(yre + i yim, s=(H, W)) for any Y (the edge columns' imaginary parts drop out of the formula)."""
    H = yre.shape[-2]
    K = W // 2 + 1
    cw, sw = dft_tables(W, K, yre.dtype)
    ch, sh = dft_tables(H, H, yre.dtype)
    wl = col_weights(W, yre.dtype)
    vre, vim = ch @ yre - sh @ yim, ch @ yim + sh @ yre   # V = conj(E_H) . Y
    return ((vre * wl) @ cw.t() - (vim * wl) @ sw.t()) / (H * W)


def polar(zre, zim):
    """-> (mag, Re u, Im u); u = (1, 0) and no gradient where mag == 0."""
    s2 = zre * zre + zim * zim
    live = s2 > 0
    mag = torch.sqrt(torch.where(live, s2, torch.ones_like(s2))) * live
    den = torch.where(live, mag, torch.ones_like(mag))
    return mag, torch.where(live, zre / den, torch.ones_like(zre)), torch.where(live, zim / den, torch.zeros_like(zim))


def fremlp_dense(x, sd, rnd=_id):
    x = rnd(x)
    zre, zim = r2c_dense(x)
    mag, ur, ui = polar(zre, zim)
    mag = mlp(mag, sd)
    return rnd(c2r_dense(mag * ur, mag * ui, x.shape[-1]))


# ---------------------------------------------------------------- parameter shapes (reference state_dict order) and values
def fremlp_shapes(nc, expand=2):
    s = OrderedDict()
    s["process1.0.weight"] = (expand * nc, nc, 1, 1)
    s["process1.0.bias"] = (expand * nc,)
    s["process1.2.weight"] = (nc, expand * nc, 1, 1)
    s["process1.2.bias"] = (nc,)
    return s


def run(x, cot, sd, dtype=torch.float64, rnd=_id, dense=False):
    """Forward and backward in ``dtype``: -> {"y", "dx", "g.<key>"...} (detached, in ``dtype``)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xr = x.detach().to(dtype).requires_grad_(True)
    y = fremlp_dense(xr, p, rnd) if dense else fremlp(xr, p)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad}
    out.update({"g." + k: v.grad for k, v in p.items()})
    return out


def spectrum_floor(x):
    """min |Z| / rms |Z| of the fp64 spectrum of x."""
    a = torch.fft.rfft2(x.double()).abs()
    return float(a.min() / a.pow(2).mean().sqrt())


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_fremlp.py
# (B, nc, H, W), expand, seed.  The seeds are recorded: with them every case's fp64 spectrum (of the fp32 and of the bf16-rounded
# input) keeps min |Z| >= FLOOR * rms |Z| (tools/fremlp_bounds.py prints the margins).
PARITY_CASES = OrderedDict([
    ("tiny", ((2, 4, 2, 2), 2, 4100)),          # K = 2, every twiddle exact
    ("thin_h", ((2, 16, 2, 70), 2, 4101)),      # the smallest H
    ("thin_w", ((2, 16, 70, 2), 2, 4102)),      # the smallest W
    ("odd", ((2, 8, 5, 7), 2, 4103)),           # odd H, odd W, no Nyquist column
    ("seams", ((3, 5, 100, 130), 2, 4104)),     # several 64-row tiles with ragged ends, K = 66 over two column tiles, B = 3, nc = 5
    ("c256", ((1, 256, 8, 8), 2, 4117)),        # hidden width 512 (seed 4105 misses the floor once rounded to bf16)
    ("expand1", ((2, 12, 9, 16), 1, 4106)),
    ("expand3", ((2, 12, 9, 16), 3, 4107)),
    ("plane256", ((1, 4, 256, 256), 2, 4108)),  # one real plane
    ("max", ((1, 2, 512, 512), 2, 4109)),       # the size limit
])


def parity_io(name):
    """-> (state, input, cotangent, expand) of a parity case, float32; inputs are standard normal, like LayerNorm2d outputs."""
    (B, nc, H, W), expand, seed = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, nc, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, nc, H, W))).float()
    return make_state(fremlp_shapes(nc, expand), seed + 50), x, cot, expand


def host_errors(name, dtype):
    """Error of the DENSE form evaluated on the host in the device's storage precision (float32 throughout, or float32 with x,
    out, the cotangent and dx rounded to bfloat16) against the fp64 torch.fft form, per tensor, in the parity metric.
    -> ({tensor: error}, the fp64 results)."""
    sd, x, cot, _ = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    ref = run(x, cot, sd)
    got = run(x, cot, sd, torch.float32, _id if dtype == torch.float32 else round_bf16, dense=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
