"""fp64-capable CPU restatement of SFHformer's TokenMixer_For_Gloal and Mixer (TEST INFRASTRUCTURE), in plain torch so that autograd
supplies the backward.  The FourierUnit comes from ``sfh_ref``, the local mixer from ``sfh_ffn_ref``.

    gloal  u1 = Wi b + bi [2 dim];  p = gelu(u1);  f = FourierUnit(2 dim, 2 dim, groups 4)(p);  r = f + p;  u2 = Wf r + bf [dim];
           q = gelu(u2)
    mixer  [a; b] = conv_init(x);  l = local(a);  q = gloal(b);  g = gelu(cat(l, q));  m = mean over the plane of g;
           s = sigmoid(W2 relu(W1 m + b1) + b2);  out = Wc (s g) + bc

Two forms of the same functions:

``gloal`` / ``mixer``                written from the formulas with ``F.conv2d`` and ``sfh_ref.fourier_unit``: the reference of every
                                     comparison.
``gloal_device`` / ``mixer_device``  the way the device computes them.  ``rnd=`` (identity, or ``round_bf16``, which rounds a tensor
                                     and the gradient arriving at it) is applied exactly where the kernels store a tensor in the
                                     activation dtype: x, a, b, l, u1, r, u2 and the output, with their gradients dx, da, db, dl, du1,
                                     dr, du2 and the cotangent; p and g are stored in the forward but the gradients arriving at them
                                     are sums formed in fp32 registers (dr + dp into du1; e + dm / N into dl and du2), of which only
                                     dr, the FourierUnit's input gradient dp and e = (Wc diag(s))^T dout are stored; q is never
                                     stored in the mixer.  Every 1x1 product reads its weight matrix through the hook (the matrix-
                                     core path keeps a packed image in the activation dtype), forward and transposed; that includes
                                     the per-image folded weight Wc diag(s_b), whose gradient (the per-image Gram) is summed
                                     along the pixel axis in the Gram kernel's order (``_PerImageProduct``).  m (the mean of g AS STORED), the hidden layer, s, the
                                     gate's backward, biases and every accumulation are fp32 and unrounded.  Evaluated in float32
                                     this form is the host-side error model of the kernels.

State dicts carry the reference's keys in its order (buffers behind their module's parameters).

Two preconditions are asserted while PARITY_CASES is built (``_checked``), with the recorded seeds; no case is dropped for them:
 1. ``sfh_ref.variances_ok`` on p, the FourierUnit's actual input (VAR_FLOOR as it stands);
 2. (mixer) every hidden pre-activation W1 m + b1 of every image is at least HIDDEN_MARGIN x its own error in the bf16 device form
    (host model against fp64) away from 0: ReLU's gradient is discontinuous there.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import sfh_ffn_ref as FR
import sfh_ref as S
from darkir_ref import _id, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)
from sfh_ffn_ref import PACK_ELEMS, _RoundFwd, _pw, check  # noqa: F401

GROUPS = 4
HIDDEN_MARGIN = 8.0
FU_PARAMS = tuple("FFC." + k for k in S.PARAMS)
GLOBAL_PARAMS = ("conv_init.0.weight", "conv_init.0.bias", "conv_fina.0.weight", "conv_fina.0.bias") + FU_PARAMS
MIXER_PARAMS = (tuple("mixer_local." + k for k in FR.LOCAL_PARAMS) + tuple("mixer_gloal." + k for k in GLOBAL_PARAMS) +
                ("ca_conv.0.weight", "ca_conv.0.bias", "ca.1.weight", "ca.1.bias", "ca.3.weight", "ca.3.bias", "conv_init.0.weight",
                 "conv_init.0.bias"))
PARAMS = {"global": GLOBAL_PARAMS, "mixer": MIXER_PARAMS}
RM = {"global": "FFC.bn.running_mean", "mixer": "mixer_gloal.FFC.bn.running_mean"}
RV = {"global": "FFC.bn.running_var", "mixer": "mixer_gloal.FFC.bn.running_var"}


def state_dict_layout(kind, dim):
    """(key, shape) in the reference's state_dict order, num_batches_tracked included."""
    if kind == "global":
        out = [("conv_init.0.weight", (2 * dim, dim, 1, 1)), ("conv_init.0.bias", (2 * dim,)), ("conv_fina.0.weight", (dim, 2 * dim, 1, 1)),
               ("conv_fina.0.bias", (dim,))]
        return out + [("FFC." + k, s) for k, s in S.state_dict_layout(2 * dim, GROUPS)]
    out = [("mixer_local." + k, s) for k, s in FR.state_dict_layout("local", dim)]
    out += [("mixer_gloal." + k, s) for k, s in state_dict_layout("global", dim)]
    return out + [("ca_conv.0.weight", (dim, 2 * dim, 1, 1)), ("ca_conv.0.bias", (dim,)), ("ca.1.weight", (dim, 2 * dim, 1, 1)),
                  ("ca.1.bias", (dim,)), ("ca.3.weight", (2 * dim, dim, 1, 1)), ("ca.3.bias", (2 * dim,)),
                  ("conv_init.0.weight", (2 * dim, dim, 1, 1)), ("conv_init.0.bias", (2 * dim,))]


def make_state(kind, dim, seed, trivial_stats=True):
    """Seeded float32 parameters, drawn the way ``sfh_ref.make_state`` draws them (convs N(0,1) / sqrt(fan-in), biases 0.1 N(0,1),
    BatchNorm's gamma 1 + 0.3 N(0,1)), and running statistics 0 / 1 or seeded non-trivial ones; no num_batches_tracked."""
    rng = np.random.default_rng(seed)
    fu = S.make_state(2 * dim, GROUPS, seed + 1, trivial_stats)
    loc = FR.make_state("local", dim, seed + 2) if kind == "mixer" else {}
    sd = OrderedDict()
    for k, shape in state_dict_layout(kind, dim):
        tail = k.split("FFC.")[-1]
        if k.endswith("num_batches_tracked"):
            continue
        if "FFC." in k:
            sd[k] = fu[tail]
        elif k.startswith("mixer_local."):
            sd[k] = loc[k[len("mixer_local."):]]
        else:
            z = rng.standard_normal(shape)
            v = 0.1 * z if k.endswith("bias") else z / math.sqrt(int(np.prod(shape[1:])))
            sd[k] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


def module_state(kind, sd, steps=0):
    """The dict ``load_state_dict(strict=True)`` takes: ``sd`` plus num_batches_tracked, in the reference's order."""
    dim = sd["conv_init.0.weight"].shape[1]
    out = OrderedDict()
    for k, _ in state_dict_layout(kind, dim):
        out[k] = torch.tensor(steps, dtype=torch.long) if k.endswith("num_batches_tracked") else sd[k]
    return out


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


# ---------------------------------------------------------------- the formulas
def gloal(x, sd, training=True, tap=None):
    p = F.gelu(F.conv2d(x, sd["conv_init.0.weight"], sd["conv_init.0.bias"]))
    f, rm, rv = S.fourier_unit(p, sub(sd, "FFC."), GROUPS, training)
    if tap is not None:
        tap["p"] = p.detach()
    return F.gelu(F.conv2d(f + p, sd["conv_fina.0.weight"], sd["conv_fina.0.bias"])), rm, rv


def mixer(x, sd, training=True, tap=None):
    dim = x.shape[1]
    h = F.conv2d(x, sd["conv_init.0.weight"], sd["conv_init.0.bias"])
    l = FR.local(h[:, :dim], sub(sd, "mixer_local."))
    q, rm, rv = gloal(h[:, dim:], sub(sd, "mixer_gloal."), training, tap)
    g = F.gelu(torch.cat([l, q], dim=1))
    pre = F.conv2d(g.mean(dim=(2, 3), keepdim=True), sd["ca.1.weight"], sd["ca.1.bias"])
    s = torch.sigmoid(F.conv2d(F.relu(pre), sd["ca.3.weight"], sd["ca.3.bias"]))
    if tap is not None:
        tap["pre"] = pre.detach()
    return F.conv2d(s * g, sd["ca_conv.0.weight"], sd["ca_conv.0.bias"]), rm, rv


# ---------------------------------------------------------------- the device's formulation
def _gloal_u2(b, sd, training, rnd, tap):
    """b as stored -> u2 as stored"""
    u1 = rnd(_pw(b, sd["conv_init.0.weight"], sd["conv_init.0.bias"], rnd))
    p = _RoundFwd.apply(F.gelu(u1), rnd)
    f, rm, rv = S.fourier_unit_dense(p, sub(sd, "FFC."), GROUPS, training, rnd)
    if tap is not None:
        tap["p"] = p.detach()
    r = rnd(f + p)
    return rnd(_pw(r, sd["conv_fina.0.weight"], sd["conv_fina.0.bias"], rnd)), rm, rv


class _PerImageProduct(torch.autograd.Function):
    """out[b] = M[b] g[b] (M [B, m, k], g [B, k, H, W]).  The gradient at M is the per-image Gram dout_b g_b^T summed the way the
    device's Gram kernel sums it: along the pixel axis, one matrix-core step of ``group`` pixels after the other into one
    accumulator (4 pixels a step on fp32 operands, 32 on bf16).  ONE chain over the whole plane: an upper model, not the device's exact
    order (the kernel splits the pixel axis over workgroups by its plan and a second kernel sums the partial tiles, which only
    shortens the chains).  torch's own contraction sums in blocks and came out an order of
    magnitude more accurate than any sequential fp32 sum over a few thousand pixels; ds = sum_m Wc . P_b and the whole gate backward
    behind it cancel heavily, so that difference decided their error."""

    @staticmethod
    def forward(ctx, M, g, group):
        ctx.save_for_backward(M, g)
        ctx.group = group
        return torch.einsum("bmk,bkhw->bmhw", M, g)

    @staticmethod
    def backward(ctx, dout):
        M, g = ctx.saved_tensors
        d, gg = dout.flatten(2), g.flatten(2)
        acc = torch.zeros_like(M)
        for n0 in range(0, d.shape[2], ctx.group):
            acc = acc + torch.einsum("bmn,bkn->bmk", d[:, :, n0:n0 + ctx.group], gg[:, :, n0:n0 + ctx.group])
        return acc, torch.einsum("bmk,bmhw->bkhw", M, dout), None


def gloal_device(x, sd, training=True, rnd=_id, tap=None):
    u2, rm, rv = _gloal_u2(rnd(x), sd, training, rnd, tap)
    return rnd(F.gelu(u2)), rm, rv


def mixer_device(x, sd, training=True, rnd=_id, tap=None):
    dim = x.shape[1]
    h = rnd(_pw(rnd(x), sd["conv_init.0.weight"], sd["conv_init.0.bias"], rnd))       # two products on the device: a and b
    l = FR.local_device(h[:, :dim], sub(sd, "mixer_local."), rnd)
    u2, rm, rv = _gloal_u2(h[:, dim:], sub(sd, "mixer_gloal."), training, rnd, tap)
    g = _RoundFwd.apply(F.gelu(torch.cat([l, F.gelu(u2)], dim=1)), rnd)
    m = g.mean(dim=(2, 3))
    pre = m @ sd["ca.1.weight"][:, :, 0, 0].t() + sd["ca.1.bias"]
    s = torch.sigmoid(F.relu(pre) @ sd["ca.3.weight"][:, :, 0, 0].t() + sd["ca.3.bias"])
    if tap is not None:
        tap["pre"] = pre.detach()
    fold = _RoundFwd.apply(sd["ca_conv.0.weight"][:, :, 0, 0].unsqueeze(0) * s.unsqueeze(1), rnd)      # [B, dim, 2 dim]
    out = _PerImageProduct.apply(fold, rnd(g), 4 if rnd is _id else 32) + sd["ca_conv.0.bias"].view(1, -1, 1, 1)   # rnd(g): e is stored
    return rnd(out), rm, rv


FORMS = {("global", False): lambda x, p, t, rnd, tap: gloal(x, p, t, tap), ("mixer", False): lambda x, p, t, rnd, tap: mixer(x, p, t, tap),
         ("global", True): gloal_device, ("mixer", True): mixer_device}


def run(kind, x, cot, sd, training=True, dtype=torch.float64, rnd=_id, device=False, tap=None):
    """Forward and backward in ``dtype``: -> {"y", "dx", "rm", "rv", "g.<key>"...} (detached; rm / rv: the running statistics after
    the call)."""
    p = {k: v.detach().to(dtype).requires_grad_(k in PARAMS[kind]) for k, v in sd.items()}
    xr = x.detach().to(dtype).requires_grad_(True)
    y, rm, rv = FORMS[(kind, device)](xr, p, training, rnd, tap)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad, "rm": rm.detach(), "rv": rv.detach()}
    out.update({"g." + k: p[k].grad for k in PARAMS[kind]})
    return out


def tensors(kind):
    return {"y", "dx", "rm", "rv"} | {"g." + k for k in PARAMS[kind]}


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_sfh_mixer.py
# name -> (kind, (B, dim, H, W), seed, training).  The pool pass walks a plane in 1024-element blocks (256 threads x 4), 16 of them
# at the most side by side; rows are 4 wide where H W % 4 == 0 and element by element otherwise, so both kinds occur.
_CASES = OrderedDict([
    ("tiny", ("mixer", (1, 2, 4, 4), 7100, True)),           # segment width 1, 12 spectral bins per channel
    ("odd", ("mixer", (2, 6, 9, 11), 7101, True)),           # odd H and W, N = 99 (element rows), segment width 3
    ("tile_plus_1", ("mixer", (1, 4, 17, 65), 7102, True)),  # one row and column past the local mixer's 64 x 16 tile; N = 1105, odd
    ("b3", ("mixer", (3, 8, 16, 64), 7103, True)),           # exactly one tile and one pool block; three folded weights, one statistic
    ("ragged", ("mixer", (1, 4, 40, 70), 7104, True)),       # N = 2800: 4-wide rows, a ragged third pool block per thread
    ("pool2", ("mixer", (1, 2, 64, 66), 7109, True)),        # N = 4224 > 4096: two pool partials per plane (the seam of the pool split)
    ("deep", ("mixer", (2, 64, 8, 8), 7205, True)),           # (seed 7105 left a hidden pre-activation 7.8 x its error from 0)
    ("wide", ("mixer", (1, 128, 4, 6), 7106, True)),         # c = 256, the FourierUnit's limit
    ("odd_eval", ("mixer", (2, 6, 9, 11), 7107, False)),     # seeded non-trivial running statistics, nothing updated
    ("b3_eval", ("mixer", (3, 8, 16, 64), 7108, False)),
    ("glo_odd", ("global", (2, 3, 9, 11), 7110, True)),      # an odd dim
    ("glo_b3", ("global", (3, 8, 16, 64), 7111, True)),
    ("glo_wide", ("global", (1, 128, 4, 6), 7112, True)),
    ("glo_eval", ("global", (2, 3, 9, 11), 7113, False)),
])


def _io(name):
    kind, (B, dim, H, W), seed, training = _CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, dim, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, dim, H, W))).float()
    return kind, make_state(kind, dim, seed + 50, trivial_stats=training), x, cot, training


def preconditions(name):
    """-> (variances_ok on p, the smallest |hidden pre-activation| / its error in the bf16 device form (inf for the global mixer))"""
    kind, sd, x, cot, training = _io(name)
    xb, _ = storage_io(x, cot, torch.bfloat16)
    ok, margin = True, float("inf")
    with torch.no_grad():
        for xin in (x, xb):
            ref, dev = {}, {}
            p64 = {k: v.double() for k, v in sd.items()}
            FORMS[(kind, False)](xin.double(), p64, training, _id, ref)
            ok = ok and S.variances_ok(ref["p"])
        if kind == "mixer":
            FORMS[(kind, True)](xb, {k: v.clone() for k, v in sd.items()}, training, lambda t: t.to(torch.bfloat16).to(t.dtype), dev)
            err = (dev["pre"].double() - ref["pre"].flatten(1)).abs().clamp_min(1e-30)
            margin = float((ref["pre"].flatten(1).abs() / err).min())
    return ok, margin


def _checked(cases):
    for name in cases:
        ok, margin = preconditions(name)
        assert ok, f"{name}: a spectral channel's variance is below VAR_FLOOR x the median (pick another seed)"
        assert margin >= HIDDEN_MARGIN, f"{name}: a hidden pre-activation is {margin:.1f} x its bf16 error from 0 (pick another seed)"
    return cases


PARITY_CASES = _checked(_CASES)


def parity_io(name):
    """-> (kind, state, input, cotangent, training) of a parity case, float32."""
    return _io(name)


def host_errors(name, dtype):
    """Error of the DEVICE form evaluated on the host in the device's storage precision against the fp64 form, per tensor, in the
    parity metric.  -> ({tensor: error}, the fp64 results)."""
    kind, sd, x, cot, training = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    ref = run(kind, x, cot, sd, training)
    got = run(kind, x, cot, sd, training, torch.float32, _id if dtype == torch.float32 else round_bf16, device=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref
