"""fp64 CPU restatement of DarkIR's encoder block, EBlock, and of the whole DarkIR network (TEST INFRASTRUCTURE).

Written from the formulas, in plain torch so that autograd supplies the backward:

    x0 = LN2d(inp; norm1, eps 1e-6)
    xe = extra_conv(x0)                        plain depthwise 3x3, pad 1, groups = c (when the state has extra_conv.weight)
    x1 = conv1(xe)                             1x1, c -> 2c
    z  = sum_i dw3x3(x1; dilation d_i, pad d_i) + b_i        g = z[:, :c] * z[:, c:]
    s  = W_sca . mean_hw(g) + b_sca            y = inp + beta * conv3(s * g)
    y0 = LN2d(y; norm2)                        f = FreMLP(y0)   (nc = c, expand = 2)
    out = y * (1 + gamma * f)                  (= y + gamma * (y * f))

The network is archs/DarkIR.py: intro, EBlock encoders with 2x2 stride-2 downs, EBlock / DBlock middle, 1x1 + PixelShuffle ups
with skip sums, DBlock decoders, ending plus the (zero padded) input, cropped back.

``rnd=`` is applied to every activation the device stores (x0, xe, x1, g, y, y0, f, out; in the network also the glue convs'
outputs and the skip sums), and through ``round_bf16``'s backward to every activation gradient it stores - among them the
residual's share of the gradient at y, which the tail's backward writes on its own: identity, or ``round_bf16``.  ``dense=True`` runs FreMLP in the form the device computes
(``fremlp_ref.fremlp_dense``); ``dense=False`` in its ``torch.fft`` form, the reference of every comparison.  The host-error
model of a storage precision is the dense form in float32 with that ``rnd``.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import darkir_ref as D
import fremlp_ref as FR
from darkir_ref import _id, make_state, rel_err, round_bf16, storage_io  # noqa: F401  (re-exported for the tests)

FLOOR = FR.FLOOR


def sub_state(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def fregate(y, f, gamma):
    return y * (1 + gamma.view(1, -1, 1, 1) * f)


def eblock(inp, sd, dilations, rnd=_id, dense=False, probe=None):
    """``probe``: a list that receives the detached FreMLP input y0 (for the spectral-floor precondition)."""
    c = inp.shape[1]
    x = rnd(D.layer_norm2d(inp, sd["norm1.weight"], sd["norm1.bias"]))
    if "extra_conv.weight" in sd:
        x = rnd(F.conv2d(x, sd["extra_conv.weight"], sd["extra_conv.bias"], padding=1, groups=c))
    x = rnd(F.conv2d(x, sd["conv1.weight"], sd["conv1.bias"]))
    g = D.simple_gate(D.dilated_sum(x, sd, dilations))
    s = F.conv2d(g.mean(dim=(2, 3), keepdim=True), sd["sca.1.weight"], sd["sca.1.bias"])
    g = rnd(g)
    y = rnd(inp + sd["beta"] * F.conv2d(s * g, sd["conv3.weight"], sd["conv3.bias"]))
    y0 = rnd(D.layer_norm2d(y, sd["norm2.weight"], sd["norm2.bias"]))
    if probe is not None:
        probe.append(y0.detach())
    fsd = sub_state(sd, "freq.")
    f = FR.fremlp_dense(y0, fsd, rnd) if dense else rnd(FR.fremlp(y0, fsd))
    # rnd(y): y is stored already, so the value is unchanged; the gradient arriving here is the residual's share dyr, which the
    # device stores on its own (mi_fregate_bwd writes it, mi_ln_bwd adds it as dres) before the sum at y is stored
    return rnd(fregate(rnd(y), f, sd["gamma"]))


# ---------------------------------------------------------------- parameter shapes (reference state_dict order)
def eblock_shapes(c, n_dil, extra_depth_wise):
    s = OrderedDict()
    s["gamma"] = (1, c, 1, 1)
    s["beta"] = (1, c, 1, 1)
    if extra_depth_wise:
        s["extra_conv.weight"] = (c, 1, 3, 3)
        s["extra_conv.bias"] = (c,)
    s["conv1.weight"] = (2 * c, c, 1, 1)
    s["conv1.bias"] = (2 * c,)
    for i in range(n_dil):
        s[f"branches.{i}.branch.0.weight"] = (2 * c, 1, 3, 3)
        s[f"branches.{i}.branch.0.bias"] = (2 * c,)
    s["sca.1.weight"] = (c, c, 1, 1)
    s["sca.1.bias"] = (c,)
    s["conv3.weight"] = (c, c, 1, 1)
    s["conv3.bias"] = (c,)
    for n in ("norm1", "norm2"):
        s[n + ".weight"] = (c,)
        s[n + ".bias"] = (c,)
    for k, v in FR.fremlp_shapes(c, 2).items():
        s["freq." + k] = v
    return s


def net_config(img_channel=3, width=32, middle_blk_num_enc=2, middle_blk_num_dec=2, enc_blk_nums=(1, 2, 3), dec_blk_nums=(3, 1, 1),
               dilations=(1, 4, 9), extra_depth_wise=True):
    return dict(img_channel=img_channel, width=width, middle_blk_num_enc=middle_blk_num_enc, middle_blk_num_dec=middle_blk_num_dec,
                enc_blk_nums=list(enc_blk_nums), dec_blk_nums=list(dec_blk_nums), dilations=list(dilations),
                extra_depth_wise=extra_depth_wise)


SMALL_NET = net_config(width=8, middle_blk_num_enc=1, middle_blk_num_dec=1, enc_blk_nums=(1, 1), dec_blk_nums=(1, 1))
SMALL_NET_INPUT = (2, 3, 18, 27)
SMALL_NET_SEED = 7401          # (7301 misses the spectral floor in one block)


def net_shapes(cfg):
    """The reference DarkIR's state_dict keys and shapes, in its order."""
    ic, w, ex, nd = cfg["img_channel"], cfg["width"], cfg["extra_depth_wise"], len(cfg["dilations"])
    s = OrderedDict()
    s["intro.weight"], s["intro.bias"] = (w, ic, 3, 3), (w,)
    s["ending.weight"], s["ending.bias"] = (ic, w, 3, 3), (ic,)
    enc, dec, ups, downs = OrderedDict(), OrderedDict(), OrderedDict(), OrderedDict()
    chan = w
    for i, num in enumerate(cfg["enc_blk_nums"]):
        for j in range(num):
            for k, v in eblock_shapes(chan, 1, ex).items():
                enc[f"encoders.{i}.modules_list.{j}.{k}"] = v
        downs[f"downs.{i}.weight"], downs[f"downs.{i}.bias"] = (2 * chan, chan, 2, 2), (2 * chan,)
        chan *= 2
    mid = OrderedDict()
    for j in range(cfg["middle_blk_num_enc"]):
        for k, v in eblock_shapes(chan, 1, ex).items():
            mid[f"middle_blks_enc.modules_list.{j}.{k}"] = v
    for j in range(cfg["middle_blk_num_dec"]):
        for k, v in D.dblock_shapes(chan, nd, ex).items():
            mid[f"middle_blks_dec.modules_list.{j}.{k}"] = v
    deepest = chan
    for i, num in enumerate(cfg["dec_blk_nums"]):
        ups[f"ups.{i}.0.weight"] = (2 * chan, chan, 1, 1)
        chan //= 2
        for j in range(num):
            for k, v in D.dblock_shapes(chan, nd, ex).items():
                dec[f"decoders.{i}.modules_list.{j}.{k}"] = v
    for part in (enc, dec, ups, downs, mid):      # the reference registers middle_blks_enc / _dec after the four ModuleLists
        s.update(part)
    s["side_out.weight"], s["side_out.bias"] = (ic, deepest, 3, 3), (ic,)
    return s


def darkir_net(inp, sd, cfg, side_loss=False, rnd=_id, dense=False, probe=None):
    levels = len(cfg["enc_blk_nums"])
    m = 2 ** levels
    _, _, H, W = inp.shape
    inp = F.pad(inp, (0, (m - W % m) % m, 0, (m - H % m) % m), value=0)
    dil = cfg["dilations"]
    x = rnd(F.conv2d(inp, sd["intro.weight"], sd["intro.bias"], padding=1))
    skips = []
    for i, num in enumerate(cfg["enc_blk_nums"]):
        for j in range(num):
            x = eblock(x, sub_state(sd, f"encoders.{i}.modules_list.{j}."), (1,), rnd, dense, probe)
        skips.append(x)
        x = rnd(F.conv2d(x, sd[f"downs.{i}.weight"], sd[f"downs.{i}.bias"], stride=2))
    for j in range(cfg["middle_blk_num_enc"]):
        x = eblock(x, sub_state(sd, f"middle_blks_enc.modules_list.{j}."), (1,), rnd, dense, probe)
    x_light = x
    out_side = rnd(F.conv2d(x_light, sd["side_out.weight"], sd["side_out.bias"], padding=1)) if side_loss else None
    for j in range(cfg["middle_blk_num_dec"]):
        x = D.dblock(x, sub_state(sd, f"middle_blks_dec.modules_list.{j}."), dil, rnd)
    x = rnd(x + x_light)
    for i, num in enumerate(cfg["dec_blk_nums"]):
        x = F.pixel_shuffle(rnd(F.conv2d(x, sd[f"ups.{i}.0.weight"])), 2)
        x = rnd(x + skips[levels - 1 - i])
        for j in range(num):
            x = D.dblock(x, sub_state(sd, f"decoders.{i}.modules_list.{j}."), dil, rnd)
    x = rnd(F.conv2d(x, sd["ending.weight"], sd["ending.bias"], padding=1) + inp)
    out = x[:, :, :H, :W]
    return (out_side, out) if side_loss else out


# ---------------------------------------------------------------- forward + backward
def run(inp, cot, sd, dilations, dtype=torch.float64, rnd=_id, dense=False, probe=None):
    """Forward and backward of the block in ``dtype``: -> {"y", "dx", "g.<key>"...} (detached, in ``dtype``)."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = inp.detach().to(dtype).requires_grad_(True)
    y = eblock(rnd(x), p, dilations, rnd, dense, probe)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": x.grad}
    out.update({"g." + k: v.grad for k, v in p.items()})
    return out


def run_net(inp, cots, sd, cfg, dtype=torch.float64, rnd=_id, dense=False, probe=None):
    """Forward (side_loss=True) and backward of the network: cots = (cotangent of out_side, of out).
    -> {"side", "y", "dx", "g.<key>"...}."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = inp.detach().to(dtype).requires_grad_(True)
    side, y = darkir_net(rnd(x), p, cfg, True, rnd, dense, probe)
    torch.autograd.backward([side, y], [cots[0].to(dtype), cots[1].to(dtype)])
    out = {"side": side.detach(), "y": y.detach(), "dx": x.grad}
    out.update({"g." + k: v.grad for k, v in p.items()})
    return out


def floor_margin(probe):
    """The smallest min |Z| / rms |Z| over the recorded FreMLP inputs."""
    return min(FR.spectrum_floor(t) for t in probe)


# ---------------------------------------------------------------- the parity case list of tests/test_gpu_eblock.py
# (B, c, H, W), dilations, extra_depth_wise, seed.  The seeds are recorded: with them the FreMLP input of every case keeps
# min |Z| >= FLOOR * rms |Z| in the fp64 evaluation of the fp32 and of the bf16-rounded input (tools/eblock_bounds.py prints them).
PARITY_CASES = OrderedDict([
    ("tiny", ((2, 4, 2, 2), (1,), False, 5200)),             # the smallest plane FreMLP takes (seed 5100 misses the floor)
    ("sub_halo", ((2, 8, 5, 7), (1, 4, 9), True, 5101)),     # an odd plane under every halo
    ("seams_b3", ((3, 6, 40, 70), (1,), True, 5102)),        # crosses the 32-row and 64-column tile seams, ragged, B = 3
    ("c12", ((2, 12, 9, 16), (1, 4), True, 5103)),           # channel count not a multiple of 8
    ("c256", ((1, 256, 8, 8), (1,), True, 5104)),            # the network's deepest level
    ("net_level", ((2, 32, 16, 16), (1,), True, 5105)),
    ("max_dil", ((1, 8, 20, 24), (16, 16, 1, 2), False, 5106)),
    ("plane128", ((1, 4, 128, 128), (1,), True, 5107)),
])


def parity_io(name):
    """-> (state, input, cotangent, dilations) of a parity case, float32."""
    (B, c, H, W), dil, extra, seed = PARITY_CASES[name]
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    cot = torch.from_numpy(rng.standard_normal((B, c, H, W))).float()
    return make_state(eblock_shapes(c, len(dil), extra), seed + 50), x, cot, dil


def host_errors(name, dtype):
    """Error of the restatement evaluated on the host in the device's storage precision (float32 throughout, or float32 with every
    stored activation and activation gradient rounded to bfloat16; FreMLP in its dense form) against fp64 with torch.fft, per
    tensor, in the parity metric.  -> ({tensor: error}, the fp64 results, the spectral-floor margin of the fp64 run)."""
    sd, x, cot, dil = parity_io(name)
    x, cot = storage_io(x, cot, dtype)
    probe = []
    ref = run(x, cot, sd, dil, probe=probe)
    got = run(x, cot, sd, dil, torch.float32, _id if dtype == torch.float32 else round_bf16, dense=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref, floor_margin(probe)


def net_io():
    """-> (state, input, (cotangent of out_side, of out)) of the small network case, float32."""
    cfg = SMALL_NET
    rng = np.random.default_rng(SMALL_NET_SEED)
    B, ic, H, W = SMALL_NET_INPUT
    m = 2 ** len(cfg["enc_blk_nums"])
    x = torch.from_numpy(rng.standard_normal(SMALL_NET_INPUT)).float()
    cot_side = torch.from_numpy(rng.standard_normal((B, ic, -(-H // m), -(-W // m)))).float()
    cot = torch.from_numpy(rng.standard_normal(SMALL_NET_INPUT)).float()
    return make_state(net_shapes(cfg), SMALL_NET_SEED + 50), x, (cot_side, cot)


def net_host_errors(dtype):
    sd, x, cots = net_io()
    x, c1 = storage_io(x, cots[1], dtype)
    c0 = cots[0].to(dtype).float()
    probe = []
    ref = run_net(x, (c0, c1), sd, SMALL_NET, probe=probe)
    got = run_net(x, (c0, c1), sd, SMALL_NET, torch.float32, _id if dtype == torch.float32 else round_bf16, dense=True)
    return {k: rel_err(got[k], ref[k]) for k in ref}, ref, floor_margin(probe)


# ---------------------------------------------------------------- the training case of tests/test_gpu_eblock.py
TRAIN_C, TRAIN_SHAPE, TRAIN_DIL, TRAIN_LR, TRAIN_WD, TRAIN_STEPS = 32, (2, 32, 32, 32), (1, 4, 9), 1e-3, 0.01, 3
TRAIN_SEED = 91           # picked on the CPU: with it the fp32 host restatement meets the trajectory bars against fp64


def train_io(seed=None):
    """-> (state of Sequential(EBlock, DBlock), input, target), float32."""
    seed = TRAIN_SEED if seed is None else seed
    shapes = OrderedDict()
    for k, v in eblock_shapes(TRAIN_C, 1, True).items():
        shapes["0." + k] = v
    for k, v in D.dblock_shapes(TRAIN_C, len(TRAIN_DIL), True).items():
        shapes["1." + k] = v
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal(TRAIN_SHAPE)).float()
    tgt = torch.from_numpy(rng.standard_normal(TRAIN_SHAPE)).float()
    return make_state(shapes, seed), x, tgt


def train_reference(sd0, x, tgt, dtype=torch.float64, dense=False):
    """TRAIN_STEPS steps of torch.optim.AdamW on the L1 loss of the two-block stack in ``dtype`` -> (losses, final state)."""
    ps = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd0.items()}
    opt = torch.optim.AdamW(list(ps.values()), lr=TRAIN_LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=TRAIN_WD)
    losses = []
    for _ in range(TRAIN_STEPS):
        opt.zero_grad()
        h = eblock(x.to(dtype), sub_state(ps, "0."), (1,), _id, dense)
        h = D.dblock(h, sub_state(ps, "1."), TRAIN_DIL)
        loss = (h - tgt.to(dtype)).abs().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, {k: v.detach() for k, v in ps.items()}


def trajectory_misses(losses, got, ref_losses, ref, sd0):
    """The bars of test_gpu_darkir's trajectory test: -> the list of misses (empty: every bar is met)."""
    lr, bad = TRAIN_LR, []
    for step, (a, r) in enumerate(zip(losses, ref_losses)):
        if not abs(a - r) < 1e-4 * r:
            bad.append(("loss", step, a, r))
    for k, v in ref.items():
        w0 = sd0[k].double()
        a, r = got[k].double(), v.double()
        d = (a - r).abs()
        ua, ur = (a - w0).flatten(), (r - w0).flatten()
        cos = float((ua @ ur) / (ua.norm() * ur.norm()).clamp_min(1e-30))
        if not cos >= 0.9995:
            bad.append((k, "cos", cos))
        if not (float(d.mean()) <= 0.02 * lr and float(d.max()) <= 2.0 * lr):
            bad.append((k, "displacement / lr", float(d.mean()) / lr, float(d.max()) / lr))
    return bad
