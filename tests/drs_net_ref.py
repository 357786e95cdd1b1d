"""fp64 CPU restatement of DRSformer's MEFC and whole network (TEST INFRASTRUCTURE).

Written from the semantics of DRSformer_arch.py: the Mixture of Experts Feature Compensator (``subnet``, :328-354, with its
OALayer routing head, GroupOLs and OperationLayer) and the U-Net of :388-480, in plain torch so that autograd supplies the
backward.  The sparse transformer blocks come from ``drs_ref.stb``.  Parameters are flat ``{name: tensor}`` dicts with the
reference's state_dict keys (relative to the ``subnet`` for ``subnet``).

``masks=`` hands in the device's ReLU decisions, which flip where a pre-activation sits within rounding of 0: per layer pair a
dict (``image_restoration_amd.drsformer._mefc_record``) with pre0 (preprocess), h (routing hidden layer), and per step u (the
four SepConv inner ReLUs, [B, 4C, H, W]), pre (the out projection's ReLU) and out (the residual ReLU).  The network takes, per
STB, the (top-k masks, MSFN ReLU masks) pair of ``drs_ref.stb`` and, per subnet, the list of pair dicts.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import drs_ref as D

SEP_K = (1, 3, 5, 7)
DIL_K = (3, 5, 7)
NUM_OPS = 8


def _relu(z, mask):
    return F.relu(z) if mask is None else z * mask.to(z.dtype)


def _get(m, key, t=None):
    if m is None:
        return None
    return m[key] if t is None else m[key][t]


def mefc_pair(x, sd, i, steps, m=None):
    """Layer pair i (OALayer ``layers.{2i}``, GroupOLs ``layers.{2i+1}``) -> (out, routing weights [B, steps, 8])."""
    oal, g = D.sub(sd, f"layers.{2 * i}."), D.sub(sd, f"layers.{2 * i + 1}.")
    C = x.shape[1]
    h = _relu(F.linear(x.mean((2, 3)), oal["ca_fc.0.weight"], oal["ca_fc.0.bias"]), _get(m, "h"))
    w = F.linear(h, oal["ca_fc.2.weight"], oal["ca_fc.2.bias"]).view(-1, steps, NUM_OPS).softmax(-1)
    s = _relu(F.conv2d(x, g["preprocess.op.0.weight"]), _get(m, "pre0"))
    for t in range(steps):
        o = D.sub(g, f"_ops.{t}.")
        u = _get(m, "u", t)
        states = []
        for j, k in enumerate(SEP_K):
            q = D.sub(o, f"_ops.{j}.op.")
            a = F.conv2d(F.conv2d(s, q["0.weight"], padding=k // 2, groups=C), q["1.weight"])
            a = _relu(a, None if u is None else u[:, j * C:(j + 1) * C])
            states.append(F.conv2d(F.conv2d(a, q["3.weight"], padding=k // 2, groups=C), q["4.weight"]))
        for j, k in enumerate(DIL_K):
            q = D.sub(o, f"_ops.{4 + j}.op.")
            states.append(F.conv2d(F.conv2d(s, q["0.weight"], padding=k - 1, dilation=2, groups=C), q["1.weight"]))
        states.append(F.avg_pool2d(s, 3, stride=1, padding=1, count_include_pad=False))
        z = torch.cat([st * w[:, t, j].view(-1, 1, 1, 1) for j, st in enumerate(states)], dim=1)
        r = _relu(F.conv2d(z, o["_out.0.weight"]), _get(m, "pre", t))
        s = _relu(r + s, _get(m, "out", t))
    return s, w


def subnet(x, sd, layer_num=1, steps=4, masks=None):
    """-> (out, [routing weights of each pair])."""
    ws = []
    for i in range(layer_num):
        x, w = mefc_pair(x, sd, i, steps, None if masks is None else masks[i])
        ws.append(w)
    return x, ws


def _conv3(h, sd, name):
    return F.conv2d(h, sd[name + ".weight"], sd.get(name + ".bias"), padding=1)


def drsformer(x, sd, cfg, stb_masks=None, mefc_masks=None):
    """The whole network.  stb_masks: {"encoder_level1.0": (topk masks, msfn relu masks), ...}; mefc_masks: {"encoder_level0":
    [pair dicts], "refinement": [...]}."""
    nb, heads = cfg["num_blocks"], cfg["heads"]

    def stage(h, name, n, hd):
        for j in range(n):
            key = f"{name}.{j}"
            mk = stb_masks[key] if stb_masks is not None else (None, None)
            h, _ = D.stb(h, D.sub(sd, key + "."), hd, *mk)
        return h

    def mefc(h, name):
        return subnet(h, D.sub(sd, name + "."), 1, 4, None if mefc_masks is None else mefc_masks[name])[0]

    e1 = stage(mefc(_conv3(x, sd, "patch_embed.proj"), "encoder_level0"), "encoder_level1", nb[0], heads[0])
    e2 = stage(F.pixel_unshuffle(_conv3(e1, sd, "down1_2.body.0"), 2), "encoder_level2", nb[1], heads[1])
    e3 = stage(F.pixel_unshuffle(_conv3(e2, sd, "down2_3.body.0"), 2), "encoder_level3", nb[2], heads[2])
    lat = stage(F.pixel_unshuffle(_conv3(e3, sd, "down3_4.body.0"), 2), "latent", nb[3], heads[3])
    d3 = torch.cat([F.pixel_shuffle(_conv3(lat, sd, "up4_3.body.0"), 2), e3], 1)
    d3 = stage(F.conv2d(d3, sd["reduce_chan_level3.weight"], sd.get("reduce_chan_level3.bias")), "decoder_level3", nb[2], heads[2])
    d2 = torch.cat([F.pixel_shuffle(_conv3(d3, sd, "up3_2.body.0"), 2), e2], 1)
    d2 = stage(F.conv2d(d2, sd["reduce_chan_level2.weight"], sd.get("reduce_chan_level2.bias")), "decoder_level2", nb[1], heads[1])
    d1 = torch.cat([F.pixel_shuffle(_conv3(d2, sd, "up2_1.body.0"), 2), e1], 1)
    d1 = mefc(stage(d1, "decoder_level1", nb[0], heads[0]), "refinement")
    return _conv3(d1, sd, "output") + x


# ---------------------------------------------------------------- parameter shapes (reference state_dict order)
def subnet_shapes(dim, layer_num=1, steps=4):
    s = OrderedDict()
    hid, out = 2 * steps * NUM_OPS, steps * NUM_OPS
    for i in range(layer_num):
        a, g = f"layers.{2 * i}.", f"layers.{2 * i + 1}."
        s[a + "ca_fc.0.weight"] = (hid, dim)
        s[a + "ca_fc.0.bias"] = (hid,)
        s[a + "ca_fc.2.weight"] = (out, hid)
        s[a + "ca_fc.2.bias"] = (out,)
        s[g + "preprocess.op.0.weight"] = (dim, dim, 1, 1)
        for t in range(steps):
            o = f"{g}_ops.{t}."
            for j, k in enumerate(SEP_K):
                for n, shape in (("0", (dim, 1, k, k)), ("1", (dim, dim, 1, 1)), ("3", (dim, 1, k, k)), ("4", (dim, dim, 1, 1))):
                    s[f"{o}_ops.{j}.op.{n}.weight"] = shape
            for j, k in enumerate(DIL_K):
                s[f"{o}_ops.{4 + j}.op.0.weight"] = (dim, 1, k, k)
                s[f"{o}_ops.{4 + j}.op.1.weight"] = (dim, dim, 1, 1)
            s[o + "_out.0.weight"] = (dim, NUM_OPS * dim, 1, 1)
    return s


def drsformer_shapes(cfg):
    dim, nb, heads, f, bias, ln = (cfg["dim"], cfg["num_blocks"], cfg["heads"], cfg["ffn_expansion_factor"], cfg["bias"],
                                   cfg["LayerNorm_type"])
    s = OrderedDict()

    def conv(name, cout, cin, k):
        s[name + ".weight"] = (cout, cin, k, k)
        if bias:
            s[name + ".bias"] = (cout,)

    def stage(name, n, d, hd):
        for j in range(n):
            for k, v in D.stb_shapes(d, hd, f, bias, ln).items():
                s[f"{name}.{j}.{k}"] = v

    def mefc(name, d):
        for k, v in subnet_shapes(d).items():
            s[f"{name}.{k}"] = v

    s["patch_embed.proj.weight"] = (dim, cfg["inp_channels"], 3, 3)
    mefc("encoder_level0", dim)
    stage("encoder_level1", nb[0], dim, heads[0])
    s["down1_2.body.0.weight"] = (dim // 2, dim, 3, 3)
    stage("encoder_level2", nb[1], 2 * dim, heads[1])
    s["down2_3.body.0.weight"] = (dim, 2 * dim, 3, 3)
    stage("encoder_level3", nb[2], 4 * dim, heads[2])
    s["down3_4.body.0.weight"] = (2 * dim, 4 * dim, 3, 3)
    stage("latent", nb[3], 8 * dim, heads[3])
    s["up4_3.body.0.weight"] = (16 * dim, 8 * dim, 3, 3)
    conv("reduce_chan_level3", 4 * dim, 8 * dim, 1)
    stage("decoder_level3", nb[2], 4 * dim, heads[2])
    s["up3_2.body.0.weight"] = (8 * dim, 4 * dim, 3, 3)
    conv("reduce_chan_level2", 2 * dim, 4 * dim, 1)
    stage("decoder_level2", nb[1], 2 * dim, heads[1])
    s["up2_1.body.0.weight"] = (4 * dim, 2 * dim, 3, 3)
    stage("decoder_level1", nb[0], 2 * dim, heads[0])
    mefc("refinement", 2 * dim)
    conv("output", cfg["out_channels"], 2 * dim, 3)
    return s


# ---------------------------------------------------------------- fixtures of tools/capture_golden_drs_net.py
def check_packed(prefix, got, gold, rtol, what=""):
    """``oracle.fixtures.check`` at the fixture's own compaction (``max_elems``)."""
    from oracle.fixtures import compact
    c = compact(got, int(gold["max_elems"]))
    ref = np.asarray(gold[f"{prefix}.sub"], dtype=np.float64)
    _close(c, ref, float(gold[f"{prefix}.l2"]), rtol, f"{what}{prefix}")


def check_grads(grads, gold, rtol, what=""):
    """Every parameter gradient against the fixture's g.* arrays; ``grads``: {state_dict key: gradient}."""
    from oracle.fixtures import compact
    names = [str(n) for n in gold["g.names"]]
    assert sorted(names) == sorted(grads), f"{what}gradient names differ"
    off, ms = gold["g.off"], int(gold["max_elems_g"])
    for i, n in enumerate(names):
        c = compact(grads[n], ms)
        _close(c, np.asarray(gold["g.sub"][off[i]:off[i + 1]], dtype=np.float64), float(gold["g.l2"][i]), rtol, f"{what}g.{n}")


def _close(c, ref, l2, rtol, what):
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(c["sub"].astype(np.float64) - ref).max()) / scale
    assert err <= rtol, f"{what}: max rel err {err:.3e} > {rtol:.1e}"
    assert abs(c["l2"] - l2) <= 10 * rtol * max(l2, 1e-30), f"{what}: l2 {c['l2']:.6e} vs {l2:.6e}"
