"""fp64-capable CPU restatement of SFHformer's Block, Stage and Backbone (TEST INFRASTRUCTURE), in plain torch so that autograd
supplies the backward.  Nothing but the composition of formulas that already exist: BatchNorm and the scaled residual from
``bn2d_ref``, the Mixer from ``sfh_mixer_ref``, the FFN from ``sfh_ffn_ref``; the Backbone's glue is ``F.conv2d`` / ``F.pixel_shuffle``.

    block   x1 = mixer(norm1(x)) beta + x;  out = ffn(norm2(x1)) gamma + x1
    stage   the blocks one after the other
    net     patch_embed (3x3), layer1, downsample1 (2x2 stride 2), layer2, downsample2, layer3, upsample3 (1x1 + PixelShuffle 2),
            skip2(cat(., copy2)), layer8, upsample4, skip1(cat(., copy1)), layer9, patch_unembed (3x3) + the input

State dicts carry the reference's keys in its order (a module's own parameters, then its children; buffers behind their module's
parameters).  Also here: the state generator (``beta`` / ``gamma`` of order 1: with the reference's zero initialisation a Block is
the identity and tests nothing) and the case list of the fixtures and of the GPU tests.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import bn2d_ref as B
import sfh_ffn_ref as FR
import sfh_mixer_ref as M
from oracle.fixtures import seeded_input

NORM_KEYS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
# the 40 parameters in the module's named_parameters() order: what ops.sfh_block_fwd takes
BLOCK_PARAMS = (("beta", "gamma", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias") + tuple("mixer." + k for k in M.MIXER_PARAMS) +
                tuple("ffn." + k for k in FR.FFN_PARAMS))
BLOCK_NORMS = ("norm1", "norm2", "mixer.mixer_gloal.FFC.bn")
STAGES = ("layer1", "layer2", "layer3", "layer8", "layer9")

# name -> (kind, constructor arguments, (B, H, W), seed, training): the smallest cases that still reach every form
NET = dict(embed_dim=[4, 8, 16, 8, 4], depth=[1, 1, 2, 1, 1])
CASES = OrderedDict([
    ("sfh_block_d4", ("block", dict(dim=4), (2, 9, 11), 301, True)),             # odd plane, narrow access form
    ("sfh_block_d6_eval", ("block", dict(dim=6), (2, 8, 10), 302, False)),       # segment width 3; seeded running statistics
    ("sfh_block_d32", ("block", dict(dim=32), (1, 12, 16), 303, True)),
    ("sfh_block_d4_two_chunks", ("block", dict(dim=4), (1, 72, 64), 304, True)),  # N = 4608: two chunks per plane, the seam merges pairs
    ("sfh_stage_d4_n2", ("stage", dict(depth=2, in_channels=4), (2, 9, 11), 305, True)),
    ("sfh_stage_d4_n3_eval", ("stage", dict(depth=3, in_channels=4), (2, 9, 11), 306, False)),
    ("sfh_net_tiny", ("net", NET, (2, 16, 20), 307, True)),                      # deepest plane 4 x 5
    ("sfh_net_tiny_eval", ("net", NET, (2, 16, 20), 308, False)),
])
# the constructor arguments whose state_dict keys and shapes sfh_block_keys.npz records ("t": SFHformer_t())
KEY_CASES = (("block_d8", "block", dict(dim=8)), ("stage_d6_n2", "stage", dict(depth=2, in_channels=6)), ("net_tiny", "net", NET),
             ("t", "net", dict(embed_dim=[32, 64, 128, 64, 32], depth=[1, 1, 2, 1, 1])))


def in_channels(kind, args):
    return 3 if kind == "net" else args["dim"] if kind == "block" else args["in_channels"]


def block_prefixes(kind, args):
    """The state_dict prefix of every Block, in the order the forward runs them."""
    if kind == "block":
        return [""]
    if kind == "stage":
        return [f"blocks.{i}." for i in range(args["depth"])]
    return [f"{s}.blocks.{i}." for s, d in zip(STAGES, args["depth"]) for i in range(d)]


def _block_layout(dim):
    out = [("beta", (1, dim, 1, 1)), ("gamma", (1, dim, 1, 1))]
    for n in ("norm1", "norm2"):
        out += [(f"{n}.{k}", () if k == "num_batches_tracked" else (dim,)) for k in NORM_KEYS]
    out += [("mixer." + k, s) for k, s in M.state_dict_layout("mixer", dim)]
    return out + [("ffn." + k, s) for k, s in FR.state_dict_layout("ffn", dim)]


def _stage_layout(depth, dim):
    return [(f"blocks.{i}.{k}", s) for i in range(depth) for k, s in _block_layout(dim)]


def state_dict_layout(kind, args):
    """(key, shape) in the reference's state_dict order, num_batches_tracked included."""
    if kind == "block":
        return _block_layout(args["dim"])
    if kind == "stage":
        return _stage_layout(args["depth"], args["in_channels"])
    e, d = args["embed_dim"], args["depth"]

    def conv(name, co, ci, k, bias=True):
        return [(name + ".weight", (co, ci, k, k))] + ([(name + ".bias", (co,))] if bias else [])

    def stage(i):
        return [(f"{STAGES[i]}.{k}", s) for k, s in _stage_layout(d[i], e[i])]
    return (conv("patch_embed.proj", e[0], 3, 3) + stage(0) + conv("skip1", e[0], e[1], 1) + conv("downsample1.proj.0", 2 * e[0], e[0], 2) +
            stage(1) + conv("skip2", e[1], e[2], 1) + conv("downsample2.proj.0", 2 * e[1], e[1], 2) + stage(2) +
            conv("upsample3.proj.0", 4 * e[3], e[2], 1, False) + stage(3) + conv("upsample4.proj.0", 4 * e[4], e[3], 1, False) + stage(4) +
            conv("patch_unembed.proj.0", 3, e[4], 3))


def params_of(kind, args):
    """The parameter keys in named_parameters() order."""
    return [k for k, _ in state_dict_layout(kind, args) if k.rsplit(".", 1)[-1] not in NORM_KEYS[2:]]


def buffers_of(kind, args):
    """The running statistics' keys (what a training step updates beside num_batches_tracked)."""
    return [k for k, _ in state_dict_layout(kind, args) if k.rsplit(".", 1)[-1] in NORM_KEYS[2:4]]


def make_state(kind, args, seed, trivial_stats=True):
    """Seeded float32 state without num_batches_tracked.  A Block: the Mixer's and the FFN's own generators, norm weights
    1 + 0.3 N(0,1), norm biases 0.1 N(0,1), running statistics 0 / 1 or seeded non-trivial ones, beta and gamma of magnitude
    0.5..1.5 with a random sign.  Glue convolutions: N(0,1) / sqrt(fan-in), biases 0.1 N(0,1)."""
    rng = np.random.default_rng(seed)
    blocks = {}
    for n, pre in enumerate(block_prefixes(kind, args)):
        blocks[pre] = (M.make_state("mixer", _dim_of(kind, args, pre), seed + 10 * n + 1, trivial_stats),
                       FR.make_state("ffn", _dim_of(kind, args, pre), seed + 10 * n + 2))
    sd = OrderedDict()

    def f32(v):
        return torch.from_numpy(np.asarray(v, dtype=np.float32))
    for k, shape in state_dict_layout(kind, args):
        leaf = k.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            continue
        pre = next((p for p in sorted(blocks, key=len, reverse=True) if k.startswith(p)), None) if blocks else None
        rest = k[len(pre):] if pre is not None else None
        if rest is not None and rest.startswith("mixer."):
            sd[k] = blocks[pre][0][rest[len("mixer."):]]
        elif rest is not None and rest.startswith("ffn."):
            sd[k] = blocks[pre][1][rest[len("ffn."):]]
        elif rest in ("beta", "gamma"):
            sd[k] = f32(rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape))
        elif rest is not None and rest.startswith("norm"):
            z = rng.standard_normal(shape)
            if leaf == "weight":
                sd[k] = f32(1.0 + 0.3 * z)
            elif leaf == "bias":
                sd[k] = f32(0.1 * z)
            elif leaf == "running_mean":
                sd[k] = f32(np.zeros(shape) if trivial_stats else 0.2 * z)
            else:
                sd[k] = f32(np.ones(shape) if trivial_stats else 0.5 + rng.random(shape))
        else:
            z = rng.standard_normal(shape)
            sd[k] = f32(0.1 * z if leaf == "bias" else z / math.sqrt(int(np.prod(shape[1:]))))
    return sd


def _dim_of(kind, args, prefix):
    if kind == "block":
        return args["dim"]
    if kind == "stage":
        return args["in_channels"]
    return args["embed_dim"][STAGES.index(prefix.split(".", 1)[0])]


def module_state(kind, args, sd, steps=0):
    """The dict ``load_state_dict(strict=True)`` takes: ``sd`` plus num_batches_tracked, in the reference's order."""
    return OrderedDict((k, torch.tensor(steps, dtype=torch.long) if k.endswith("num_batches_tracked") else sd[k])
                       for k, _ in state_dict_layout(kind, args))


def case_io(name):
    """-> (input, cotangent) of a case, float32, from oracle.fixtures.seeded_input."""
    kind, args, (Bn, H, W), seed, _ = CASES[name]
    c = in_channels(kind, args)
    return seeded_input((Bn, c, H, W), 1000 + seed), seeded_input((Bn, c, H, W), 2000 + seed)


def case_state(name):
    kind, args, _, seed, training = CASES[name]
    return make_state(kind, args, seed, trivial_stats=training)


# ---------------------------------------------------------------- the formulas
def block(x, p, pre, training, bufs):
    """One Block on the state ``p`` under the key prefix ``pre``; the running statistics after the call go to ``bufs`` under their
    state_dict keys."""
    def norm(name, t):
        y, rm, rv = B.batch_norm(t, p[f"{pre}{name}.weight"], p[f"{pre}{name}.bias"], p[f"{pre}{name}.running_mean"],
                                 p[f"{pre}{name}.running_var"], training)
        bufs[f"{pre}{name}.running_mean"], bufs[f"{pre}{name}.running_var"] = rm, rv
        return y
    m, rm, rv = M.mixer(norm("norm1", x), M.sub(p, pre + "mixer."), training)
    bufs[pre + "mixer.mixer_gloal.FFC.bn.running_mean"], bufs[pre + "mixer.mixer_gloal.FFC.bn.running_var"] = rm, rv
    x1 = B.scaled_residual(m, x, p[pre + "beta"])
    return B.scaled_residual(FR.ffn(norm("norm2", x1), M.sub(p, pre + "ffn.")), x1, p[pre + "gamma"])


def stage(x, p, pre, depth, training, bufs):
    for i in range(depth):
        x = block(x, p, f"{pre}blocks.{i}.", training, bufs)
    return x


def net(x, p, args, training, bufs):
    d = args["depth"]

    def conv(name, t, **kw):
        return F.conv2d(t, p[name + ".weight"], p.get(name + ".bias"), **kw)
    copy0 = x
    copy1 = x = stage(conv("patch_embed.proj", x, padding=1), p, "layer1.", d[0], training, bufs)
    copy2 = x = stage(conv("downsample1.proj.0", x, stride=2), p, "layer2.", d[1], training, bufs)
    x = stage(conv("downsample2.proj.0", x, stride=2), p, "layer3.", d[2], training, bufs)
    x = conv("skip2", torch.cat([F.pixel_shuffle(conv("upsample3.proj.0", x), 2), copy2], dim=1))
    x = stage(x, p, "layer8.", d[3], training, bufs)
    x = conv("skip1", torch.cat([F.pixel_shuffle(conv("upsample4.proj.0", x), 2), copy1], dim=1))
    x = stage(x, p, "layer9.", d[4], training, bufs)
    return copy0 + conv("patch_unembed.proj.0", x, padding=1)


def forward(kind, args, x, p, training, bufs):
    if kind == "block":
        return block(x, p, "", training, bufs)
    if kind == "stage":
        return stage(x, p, "", args["depth"], training, bufs)
    return net(x, p, args, training, bufs)


def run(kind, args, x, cot, sd, training=True, dtype=torch.float64):
    """Forward and backward in ``dtype``: -> {"y", "dx", "g.<parameter>"..., "buf.<running statistic>"...} (detached; buf.*: the
    running statistics after the call)."""
    params = set(params_of(kind, args))
    p = {k: v.detach().to(dtype).requires_grad_(k in params) for k, v in sd.items()}
    xr = x.detach().to(dtype).requires_grad_(True)
    bufs = {}
    y = forward(kind, args, xr, p, training, bufs)
    y.backward(cot.to(dtype))
    out = {"y": y.detach(), "dx": xr.grad}
    out.update({"g." + k: p[k].grad for k in params_of(kind, args)})
    out.update({"buf." + k: bufs[k].detach() for k in buffers_of(kind, args)})
    return out


def tensors(kind, args):
    return {"y", "dx"} | {"g." + k for k in params_of(kind, args)} | {"buf." + k for k in buffers_of(kind, args)}

