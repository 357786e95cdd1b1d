"""SFHformer on the MI355X: the spectral token mixer core ``FourierUnit``, the feed-forward ``FFN``, the local token mixer
``TokenMixer_For_Local``, the global one and the ``Mixer``, the Block's ``BatchNorm2d`` and ``scaled_residual``, and over them ``Block``,
``Stage`` and the ``Backbone`` network with its four sizes (below).

``FourierUnit`` (``SFHformer.py:143-180``) with the reference's constructor
arguments and ``state_dict`` keys (``bn.*``, ``fdc.*``, ``weight.0.*``, ``fpe.*``), so a checkpoint slice loads with
``strict=True``.

``FourierUnit.forward`` is ONE autograd node over ``mi_fourier_unit_*`` (``csrc/sfh.hip``): ``rfft2`` and ``irfft2`` (``norm='ortho'``)
as the dense-DFT GEMMs of ``csrc/dft2.hip``, and between them BatchNorm over the interleaved real / imaginary channels (training
or eval mode, running statistics updated on the device), the depthwise 3x3 with its residual, the softmax gate over the groups and
the grouped 1x1 folded into one dense product, then GELU.  The submodules are parameter containers only.

Limits: ``in_channels == out_channels`` (the reference's ``view`` and ``bn`` only work then; anything else raises
``NotImplementedError``), 1 <= c <= 256, 1 <= groups <= 8 with 2c % groups == 0, planes of 2..512 pixels a side, fp32 or bf16
activations; BatchNorm with running statistics and a fixed momentum.  CPU tensors are refused (``RuntimeError``).

``FFN(dim)`` (``SFHformer.py:76-119``, keys ``conv_init.0.*``, ``conv1_1.0.*``, ``conv1_2.0.*``, ``conv1_3.0.*``, ``conv_fina.0.*``) and
``TokenMixer_For_Local(dim)`` (``:122-140``, keys ``CDilated_1.*``, ``CDilated_2.*``) are each ONE autograd node over ``mi_sfh_ffn_*`` /
``mi_sfh_local_*`` (``csrc/sfh_ffn.hip``): the channel axis in segments of ``dim / 2`` channels, each with its own depthwise stencil
(identity, 3x3, 5x5, 7x7 and erf-GELU between two biased 1x1 products; 3x3 at dilation 1 and 2).  Limits: ``dim`` even (an odd
``dim`` changes the reference's chunk count: ``NotImplementedError``), 2 <= dim <= 256, any plane, fp32 or bf16 activations.

``TokenMixer_For_Gloal(dim)`` (``:183-206``, keys ``conv_init.0.*``, ``conv_fina.0.*``, ``FFC.*``) and ``Mixer(dim)`` (``:209-251``, keys
``mixer_local.*``, ``mixer_gloal.*``, ``ca_conv.0.*``, ``ca.1.*``, ``ca.3.*``, ``conv_init.0.*``) are each ONE autograd node over
``mi_sfh_global_*`` / ``mi_sfh_mixer_*`` (``csrc/sfh_mixer.hip``): the 1x1 products, the FourierUnit and the local mixer through the
library's own entry points, and between them the file's streaming kernels (GELU, the residual add, the GELU / pool tail that writes
the concatenated tensor once, the channel attention folded into a per-image ``ca_conv`` weight).  ``FFC.bn`` behaves as in
``FourierUnit.forward``.  ``Mixer`` takes the reference's default token mixers only.  Limits: ``Mixer`` even 2 <= dim <= 128,
``TokenMixer_For_Gloal`` 1 <= dim <= 128 (the FourierUnit inside has 2 dim channels), planes of 2..512 pixels a side.

``BatchNorm2d(num_features)`` is ``torch.nn.BatchNorm2d`` (constructor, parameters, buffers and ``state_dict`` keys) whose ``forward``
is ONE autograd node over ``mi_bn2d_*`` (``csrc/bn2d.hip``): training mode normalises with the batch statistics and updates the
running ones on the device, eval mode normalises with the running ones in a single launch.  ``scaled_residual(f, x, scale)`` is the
Block's ``f * scale + x`` with ``scale`` of shape ``(1, C, 1, 1)`` or ``(C,)``, ONE autograd node over ``mi_scale_res_*``; the gradient
towards ``x`` is the cotangent itself.  Limits: 1 <= C <= 4096, any plane, fp32 or bf16 activations; BatchNorm affine, with running
statistics and a fixed momentum; training needs more than one value per channel.

``Block(dim)`` (``:254-282``, keys ``norm1.*``, ``norm2.*``, ``mixer.*``, ``ffn.*``, ``beta``, ``gamma``) and ``Stage(depth, in_channels)``
(``:287-306``, keys ``blocks.<i>.*``) are each ONE autograd node over ``mi_sfh_block_*`` (``csrc/sfh_block.hip``), a launch sequence
with no kernel of its own: BatchNorm, Mixer, scaled residual, BatchNorm, FFN, scaled residual through the entry points above, the
first residual handing the second BatchNorm its statistics pairs and, in a Stage, each Block's last residual handing them to the
next Block's first BatchNorm; the backward folds both residual gradients into the BatchNorm backwards.  The results are those of
the six public pieces called one after the other, bit for bit.  The submodules are parameter containers; training mode advances
``num_batches_tracked`` of all three norms of a Block.  Limits: the reference's default ``norm_layer`` and ``token_mixer`` only
(``NotImplementedError``), even 2 <= dim <= 128, planes of 2..512 pixels a side, one eps / momentum / mode for the norms.

``Backbone`` (``:309-357``) and ``SFHformer_t / _s / _m / _l`` take the reference's constructor arguments, attribute names and
``state_dict``; ``PatchEmbed``, ``PatchUnEmbed``, ``PatchUnEmbed_for_upsample`` and ``DownSample`` likewise.  Every convolution runs on the
glue that DarkIR and Restormer use: the dense 3x3 for ``patch_embed`` and ``patch_unembed`` (the latter with the input residual
folded in), PixelUnshuffle plus the 1x1 product on the weight viewed as [2c, 4c] for ``DownSample``, the 1x1 product plus
PixelShuffle for the upsamples, and ``skipN(cat(up, copy))`` concat-free in float32 (two K panels) or with the shuffle writing into
the concatenation buffer in bfloat16.  ``patch_size != 1`` or ``embed_kernel_size != 3`` raise ``NotImplementedError``; inputs whose H
or W is no multiple of 4, or below 8, raise ``ValueError``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._autograd import _apply, module_op
from .darkir import _glue_conv
from .restormer import _conv1x1_module, _shuffle, _UpCatFn

Tensor = torch.Tensor

__all__ = ["Backbone", "BatchNorm2d", "Block", "DownSample", "FFN", "FourierUnit", "Mixer", "PatchEmbed", "PatchUnEmbed",
           "PatchUnEmbed_for_upsample", "SFHformer_l", "SFHformer_m", "SFHformer_s", "SFHformer_t", "Stage", "TokenMixer_For_Gloal",
           "TokenMixer_For_Local", "scaled_residual"]


class _FourierUnitOp:
    """FourierUnit.forward as one module op.  params: bn, fdc, gate and fpe weights and biases; saved = [the kernels' blob]."""

    def __init__(self, bn: nn.BatchNorm2d, training: bool):
        self.rm, self.rv, self.training, self.eps, self.momentum = bn.running_mean, bn.running_var, training, bn.eps, bn.momentum

    def forward(self, acts, params, need):
        out, blob = ops.fourier_unit_fwd(acts[0], params, self.rm, self.rv, self.training, need, self.eps, self.momentum)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.fourier_unit_bwd(dout, params, saved[0], grads, acc, self.training, self.eps, self.momentum),)


class FourierUnit(nn.Module):
    """irfft2(gelu(sum_g softmax_g(weight(t)) fdc_g(t))), t = fpe(bn(Z)) + bn(Z), Z = rfft2(x) with its real and imaginary parts
    as interleaved channels (both transforms ``norm='ortho'``)."""

    def __init__(self, in_channels, out_channels, groups=4):
        super().__init__()
        if in_channels != out_channels:
            raise NotImplementedError(f"image_restoration_amd: FourierUnit(in_channels={in_channels!r}, out_channels={out_channels!r}) "
                                      "not covered: the unit is defined for in_channels == out_channels only")
        c = in_channels
        if not (isinstance(c, int) and isinstance(groups, int) and 1 <= c <= ops.FOURIER_UNIT_MAX_C and
                1 <= groups <= ops.FOURIER_UNIT_MAX_GROUPS and (2 * c) % groups == 0):
            raise NotImplementedError(f"image_restoration_amd: FourierUnit(in_channels={c!r}, groups={groups!r}) not covered; the "
                                      f"kernels were built for 1 <= channels <= {ops.FOURIER_UNIT_MAX_C}, 1 <= groups <= "
                                      f"{ops.FOURIER_UNIT_MAX_GROUPS}, 2 * channels a multiple of groups")
        self.groups = groups
        self.bn = nn.BatchNorm2d(2 * c)
        self.fdc = nn.Conv2d(2 * c, 2 * c * groups, 1, 1, 0, groups=groups, bias=True)
        self.weight = nn.Sequential(nn.Conv2d(2 * c, groups, 1, 1, 0), nn.Softmax(dim=1))
        self.fpe = nn.Conv2d(2 * c, 2 * c, 3, 1, 1, groups=2 * c, bias=True)

    def forward(self, x):
        bn = self.bn
        if not (bn.track_running_stats and bn.affine and bn.momentum is not None and bn.running_mean is not None):
            raise NotImplementedError("image_restoration_amd: FourierUnit's BatchNorm runs affine, with running statistics and a "
                                      "fixed momentum (the form the kernels were built for)")
        ops._gpu(x)
        training = bool(bn.training)
        gate = self.weight[0]
        out = module_op(_FourierUnitOp(bn, training), (x,), (bn.weight, bn.bias, self.fdc.weight, self.fdc.bias, gate.weight, gate.bias,
                                                             self.fpe.weight, self.fpe.bias))
        if training:
            with torch.no_grad():
                bn.num_batches_tracked += 1
        return out


def _check_dim(name, dim):
    if not (isinstance(dim, int) and 2 <= dim <= ops.SFH_FFN_MAX_DIM and dim % 2 == 0):
        raise NotImplementedError(f"image_restoration_amd: {name}(dim={dim!r}) not covered; the kernels were built for even "
                                  f"2 <= dim <= {ops.SFH_FFN_MAX_DIM} (an odd dim changes the reference's chunk count)")


class _FfnOp:
    """FFN.forward as one module op.  params: ops.sfh_ffn_fwd; saved = [the kernels' blob (h, u)]."""

    def forward(self, acts, params, need):
        out, blob = ops.sfh_ffn_fwd(acts[0], params, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.sfh_ffn_bwd(acts[0], dout, params, saved[0], grads, acc),)


class _LocalOp:
    """TokenMixer_For_Local.forward as one module op.  params: ops.sfh_local_fwd; nothing is saved beyond the input."""

    def forward(self, acts, params, need):
        return ops.sfh_local_fwd(acts[0], params), []

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.sfh_local_bwd(acts[0], dout, params, grads, acc),)


class FFN(nn.Module):
    """conv_fina(gelu(cat(h_0, conv1_1(h_1), conv1_2(h_2), conv1_3(h_3)))), h = conv_init(x) split into four dim/2-wide segments."""

    def __init__(self, dim):
        super().__init__()
        _check_dim("FFN", dim)
        self.dim, self.dim_sp = dim, dim // 2
        sp = self.dim_sp
        self.conv_init = nn.Sequential(nn.Conv2d(dim, dim * 2, 1))
        self.conv1_1 = nn.Sequential(nn.Conv2d(sp, sp, kernel_size=3, padding=1, groups=sp))
        self.conv1_2 = nn.Sequential(nn.Conv2d(sp, sp, kernel_size=5, padding=2, groups=sp))
        self.conv1_3 = nn.Sequential(nn.Conv2d(sp, sp, kernel_size=7, padding=3, groups=sp))
        self.gelu = nn.GELU()
        self.conv_fina = nn.Sequential(nn.Conv2d(dim * 2, dim, 1))

    def forward(self, x):
        ops._gpu(x)
        convs = (self.conv_init[0], self.conv1_1[0], self.conv1_2[0], self.conv1_3[0], self.conv_fina[0])
        return module_op(_FfnOp(), (x,), tuple(t for c in convs for t in (c.weight, c.bias)))


class TokenMixer_For_Local(nn.Module):
    """cat(CDilated_1(x[:, :dim/2]), CDilated_2(x[:, dim/2:])): depthwise 3x3 at dilation 1 and at dilation 2."""

    def __init__(self, dim):
        super().__init__()
        _check_dim("TokenMixer_For_Local", dim)
        self.dim, self.dim_sp = dim, dim // 2
        sp = self.dim_sp
        self.CDilated_1 = nn.Conv2d(sp, sp, 3, stride=1, padding=1, dilation=1, groups=sp)
        self.CDilated_2 = nn.Conv2d(sp, sp, 3, stride=1, padding=2, dilation=2, groups=sp)

    def forward(self, x):
        ops._gpu(x)
        return module_op(_LocalOp(), (x,), (self.CDilated_1.weight, self.CDilated_1.bias, self.CDilated_2.weight, self.CDilated_2.bias))


class _MixerOp:
    """TokenMixer_For_Gloal.forward / Mixer.forward as one module op.  params: ops.sfh_global_fwd / ops.sfh_mixer_fwd; saved = [the
    kernels' blob]; the running statistics are those of the FourierUnit inside."""

    def __init__(self, fwd, bwd, bn: nn.BatchNorm2d, training: bool):
        self.fwd, self.bwd = fwd, bwd
        self.rm, self.rv, self.training, self.eps, self.momentum = bn.running_mean, bn.running_var, training, bn.eps, bn.momentum

    def forward(self, acts, params, need):
        out, blob = self.fwd(acts[0], params, self.rm, self.rv, self.training, need, self.eps, self.momentum)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (self.bwd(acts[0], dout, params, saved[0], grads, acc, self.training, self.eps, self.momentum),)


def _run_mixer(mod, fwd, bwd, bn, x):
    if not (bn.track_running_stats and bn.affine and bn.momentum is not None and bn.running_mean is not None):
        raise NotImplementedError("image_restoration_amd: FourierUnit's BatchNorm runs affine, with running statistics and a "
                                  "fixed momentum (the form the kernels were built for)")
    ops._gpu(x)
    training = bool(bn.training)
    out = module_op(_MixerOp(fwd, bwd, bn, training), (x,), tuple(mod.parameters()))
    if training:
        with torch.no_grad():
            bn.num_batches_tracked += 1
    return out


class TokenMixer_For_Gloal(nn.Module):
    """conv_fina(FFC(p) + p), p = conv_init(x): two biased 1x1 convs, each followed by GELU, around a FourierUnit(2 dim, 2 dim)."""

    def __init__(self, dim):
        super().__init__()
        if not (isinstance(dim, int) and 1 <= dim <= ops.SFH_MIXER_MAX_DIM):
            raise NotImplementedError(f"image_restoration_amd: TokenMixer_For_Gloal(dim={dim!r}) not covered; the kernels were built "
                                      f"for 1 <= dim <= {ops.SFH_MIXER_MAX_DIM}")
        self.dim = dim
        self.conv_init = nn.Sequential(nn.Conv2d(dim, dim * 2, 1), nn.GELU())
        self.conv_fina = nn.Sequential(nn.Conv2d(dim * 2, dim, 1), nn.GELU())
        self.FFC = FourierUnit(dim * 2, dim * 2)

    def forward(self, x):
        return _run_mixer(self, ops.sfh_global_fwd, ops.sfh_global_bwd, self.FFC.bn, x)


class Mixer(nn.Module):
    """ca_conv(ca(g) g), g = gelu(cat(mixer_local(a), mixer_gloal(b))), [a, b] = conv_init(x) split in halves; ca: global average
    pool, 1x1 to dim, ReLU, 1x1 to 2 dim, sigmoid."""

    def __init__(self, dim, token_mixer_for_local=TokenMixer_For_Local, token_mixer_for_gloal=TokenMixer_For_Gloal):
        super().__init__()
        if token_mixer_for_local is not TokenMixer_For_Local or token_mixer_for_gloal is not TokenMixer_For_Gloal:
            raise NotImplementedError("image_restoration_amd: Mixer runs the reference's default token mixers only "
                                      "(TokenMixer_For_Local, TokenMixer_For_Gloal)")
        if not (isinstance(dim, int) and 2 <= dim <= ops.SFH_MIXER_MAX_DIM and dim % 2 == 0):
            raise NotImplementedError(f"image_restoration_amd: Mixer(dim={dim!r}) not covered; the kernels were built for even "
                                      f"2 <= dim <= {ops.SFH_MIXER_MAX_DIM} (the FourierUnit inside has 2 dim <= 256 channels)")
        self.dim = dim
        self.mixer_local = token_mixer_for_local(dim=dim)
        self.mixer_gloal = token_mixer_for_gloal(dim=dim)
        self.ca_conv = nn.Sequential(nn.Conv2d(2 * dim, dim, 1))
        self.ca = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Conv2d(2 * dim, 2 * dim // 2, kernel_size=1), nn.ReLU(inplace=True),
                                nn.Conv2d(2 * dim // 2, 2 * dim, kernel_size=1), nn.Sigmoid())
        self.gelu = nn.GELU()
        self.conv_init = nn.Sequential(nn.Conv2d(dim, 2 * dim, 1))

    def forward(self, x):
        return _run_mixer(self, ops.sfh_mixer_fwd, ops.sfh_mixer_bwd, self.mixer_gloal.FFC.bn, x)


_BN_FORM = ("image_restoration_amd: BatchNorm2d runs affine, with running statistics and a fixed momentum (the form the kernels "
            "were built for)")


class _Bn2dOp:
    """BatchNorm2d.forward as one module op.  params: weight, bias; saved = [stat = (mu, r)] beside the input."""

    def __init__(self, bn: nn.BatchNorm2d, training: bool):
        self.rm, self.rv, self.training, self.eps, self.momentum = bn.running_mean, bn.running_var, training, bn.eps, bn.momentum

    def forward(self, acts, params, need):
        y, stat = ops.bn2d_fwd(acts[0], params[0], params[1], self.rm, self.rv, self.training, need, self.eps, self.momentum)
        return y, [stat]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.bn2d_bwd(acts[0], dout, params[0], saved[0], grads, acc, self.training, self.eps, self.momentum),)


class BatchNorm2d(nn.BatchNorm2d):
    """``torch.nn.BatchNorm2d`` on the library's kernels: y = (x - mu) / sqrt(var + eps) * weight + bias per channel."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, device=None, dtype=None):
        if not (affine and track_running_stats and momentum is not None):
            raise NotImplementedError(_BN_FORM)
        if not (isinstance(num_features, int) and 1 <= num_features <= ops.BN2D_MAX_C):
            raise NotImplementedError(f"image_restoration_amd: BatchNorm2d(num_features={num_features!r}) not covered; the kernels were "
                                      f"built for 1 <= num_features <= {ops.BN2D_MAX_C}")
        super().__init__(num_features, eps, momentum, affine, track_running_stats, device=device, dtype=dtype)

    def forward(self, x):
        if not (self.track_running_stats and self.affine and self.momentum is not None and self.running_mean is not None):
            raise NotImplementedError(_BN_FORM)
        self._check_input_dim(x)
        ops._gpu(x)
        training = bool(self.training)
        out = module_op(_Bn2dOp(self, training), (x,), (self.weight, self.bias))
        if training:
            with torch.no_grad():
                self.num_batches_tracked += 1
        return out


class _ScaledResidualOp:
    """f * scale + x as one module op over acts (f, x) and params (scale,); nothing is saved beyond f."""

    def forward(self, acts, params, need):
        return ops.scale_res_fwd(acts[0], acts[1], params[0]), []

    def backward(self, acts, saved, dout, params, grads, acc):
        return ops.scale_res_bwd(acts[0], dout, params[0], grads[0], acc), dout


def scaled_residual(f: Tensor, x: Tensor, scale: Tensor) -> Tensor:
    """``f * scale + x`` (SFHformer.py:275, :280) with a per-channel ``scale`` of shape ``(1, C, 1, 1)`` or ``(C,)``."""
    ops._gpu(f, x, scale)
    if f.dim() != 4 or tuple(scale.shape) not in ((1, f.shape[1], 1, 1), (f.shape[1],)):
        raise ValueError(f"scaled_residual: scale of shape {tuple(scale.shape)} does not fit f {tuple(f.shape)}")
    return module_op(_ScaledResidualOp(), (f, x), (scale,))


def _block_norms(block):
    return block.norm1, block.norm2, block.mixer.mixer_gloal.FFC.bn


def _block_params(block):
    """The 40 parameters in the order ops.sfh_block_fwd takes them (the module's named_parameters() order)."""
    return (block.beta, block.gamma, block.norm1.weight, block.norm1.bias, block.norm2.weight, block.norm2.bias,
            *block.mixer.parameters(), *block.ffn.parameters())


class _StageOp:
    """A run of Blocks as one module op over ops.sfh_block_*: forward block by block, each handing the BatchNorm pairs of its
    output to the next one's norm1 (``part_in``); backward in reverse.  params: the blocks' 40 each, in order;
    saved = [blob_0, x_1, blob_1, x_2, ..., blob_{n-1}] (x_i: the input of block i; x_0 is the op's activation)."""

    def __init__(self, blocks, training: bool):
        self.stats = [[t for bn in _block_norms(b) for t in (bn.running_mean, bn.running_var)] for b in blocks]
        self.training, self.eps, self.momentum = training, blocks[0].norm1.eps, blocks[0].norm1.momentum

    def forward(self, acts, params, need):
        x, part, saved, n = acts[0], None, [], len(self.stats)
        for i, stats in enumerate(self.stats):
            if i:
                saved.append(x)
            x, blob, part = ops.sfh_block_fwd(x, params[ops.SFH_BLOCK_PARAMS * i:ops.SFH_BLOCK_PARAMS * (i + 1)], stats, self.training, need,
                                              self.eps, self.momentum, part_in=part, want_part=i + 1 < n)
            saved.append(blob)
        return x, saved

    def backward(self, acts, saved, dout, params, grads, acc):
        k = ops.SFH_BLOCK_PARAMS
        for i in reversed(range(len(self.stats))):
            dout = ops.sfh_block_bwd(saved[2 * i - 1] if i else acts[0], dout, params[k * i:k * (i + 1)], saved[2 * i], grads[k * i:k * (i + 1)],
                                     acc, self.training, self.eps, self.momentum)
        return (dout,)


def _run_blocks(blocks, x):
    """``blocks`` (in the same mode, with the same BatchNorm constants) over x as ONE autograd node."""
    norms = [bn for b in blocks for bn in _block_norms(b)]
    if not all(bn.track_running_stats and bn.affine and bn.momentum is not None and bn.running_mean is not None for bn in norms):
        raise NotImplementedError(_BN_FORM)
    first = norms[0]
    if any((bn.eps, bn.momentum, bool(bn.training)) != (first.eps, first.momentum, bool(first.training)) for bn in norms):
        raise NotImplementedError("image_restoration_amd: the BatchNorms of a Block / Stage share one eps, one momentum and one mode "
                                  "(the launch sequence takes a single pair)")
    ops._gpu(x)
    training = bool(first.training)
    out = module_op(_StageOp(blocks, training), (x,), tuple(p for b in blocks for p in _block_params(b)))
    if training:
        with torch.no_grad():
            for bn in norms:
                bn.num_batches_tracked += 1
    return out


class Block(nn.Module):
    """ffn(norm2(x1)) * gamma + x1, x1 = mixer(norm1(x)) * beta + x (SFHformer.py:254-282); ONE autograd node."""

    def __init__(self, dim, norm_layer=nn.BatchNorm2d, token_mixer=Mixer):
        super().__init__()
        if norm_layer not in (nn.BatchNorm2d, BatchNorm2d) or token_mixer is not Mixer:
            raise NotImplementedError("image_restoration_amd: Block runs the reference's defaults only (norm_layer BatchNorm2d, "
                                      "token_mixer Mixer)")
        if not (isinstance(dim, int) and 2 <= dim <= ops.SFH_BLOCK_MAX_DIM and dim % 2 == 0):
            raise NotImplementedError(f"image_restoration_amd: Block(dim={dim!r}) not covered; the kernels were built for even "
                                      f"2 <= dim <= {ops.SFH_BLOCK_MAX_DIM}")
        self.dim = dim
        self.norm1 = BatchNorm2d(dim)
        self.norm2 = BatchNorm2d(dim)
        self.mixer = token_mixer(dim=self.dim)
        self.ffn = FFN(dim=self.dim)
        self.beta = nn.Parameter(torch.zeros((1, dim, 1, 1)), requires_grad=True)
        self.gamma = nn.Parameter(torch.zeros((1, dim, 1, 1)), requires_grad=True)

    def forward(self, x):
        return _run_blocks([self], x)


class Stage(nn.Module):
    """``depth`` Blocks of ``in_channels`` channels (SFHformer.py:287-306) as ONE autograd node."""

    def __init__(self, depth=int, in_channels=int):   # (the reference's signature)
        super().__init__()
        if not (isinstance(depth, int) and depth >= 1):
            raise ValueError(f"Stage: depth={depth!r} must be a positive int")
        self.blocks = nn.Sequential(*[Block(dim=in_channels, norm_layer=nn.BatchNorm2d, token_mixer=Mixer) for _ in range(depth)])

    def forward(self, input):
        return _run_blocks(list(self.blocks), input)


class PatchEmbed(nn.Module):
    """The embedding convolution (SFHformer.py:7-21): the dense 3x3 glue; ``patch_size`` 1 and ``kernel_size`` 3 only."""

    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, kernel_size=None):
        super().__init__()
        if kernel_size is None:
            kernel_size = patch_size
        if patch_size != 1 or kernel_size != 3:
            raise NotImplementedError(f"image_restoration_amd: PatchEmbed(patch_size={patch_size!r}, kernel_size={kernel_size!r}) not "
                                      "covered; the glue was built for patch_size 1 and kernel_size 3")
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=kernel_size, stride=patch_size,
                              padding=(kernel_size - patch_size + 1) // 2, bias=True)

    def forward(self, x):
        return _glue_conv(x, self.proj)


class PatchUnEmbed(nn.Module):
    """The output convolution (SFHformer.py:24-40): the dense 3x3 glue; ``forward(x, residual)`` folds a residual into it."""

    def __init__(self, patch_size=4, out_chans=3, embed_dim=96, kernel_size=None):
        super().__init__()
        if kernel_size is None:
            kernel_size = 1
        if kernel_size != 3:
            raise NotImplementedError(f"image_restoration_amd: PatchUnEmbed(kernel_size={kernel_size!r}) not covered; the glue was "
                                      "built for kernel_size 3")
        self.out_chans, self.embed_dim = out_chans, embed_dim
        self.proj = nn.Sequential(nn.Conv2d(embed_dim, out_chans, kernel_size=kernel_size, padding=kernel_size // 2, bias=True))

    def forward(self, x, residual=None):
        return _glue_conv(x, self.proj[0], residual=residual)


class PatchUnEmbed_for_upsample(nn.Module):
    """1x1 product to ``out_dim * 4`` channels, then PixelShuffle(2) (SFHformer.py:43-55); ``patch_size`` 2 only."""

    def __init__(self, patch_size=4, embed_dim=96, out_dim=64):
        super().__init__()
        if patch_size != 2:
            raise NotImplementedError(f"image_restoration_amd: PatchUnEmbed_for_upsample(patch_size={patch_size!r}) not covered; the "
                                      "native shuffle is PixelShuffle(2)")
        self.embed_dim = embed_dim
        self.proj = nn.Sequential(nn.Conv2d(embed_dim, out_dim * patch_size ** 2, kernel_size=1, bias=False), nn.PixelShuffle(patch_size))

    def product(self, x):
        """The 1x1 product alone: what the shuffle (or the shuffle into a concatenation buffer) reads."""
        return _glue_conv(x, self.proj[0], three=False)

    def forward(self, x):
        return _shuffle(self.product(x), False)


class DownSample(nn.Module):
    """The 2x2 / stride 2 convolution (SFHformer.py:58-73) as PixelUnshuffle(2) plus the 1x1 product on the module's own weight
    viewed as [2c, 4c]."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.input_dim, self.embed_dim = input_dim, output_dim
        self.proj = nn.Sequential(nn.Conv2d(input_dim, input_dim * 2, kernel_size=2, stride=2))

    def forward(self, x):
        return _glue_conv(_shuffle(x, True), self.proj[0], three=False)


def _up_skip(up, x, skip, conv):
    """``conv(cat([up(x), skip], 1))`` (SFHformer.py:346-348, :350-352): float32 concat-free, as two K panels of the 1x1 product;
    bfloat16 (whose split-weight product has no second panel left) with the shuffle writing straight into the concatenation."""
    z = up.product(x)
    ops._gpu(skip)
    if x.dtype == torch.bfloat16:
        return _glue_conv(_apply(_UpCatFn, z, skip), conv, three=False)
    return _conv1x1_module(_shuffle(z, False), skip, conv)


class Backbone(nn.Module):
    """The SFHformer U-Net (SFHformer.py:309-357) with the reference's constructor, attribute names and ``state_dict``: five
    Stages (one autograd node each) between the glue convolutions of :mod:`.darkir` / :mod:`.restormer`.  ``patch_size`` 1 and
    ``embed_kernel_size`` 3 only; inputs of at least 8 pixels a side, H and W multiples of 4 (two 2x downsamplings, and the
    deepest Mixer needs a plane of 2 x 2)."""

    def __init__(self, in_chans=3, out_chans=3, patch_size=1, embed_dim=[48, 96, 192, 96, 48], depth=[2, 2, 2, 2, 2],  # noqa: B006
                 embed_kernel_size=3):
        super().__init__()
        if patch_size != 1 or embed_kernel_size != 3:
            raise NotImplementedError(f"image_restoration_amd: Backbone(patch_size={patch_size!r}, embed_kernel_size="
                                      f"{embed_kernel_size!r}) not covered; the glue was built for patch_size 1 and embed_kernel_size 3")
        if len(embed_dim) != 5 or len(depth) != 5:
            raise ValueError("Backbone: embed_dim and depth take five entries (one per stage)")
        if (embed_dim[1], embed_dim[2]) != (2 * embed_dim[0], 2 * embed_dim[1]) or tuple(embed_dim[3:]) != (embed_dim[1], embed_dim[0]):
            raise ValueError(f"Backbone: embed_dim={embed_dim!r} does not fit the reference's forward (DownSample doubles the "
                             "channels, and the skips meet stages of the encoder's widths)")
        self.patch_size = patch_size
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim[0], kernel_size=embed_kernel_size)
        self.layer1 = Stage(depth=depth[0], in_channels=embed_dim[0])
        self.skip1 = nn.Conv2d(embed_dim[1], embed_dim[0], 1)
        self.downsample1 = DownSample(input_dim=embed_dim[0], output_dim=embed_dim[1])
        self.layer2 = Stage(depth=depth[1], in_channels=embed_dim[1])
        self.skip2 = nn.Conv2d(embed_dim[2], embed_dim[1], 1)
        self.downsample2 = DownSample(input_dim=embed_dim[1], output_dim=embed_dim[2])
        self.layer3 = Stage(depth=depth[2], in_channels=embed_dim[2])
        self.upsample3 = PatchUnEmbed_for_upsample(patch_size=2, embed_dim=embed_dim[2], out_dim=embed_dim[3])
        self.layer8 = Stage(depth=depth[3], in_channels=embed_dim[3])
        self.upsample4 = PatchUnEmbed_for_upsample(patch_size=2, embed_dim=embed_dim[3], out_dim=embed_dim[4])
        self.layer9 = Stage(depth=depth[4], in_channels=embed_dim[4])
        self.patch_unembed = PatchUnEmbed(patch_size=patch_size, out_chans=out_chans, embed_dim=embed_dim[4], kernel_size=3)

    def forward(self, x):
        ops._gpu(x)
        if x.dim() != 4 or x.shape[2] % 4 or x.shape[3] % 4 or min(x.shape[2:]) < 8:
            raise ValueError(f"Backbone: input of shape {tuple(x.shape)} not covered; H and W must be multiples of 4, at least 8")
        copy0 = x
        copy1 = x = self.layer1(self.patch_embed(x))
        copy2 = x = self.layer2(self.downsample1(x))
        x = self.layer3(self.downsample2(x))
        x = self.layer8(_up_skip(self.upsample3, x, copy2, self.skip2))
        x = self.layer9(_up_skip(self.upsample4, x, copy1, self.skip1))
        return self.patch_unembed(x, copy0)


def SFHformer_t():
    return Backbone(patch_size=1, embed_dim=[32, 64, 128, 64, 32], depth=[1, 1, 2, 1, 1], embed_kernel_size=3)


def SFHformer_s():
    return Backbone(patch_size=1, embed_dim=[32, 64, 128, 64, 32], depth=[2, 2, 4, 2, 2], embed_kernel_size=3)


def SFHformer_m():
    return Backbone(patch_size=1, embed_dim=[32, 64, 128, 64, 32], depth=[4, 4, 8, 4, 4], embed_kernel_size=3)


def SFHformer_l():
    return Backbone(patch_size=1, embed_dim=[32, 64, 128, 64, 32], depth=[6, 6, 10, 6, 6], embed_kernel_size=3)
