"""SFHformer on the MI355X, the pieces built so far: the spectral token mixer core ``FourierUnit``, the feed-forward ``FFN``, the
local token mixer ``TokenMixer_For_Local``, the global one and the ``Mixer``, and the Block's ``BatchNorm2d`` and ``scaled_residual``
(below).

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

``Block`` and ``Backbone`` stay the reference's PyTorch modules, but their norm and their residual are now available natively: the
reference's ``Block(dim, norm_layer=BatchNorm2d)`` takes the class as it is.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._autograd import module_op

Tensor = torch.Tensor

__all__ = ["BatchNorm2d", "FFN", "FourierUnit", "Mixer", "TokenMixer_For_Gloal", "TokenMixer_For_Local", "scaled_residual"]


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
