"""Drop-in replacements for DarkIR's blocks and the whole network (``DarkIR-main/archs/arch_model.py``: ``DBlock`` :72-139 with
``SimpleGate`` :12-15 and ``Branch`` :57-70, ``FreMLP`` :36-55, ``EBlock`` :141-204; ``archs/arch_util.py``: ``LayerNorm2d`` :35-44,
``CustomSequential`` :47-61; ``archs/DarkIR.py``: ``DarkIR``).

The classes keep the reference's names, constructor signatures, parameter names and shapes (``state_dict`` interchangeable) and
``forward`` signatures; ``DBlock.forward`` runs the gfx950 kernels through the C-ABI (``mi_dblock_*``: the multi-dilation
depthwise sum with SimpleGate and the SCA pool in one stencil pass, the pair-grouped ``extra_conv``, the c x c folds that make
``conv3`` / ``conv5`` with their scales and residuals one 1x1 GEMM each) as ONE autograd node.  The submodules are parameter
containers; ``SimpleGate`` and ``LayerNorm2d`` also run on their own, each on its kernel (a lone ``Branch`` raises: the
branches of a block are one stencil pass).  ``LayerNorm2d`` normalises
over channels with a biased variance and ``eps = 1e-6`` (the other families' LayerNorm uses 1e-5).  Activations may be float32
(the parity path) or bfloat16; parameters and their gradients stay float32.  ``main_grad`` accumulation (FlatTrainer) as in
:mod:`image_restoration_amd.restormer`.  CPU tensors are refused: there is no fallback.

The kernels were built for ``DW_Expand = FFN_Expand = 2``, one to four branches with dilations 1..16 and c <= 256; anything else
raises ``NotImplementedError``.

``FreMLP.forward`` is one autograd node too (``mi_fremlp_*``): ``rfft2`` and ``irfft2`` as dense-DFT GEMMs on the fp32 MFMA (no
FFT library), the polar form as ``|Z|`` and ``Z / |Z|`` (no ``atan2``, ``cos`` or ``sin``), the two 1x1 convs of ``process1`` per
frequency bin in fp32.  Planes of 2..512 pixels a side, ``nc <= 256``, ``expand * nc <= 512``; larger images need tiling or a
factored DFT, which is not built.

``EBlock.forward`` is one autograd node (``mi_eblock_*``): DBlock's first half (the library runs one launch sequence for both,
and one op class and one constructor check serve both here) with a plain depthwise ``extra_conv`` in front of ``conv1``, then
``norm2``, FreMLP and the streaming tail ``y * (1 + gamma * f)`` (``mi_fregate_*``).  1 <= c <= 256, planes of
2..512 pixels a side.  ``DarkIR`` assembles the U-Net with the reference's attribute names and ``state_dict``; its glue convolutions
run on the native 1x1 / 3x3 kernels (split weights with bf16 activations).  Width 32 (DarkIR-m) runs; width 64 reaches c = 512 and
is refused at construction; a padded input above 512 pixels a side is refused in ``forward``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._autograd import _apply, _grad_mode, _main_grads, module_op
from .restormer import _Conv1x1Fn, _conv2d, _fire_forward_hooks, _shuffle

Tensor = torch.Tensor

__all__ = ["SimpleGate", "LayerNorm2d", "Branch", "DBlock", "FreMLP", "EBlock", "CustomSequential", "DarkIR"]

LN_EPS = 1e-6


class _GateOp:
    """x1 * x2 of the two channel halves (mi_ewise, op 0, on channel slices)."""

    def forward(self, acts, params, need):
        x = acts[0]
        ops._gpu(x)
        c = x.shape[1] // 2
        return ops.ewise_fwd(x[:, :c], x[:, c:], 0), []

    def backward(self, acts, saved, dout, params, grads, acc):
        x = acts[0]
        c = x.shape[1] // 2
        dx = torch.empty_like(x)
        ops.ewise_bwd(x[:, :c], x[:, c:], dout, 0, da=dx[:, :c], db=dx[:, c:])
        return (dx,)


class SimpleGate(nn.Module):
    def forward(self, x):
        return module_op(_GateOp(), (x,), ())


class _Ln2dOp:
    def __init__(self, eps):
        self.eps = eps

    def forward(self, acts, params, need):
        y, mean, rstd = ops.ln_fwd_eps(acts[0], params[0], params[1], True, self.eps, want_stats=need)
        return y, [mean, rstd]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.ln_bwd(dout, acts[0], params[0], saved[0], saved[1], None, True, grads[0], grads[1], acc),)


class LayerNorm2d(nn.Module):
    """Channel LayerNorm on NCHW with weight and bias, biased variance, eps 1e-6 by default (arch_util.py:35-44)."""

    def __init__(self, channels, eps=1e-6):
        super().__init__()
        self.register_parameter('weight', nn.Parameter(torch.ones(channels)))
        self.register_parameter('bias', nn.Parameter(torch.zeros(channels)))
        self.eps = eps

    def forward(self, x):
        return module_op(_Ln2dOp(self.eps), (x,), (self.weight, self.bias))


def _check_dilation(d):
    if not (isinstance(d, int) and 1 <= d <= ops.DILGATE_MAX_DILATION):
        raise NotImplementedError(f"image_restoration_amd: dilation {d!r} not covered; the dilated-gate kernels were built for "
                                  f"integer dilations 1..{ops.DILGATE_MAX_DILATION}")


class Branch(nn.Module):
    """The dilated depthwise 3x3 conv of one branch (arch_model.py:57-70); a parameter container: DBlock sums its branches in
    one stencil pass."""

    def __init__(self, c, DW_Expand, dilation=1):
        super().__init__()
        _check_dilation(dilation)
        self.dw_channel = DW_Expand * c
        self.branch = nn.Sequential(
            nn.Conv2d(in_channels=self.dw_channel, out_channels=self.dw_channel, kernel_size=3, padding=dilation, stride=1,
                      groups=self.dw_channel, bias=True, dilation=dilation))

    def forward(self, input):
        raise NotImplementedError("image_restoration_amd: Branch runs inside DBlock only (the branches of a block are one "
                                  "mi_dilgate_* stencil pass); the module holds the parameters")


class _BlockOp:
    """DBlock.forward or EBlock.forward as one module op: ``fwd`` / ``bwd`` are ops.dblock_fwd / _bwd or ops.eblock_fwd / _bwd.
    params: the flat list of ops._dblock_struct / ops._eblock_struct; saved = [the kernels' blob]."""

    def __init__(self, fwd, bwd, dilations, extra):
        self.fwd, self.bwd, self.dilations, self.extra = fwd, bwd, dilations, extra

    def forward(self, acts, params, need):
        out, blob = self.fwd(acts[0], params, self.dilations, self.extra, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (self.bwd(acts[0], dout, params, self.dilations, self.extra, saved[0], grads, acc),)


def _block_args(name, dilations=None, **expand):
    """The constructor checks that DBlock and EBlock share.  ``expand``: the block's expansion factors (DW_Expand, and DBlock's
    FFN_Expand), which the kernels take as 2; ``dilations``: checked and returned as a list.  (EBlock calls it once for each, with
    its own check of c between the two, which is where that check has always stood.)"""
    if any(v != 2 for v in expand.values()):
        raise NotImplementedError(f"image_restoration_amd: {name} with {', '.join(f'{k}={v}' for k, v in expand.items())} not "
                                  f"covered; the kernels were built for {' = '.join(expand)} = 2")
    if dilations is None:
        return None
    dilations = list(dilations)
    if not 1 <= len(dilations) <= ops.DILGATE_MAX_BRANCHES:
        raise NotImplementedError(f"image_restoration_amd: {name} with {len(dilations)} branches not covered; the kernels "
                                  f"were built for 1..{ops.DILGATE_MAX_BRANCHES} dilations")
    for d in dilations:
        _check_dilation(d)
    return dilations


class DBlock(nn.Module):
    """norm1 -> conv1 -> extra_conv -> summed dilated branches -> SimpleGate -> SCA -> conv3 -> + beta; norm2 -> conv4 ->
    SimpleGate -> conv5 -> + gamma (arch_model.py:72-139), one autograd node."""

    def __init__(self, c, DW_Expand=2, FFN_Expand=2, dilations=[1], extra_depth_wise=False):  # noqa: B006 (the reference's signature)
        super().__init__()
        dilations = _block_args("DBlock", dilations, DW_Expand=DW_Expand, FFN_Expand=FFN_Expand)
        self.dw_channel = DW_Expand * c
        self.conv1 = nn.Conv2d(in_channels=c, out_channels=self.dw_channel, kernel_size=1, padding=0, stride=1, groups=1, bias=True,
                               dilation=1)
        self.extra_conv = nn.Conv2d(self.dw_channel, self.dw_channel, kernel_size=3, padding=1, stride=1, groups=c, bias=True,
                                    dilation=1) if extra_depth_wise else nn.Identity()
        self.branches = nn.ModuleList()
        for dilation in dilations:
            self.branches.append(Branch(self.dw_channel, DW_Expand=1, dilation=dilation))
        self.sca = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(in_channels=self.dw_channel // 2, out_channels=self.dw_channel // 2, kernel_size=1, padding=0, stride=1,
                      groups=1, bias=True, dilation=1))
        self.sg1 = SimpleGate()
        self.sg2 = SimpleGate()
        self.conv3 = nn.Conv2d(in_channels=self.dw_channel // 2, out_channels=c, kernel_size=1, padding=0, stride=1, groups=1,
                               bias=True, dilation=1)
        ffn_channel = FFN_Expand * c
        self.conv4 = nn.Conv2d(in_channels=c, out_channels=ffn_channel, kernel_size=1, padding=0, stride=1, groups=1, bias=True)
        self.conv5 = nn.Conv2d(in_channels=ffn_channel // 2, out_channels=c, kernel_size=1, padding=0, stride=1, groups=1, bias=True)
        self.norm1 = LayerNorm2d(c)
        self.norm2 = LayerNorm2d(c)
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)), requires_grad=True)
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)), requires_grad=True)
        self._dilations = tuple(dilations)
        self._extra = bool(extra_depth_wise)

    def _params(self):
        ex = self.extra_conv if self._extra else None
        convs = [b.branch[0] for b in self.branches]
        return (self.norm1.weight, self.norm1.bias, self.conv1.weight, self.conv1.bias,
                None if ex is None else ex.weight, None if ex is None else ex.bias,
                *[m.weight for m in convs], *[m.bias for m in convs],
                self.sca[1].weight, self.sca[1].bias, self.conv3.weight, self.conv3.bias, self.beta,
                self.norm2.weight, self.norm2.bias, self.conv4.weight, self.conv4.bias, self.conv5.weight, self.conv5.bias,
                self.gamma)

    def forward(self, inp, adapter=None):
        if self.norm1.eps != LN_EPS or self.norm2.eps != LN_EPS:
            raise NotImplementedError(f"image_restoration_amd: DBlock's LayerNorm2d runs with eps = {LN_EPS} (the value the block "
                                      "kernels were built for)")
        return module_op(_BlockOp(ops.dblock_fwd, ops.dblock_bwd, self._dilations, self._extra), (inp,), self._params())


class _FreMlpOp:
    """FreMLP.forward as one module op.  params: process1's two weights and biases; saved = [the kernels' blob]."""

    def forward(self, acts, params, need):
        out, blob = ops.fremlp_fwd(acts[0], params, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.fremlp_bwd(dout, params, saved[0], grads, acc),)


class FreMLP(nn.Module):
    """irfft2(process1(|Z|) * Z / |Z|), Z = rfft2(x) (arch_model.py:36-55), one autograd node.  ``process1`` holds the
    parameters (a DarkIR checkpoint loads unchanged); its LeakyReLU(0.1) runs inside the kernels."""

    def __init__(self, nc, expand=2):
        super().__init__()
        if not (isinstance(nc, int) and isinstance(expand, int) and 1 <= nc <= ops.FREMLP_MAX_NC and expand >= 1 and
                expand * nc <= ops.FREMLP_MAX_HIDDEN):
            raise NotImplementedError(f"image_restoration_amd: FreMLP(nc={nc!r}, expand={expand!r}) not covered; the kernels were "
                                      f"built for 1 <= nc <= {ops.FREMLP_MAX_NC}, expand >= 1, expand * nc <= "
                                      f"{ops.FREMLP_MAX_HIDDEN}")
        self.process1 = nn.Sequential(
            nn.Conv2d(nc, expand * nc, 1, 1, 0),
            nn.LeakyReLU(0.1, inplace=True),
            nn.Conv2d(expand * nc, nc, 1, 1, 0))

    def forward(self, x):
        if self.process1[1].negative_slope != 0.1:
            raise NotImplementedError("image_restoration_amd: FreMLP's LeakyReLU runs with slope 0.1 (the value the kernels were "
                                      "built for)")
        c1, c2 = self.process1[0], self.process1[2]
        return module_op(_FreMlpOp(), (x,), (c1.weight, c1.bias, c2.weight, c2.bias))


class EBlock(nn.Module):
    """norm1 -> extra_conv -> conv1 -> summed dilated branches -> SimpleGate -> SCA -> conv3 -> + beta; norm2 -> FreMLP ->
    y + gamma (y * f) (arch_model.py:141-204), one autograd node.  ``extra_conv`` is a plain depthwise 3x3 in FRONT of ``conv1``
    (DBlock's is pair-grouped and behind it); there is no conv4 / conv5."""

    def __init__(self, c, DW_Expand=2, dilations=[1], extra_depth_wise=False):  # noqa: B006 (the reference's signature)
        super().__init__()
        _block_args("EBlock", DW_Expand=DW_Expand)
        if not (isinstance(c, int) and 1 <= c <= ops.EBLOCK_MAX_C):
            raise NotImplementedError(f"image_restoration_amd: EBlock(c={c!r}) not covered; the block kernels were built for "
                                      f"1 <= c <= {ops.EBLOCK_MAX_C}")
        dilations = _block_args("EBlock", dilations)
        self.dw_channel = DW_Expand * c
        self.extra_conv = nn.Conv2d(c, c, kernel_size=3, padding=1, stride=1, groups=c, bias=True,
                                    dilation=1) if extra_depth_wise else nn.Identity()
        self.conv1 = nn.Conv2d(in_channels=c, out_channels=self.dw_channel, kernel_size=1, padding=0, stride=1, groups=1, bias=True,
                               dilation=1)
        self.branches = nn.ModuleList()
        for dilation in dilations:
            self.branches.append(Branch(c, DW_Expand, dilation=dilation))
        self.sca = nn.Sequential(
            nn.AdaptiveAvgPool2d(1),
            nn.Conv2d(in_channels=self.dw_channel // 2, out_channels=self.dw_channel // 2, kernel_size=1, padding=0, stride=1,
                      groups=1, bias=True, dilation=1))
        self.sg1 = SimpleGate()
        self.conv3 = nn.Conv2d(in_channels=self.dw_channel // 2, out_channels=c, kernel_size=1, padding=0, stride=1, groups=1,
                               bias=True, dilation=1)
        self.norm1 = LayerNorm2d(c)
        self.norm2 = LayerNorm2d(c)
        self.freq = FreMLP(nc=c, expand=2)
        self.gamma = nn.Parameter(torch.zeros((1, c, 1, 1)), requires_grad=True)
        self.beta = nn.Parameter(torch.zeros((1, c, 1, 1)), requires_grad=True)
        self._dilations = tuple(dilations)
        self._extra = bool(extra_depth_wise)

    def _params(self):
        ex = self.extra_conv if self._extra else None
        convs = [b.branch[0] for b in self.branches]
        p1 = self.freq.process1
        return (self.norm1.weight, self.norm1.bias, None if ex is None else ex.weight, None if ex is None else ex.bias,
                self.conv1.weight, self.conv1.bias, *[m.weight for m in convs], *[m.bias for m in convs],
                self.sca[1].weight, self.sca[1].bias, self.conv3.weight, self.conv3.bias, self.beta,
                self.norm2.weight, self.norm2.bias, p1[0].weight, p1[0].bias, p1[2].weight, p1[2].bias, self.gamma)

    def forward(self, inp):
        if self.norm1.eps != LN_EPS or self.norm2.eps != LN_EPS:
            raise NotImplementedError(f"image_restoration_amd: EBlock's LayerNorm2d runs with eps = {LN_EPS} (the value the block "
                                      "kernels were built for)")
        if self.freq.process1[1].negative_slope != 0.1:
            raise NotImplementedError("image_restoration_amd: FreMLP's LeakyReLU runs with slope 0.1 (the value the kernels were "
                                      "built for)")
        return module_op(_BlockOp(ops.eblock_fwd, ops.eblock_bwd, self._dilations, self._extra), (inp,), self._params())


def _split_weight(w2):
    """[M, K] fp32 -> [M, 2K] = [hi | lo], hi = w rounded to bfloat16, lo = w - hi: the two K panels of a split product."""
    hi = w2.to(torch.bfloat16).to(torch.float32)
    return torch.cat([hi, w2 - hi], 1)


def _split_product(x, w2, bias=None, residual=None):
    """W x (+ bias) (+ residual) for bf16 activations with the weights at 16 mantissa bits: [hi | lo] . [x ; x] through the 1x1
    GEMM's two K panels, as the block kernels do (the MFMA path alone would round each weight to 8 bits: an error common to a
    channel, which the pixel sums of the bias gradients keep whole)."""
    return ops.conv1x1(x, _split_weight(w2), bias, residual, False, x)


class _GlueConvFn(torch.autograd.Function):
    """The network's glue convolutions on bf16 activations: a 1x1 product (``ups``; ``downs`` on the unshuffled planes, with the
    module's [2c, c, 2, 2] weight read as [2c, 4c]) or a dense 3x3 with padding 1 (``intro``, ``ending``, ``side_out``) in the
    layout forms of :class:`.restormer._Conv3x3Fn` (im2col when Cin <= Cout, col2im otherwise), every product on split weights.
    float32 activations take :mod:`.restormer`'s functions, which read the weights as they are."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, three):
        cout = weight.shape[0]
        ctx.three, ctx.small_in = three, three and weight.shape[1] <= cout
        if not three:
            y, saved = _split_product(x, weight.reshape(cout, -1), bias, residual), x
        elif ctx.small_in:
            saved = ops.im2col3x3(x)
            y = _split_product(saved, weight.reshape(cout, -1), bias, residual)
        else:
            wz = weight.permute(0, 2, 3, 1).reshape(cout * 9, -1)                       # [(co,ky,kx), ci]
            y, saved = ops.col2im3x3(_split_product(x, wz), bias, residual), x
        if _grad_mode() and any(ctx.needs_input_grad):
            ctx.save_for_backward(saved, weight)
            ctx.has_bias = bias is not None
            ctx.mg = _main_grads((weight, bias))
        return y

    @staticmethod
    def backward(ctx, dy):
        saved, weight = ctx.saved_tensors
        dy = dy.contiguous()
        cout = weight.shape[0]
        acc = ctx.mg is not None
        dx = None
        if not ctx.three or ctx.small_in:
            w2 = weight.reshape(cout, -1)
            dw = ops.gram(dy, saved, 1, True)[0].reshape(weight.shape)
            if ctx.needs_input_grad[0]:
                dx = _split_product(dy, w2.t().contiguous())
                if ctx.three:
                    dx = ops.col2im3x3(dx, flip=True)
        else:
            dz = ops.im2col3x3(dy, flip=True)                                          # [(co,ky,kx)] planes
            dw = ops.gram(dz, saved, 1, True)[0].reshape(cout, 3, 3, -1).permute(0, 3, 1, 2)
            if ctx.needs_input_grad[0]:
                dx = _split_product(dz, weight.permute(1, 0, 2, 3).reshape(weight.shape[1], cout * 9))
        db = None
        if ctx.has_bias:
            db = ops.chan_sum(dy, ctx.mg[1] if acc else None, acc)
        dres = dy if ctx.needs_input_grad[3] else None
        if acc:
            ctx.mg[0].add_(dw)
            return dx, None, None, dres, None
        return dx, dw.contiguous(), db, dres, None


def _glue_conv(x, conv, residual=None, three=True):
    """``conv`` on the native kernels: bf16 activations through the split-weight forms above, float32 through
    :func:`.restormer._conv2d` / ``_Conv1x1Fn``.  ``three=False``: a 1x1 product on the module's weight viewed as [Cout, -1]."""
    if x.dtype != torch.bfloat16 and three:
        return _conv2d(x, conv, residual)
    if three and not (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.groups == 1):
        raise NotImplementedError("image_restoration_amd: only the dense 3x3 / stride 1 / pad 1 glue convolution is built")
    ops._gpu(x, residual)
    if x.dtype != torch.bfloat16:
        y = _apply(_Conv1x1Fn, x, None, conv.weight, conv.bias)
    else:
        y = _apply(_GlueConvFn, x, conv.weight, conv.bias, residual, three)
    _fire_forward_hooks(conv, (x,), y)          # the module is used functionally: observers still see it take part
    return y


class CustomSequential(nn.Module):
    """The reference's container (arch_util.py:47-61): ``modules_list`` keeps its name so that checkpoints load; the second
    argument is the reference's adapter switch, which its blocks no longer have."""

    def __init__(self, *args):
        super().__init__()
        self.modules_list = nn.ModuleList(args)

    def forward(self, x, use_adapter=False):
        for module in self.modules_list:
            if hasattr(module, 'set_use_adapters'):
                module.set_use_adapters(use_adapter)
            x = module(x)
        return x


class DarkIR(nn.Module):
    """The DarkIR U-Net (archs/DarkIR.py): EBlock encoders, DBlock decoders, strided-conv downs, 1x1 + PixelShuffle ups; the
    reference's attribute names, ``state_dict`` and ``forward(input, side_loss=False, use_adapter=None)``.  Every convolution runs
    on the native kernels: ``intro`` / ``ending`` / ``side_out`` through the dense 3x3 glue of :mod:`.restormer`, a ``downs[i]``
    (2x2, stride 2) as PixelUnshuffle(2) plus the 1x1 product on the module's own weight viewed as [2c, 4c], an ``ups[i]`` as
    the 1x1 product plus PixelShuffle(2).  The deepest level may have at most 256 channels and the padded input at most 512
    pixels a side (FreMLP's dense transforms)."""

    def __init__(self, img_channel=3, width=32, middle_blk_num_enc=2, middle_blk_num_dec=2, enc_blk_nums=[1, 2, 3],  # noqa: B006
                 dec_blk_nums=[3, 1, 1], dilations=[1, 4, 9], extra_depth_wise=True):  # noqa: B006 (the reference's signature)
        super().__init__()
        deepest = width * 2 ** len(enc_blk_nums)
        if not (isinstance(width, int) and width >= 1 and deepest <= ops.EBLOCK_MAX_C):
            raise NotImplementedError(f"image_restoration_amd: DarkIR(width={width!r}) with {len(enc_blk_nums)} levels reaches "
                                      f"c = {deepest} at its deepest level; the block kernels were built for c <= {ops.EBLOCK_MAX_C}")
        if len(dec_blk_nums) != len(enc_blk_nums):
            raise ValueError("DarkIR: enc_blk_nums and dec_blk_nums must have the same length (one skip per level)")
        self.intro = nn.Conv2d(in_channels=img_channel, out_channels=width, kernel_size=3, padding=1, stride=1, groups=1, bias=True)
        self.ending = nn.Conv2d(in_channels=width, out_channels=img_channel, kernel_size=3, padding=1, stride=1, groups=1, bias=True)
        self.encoders = nn.ModuleList()
        self.decoders = nn.ModuleList()
        self.middle_blks = nn.ModuleList()
        self.ups = nn.ModuleList()
        self.downs = nn.ModuleList()
        chan = width
        for num in enc_blk_nums:
            self.encoders.append(CustomSequential(*[EBlock(chan, extra_depth_wise=extra_depth_wise) for _ in range(num)]))
            self.downs.append(nn.Conv2d(chan, 2 * chan, 2, 2))
            chan = chan * 2
        self.middle_blks_enc = CustomSequential(*[EBlock(chan, extra_depth_wise=extra_depth_wise) for _ in range(middle_blk_num_enc)])
        self.middle_blks_dec = CustomSequential(*[DBlock(chan, dilations=dilations, extra_depth_wise=extra_depth_wise)
                                                  for _ in range(middle_blk_num_dec)])
        for num in dec_blk_nums:
            self.ups.append(nn.Sequential(nn.Conv2d(chan, chan * 2, 1, bias=False), nn.PixelShuffle(2)))
            chan = chan // 2
            self.decoders.append(CustomSequential(*[DBlock(chan, dilations=dilations, extra_depth_wise=extra_depth_wise)
                                                    for _ in range(num)]))
        self.padder_size = 2 ** len(self.encoders)
        # the layer behind the reference's middle ("side") loss
        self.side_out = nn.Conv2d(in_channels=width * 2 ** len(self.encoders), out_channels=img_channel, kernel_size=3, stride=1,
                                  padding=1)

    def forward(self, input, side_loss=False, use_adapter=None):
        ops._gpu(input)
        _, _, H, W = input.shape
        input = self.check_image_size(input)
        if max(input.shape[-2:]) > ops.EBLOCK_MAX_HW:
            raise NotImplementedError(f"image_restoration_amd: DarkIR on a padded input of {input.shape[-2]} x {input.shape[-1]} not "
                                      f"covered; FreMLP's dense transforms take at most {ops.EBLOCK_MAX_HW} pixels a side "
                                      "(tile the image)")
        x = _glue_conv(input, self.intro)
        skips = []
        for encoder, down in zip(self.encoders, self.downs):
            x = encoder(x)
            skips.append(x)
            x = _glue_conv(_shuffle(x, True), down, three=False)
        x_light = self.middle_blks_enc(x)
        if side_loss:
            out_side = _glue_conv(x_light, self.side_out)
        x = self.middle_blks_dec(x_light)
        x = x + x_light
        for decoder, up, skip in zip(self.decoders, self.ups, skips[::-1]):
            x = _shuffle(_glue_conv(x, up[0], three=False), False)
            x = x + skip
            x = decoder(x)
        x = _glue_conv(x, self.ending, residual=input)
        out = x[:, :, :H, :W]            # the original size of the image
        if side_loss:
            return out_side, out
        return out

    def check_image_size(self, x):
        _, _, h, w = x.size()
        mod_pad_h = (self.padder_size - h % self.padder_size) % self.padder_size
        mod_pad_w = (self.padder_size - w % self.padder_size) % self.padder_size
        if mod_pad_h or mod_pad_w:
            x = torch.nn.functional.pad(x, (0, mod_pad_w, 0, mod_pad_h), value=0)
        return x
