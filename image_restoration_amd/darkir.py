"""Drop-in replacements for DarkIR's dilated-gate decoder block and its frequency MLP (``DarkIR-main/archs/arch_model.py``:
``DBlock`` :72-139 with ``SimpleGate`` :12-15 and ``Branch`` :57-70, ``FreMLP`` :36-55; ``archs/arch_util.py``: ``LayerNorm2d``
:35-44).

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
factored DFT, which is not built.  ``EBlock`` and the whole ``DarkIR`` network are not part of this module yet.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from ._autograd import module_op

Tensor = torch.Tensor

__all__ = ["SimpleGate", "LayerNorm2d", "Branch", "DBlock", "FreMLP"]

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


class _DBlockOp:
    """DBlock.forward as one module op.  params: ops._dblock_struct's flat list; saved = [the kernels' blob]."""

    def __init__(self, dilations, extra):
        self.dilations, self.extra = dilations, extra

    def forward(self, acts, params, need):
        out, blob = ops.dblock_fwd(acts[0], params, self.dilations, self.extra, need)
        return out, [blob]

    def backward(self, acts, saved, dout, params, grads, acc):
        return (ops.dblock_bwd(acts[0], dout, params, self.dilations, self.extra, saved[0], grads, acc),)


class DBlock(nn.Module):
    """norm1 -> conv1 -> extra_conv -> summed dilated branches -> SimpleGate -> SCA -> conv3 -> + beta; norm2 -> conv4 ->
    SimpleGate -> conv5 -> + gamma (arch_model.py:72-139), one autograd node."""

    def __init__(self, c, DW_Expand=2, FFN_Expand=2, dilations=[1], extra_depth_wise=False):  # noqa: B006 (the reference's signature)
        super().__init__()
        if DW_Expand != 2 or FFN_Expand != 2:
            raise NotImplementedError(f"image_restoration_amd: DBlock with DW_Expand={DW_Expand}, FFN_Expand={FFN_Expand} not "
                                      "covered; the kernels were built for DW_Expand = FFN_Expand = 2")
        dilations = list(dilations)
        if not 1 <= len(dilations) <= ops.DILGATE_MAX_BRANCHES:
            raise NotImplementedError(f"image_restoration_amd: DBlock with {len(dilations)} branches not covered; the kernels "
                                      f"were built for 1..{ops.DILGATE_MAX_BRANCHES} dilations")
        for d in dilations:
            _check_dilation(d)
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
        return module_op(_DBlockOp(self._dilations, self._extra), (inp,), self._params())


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
