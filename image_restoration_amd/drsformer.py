"""Drop-in replacements for the transformer blocks of the reference's ``DRSformer_arch.py``.

``Attention`` (TKSA, top-k sparse attention, :101-171), ``FeedForward`` (MSFN, mixed-scale FFN, :62-98) and
``TransformerBlock`` (STB, :174-187) keep the reference's class names, constructor arguments, parameter names and shapes
(``state_dict`` interchangeable) and ``forward`` signatures; ``forward`` runs the gfx950 kernels through the C-ABI
(``mi_tksa_*``, ``mi_msfn_*``, ``mi_ln_*``).  The conv submodules are parameter containers only.  Activations may be float32
(the parity path) or bfloat16; parameters and their gradients stay float32.  ``main_grad`` accumulation (FlatTrainer) as in
:mod:`image_restoration_amd.restormer`.  CPU tensors are refused: there is no fallback.

The top-k sizes are computed here with the reference's own expressions (``ops.tksa_topk``) and handed to the kernels; the
masks are ranked on the device from the fp32 scores, so nothing syncs with the host and the modules capture into HIP graphs.
``Attention.record_scores = True`` keeps the last forward's scores (``Attention.scores``, [B, heads, c, c] fp32): the S the
masks were ranked from, for tests and inspection.  Likewise ``FeedForward.record_masks = True`` keeps the last training
forward's ReLU decisions (``FeedForward.relu_masks``: a > 0, b > 0, y > 0 of the saved planes, [B, 2h, H, W] bool).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .restormer import LayerNorm, _apply, _fresh_grads, _grad_mode, _main_grads

Tensor = torch.Tensor

__all__ = ["Attention", "FeedForward", "TransformerBlock", "LayerNorm"]


def _unpack(ctx, rest):
    it = iter(rest)
    return tuple(next(it) if pr else None for pr in ctx.present)


def _scores_to(owner, scores) -> None:
    if scores is not None:
        owner.scores = scores


def _relu_masks_to(ffn, x, saved) -> None:
    if ffn.record_masks and saved is not None:
        v = ops.msfn_saved_views(saved, x, ffn.dwconv3x3_1.weight.shape[0])
        ffn.relu_masks = (v["a"] > 0, v["b"] > 0, v["y"] > 0)


class _TksaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, owner, *params):
        need = _grad_mode() and any(ctx.needs_input_grad)
        heads, topk = owner.num_heads, owner.topk(x.shape[1])
        res = ops.tksa_fwd(x, None, params, heads, topk, need, want_scores=owner.record_scores)
        out, saved = res[0], res[1]
        _scores_to(owner, res[2] if owner.record_scores else None)
        if need:
            ctx.heads, ctx.topk = heads, topk
            ctx.mg = _main_grads(params)
            ctx.present = [p is not None for p in params]
            ctx.save_for_backward(x, saved, *[p for p in params if p is not None])
        return out

    @staticmethod
    def backward(ctx, dout):
        x, saved, *rest = ctx.saved_tensors
        params = _unpack(ctx, rest)
        acc = ctx.mg is not None
        grads = ctx.mg if acc else _fresh_grads(params)
        dx = ops.tksa_bwd(x, dout.contiguous(), params, ctx.heads, ctx.topk, saved, grads, acc)
        return (dx, None) + tuple(None if acc else g for g in grads)


class _MsfnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, owner, *params):
        need = _grad_mode() and any(ctx.needs_input_grad)
        out, saved = ops.msfn_fwd(x, None, params, need)
        _relu_masks_to(owner, x, saved)
        if need:
            ctx.mg = _main_grads(params)
            ctx.present = [p is not None for p in params]
            ctx.save_for_backward(x, saved, *[p for p in params if p is not None])
        return out

    @staticmethod
    def backward(ctx, dout):
        x, saved, *rest = ctx.saved_tensors
        params = _unpack(ctx, rest)
        acc = ctx.mg is not None
        grads = ctx.mg if acc else _fresh_grads(params)
        dx = ops.msfn_bwd(x, dout.contiguous(), params, saved, grads, acc)
        return (dx, None) + tuple(None if acc else g for g in grads)


class _StbFn(torch.autograd.Function):
    """x + attn(norm1(x)), then + ffn(norm2(.)) (DRSformer_arch.py:183-187) as one autograd node; both residual adds run in
    the epilogue of the producing 1x1 GEMM, and their gradients enter the LayerNorm backward kernels (dres)."""

    N_LN, N_ATT, N_FFN = 2, 11, 12

    @staticmethod
    def forward(ctx, x, owner, *params):
        need = _grad_mode() and any(ctx.needs_input_grad)
        n1, att, n2, ffn = params[0:2], params[2:13], params[13:15], params[15:27]
        wb = n1[1] is not None
        attn = owner.attn
        heads, topk = attn.num_heads, attn.topk(x.shape[1])
        xn, mean1, rstd1 = ops.ln_fwd(x, n1[0], n1[1], wb, want_stats=need)
        res = ops.tksa_fwd(xn, x, att, heads, topk, need, want_scores=attn.record_scores)
        y, sv_a = res[0], res[1]
        _scores_to(attn, res[2] if attn.record_scores else None)
        yn, mean2, rstd2 = ops.ln_fwd(y, n2[0], n2[1], wb, want_stats=need)
        out, sv_f = ops.msfn_fwd(yn, y, ffn, need)
        _relu_masks_to(owner.ffn, yn, sv_f)
        if need:
            ctx.heads, ctx.topk, ctx.wb = heads, topk, wb
            ctx.mg = _main_grads(params)
            ctx.present = [p is not None for p in params]
            ctx.save_for_backward(x, xn, y, yn, mean1, rstd1, mean2, rstd2, sv_a, sv_f, *[p for p in params if p is not None])
        return out

    @staticmethod
    def backward(ctx, dout):
        x, xn, y, yn, mean1, rstd1, mean2, rstd2, sv_a, sv_f, *rest = ctx.saved_tensors
        params = _unpack(ctx, rest)
        acc = ctx.mg is not None
        grads = ctx.mg if acc else _fresh_grads(params)
        n1, att, n2, ffn = params[0:2], params[2:13], params[13:15], params[15:27]
        g1, ga, g2, gf = grads[0:2], grads[2:13], grads[13:15], grads[15:27]
        dout = dout.contiguous()
        dyn = ops.msfn_bwd(yn, dout, ffn, sv_f, gf, acc)
        dy = ops.ln_bwd(dyn, y, n2[0], mean2, rstd2, dout, ctx.wb, g2[0], g2[1], acc)
        dxn = ops.tksa_bwd(xn, dy, att, ctx.heads, ctx.topk, sv_a, ga, acc)
        dx = ops.ln_bwd(dxn, x, n1[0], mean1, rstd1, dy, ctx.wb, g1[0], g1[1], acc)
        return (dx, None) + tuple(None if acc else g for g in grads)


class FeedForward(nn.Module):
    """MSFN (DRSformer_arch.py:62-98)."""

    def __init__(self, dim, ffn_expansion_factor, bias):
        super().__init__()
        hidden_features = int(dim * ffn_expansion_factor)
        h2 = hidden_features * 2
        self.project_in = nn.Conv2d(dim, h2, kernel_size=1, bias=bias)
        self.dwconv3x3 = nn.Conv2d(h2, h2, kernel_size=3, stride=1, padding=1, groups=h2, bias=bias)
        self.dwconv5x5 = nn.Conv2d(h2, h2, kernel_size=5, stride=1, padding=2, groups=h2, bias=bias)
        self.relu3 = nn.ReLU()
        self.relu5 = nn.ReLU()
        self.dwconv3x3_1 = nn.Conv2d(h2, hidden_features, kernel_size=3, stride=1, padding=1, groups=hidden_features, bias=bias)
        self.dwconv5x5_1 = nn.Conv2d(h2, hidden_features, kernel_size=5, stride=1, padding=2, groups=hidden_features, bias=bias)
        self.relu3_1 = nn.ReLU()
        self.relu5_1 = nn.ReLU()
        self.project_out = nn.Conv2d(h2, dim, kernel_size=1, bias=bias)
        self.record_masks = False
        self.relu_masks = None

    def _params(self):
        return (self.project_in.weight, self.project_in.bias, self.dwconv3x3.weight, self.dwconv3x3.bias,
                self.dwconv5x5.weight, self.dwconv5x5.bias, self.dwconv3x3_1.weight, self.dwconv3x3_1.bias,
                self.dwconv5x5_1.weight, self.dwconv5x5_1.bias, self.project_out.weight, self.project_out.bias)

    def forward(self, x):
        return _apply(_MsfnFn, x, self, *self._params())


class Attention(nn.Module):
    """TKSA (DRSformer_arch.py:101-171)."""

    def __init__(self, dim, num_heads, bias):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, kernel_size=1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, kernel_size=3, stride=1, padding=1, groups=dim * 3, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)
        self.attn_drop = nn.Dropout(0.)
        self.attn1 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn2 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn3 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.attn4 = nn.Parameter(torch.tensor([0.2]), requires_grad=True)
        self.record_scores = False
        self.scores = None

    def topk(self, dim: int):
        return ops.tksa_topk(dim // self.num_heads)

    def _params(self):
        return (self.temperature, self.qkv.weight, self.qkv.bias, self.qkv_dwconv.weight, self.qkv_dwconv.bias,
                self.project_out.weight, self.project_out.bias, self.attn1, self.attn2, self.attn3, self.attn4)

    def forward(self, x):
        return _apply(_TksaFn, x, self, *self._params())


class TransformerBlock(nn.Module):
    """Sparse Transformer Block: norm1 -> attn -> +x -> norm2 -> ffn -> +x (DRSformer_arch.py:174-187), one autograd node."""

    def __init__(self, dim, num_heads, ffn_expansion_factor, bias, LayerNorm_type):
        super().__init__()
        self.norm1 = LayerNorm(dim, LayerNorm_type)
        self.attn = Attention(dim, num_heads, bias)
        self.norm2 = LayerNorm(dim, LayerNorm_type)
        self.ffn = FeedForward(dim, ffn_expansion_factor, bias)

    def forward(self, x):
        params = self.norm1._params() + self.attn._params() + self.norm2._params() + self.ffn._params()
        return _apply(_StbFn, x, self, *params)
