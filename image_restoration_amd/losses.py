"""Loss terms of the reference's training step on native kernels.

``L1Loss`` stands in for ``nn.L1Loss()`` (MoCE-IR-main/src/train.py:51,54) and ``FFTLoss`` for
``MoCE-IR-main/src/utils/loss_utils.py:139-152`` (``--loss_type fft``): the mean absolute difference of the real and
imaginary parts of ``rfft2`` of prediction and target.  ``L1Loss`` and the default ``FFTLoss`` reduce with ``mi_l1_loss``
(one pass that also produces the gradient); in the default ``FFTLoss`` the transform itself is ``torch.fft.rfft2`` - rocFFT
is a library call here, plumbing like device memory - and its backward is autograd's.  ``FFTLoss(native=True)`` (opt-in)
takes the whole term, transform included, through ``mi_fft_l1_loss``: dense-DFT GEMMs on the fp32 MFMA that return the
loss and the gradient from one call, bitwise reproducible, with no FFT library and no plan to capture (2 <= H, W <= 512).
GPU tensors only: the product has no CPU path."""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import ops


class _L1MeanFn(torch.autograd.Function):
    """mean|a - b| with the gradient taken in the same kernel pass."""

    @staticmethod
    def forward(ctx, a: Tensor, b: Tensor):
        a, b = a.contiguous(), b.contiguous()
        loss, da = ops.l1_loss(a, b, want_grad=True)
        ctx.save_for_backward(da)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        (da,) = ctx.saved_tensors
        ga = da * g.to(da.dtype)
        return ga, (-ga if ctx.needs_input_grad[1] else None)


class L1Loss(nn.Module):
    """``nn.L1Loss(reduction='mean')`` on the native kernel."""

    def __init__(self, reduction: str = "mean") -> None:
        super().__init__()
        if reduction != "mean":
            raise ValueError("only reduction='mean' is implemented (the reference uses the default)")

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return _L1MeanFn.apply(pred, target.to(pred.dtype))


class _FFTL1Fn(torch.autograd.Function):
    """loss_weight * mean(|Re| + |Im|) of rfft2(pred - target), the gradient taken in the same library call."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, loss_weight: float):
        pred, target = pred.contiguous(), target.contiguous()
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, dpred = ops.fft_l1_loss(pred, target, loss_weight, want_grad=want)
        if want:
            ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        (dpred,) = ctx.saved_tensors
        ga = dpred * g.to(dpred.dtype)
        return (ga if ctx.needs_input_grad[0] else None), (-ga if ctx.needs_input_grad[1] else None), None


class FFTLoss(nn.Module):
    """``loss_weight * L1(stack(re, im)(rfft2(pred)), stack(re, im)(rfft2(target)))`` - loss_utils.py:139-152.
    ``native=True``: the transform, the reduction and the gradient run in ``mi_fft_l1_loss`` instead of rocFFT + autograd."""

    def __init__(self, loss_weight: float = 1.0, reduction: str = "mean", native: bool = False) -> None:
        super().__init__()
        if reduction != "mean":
            raise ValueError("only reduction='mean' is implemented (the reference passes the default)")
        self.loss_weight = loss_weight
        self.native = native

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        if self.native:
            if pred.dtype != target.dtype:
                pred, target = pred.float(), target.float()
            return _FFTL1Fn.apply(pred, target, self.loss_weight)
        # view_as_real lays (re, im) out innermost, exactly what the reference's torch.stack(..., dim=-1) builds
        pf = torch.view_as_real(torch.fft.rfft2(pred.float()))
        tf = torch.view_as_real(torch.fft.rfft2(target.float()))
        return self.loss_weight * _L1MeanFn.apply(pf, tf)
