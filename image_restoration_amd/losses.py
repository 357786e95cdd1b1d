"""Loss terms of the reference's training step on native kernels.

``L1Loss`` stands in for ``nn.L1Loss()`` (MoCE-IR-main/src/train.py:51,54) and ``FFTLoss`` for
``MoCE-IR-main/src/utils/loss_utils.py:139-152`` (``--loss_type fft``): the mean absolute difference of the real and
imaginary parts of ``rfft2`` of prediction and target.  ``L1Loss`` and the default ``FFTLoss`` reduce with ``mi_l1_loss``
(one pass that also produces the gradient); in the default ``FFTLoss`` the transform itself is ``torch.fft.rfft2`` - rocFFT
is a library call here, plumbing like device memory - and its backward is autograd's.  ``FFTLoss(native=True)`` (opt-in)
takes the whole term, transform included, through ``mi_fft_l1_loss``: dense-DFT GEMMs on the fp32 MFMA that return the
loss and the gradient from one call, bitwise reproducible, with no FFT library and no plan to capture (2 <= H, W <= 512).

``FocalL1Loss``, ``SSIMloss`` / ``SSIM`` and ``EdgeLoss`` carry the names and constructor signatures of
``loss_utils.py:100-136``, ``:35-55`` and ``:155-190``, the other terms of the reference's training steps
(20260104_CG_IR/src/train.py:102-128: focal L1 + FFT; MoCE-IR-main/src/train_original_mulloss.py:52-92: l1 + ssim + edge +
fft).  Each is one library call (``mi_focal_l1_loss``, ``mi_ssim_loss``, ``mi_edge_loss``, csrc/losses.hip) that returns the
loss and ``d loss / d pred`` together, bitwise reproducible, with no convolution library in the step.  The SSIM is
``pytorch_msssim.ssim`` with its defaults restated (that package is not a dependency; include/mi_restore.h is the contract).
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


def _same_dtype(pred: Tensor, target: Tensor):
    """Mixed dtypes are widened to fp32, as FFTLoss(native=True) does."""
    return (pred.float(), target.float()) if pred.dtype != target.dtype else (pred, target)


def _scaled(ctx, g: Tensor, target_sign):
    """backward of a term whose gradient w.r.t. pred was saved in forward; d target = target_sign * d pred."""
    (dpred,) = ctx.saved_tensors
    ga = dpred * g.to(dpred.dtype)
    return (ga if ctx.needs_input_grad[0] else None), (target_sign * ga if ctx.needs_input_grad[1] else None)


class _FocalL1Fn(torch.autograd.Function):
    """mean(log1p(a + epsilon)^gamma * a), a = |pred - target| / alpha, the gradient taken in the same kernel pass."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, gamma: float, epsilon: float, alpha: float):
        pred, target = pred.contiguous(), target.contiguous()
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, dpred = ops.focal_l1_loss(pred, target, gamma, epsilon, alpha, want_grad=want)
        if want:
            ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        return (*_scaled(ctx, g, -1), None, None, None)


class FocalL1Loss(nn.Module):
    """``(log(1 + a + epsilon) ** gamma * a).mean()``, ``a = |pred - target| / alpha`` - loss_utils.py:100-136 (evaluated as
    ``log1p(a + epsilon)``: in fp32 ``1 + a + 1e-6`` would lose the epsilon)."""

    def __init__(self, gamma: float = 2.0, epsilon: float = 1e-6, alpha: float = 0.1) -> None:
        super().__init__()
        self.gamma = gamma
        self.epsilon = epsilon
        self.alpha = alpha

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return _FocalL1Fn.apply(*_same_dtype(pred, target), self.gamma, self.epsilon, self.alpha)


class _SSIMFn(torch.autograd.Function):
    """loss_weight * (1 - m) (``as_loss``) or loss_weight * m of the mean SSIM m, both from mi_ssim_loss with its gradient."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, loss_weight: float, data_range: float, as_loss: bool):
        if ctx.needs_input_grad[1]:
            raise RuntimeError("the SSIM terms have no gradient with respect to the target (the reference never asks for one)")
        pred, target = pred.contiguous(), target.contiguous()
        want = ctx.needs_input_grad[0]
        out, dpred = ops.ssim_loss(pred, target, loss_weight, data_range, want_grad=want)
        if want:
            ctx.save_for_backward(dpred if as_loss else -dpred)      # d (w m) = -d (w (1 - m))
        return out[0].reshape(()) if as_loss else (loss_weight * out[1]).reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        return (*_scaled(ctx, g, 0), None, None, None)       # forward refused a target that wants a gradient


class SSIMloss(nn.Module):
    """``loss_weight * (1 - ssim(pred, target, data_range))`` - loss_utils.py:48-55."""

    def __init__(self, loss_weight: float = 1.0, data_range: float = 1.) -> None:
        super().__init__()
        self.loss_weight = loss_weight
        self.data_range = data_range

    def forward(self, pred: Tensor, target: Tensor, **kwargs) -> Tensor:
        return _SSIMFn.apply(*_same_dtype(pred, target), self.loss_weight, self.data_range, True)


class SSIM(nn.Module):
    """``loss_weight * ssim(pred, target, data_range)`` - loss_utils.py:39-46."""

    def __init__(self, loss_weight: float = 1.0, data_range: float = 1.) -> None:
        super().__init__()
        self.loss_weight = loss_weight
        self.data_range = data_range

    def forward(self, pred: Tensor, target: Tensor, **kwargs) -> Tensor:
        return _SSIMFn.apply(*_same_dtype(pred, target), self.loss_weight, self.data_range, False)


class _EdgeFn(torch.autograd.Function):
    """loss_weight * mean(e^2) or mean|e| of e = Laplacian(pred - target), the gradient taken in the same library call."""

    @staticmethod
    def forward(ctx, pred: Tensor, target: Tensor, loss_weight: float, criterion: str):
        pred, target = pred.contiguous(), target.contiguous()
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, dpred = ops.edge_loss(pred, target, loss_weight, criterion, want_grad=want)
        if want:
            ctx.save_for_backward(dpred)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g: Tensor):
        return (*_scaled(ctx, g, -1), None, None)


class EdgeLoss(nn.Module):
    """``loss_weight * criterion(laplacian(pred), laplacian(target))`` - loss_utils.py:155-190; any channel count (the
    reference's kernel is hard-wired to 3)."""

    def __init__(self, loss_weight: float = 1.0, criterion: str = "l2", reduction: str = "mean") -> None:
        super().__init__()
        if reduction != "mean":
            raise ValueError("only reduction='mean' is implemented (the reference passes the default)")
        if criterion not in ops.EDGE_CRITERIA:
            raise NotImplementedError("Unsupported criterion loss")
        self.weight = loss_weight
        self.criterion = criterion

    def forward(self, pred: Tensor, target: Tensor) -> Tensor:
        return _EdgeFn.apply(*_same_dtype(pred, target), self.weight, self.criterion)
