"""Autograd glue shared by every network of the package: the caller's grad mode, the trainer's ``main_grad`` buffers, the
packing of optional tensors, and ONE ``torch.autograd.Function`` for module ops.

A module op is "k activation tensors + a parameter list with optional holes -> one output", written as a function pair on an
object that carries its non-tensor state (heads, top-k sizes, the owner module of a recording switch):

    op.forward(acts, params, need) -> (out, saved)      ``saved``: a sequence whose entries may be None; ``need`` False: no
                                                        blobs, no LayerNorm statistics
    op.backward(acts, saved, dout, params, grads, accumulate) -> the gradients of ``acts`` (a tuple); the parameter gradients
                                                        are written (accumulate: added) into ``grads``

``module_op(op, acts, params)`` runs the pair as one autograd node; the ``torch.library`` ops of ``torch_ops.py`` call the same
pairs.

Gradient accumulation: if every parameter of a module carries a ``main_grad`` attribute (a float32 tensor of the parameter's
shape, e.g. a view into a flat DDP bucket), backward accumulates into it in place and reports no autograd gradient for the
parameters; otherwise ordinary ``.grad`` flow.
"""
from __future__ import annotations

import threading
from typing import List, Optional, Sequence

import torch

Tensor = torch.Tensor


def _main_grads(params: Sequence[Optional[Tensor]]) -> Optional[List[Optional[Tensor]]]:
    """main_grad buffers if every present parameter has one, else None."""
    out = []
    for p in params:
        if p is None:
            out.append(None)
            continue
        mg = getattr(p, "main_grad", None)
        if mg is None:
            return None
        out.append(mg)
    return out


def _fresh_grads(params: Sequence[Optional[Tensor]]) -> List[Optional[Tensor]]:
    return [None if p is None else torch.empty_like(p) for p in params]


# Inside Function.forward grad mode is always off and ctx.needs_input_grad ignores torch.no_grad(), so the caller's grad
# mode is recorded right before .apply(): under no_grad nothing is saved for backward (no blobs, no LN statistics).
_tls = threading.local()


def _apply(fn, *args):
    _tls.grad = torch.is_grad_enabled()
    return fn.apply(*args)


def _grad_mode() -> bool:
    return getattr(_tls, "grad", True)


# ---- optional tensors (bias=False parameters, saved entries a fused form does not keep) around save_for_backward -------------
def _present(ts: Sequence[Optional[Tensor]]) -> List[bool]:
    return [t is not None for t in ts]


def _squeeze(ts: Sequence[Optional[Tensor]]) -> List[Tensor]:
    return [t for t in ts if t is not None]


def _refill(present: Sequence[bool], ts: Sequence[Tensor]) -> list:
    """Inverse of _squeeze: ``ts`` back at the True positions of ``present``, None in the holes."""
    it = iter(ts)
    return [next(it) if pr else None for pr in present]


class _ModuleOpFn(torch.autograd.Function):
    """The one node under every module op: decides ``need``, picks main_grad buffers or fresh gradient tensors, packs the
    holes of parameters and saved entries around save_for_backward, and builds the gradient tuple."""

    @staticmethod
    def forward(ctx, op, n_acts, *tensors):
        acts, params = tensors[:n_acts], tensors[n_acts:]
        need = _grad_mode() and any(ctx.needs_input_grad)
        out, saved = op.forward(acts, params, need)
        if need:
            ctx.op, ctx.n_acts, ctx.n_saved = op, n_acts, len(saved)
            ctx.mg = _main_grads(params)
            ctx.present = _present(saved) + _present(params)
            ctx.save_for_backward(*acts, *_squeeze(saved), *_squeeze(params))
        return out

    @staticmethod
    def backward(ctx, dout):
        tens = ctx.saved_tensors
        acts, rest = tens[:ctx.n_acts], _refill(ctx.present, tens[ctx.n_acts:])
        saved, params = rest[:ctx.n_saved], tuple(rest[ctx.n_saved:])
        acc = ctx.mg is not None
        grads = ctx.mg if acc else _fresh_grads(params)
        dacts = ctx.op.backward(acts, saved, dout.contiguous(), params, grads, acc)
        return (None, None) + tuple(dacts) + tuple(None if acc else g for g in grads)


def module_op(op, acts: Sequence[Tensor], params: Sequence[Optional[Tensor]]) -> Tensor:
    """Run the function pair ``op`` over ``acts`` and ``params`` as one autograd node."""
    return _apply(_ModuleOpFn, op, len(acts), *acts, *params)
