"""Fused bf16 LayerNorm: drop-in nn.LayerNorm subclass dispatching to the CDNA4
kernel (ops/csrc/layer_norm.hip) for bf16 CUDA inputs; eager elsewhere. State-dict
layout identical to nn.LayerNorm.

:func:`add_layer_norm` is the residual-stream form: it takes the pending pair
(branch output ``h``, shortcut ``x``) of the previous residual block and returns
``s = h + x`` together with ``LayerNorm(s)`` from one kernel pass; its backward
folds the gradient arriving on ``s`` into the LayerNorm backward, so neither the
forward add nor autograd's fan-in add runs as a pass of its own."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn

from perceiver_amd.ops import hip


class _FusedLayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, mean, rstd = hip.ext().ln_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, weight, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors
        needs_dwdb = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dw, db = hip.ext().ln_bwd(dy, x, weight, mean, rstd, needs_dwdb)
        return dx, dw if ctx.needs_input_grad[1] else None, \
            db if ctx.needs_input_grad[2] else None, None


class AddLayerNormFn(torch.autograd.Function):
    """``(h, x, weight, bias, eps) -> (s, y)`` with ``s = h + x`` (bf16, rounded once
    like torch's add) and ``y = LayerNorm(s)``. ``h`` may be None: the block opens a
    chain, ``s`` is ``x``, and only the backward differs from the plain LayerNorm.

    The backward receives ``(ds, dy)`` and returns ONE tensor ``d = bf16(dx) + ds``
    for both ``h`` and ``x``: the sum that autograd would otherwise form with an add
    kernel where the shortcut and the LayerNorm gradients meet."""

    @staticmethod
    def forward(ctx, h, x, weight, bias, eps):
        ctx.set_materialize_grads(False)
        if h is None:
            y, mean, rstd = hip.ext().ln_fwd(x, weight, bias, eps)
            s = x
        else:
            s, y, mean, rstd = hip.ext().add_ln_fwd(h, x, weight, bias, eps)
        ctx.save_for_backward(s, weight, mean, rstd)
        ctx.has_h = h is not None
        return s, y

    @staticmethod
    def backward(ctx, ds, dy):
        s, weight, mean, rstd = ctx.saved_tensors
        dw = db = None
        if dy is None:
            d = ds  # the normalised output went unused: the shortcut passes through
        else:
            needs_dwdb = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
            d, dw, db = hip.ext().ln_bwd(dy, s, weight, mean, rstd, needs_dwdb, ds)
        return (d if ctx.has_h and ctx.needs_input_grad[0] else None,
                d if ctx.needs_input_grad[1] else None,
                dw if ctx.needs_input_grad[2] else None,
                db if ctx.needs_input_grad[3] else None,
                None)


def _fused_ln_applies(ln: nn.LayerNorm, x: torch.Tensor) -> bool:
    return (
        x.is_cuda
        and x.dtype == torch.bfloat16
        and ln.weight is not None
        and ln.weight.dtype == torch.bfloat16
        and len(ln.normalized_shape) == 1
        and ln.normalized_shape[0] <= 2048
        and hip.is_available()
    )


def add_layer_norm(ln: nn.LayerNorm, h: Optional[torch.Tensor],
                   x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(s, ln(s))`` for ``s = h + x``, or ``s = x`` when ``h`` is None.

    One kernel pass where the fused LayerNorm applies and ``h`` is shaped like ``x``
    (a broadcast shortcut, such as a batch-1 latent array, is added by torch);
    the plain composition everywhere else."""
    if _fused_ln_applies(ln, x) and (
        h is None or (h.shape == x.shape and h.dtype == x.dtype and h.is_cuda)
    ):
        return AddLayerNormFn.apply(
            None if h is None else h.contiguous(), x.contiguous(), ln.weight, ln.bias, ln.eps
        )
    s = x if h is None else h + x
    return s, ln(s)


class LayerNorm(nn.LayerNorm):
    def forward(self, x):
        if _fused_ln_applies(self, x):
            return _FusedLayerNormFn.apply(x.contiguous(), self.weight, self.bias, self.eps)
        return super().forward(x)
