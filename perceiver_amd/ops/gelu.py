"""Fused bias+GELU autograd op (K6 epilogue piece): y = gelu(x + b) in one pass on
GPU; bias gradient = column-sum of the pre-activation gradient."""
from __future__ import annotations

import torch

from perceiver_amd.ops import hip


class GeluBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        y = hip.ext().gelu_bias_fwd(x, bias)
        ctx.save_for_backward(x, bias if bias is not None else torch.tensor([]))
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, bias = ctx.saved_tensors
        b = bias if ctx.has_bias else None
        dx = hip.ext().gelu_bias_bwd(x, b, dy.contiguous())
        db = None
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = _colsum(dx)
        return dx, db


def _colsum(t: torch.Tensor) -> torch.Tensor:
    """bias gradient: column sum via the coalesced kernel (torch's generic
    reduce on these tall-skinny shapes was 0.86 ms/step in the MLM trace)."""
    t2 = t.reshape(-1, t.shape[-1])
    if t2.shape[-1] <= 2048:
        return hip.ext().colsum_bf16(t2.contiguous()).to(t.dtype)
    return t2.float().sum(dim=0).to(t.dtype)


class LinearGeluBias(torch.autograd.Function):
    """MLP widening layer gelu(x @ W^T + b) with the GEMM and the bias+GELU
    epilogue fused in one gemm_bt kernel. The kernel also emits the pre-bias
    activation, so the backward is the existing gelu_bias_bwd recompute path
    (numerically identical to F.linear + GeluBias)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        lead = x.shape[:-1]
        M, K = x.numel() // x.shape[-1], x.shape[-1]
        x2 = x.reshape(M, K)
        pre, post = hip.ext().gemm_bt_gelu(x2, weight, bias)
        ctx.save_for_backward(x2, weight, bias, pre)
        return post.view(*lead, weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, weight, bias, pre = ctx.saved_tensors
        dy2 = dy.reshape(-1, dy.shape[-1]).contiguous()
        dpre = hip.ext().gelu_bias_bwd(pre, bias, dy2)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            from perceiver_amd.ops.linear import dgrad_matmul

            dx = dgrad_matmul(dpre, weight, dy.shape[:-1])
        from perceiver_amd.ops.linear import wgrad_and_bias

        dw, db = wgrad_and_bias(dpre, x2, ctx.needs_input_grad[1], ctx.needs_input_grad[2],
                                _colsum)
        return dx, dw, db


def can_fuse_gelu_bias(x: torch.Tensor) -> bool:
    return (
        x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 and hip.is_available()
    )


def can_fuse_linear_gelu(x: torch.Tensor, weight: torch.Tensor) -> bool:
    from perceiver_amd.ops.linear import _NO_CUSTOM_GEMM

    if _NO_CUSTOM_GEMM:
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
            and hip.is_available()):
        return False
    M, K = x.numel() // x.shape[-1], x.shape[-1]
    return bool(hip.ext().gemm_bt_applicable(M, weight.shape[0], K))
