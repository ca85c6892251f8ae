"""Autograd binding for the fused CDNA4 flash attention kernels."""
from __future__ import annotations

import os
from typing import Optional

import torch

from perceiver_amd.ops import hip


def _to_bf16(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


class FlashAttention(torch.autograd.Function):
    """out = softmax(mask(q k^T)) v with online softmax on device.

    q arrives pre-scaled. pad_mask: (B, Lk) bool, True = padding. causal uses the
    right-aligned convention (j > Lk - Nq + i masked). Saves (q, k, v, out, lse)
    for the recompute-based backward.
    """

    @staticmethod
    def forward(ctx, q, k, v, pad_mask: Optional[torch.Tensor], causal: bool,
                dropout_p: float, training: bool):
        # last-dim contiguity is enough (the kernels take batch/head/seq strides);
        # head-transposed views and preallocated cache buffers pass zero-copy
        q, k, v = _to_bf16(q), _to_bf16(k), _to_bf16(v)
        p = float(dropout_p) if training else 0.0
        seed = int(torch.randint(0, 2**62, (1,)).item()) if p > 0 else 0
        out, lse = hip.ext().flash_fwd(q, k, v, pad_mask, causal, p, seed)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.pad_mask = pad_mask
        ctx.causal = causal
        ctx.dropout = (p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        p, seed = ctx.dropout
        dq, dk, dv = hip.ext().flash_bwd(
            _to_bf16(dout), q, k, v, out, lse, ctx.pad_mask, ctx.causal, p, seed
        )
        return dq, dk, dv, None, None, None, None


class PackedQKVFlashAttention(torch.autograd.Function):
    """Self-attention from the merged projection ``qkv`` (B, N, [q | k | v]).

    The forward is the module's: split, head views, ``q * dp_scale`` as a torch
    multiply (q is rounded to bf16 as ever), the flash forward. The backward has
    ``flash_bwd`` write dq, dk, dv as the column slices of ONE (B, N, 2*qk + v)
    buffer, scales the dq slice in place (the rounding ``MulBackward`` makes) and
    returns the buffer as ``d_qkv``: the concatenation that the split's backward
    ran over three separate gradients (a read and a write of the whole tensor per
    layer) is gone, and every bit stays what it was.
    """

    @staticmethod
    def forward(ctx, qkv, num_heads: int, qk: int, vc: int, dp_scale: float,
                pad_mask: Optional[torch.Tensor], causal: bool, dropout_p: float,
                training: bool):
        q, k, v = _split_qkv_heads(qkv, num_heads, qk, vc)
        q = q * dp_scale
        p = float(dropout_p) if training else 0.0
        seed = int(torch.randint(0, 2**62, (1,)).item()) if p > 0 else 0
        out, lse = hip.ext().flash_fwd(q, k, v, pad_mask, causal, p, seed)
        ctx.save_for_backward(qkv, q, out, lse)
        ctx.split = (num_heads, qk, vc, dp_scale)
        ctx.pad_mask = pad_mask
        ctx.causal = causal
        ctx.dropout = (p, seed)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, q, out, lse = ctx.saved_tensors
        num_heads, qk, vc, dp_scale = ctx.split
        _, k, v = _split_qkv_heads(qkv, num_heads, qk, vc)
        p, seed = ctx.dropout
        d_qkv = torch.empty_like(qkv, memory_format=torch.contiguous_format)
        hip.ext().flash_bwd(
            _to_bf16(dout), q, k, v, out, lse, ctx.pad_mask, ctx.causal, p, seed, d_qkv
        )
        d_qkv[..., :qk].mul_(dp_scale)
        return d_qkv, None, None, None, None, None, None, None, None


def _split_qkv_heads(qkv, num_heads: int, qk: int, vc: int):
    """(B, H, N, D) head views of the q, k, v column slices of ``qkv``."""
    b, n, _ = qkv.shape
    return tuple(
        t.view(b, n, num_heads, -1).transpose(1, 2) for t in qkv.split([qk, qk, vc], dim=-1)
    )


def packed_qkv_grad_enabled() -> bool:
    """PERCEIVER_PACKED_QKV_GRAD=0 restores split + three gradients + concat."""
    return os.environ.get("PERCEIVER_PACKED_QKV_GRAD", "1") != "0"


def can_pack_qkv_grad(qkv, num_heads: int, qk: int, vc: int, pad_mask,
                      dropout_p: float, training: bool) -> bool:
    """Whether :class:`PackedQKVFlashAttention` serves this self-attention call:
    bf16 on the GPU, head dims the flash kernels take without padded copies."""
    if not (packed_qkv_grad_enabled() and qkv.is_cuda and qkv.dtype == torch.bfloat16
            and qkv.dim() == 3 and hip.is_available()):
        return False
    d_qk, d_v = qk // num_heads, vc // num_heads
    ext = hip.ext()
    return bool(ext.flash_supported(d_qk, d_v, int(training and dropout_p > 0))
                and ext.flash_bwd_packs_qkv_grad(d_qk, d_v))


def packed_qkv_attention(qkv, num_heads: int, qk: int, vc: int, dp_scale: float,
                         pad_mask=None, causal: bool = False, dropout_p: float = 0.0,
                         training: bool = False):
    return PackedQKVFlashAttention.apply(
        qkv, num_heads, qk, vc, dp_scale, pad_mask, causal, dropout_p, training
    )
