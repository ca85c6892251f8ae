"""Single-query attention over per-row key windows (ops/csrc/decode_attn.hip).

``decode_attn(q, k, v, lo, hi)``: row ``b`` of the batch attends the keys
``lo[b] .. hi[b]``, both inclusive, and nothing else. ``lo`` and ``hi`` are int64
tensors of 1 or ``B`` elements on the tensors' device (``lo=None`` means 0) that
the kernel reads itself, so a captured launch serves every window.

Rules, shared by the kernel and the mask composition:

- both ends are clamped into ``[0, cap)``, so no content of ``lo`` / ``hi`` can
  cause an out-of-range read;
- a window with ``hi < lo`` (before clamping) gives zeros. The decoder never
  produces one;
- for a non-empty window the result is attention under
  ``pad_mask = (j < lo[b]) | (j > hi[b])``.

The kernel takes bf16 on the GPU with head dims that are multiples of 8 up to
128 (``decode_attn_applicable``). Everything else, and the CPU, runs
``window_attention_composition``: build the mask, call ``scaled_dot_attention``.

A ``KeyWindow`` in the ``pad_mask`` slot of ``scaled_dot_attention`` is how the
decoder reaches this through the attention modules, which hand ``pad_mask`` on
untouched. ``PERCEIVER_DECODE_ATTN=0`` forces the mask composition on the GPU
(A/B lever).
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

import torch

from perceiver_amd.ops import hip

MAX_HEAD_DIM = 128
SLICE_KEYS_PER_PARTIAL = 32
FULL_GRID = 512


class KeyWindow(NamedTuple):
    """Keys ``lo[b] .. hi[b]`` (inclusive) of row ``b``; ``lo=None`` means 0."""

    lo: Optional[torch.Tensor]
    hi: torch.Tensor


def kernel_enabled() -> bool:
    return os.environ.get("PERCEIVER_DECODE_ATTN", "1") != "0"


def decode_attn_applicable(d: int, dv: int) -> bool:
    """Head dims the kernel takes. Pure host; the extension holds the same rule."""
    return 8 <= d <= MAX_HEAD_DIM and 8 <= dv <= MAX_HEAD_DIM and d % 8 == 0 and dv % 8 == 0


def decode_attn_plan(b: int, h: int, cap: int, d: int) -> Tuple[int, int]:
    """(nsplit, row granule) of the kernel's static grid ``(nsplit, H, B)``.

    Pure host, shapes only. ``nsplit`` is 1 where ``B * H`` fills the chip (512
    workgroups) or the capacity is too small to split, and at most 32; the merge
    reads ``nsplit`` partials per row, so a slice of the capacity keeps at least
    32 keys for each of them (``32 * nsplit**2 <= cap``). The granule is the
    number of key rows one load instruction of a wave covers,
    ``64 / pow2ceil(D / 8)``; a row's slices are multiples of it."""
    lanes = 1
    while lanes < (d + 7) // 8:
        lanes *= 2
    blocks = b * h
    by_cap = 1
    while SLICE_KEYS_PER_PARTIAL * (by_cap + 1) ** 2 <= cap:
        by_cap += 1
    nsplit = 1 if blocks >= FULL_GRID else min(FULL_GRID // blocks + 1, by_cap, 32)
    return nsplit, 64 // lanes


def _rows_aligned(t: torch.Tensor) -> bool:
    return (t.stride(-1) == 1 and t.data_ptr() % 16 == 0
            and all(t.size(i) == 1 or t.stride(i) % 8 == 0 for i in range(3)))


def kernel_applicable(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> bool:
    """Whether ``decode_attn`` runs the HIP kernel for these tensors."""
    return (q.is_cuda and kernel_enabled() and hip.is_available()
            and q.dtype == k.dtype == v.dtype == torch.bfloat16
            and q.dim() == 4 and q.shape[2] == 1
            and decode_attn_applicable(q.shape[-1], v.shape[-1])
            and _rows_aligned(q) and _rows_aligned(k) and _rows_aligned(v))


def _window_end(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return t.to(device=like.device, dtype=torch.long).reshape(-1).contiguous()


def window_attention_composition(q, k, v, lo, hi, causal: bool = False, dropout_p: float = 0.0,
                                 training: bool = False, max_heads_parallel=None):
    """The window as a pad mask through ``scaled_dot_attention``: same rules as
    the kernel (clamped ends, zeros for an empty window), any device and dtype.
    ``causal`` is right-aligned to the capacity and masks nothing at one query."""
    from perceiver_amd.ops.attention import scaled_dot_attention

    cap = k.shape[-2]
    hi = _window_end(hi, k)
    lo = torch.zeros_like(hi) if lo is None else _window_end(lo, k)
    empty = hi < lo
    j = torch.arange(cap, device=k.device)[None, :]
    pad = (j < lo.clamp(0, cap - 1)[:, None]) | (j > hi.clamp(0, cap - 1)[:, None])
    pad = pad.expand(max(q.shape[0], k.shape[0]), cap)
    out = scaled_dot_attention(q, k, v, pad_mask=pad, causal=causal, dropout_p=dropout_p,
                               training=training, max_heads_parallel=max_heads_parallel)
    return out.masked_fill(empty.expand(out.shape[0])[:, None, None, None], 0.0)


def decode_attn(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                lo: Optional[torch.Tensor], hi: torch.Tensor) -> torch.Tensor:
    """q (B, H, 1, D) pre-scaled, k (B, H, cap, D), v (B, H, cap, Dv) ->
    (B, H, 1, Dv), a view of merged-heads (B, 1, H * Dv) memory on the kernel
    path. Strided views (head-transposed cache buffers, batch-stride-0 ``q``)
    pass without copies."""
    if q.shape[0] != k.shape[0] and q.shape[0] == 1:
        q = q.expand(k.shape[0], *q.shape[1:])
    if kernel_applicable(q, k, v):
        hi = _window_end(hi, k)
        lo = None if lo is None else _window_end(lo, k)
        return hip.ext().decode_attn(q, k, v, lo, hi)
    return window_attention_composition(q, k, v, lo, hi)
