"""Token selection for decode: greedy, or temperature / top-k / top-p sampling.

On the GPU the whole selection is one launch of the ``decode_select`` kernel
(ops/csrc/decode_select.hip), which reads every parameter per row from device
memory. ``keep_mask_reference`` states the kept-set rules in plain torch and is
what the kernel is tested against:

- order is the order of the raw fp32 logits (temperature T > 0 is monotone);
- top-k keeps every token whose logit is >= the k-th largest, ties included;
  ``top_k <= 0`` or ``>= V`` is off;
- top-p runs after top-k on ``exp((x - max) / T)`` renormalised over the top-k
  set: token i stays iff the mass of tokens with a strictly larger logit is
  <= ``top_p``, so tied tokens stay or go together; ``top_p <= 0`` or ``>= 1``
  is off.

``PERCEIVER_DECODE_SELECT=0`` forces the torch composition (A/B lever).
"""
from __future__ import annotations

import os
from typing import Optional, Union

import torch

from perceiver_amd.ops import hip

Param = Union[None, int, float, bool, torch.Tensor]


def kernel_enabled() -> bool:
    return os.environ.get("PERCEIVER_DECODE_SELECT", "1") != "0"


def kernel_applicable(device: torch.device, vocab: int) -> bool:
    """Whether ``select_tokens`` / ``GraphedDecoder`` run the HIP kernel for
    logits of ``vocab`` entries on ``device``."""
    return (device.type == "cuda" and kernel_enabled() and hip.is_available()
            and bool(hip.ext().decode_select_applicable(int(vocab))))


def row_param(value: Param, batch: int, dtype: torch.dtype, device, off) -> torch.Tensor:
    """A scalar or (batch,) tensor as a contiguous (batch,) tensor; None means ``off``."""
    if value is None:
        value = off
    if isinstance(value, torch.Tensor):
        t = value.to(device=device, dtype=dtype).reshape(-1)
        if t.numel() == 1:
            t = t.expand(batch)
        if t.numel() != batch:
            raise ValueError(f"per-row parameter has {t.numel()} entries for batch {batch}")
        return t.contiguous()
    return torch.full((batch,), value, dtype=dtype, device=device)


def keep_mask_reference(logits: torch.Tensor, temperature: Param = 1.0, top_k: Param = None,
                        top_p: Param = None) -> torch.Tensor:
    """(B, V) bool: the tokens that survive top-k then top-p, by the module's rules."""
    x = logits.float()
    B, V = x.shape
    dev = x.device
    T = row_param(temperature, B, torch.float64, dev, 1.0)
    k = row_param(top_k, B, torch.long, dev, 0)
    p = row_param(top_p, B, torch.float64, dev, 1.0)

    sv, si = torch.sort(x, dim=-1, descending=True)
    k_on = (k > 0) & (k < V)
    kth = sv.gather(1, (k.clamp(1, V) - 1)[:, None])
    keep_sorted = torch.where(k_on[:, None], sv >= kth, torch.ones_like(sv, dtype=torch.bool))

    w = torch.exp((sv.double() - sv[:, :1].double()) / T[:, None]) * keep_sorted
    excl = w.cumsum(-1) - w  # mass before each sorted position
    # a tied token looks back to the start of its run: mass of STRICTLY larger logits
    first = torch.ones_like(keep_sorted)
    first[:, 1:] = sv[:, 1:] != sv[:, :-1]
    above = torch.where(first, excl, torch.zeros_like(excl)).cummax(-1).values
    p_on = (p > 0) & (p < 1)
    keep_sorted = keep_sorted & torch.where(p_on[:, None], above <= p[:, None] * w.sum(-1, keepdim=True),
                                            torch.ones_like(keep_sorted))
    return torch.zeros_like(keep_sorted).scatter(1, si, keep_sorted)


def keep_mask(logits: torch.Tensor, temperature: Param = 1.0, top_k: Param = None,
              top_p: Param = None) -> torch.Tensor:
    """The kernel's kept set (debug entry of ``decode_select``, through the same
    device function the sampler uses); the reference off the GPU."""
    if logits.dim() != 2 or not kernel_applicable(logits.device, logits.shape[-1]):
        return keep_mask_reference(logits, temperature, top_k, top_p)
    B, dev = logits.shape[0], logits.device
    if logits.dtype not in (torch.float32, torch.bfloat16):
        logits = logits.float()
    return hip.ext().decode_keep_mask(
        logits, row_param(temperature, B, torch.float32, dev, 1.0),
        row_param(top_k, B, torch.int32, dev, 0), row_param(top_p, B, torch.float32, dev, 1.0))


def _scalar_i64(value, device) -> torch.Tensor:
    if isinstance(value, torch.Tensor):
        return value.to(device=device, dtype=torch.long).reshape(1).contiguous()
    return torch.full((1,), int(value), dtype=torch.long, device=device)


def select_reference(logits: torch.Tensor, do_sample: Param, temperature: Param, top_k: Param,
                     top_p: Param, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The torch composition: (B,) int64, drawing from torch's generator."""
    x = logits.float()
    B, dev = x.shape[0], x.device
    greedy = x.argmax(-1)
    ds = row_param(do_sample, B, torch.bool, dev, False)
    if not bool(ds.any()):
        return greedy
    T = row_param(temperature, B, torch.float32, dev, 1.0)
    keep = keep_mask_reference(x, T, top_k, top_p)
    probs = (x / T[:, None]).masked_fill(~keep, float("-inf")).softmax(-1)
    # rows that have no softmax (NaN, all -inf) are greedy rows
    bad = ~torch.isfinite(probs).all(-1) | (probs.sum(-1) <= 0)
    probs = torch.where(bad[:, None], torch.ones_like(probs), probs)
    drawn = torch.multinomial(probs, 1, generator=generator).squeeze(-1)
    return torch.where(ds & ~bad, drawn, greedy)


def select_tokens(logits: torch.Tensor, *, do_sample: Param = False, temperature: Param = 1.0,
                  top_k: Param = None, top_p: Param = None, seed=0, draw=0) -> torch.Tensor:
    """One token per row of (B, V) logits as (B,) int64.

    Parameters are scalars or (B,) tensors. With the kernel the draw is a pure
    function of (seed, row, draw, logits); otherwise the torch composition runs
    with a generator seeded from (seed, draw)."""
    if logits.dim() != 2:
        raise ValueError("select_tokens takes (B, V) logits")
    B, dev = logits.shape[0], logits.device
    if kernel_applicable(dev, logits.shape[-1]):
        if logits.dtype not in (torch.float32, torch.bfloat16):
            logits = logits.float()
        return hip.ext().decode_select(
            logits, row_param(do_sample, B, torch.int32, dev, 0),
            row_param(temperature, B, torch.float32, dev, 1.0),
            row_param(top_k, B, torch.int32, dev, 0), row_param(top_p, B, torch.float32, dev, 1.0),
            _scalar_i64(seed, dev), _scalar_i64(draw, dev))
    g = torch.Generator(device=dev)
    g.manual_seed((int(seed) * 1000003 + int(draw)) % (2 ** 63))
    return select_reference(logits, do_sample, temperature, top_k, top_p, g)


def select_step(logits: torch.Tensor, do_sample: torch.Tensor, temperature: torch.Tensor,
                top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor, draw: torch.Tensor,
                *, tok: torch.Tensor, done: torch.Tensor, eos_fill: torch.Tensor,
                out_buf: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None):
    """One in-place decode step, the launch a captured graph replays. Every
    argument is a device buffer in the kernel's own dtype (the (B,) parameters
    as ``row_param`` makes them, ``seed`` / ``draw`` / ``step`` one int64 each).
    With ``out_buf`` and ``step`` the previous ``tok`` is first recorded at
    column ``step`` of ``out_buf``; then ``tok`` (B,) takes the selected token,
    or the fill of ``eos_fill = [eos, fill]`` on a ``done`` row, and ``done``
    takes the rows that emitted EOS."""
    hip.ext().decode_select(logits, do_sample, temperature, top_k, top_p, seed, draw, tok=tok,
                            out_buf=out_buf, step=step, done=done, eos_fill=eos_fill)
