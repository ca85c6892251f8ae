"""Beam search steps for the graphed decode path.

On the GPU one step is two launches (ops/csrc/beam_select.hip): ``beam_select``
picks each group's ``num_beams`` best continuations and does the bookkeeping,
``beam_reorder`` permutes the generated rows of every KV buffer in place.
``beam_select_reference`` states the rules in plain torch and is what the
kernel is tested against:

- per row i with running fp32 score ``s_i``: ``logp = (x - max) - log(sum(exp(x - max)))``
  in fp32, candidate ``s_i + logp``;
- a frozen row (``done``) proposes ``s_i + 0`` at the fill token and
  ``s_i + (-1e9)`` everywhere else (fp32 adds, as the host loop has them);
- a group's new beams are its ``num_beams`` largest candidates ordered by
  (candidate descending, flat index ``i * V + v`` ascending); NaN compares
  largest, as in ``topk``;
- ``done' = done[src] | (tok == eos)``, ``gen_len' = gen_len[src] + !done[src]``.

``PERCEIVER_BEAM_GRAPH=0`` forces the torch composition (A/B lever).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch

from perceiver_amd.ops import hip

MIN_BEAMS, MAX_BEAMS, MAX_VOCAB = 2, 8, 32768


def kernel_enabled() -> bool:
    return os.environ.get("PERCEIVER_BEAM_GRAPH", "1") != "0"


def in_range(vocab: int, num_beams: int) -> bool:
    """The range ``beam_select`` takes (host-side twin of ``beam_select_applicable``)."""
    return 1 <= int(vocab) <= MAX_VOCAB and MIN_BEAMS <= int(num_beams) <= MAX_BEAMS


def kernel_applicable(device: torch.device, vocab: int, num_beams: int) -> bool:
    """Whether a beam ``GraphedDecoder`` on ``device`` runs the HIP kernels."""
    return (device.type == "cuda" and kernel_enabled() and hip.is_available()
            and bool(hip.ext().beam_select_applicable(int(vocab), int(num_beams))))


def beam_select_reference(logits: torch.Tensor, scores: torch.Tensor, done: torch.Tensor,
                          gen_len: torch.Tensor, num_beams: int, eos, fill,
                          dtype: torch.dtype = torch.float32):
    """One beam step by the module's rules, out of place.

    ``logits`` (G * num_beams, V); ``scores``, ``done``, ``gen_len`` (G * num_beams,);
    ``eos`` / ``fill`` are ints or 0-dim tensors (``eos < 0``: none). Returns
    ``(src, tok, scores', done', gen_len', all_done)`` with ``src`` the source
    beam inside its group and ``all_done`` (G,). ``dtype=torch.float64`` gives
    the tests' high-precision reference of the same rules."""
    B, V = logits.shape
    nb = int(num_beams)
    G = B // nb
    x = logits.to(dtype)
    s = scores.to(dtype)
    xmax = x.max(-1, keepdim=True).values
    logp = (x - xmax) - (x - xmax).exp().sum(-1, keepdim=True).log()
    fill_t = torch.as_tensor(fill, device=x.device).long()
    eos_t = torch.as_tensor(eos, device=x.device).long()
    is_fill = torch.arange(V, device=x.device)[None, :] == fill_t
    frozen = torch.where(is_fill, torch.zeros((), dtype=dtype, device=x.device),
                         torch.full((), -1e9, dtype=dtype, device=x.device))
    cand = s[:, None] + torch.where(done[:, None], frozen.expand(B, V), logp)
    # stable: among equal candidates the lowest flat index comes first
    order = cand.view(G, nb * V).sort(dim=-1, descending=True, stable=True)
    top, flat = order.values[:, :nb], order.indices[:, :nb]
    src = flat // V
    tok = (flat - src * V).reshape(-1)
    rows = (src + torch.arange(G, device=x.device)[:, None] * nb).reshape(-1)
    was = done.index_select(0, rows)
    new_done = was | (tok == eos_t)
    new_len = gen_len.index_select(0, rows) + (~was).to(gen_len.dtype)
    return (src.reshape(-1).to(torch.int32), tok, top.reshape(-1), new_done, new_len,
            new_done.view(G, nb).all(-1))


def beam_select_step(logits: torch.Tensor, scores: torch.Tensor, done: torch.Tensor,
                     gen_len: torch.Tensor, tok: torch.Tensor, src: torch.Tensor,
                     all_done: torch.Tensor, eos_fill: torch.Tensor, num_beams: int, *,
                     step: torch.Tensor, rec_offset: int, rec_tok: torch.Tensor,
                     rec_parent: torch.Tensor, rec_all_done: torch.Tensor):
    """Launch one beam step in place: ``scores``, ``done``, ``gen_len`` (int32),
    ``tok`` (int64), ``src`` (int32), all (G * num_beams,), and ``all_done`` (G,)
    take the results ``beam_select_reference`` returns, with ``eos_fill`` the
    int64 pair ``[eos, fill]``. Row ``step + rec_offset`` of the records
    ``rec_tok`` / ``rec_parent`` / ``rec_all_done`` takes ``tok`` / ``src`` /
    ``all_done``; ``step`` is one int64 on the device."""
    hip.ext().beam_select(logits, scores, done, gen_len, tok, src, all_done, eos_fill,
                          int(num_beams), step=step, rec_offset=rec_offset, rec_tok=rec_tok,
                          rec_parent=rec_parent, rec_all_done=rec_all_done)


REORDER_FIELDS = 6


def reorder_table(buffers: Sequence[torch.Tensor], row0: Sequence[int],
                  counter_index: Sequence[int]) -> torch.Tensor:
    """The (nbuf, 6) int64 descriptor table ``beam_reorder`` reads, on the host:
    base pointer, capacity, units per row, unit bytes, start row, index of the
    buffer's length counter. A (batch, capacity, C) buffer whose rows are a
    multiple of 16 bytes moves in 16-byte units; any other (a ragged C) moves
    in 2-byte units, so no unit ever straddles the end of a row."""
    rows = []
    for buf, r0, ci in zip(buffers, row0, counter_index):
        if buf.dim() != 3 or not buf.is_contiguous() or buf.element_size() not in (2, 4):
            raise ValueError("beam_reorder takes contiguous (batch, capacity, C) buffers of "
                             "2- or 4-byte elements")
        row_bytes = buf.shape[2] * buf.element_size()
        unit = 16 if row_bytes % 16 == 0 and buf.data_ptr() % 16 == 0 else 2
        rows.append([buf.data_ptr(), buf.shape[1], row_bytes // unit, unit, int(r0), int(ci)])
    return torch.tensor(rows, dtype=torch.long).reshape(-1, REORDER_FIELDS)


def beam_reorder(table: torch.Tensor, counters: torch.Tensor, src: torch.Tensor, num_beams: int,
                 batch: Optional[int] = None, buffers: Optional[Sequence[torch.Tensor]] = None):
    """Launch the in-place reorder. ``buffers`` (the tensors the table was built
    from) lets the call check that ``src`` covers exactly their batch."""
    if buffers is not None:
        for buf in buffers:
            if buf.shape[0] != src.numel():
                raise ValueError("beam_reorder: src must have one entry per buffer row")
    hip.ext().beam_reorder(table, counters, src, int(num_beams))


def reorder_reference(buffers: Sequence[torch.Tensor], src: torch.Tensor, num_beams: int):
    """Whole-buffer ``index_select`` by the per-group source beams, in place."""
    B = src.numel()
    rows = src.long() + (torch.arange(B, device=src.device) // num_beams) * num_beams
    for buf in buffers:
        buf.copy_(buf.index_select(0, rows))


def backtrack(rec_tok: torch.Tensor, rec_parent: torch.Tensor, num_beams: int,
              steps: int) -> torch.Tensor:
    """(B, steps) token histories of the current beams from the per-step
    (token, parent) records, rows 0..steps-1: one pass, newest to oldest."""
    B = rec_tok.shape[1]
    base = (torch.arange(B, device=rec_tok.device) // num_beams) * num_beams
    idx = torch.arange(B, device=rec_tok.device)
    cols = []
    for t in range(steps - 1, -1, -1):
        cols.append(rec_tok[t].index_select(0, idx))
        idx = base + rec_parent[t].index_select(0, idx).long()
    return torch.stack(cols[::-1], dim=1)
