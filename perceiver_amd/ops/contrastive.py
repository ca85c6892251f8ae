"""Contrastive search steps for the graphed decode path.

On the GPU one step is three launches (ops/csrc/contrastive.hip):
``contrastive_sim`` sweeps each group's k candidate hidden states over its
history, ``contrastive_commit`` scores, selects, records, appends to the history
and proposes the next candidates, ``contrastive_copy`` spreads the winner's new
KV row over its group. ``contrastive_reference`` and ``propose_reference`` state
the rules in plain torch; they are the step off the GPU and under the lever, and
what the kernels are tested against. Per prompt ("group") g there are k
candidate rows ``g*k .. g*k+k-1``:

- proposal, from one fp32 logit row ``x``: the k largest tokens ordered by (raw
  logit descending, index ascending), NaN largest; ``p_j = exp(x_j - max) /
  sum(exp(x - max))`` in fp32, the probabilities of the full softmax;
- similarity: ``r = 1 / max(||float(h)||_2, 1e-12)`` and ``sim_j = max over
  t < hist_len of dot(hist_t, h_j) * r_t * r_j`` with an fp32 dot; NaN
  propagates as in ``amax``. An empty history gives 0 (the one deviation from
  ``amax``; the decoder never produces it);
- score: ``(1 - a) * p_j - a * sim_j`` in fp32, ``sel`` the argmax, lowest j on
  ties, NaN largest;
- commit: the emitted token is candidate ``sel``, or the fill id for a group
  that is already done; ``done |= emitted == eos``. Row ``sel``'s hidden state
  and reciprocal norm join the history at ``hist_len``, its logits feed the next
  proposal and its freshly appended KV row is copied to the group's other rows.

``PERCEIVER_CONTRASTIVE_GRAPH=0`` forces the torch composition and sends
``generate()`` back to the host loop (A/B lever).
"""
from __future__ import annotations

import os
from typing import Optional, Sequence, Tuple

import torch

from perceiver_amd.ops import hip

MIN_K, MAX_K, MAX_VOCAB, MAX_CHANNELS = 2, 8, 32768, 4088
EPS = 1e-12


def kernel_enabled() -> bool:
    return os.environ.get("PERCEIVER_CONTRASTIVE_GRAPH", "1") != "0"


def in_range(vocab: int, k: int, channels: int) -> bool:
    """The range the kernels take (host-side twin of ``contrastive_applicable``)."""
    k, vocab, channels = int(k), int(vocab), int(channels)
    return (MIN_K <= k <= MAX_K and k <= vocab <= MAX_VOCAB
            and 8 <= channels <= MAX_CHANNELS and channels % 8 == 0)


def kernel_applicable(device: torch.device, vocab: int, k: int, channels: int,
                      dtype: torch.dtype = torch.bfloat16) -> bool:
    """Whether a contrastive ``GraphedDecoder`` on ``device`` runs the HIP kernels."""
    return (device.type == "cuda" and dtype == torch.bfloat16 and kernel_enabled()
            and in_range(vocab, k, channels) and hip.is_available()
            and bool(hip.ext().contrastive_applicable(int(vocab), int(k), int(channels))))


def recip_norm(h: torch.Tensor, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``1 / max(||h||_2, 1e-12)`` over the last dim, in ``dtype``."""
    return 1.0 / h.to(dtype).norm(dim=-1).clamp_min(EPS)


def propose_reference(logits: torch.Tensor, k: int,
                      dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k candidates of every (rows, V) logit row: ``(tok, prob)``, both (rows, k)."""
    x = logits.float()
    # stable: among equal logits the lowest token comes first; NaN sorts largest
    tok = x.sort(dim=-1, descending=True, stable=True).indices[:, :int(k)]
    xd = x.to(dtype)
    e = (xd - xd.max(-1, keepdim=True).values).exp()
    return tok, e.gather(1, tok) / e.sum(-1, keepdim=True)


def sim_reference(h: torch.Tensor, hist: torch.Tensor, rnorm: torch.Tensor, hist_len, k: int,
                  dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(G, k) max cosine of every candidate against rows ``[0, hist_len)`` of its
    group's history. ``h`` (G * k, C), ``hist`` (G, cap, C), ``rnorm`` (G, cap);
    ``hist_len`` is an int or a one-element tensor, clamped into [0, cap]."""
    G, cap, C = hist.shape
    n = torch.as_tensor(hist_len, device=hist.device).reshape(()).clamp(0, cap)
    hc = h.to(dtype).view(G, int(k), C)
    dots = torch.einsum("gtc,gkc->gkt", hist.to(dtype), hc)
    cos = dots * rnorm.to(dtype)[:, None, :] * recip_norm(h, dtype).view(G, int(k), 1)
    live = torch.arange(cap, device=hist.device) < n
    sim = cos.masked_fill(~live, float("-inf")).amax(-1)
    return torch.where(n > 0, sim, torch.zeros_like(sim))


def contrastive_reference(h: torch.Tensor, hist: torch.Tensor, rnorm: torch.Tensor, hist_len,
                          tok: torch.Tensor, prob: torch.Tensor, done: torch.Tensor, alpha,
                          eos, fill, k: int, dtype: torch.dtype = torch.float32):
    """One contrastive step by the module's rules, out of place.

    ``h`` (G * k, C) candidate hidden states; ``tok`` / ``prob`` (G * k,) the
    candidates they belong to; ``done`` (G,); ``alpha`` / ``eos`` / ``fill`` are
    numbers or 0-dim tensors (``eos < 0``: none). Returns ``(sel, emitted,
    done', sim, score)`` with ``sel`` / ``emitted`` / ``done'`` (G,) and ``sim`` /
    ``score`` (G, k). ``dtype=torch.float64`` evaluates the same rules in fp64."""
    G, k = hist.shape[0], int(k)
    sim = sim_reference(h, hist, rnorm, hist_len, k, dtype)
    a = torch.as_tensor(alpha, device=h.device).to(dtype)
    score = (1.0 - a) * prob.to(dtype).view(G, k) - a * sim
    # stable: lowest j among equal scores; NaN sorts largest
    sel = score.sort(dim=-1, descending=True, stable=True).indices[:, 0]
    eos_t = torch.as_tensor(eos, device=h.device).long()
    fill_t = torch.as_tensor(fill, device=h.device).long()
    emitted = torch.where(done, fill_t, tok.view(G, k).gather(1, sel[:, None]).squeeze(1))
    return sel, emitted, done | (emitted == eos_t), sim, score


def copy_reference(buffers: Sequence[torch.Tensor], rows: Sequence[torch.Tensor],
                   sel: torch.Tensor, k: int):
    """Row ``rows[i]`` (a one-element index tensor) of every group's row ``sel``
    goes to the group's other rows, in every (batch, capacity, C) buffer."""
    for buf, r in zip(buffers, rows):
        v = buf.view(-1, int(k), *buf.shape[1:])
        new = v.index_select(2, r)  # (G, k, 1, C)
        win = new.gather(1, sel.view(-1, 1, 1, 1).expand(-1, 1, 1, new.shape[-1]))
        v.index_copy_(2, r, win.expand_as(new).contiguous())


# ------------------------------------------------------------------- launches

def plan(groups: int, cap: int, channels: int) -> Tuple[int, int]:
    """(nsplit, row granule) of ``contrastive_sim``'s grid: pure host."""
    return tuple(int(v) for v in hip.ext().contrastive_plan(int(groups), int(cap), int(channels)))


def contrastive_sim(h: torch.Tensor, hist: torch.Tensor, rnorm: torch.Tensor,
                    hist_len: torch.Tensor, k: int) -> torch.Tensor:
    """Launch the sweep: (nsplit, G, 8) fp32 partial maxima of ``dot * r_t``,
    slots ``0 .. k-1`` written, -inf for a slice without rows."""
    return hip.ext().contrastive_sim(h, hist, rnorm, hist_len, int(k))


def propose_step(logits: torch.Tensor, tok: torch.Tensor, prob: torch.Tensor, k: int):
    """Launch the proposal alone: ``tok`` (int64) / ``prob`` (fp32), both
    (G * k,), take the k candidates of row 0 of every group of ``logits``."""
    hip.ext().contrastive_commit(logits, tok, prob, int(k))


def commit_step(logits: torch.Tensor, tok: torch.Tensor, prob: torch.Tensor, k: int, *,
                h: torch.Tensor, part: torch.Tensor, hist: torch.Tensor, rnorm: torch.Tensor,
                hist_len: torch.Tensor, done: torch.Tensor, src: torch.Tensor,
                alpha: torch.Tensor, eos_fill: torch.Tensor,
                step: Optional[torch.Tensor] = None, rec: Optional[torch.Tensor] = None,
                sim_out: Optional[torch.Tensor] = None,
                score_out: Optional[torch.Tensor] = None):
    """Launch one commit in place: ``done`` (G,) bool, ``src`` (G * k,) int32 (the
    selected row, for the copy), row ``step`` of ``rec`` (rows, G) int64 takes
    the emitted tokens, ``hist`` / ``rnorm`` take row ``sel`` at ``hist_len``,
    ``tok`` / ``prob`` the next candidates. ``alpha`` is one fp32, ``eos_fill``
    the int64 pair, ``hist_len`` / ``step`` one int64 each, all on the device.
    ``sim_out`` / ``score_out`` (G * k,) fp32 receive the step's similarities
    and scores."""
    hip.ext().contrastive_commit(logits, tok, prob, int(k), h=h, part=part, hist=hist,
                                 rnorm=rnorm, hist_len=hist_len, done=done, src=src, alpha=alpha,
                                 eos_fill=eos_fill, step=step, rec=rec, sim_out=sim_out,
                                 score_out=score_out)


def contrastive_copy(table: torch.Tensor, counters: torch.Tensor, src: torch.Tensor, k: int,
                     buffers: Sequence[torch.Tensor]):
    """Launch the row copy over the buffers of ``table`` (``ops/beam.py::reorder_table``).
    ``buffers`` are the tensors the table was built from: the kernel's grid
    follows ``src``, so the call checks that ``src`` covers exactly their batch."""
    if len(buffers) != table.shape[0]:
        raise ValueError("contrastive_copy: one buffer per table row")
    for buf in buffers:
        if buf.shape[0] != src.numel():
            raise ValueError("contrastive_copy: src must have one entry per buffer row")
    hip.ext().contrastive_copy(table, counters, src, int(k))
