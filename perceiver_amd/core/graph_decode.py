"""hipGraph-captured single-token decode for Perceiver-AR.

Small-batch decode is kernel-launch-bound: one cached token step of the flagship
(1 CA + 12 SA layers) issues ~150 small kernels whose launch latency dwarfs their
execution. This module re-expresses the cached decode step of
``CausalSequenceModel`` with every dynamic quantity in a device buffer — cache
lengths, write indices, the query position, the sampled token — so the whole step
(embed → CA → SA stack → logits → argmax → cache/length update) can be captured
once into a hipGraph and replayed per token with a single launch.

Design (vs. the host-driven path in ``PerceiverAR.forward``):

- KV caches read at FULL capacity every step; a per-step pad mask
  ``arange(capacity) > len`` masks the dead tail inside the flash kernel (same
  -inf fill as real padding). Lengths become device counters incremented
  in-graph; ``StaticKVCache.enable_graph_append`` switches the in-place append
  to ``index_copy_`` with the device index.
- Rotary tables are precomputed at full capacity (row i = absolute position i
  for the CA cache, ``prefix0 + i`` for the SA caches, both fixed for a given
  prefill). Only the query row is dynamic: it is regenerated each step from the
  device position counter through the model's own ``FrequencyPositionEncoding``,
  and for the self-attention stack written into the last row of the table
  (``right_align=True`` makes the 1-row query read exactly that row).
- Token selection (greedy, or temperature / top-k / top-p sampling), the EOS
  fill and ``done`` mask, the token round-trip and the output record at a
  device step counter are ONE launch of the ``decode_select`` kernel
  (``ops/sample.py``), which reads every sampling parameter per row from device
  buffers: one captured graph serves every sampling configuration, and
  ``set_sampling`` rewrites the buffers between requests without a recapture.
  The cache lengths, the step cursor and the draw index are views of one small
  tensor that a single ``add_`` advances after the kernel, so no block of the
  kernel races another on a counter. A decode of N tokens is N graph replays
  with zero host synchronisation.
- Beam search (``num_beams > 1``): the caches hold ``bsz * num_beams`` rows and
  the step ends with two launches instead of one, ``beam_select`` (per-group
  top-k of score + log-softmax, done / gen_len / token / parent bookkeeping)
  and ``beam_reorder`` (in-place permutation of the rows generated since the
  prefill in every KV buffer, through one device-resident descriptor table).
  The prompt rows of a group's beams are bit-identical copies of one prefill,
  so only the generated rows ever move. Each step records (token, parent);
  the histories are backtracked once, after the replays (``ops/beam.py``).
- Contrastive search (``contrastive_k=k``): the caches hold ``bsz * k`` rows,
  the k candidates of a prompt in consecutive rows, and the step ends with
  three launches (``ops/contrastive.py``): ``contrastive_sim`` (max cosine of
  the k candidate hidden states against the group's history, whose length is
  ``sa_len``), ``contrastive_commit`` (score, select, record, append to the
  history, propose the next k candidates) and ``contrastive_copy`` (the
  winner's freshly appended KV row goes to the group's other rows: O(1) rows
  per step). Invariant: at every step boundary the k rows of a group hold
  bit-identical cache rows ``[0, len)``, so no candidate ever needs a cache of
  its own. ``penalty_alpha``, EOS and fill ids are device buffers.
- Left-padded prompt batches (``ragged=True``): ``prefill`` takes an
  ``attention_mask`` whose rows are ``0…0 1…1`` and stores each row's pad count
  in the device buffer ``shift``. The step then states the live keys of every
  row as a ``KeyWindow`` of two device integers instead of a mask, keys
  ``shift[b] .. ca_len`` for the cross-attention and ``0 .. sa_len`` for the
  latent stack (which sees no pad mask on the host loop either), and the
  query position is ``ca_len - shift[b]``. On the GPU the attention is the
  ``decode_attn`` kernel (``ops/decode_attn.py``), which streams only those
  keys; no mask tensor is built. The windows read ``counters`` and ``shift``,
  so one captured graph serves every padding pattern of its batch size.

Which ``generate`` request replays a captured graph, and which cached decoder
serves it, is decided at the bottom of this module and nowhere else:
``graph_route`` is the one gate for token, beam, contrastive and left-padded requests
(``fits_graph``, ``left_padded`` and ``capacity_bucket`` are its pieces),
``decoder_for`` is the one lookup in the model's ``_graph_decoders`` and
``replay`` the one loop over ``decode``. ``models/hf_base.py`` only calls them.

The un-captured step (``_step``) runs eagerly on any device, which is what the
CPU numerics test compares against the host-driven cached forward. The reference
has no equivalent (its cached decode is host-driven Python per token,
reference modules.py:820-871); this is MI355X-native serving machinery.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional

import torch

from perceiver_amd.core.cache import StaticKVCache, allocate_kv_cache
from perceiver_amd.core.modules import MultiHeadAttention
from perceiver_amd.core.position import RotaryPositionEmbedding
from perceiver_amd.ops import beam as _beam
from perceiver_amd.ops import contrastive as _contrastive
from perceiver_amd.ops import sample as _sample
from perceiver_amd.ops.decode_attn import KeyWindow, decode_attn_applicable

_KEEP = object()  # set_sampling: leave this parameter as it is


class GraphedDecoder:
    """Owns the static buffers and the (optionally hipGraph-captured) decode step
    for a ``CausalSequenceModel``-family model driven with ``StaticKVCache``s.

    Usage::

        caches = allocate_kv_cache(model, batch, device=dev, dtype=dtype)
        gd = GraphedDecoder(model, caches)
        gd.prefill(prompt, prefix_len=prompt.shape[1] - 1)   # normal forward
        tokens = gd.decode(n)                                # n graph replays
    """

    def __init__(self, model, caches: List[StaticKVCache], use_graph: bool = True,
                 do_sample: bool = False, temperature: float = 1.0,
                 top_k: Optional[int] = None, top_p: Optional[float] = None,
                 eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None,
                 num_beams: int = 1, ragged: bool = False, contrastive_k: int = 0,
                 penalty_alpha: float = 0.6):
        """``ragged``: ``prefill`` accepts a left-padded ``attention_mask`` and the
        step attends per-row key windows (module docstring). Not with beams.
        ``num_beams > 1``: beam search. The caches' batch is ``bsz * num_beams``
        (beams of one prompt are consecutive rows), ``prefill`` takes the ``bsz``
        prompts, the sampling parameters are unused and ``best`` returns the
        winning hypotheses.
        ``contrastive_k > 0``: contrastive search over the top ``contrastive_k``
        tokens with degeneration penalty ``penalty_alpha``. The caches' batch is
        ``bsz * contrastive_k``, ``prefill`` takes the ``bsz`` prompts and returns
        the first (bsz, k) candidates, ``decode`` returns (bsz, n) committed
        tokens and ``finished`` is (bsz,). Not with ``ragged`` or beams. At every
        step boundary the k rows of a group hold bit-identical cache rows
        ``[0, len)``.
        ``do_sample``: in-graph ancestral sampling (temperature scaling,
        optional top-k and top-p truncation). On the GPU the selection is the
        ``decode_select`` kernel with a counter-hash draw keyed by a per-prefill
        seed and a device draw index, so replays draw fresh randomness with zero
        host round-trips; elsewhere it is the torch composition on torch's RNG.
        ``eos_token_id``: rows that emitted it keep emitting ``pad_token_id``
        (EOS itself when None) and are flagged in ``finished``."""
        if ragged and int(num_beams) > 1:
            raise ValueError("ragged=True with num_beams > 1: padded beam requests are not "
                             "supported by the graphed decoder")
        if int(contrastive_k) > 0 and (ragged or int(num_beams) > 1):
            raise ValueError("contrastive_k with ragged=True or num_beams > 1: contrastive "
                             "search runs unpadded and without beams on the graphed decoder")
        self.model = model
        self.caches = caches
        self.ragged = bool(ragged)
        p = next(model.parameters())
        self.device, self.dtype = p.device, p.dtype
        self.use_graph = use_graph and p.device.type == "cuda"
        self.batch = caches[0].k_buf.shape[0]
        self.ca_cap = caches[0].capacity
        self.sa_cap = caches[1].capacity if len(caches) > 1 else 0
        self.vocab = model.config.vocab_size
        # decided once: a captured graph holds whichever selection it was built with
        self.use_kernel = _sample.kernel_applicable(self.device, self.vocab)

        # full-capacity reads include not-yet-written rows: they are masked, but
        # 0-prob × garbage-NaN would still poison P@V — keep the tails finite
        for c in caches:
            c.k_buf.zero_()
            c.v_buf.zero_()

        dev = self.device
        self.tok = torch.zeros(self.batch, 1, dtype=torch.long, device=dev)
        # device counters, views of ONE tensor so a single add_ advances them:
        # current cache lengths (= index the next token is written at), the
        # output-record cursor and the sampler's draw index
        self.counters = torch.zeros(4, dtype=torch.long, device=dev)
        self.ca_len = self.counters[0:1]
        self.sa_len = self.counters[1:2]
        self.step_idx = self.counters[2:3]
        self.draw_idx = self.counters[3:4]
        self.ar_ca = torch.arange(self.ca_cap, device=dev).unsqueeze(0)
        self.ar_sa = torch.arange(self.sa_cap, device=dev).unsqueeze(0)
        self.out_buf = torch.zeros(self.batch, self.sa_cap or self.ca_cap,
                                   dtype=torch.long, device=dev)
        # ragged: pad count of every row, rewritten by each prefill
        self.shift = torch.zeros(self.batch, dtype=torch.long, device=dev)
        # sampling parameters, per row, read by the kernel every step
        self.p_do_sample = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.p_temperature = torch.ones(self.batch, dtype=torch.float32, device=dev)
        self.p_top_k = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.p_top_p = torch.ones(self.batch, dtype=torch.float32, device=dev)
        self.seed = torch.zeros(1, dtype=torch.long, device=dev)
        self.eos_fill = torch.tensor([-1, 0], dtype=torch.long, device=dev)
        self.done = torch.zeros(self.batch, dtype=torch.bool, device=dev)
        self._generator = None
        self._steps_host = 0
        self._graph = None
        self.num_beams = int(num_beams)
        if self.num_beams > 1:
            self._init_beams()
        self.contrastive_k = int(contrastive_k)
        if self.contrastive_k > 0:
            self._init_contrastive()
        self.do_sample, self.temperature, self.top_k, self.top_p = False, 1.0, None, None
        self.eos_token_id = self.pad_token_id = None
        self.penalty_alpha = float(penalty_alpha)
        self.set_sampling(do_sample=do_sample, temperature=temperature, top_k=top_k,
                          top_p=top_p, eos_token_id=eos_token_id, pad_token_id=pad_token_id)

    # -------------------------------------------------------------------- beams

    def _init_beams(self):
        nb, B, dev = self.num_beams, self.batch, self.device
        if not _beam.in_range(self.vocab, nb):
            raise ValueError(f"num_beams={nb} / vocabulary {self.vocab} outside the beam "
                             f"decoder's range")
        if B % nb:
            raise ValueError(f"cache batch {B} is not a multiple of num_beams={nb}")
        self.groups = B // nb
        # decided once, like use_kernel: a captured graph holds whichever step it was built with
        self.use_beam_kernel = _beam.kernel_applicable(dev, self.vocab, nb)
        self.beam_scores = torch.zeros(B, dtype=torch.float32, device=dev)
        self.gen_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.beam_src = torch.zeros(B, dtype=torch.int32, device=dev)
        self.group_done = torch.zeros(self.groups, dtype=torch.bool, device=dev)
        # per-step record, row r = the r'th generated token (0: from the prefill logits)
        rows = (self.sa_cap or self.ca_cap) + 1
        self.rec_tok = torch.zeros(rows, B, dtype=torch.long, device=dev)
        self.rec_parent = torch.zeros(rows, B, dtype=torch.int32, device=dev)
        self.rec_all_done = torch.zeros(rows, self.groups, dtype=torch.bool, device=dev)
        self._reorder_bufs = [b for c in self.caches for b in (c.k_buf, c.v_buf)]
        # length counter of each buffer: counters[0] (CA) or counters[1] (SA)
        self._reorder_counter = [0 if i == 0 else 1 for i, c in enumerate(self.caches)
                                 for _ in range(2)]
        self.reorder_table = None
        if self.use_beam_kernel:
            self.reorder_table = _beam.reorder_table(
                self._reorder_bufs, [0] * len(self._reorder_bufs), self._reorder_counter).to(dev)

    def _beam_select_into_tok(self, logits: torch.Tensor, rec_offset: int):
        """One beam step from (batch, vocab) logits: scores, done, gen_len, tok,
        src and the record row ``step_idx + rec_offset``. One launch on the GPU."""
        nb = self.num_beams
        if self.use_beam_kernel:
            _beam.beam_select_step(
                logits, self.beam_scores, self.done, self.gen_len, self.tok.view(-1),
                self.beam_src, self.group_done, self.eos_fill, nb, step=self.step_idx,
                rec_offset=rec_offset, rec_tok=self.rec_tok, rec_parent=self.rec_parent,
                rec_all_done=self.rec_all_done)
            return
        src, tok, score, done, gen_len, all_done = _beam.beam_select_reference(
            logits, self.beam_scores, self.done, self.gen_len, nb, self.eos_fill[0],
            self.eos_fill[1])
        self.beam_src.copy_(src)
        self.tok.copy_(tok[:, None])
        self.beam_scores.copy_(score)
        self.done.copy_(done)
        self.gen_len.copy_(gen_len)
        self.group_done.copy_(all_done)
        cur = self.step_idx + rec_offset
        self.rec_tok.index_copy_(0, cur, tok[None])
        self.rec_parent.index_copy_(0, cur, src[None])
        self.rec_all_done.index_copy_(0, cur, all_done[None])

    def _beam_reorder(self):
        if self.use_beam_kernel:
            _beam.beam_reorder(self.reorder_table, self.counters, self.beam_src, self.num_beams)
        else:
            _beam.reorder_reference(self._reorder_bufs, self.beam_src, self.num_beams)

    def hypotheses(self) -> torch.Tensor:
        """(batch, 1 + steps) tokens of every current beam since the prefill."""
        return _beam.backtrack(self.rec_tok, self.rec_parent, self.num_beams,
                               self._steps_host + 1)

    def best(self, length_penalty: float = 1.0):
        """Per prompt the hypothesis with the largest
        ``score / clamp(gen_len, 1) ** length_penalty``: ``(tokens, scores)`` of
        shapes (bsz, 1 + steps) and (bsz,). The tokens are cut after the first
        step at which every beam of every prompt was done, where the host loop
        stops."""
        nb = self.num_beams
        norm = self.gen_len.view(-1, nb).float().clamp(min=1.0) ** length_penalty
        scores = self.beam_scores.view(-1, nb)
        pick = (scores / norm).argmax(dim=-1)
        rows = pick + torch.arange(self.groups, device=self.device) * nb
        toks = self.hypotheses().index_select(0, rows)
        stop = self.rec_all_done[:self._steps_host + 1].all(dim=1)
        if bool(stop.any()):
            toks = toks[:, :int(stop.int().argmax()) + 1]
        return toks, scores.gather(1, pick[:, None]).squeeze(1)

    # -------------------------------------------------------------- contrastive

    def _init_contrastive(self):
        k, B, dev = self.contrastive_k, self.batch, self.device
        if not (_contrastive.MIN_K <= k <= _contrastive.MAX_K and k <= self.vocab):
            raise ValueError(f"contrastive_k={k} / vocabulary {self.vocab} outside the "
                             f"contrastive decoder's range")
        if B % k:
            raise ValueError(f"cache batch {B} is not a multiple of contrastive_k={k}")
        self.groups = B // k
        C = self.model.config.num_channels
        # decided once, like use_kernel: a captured graph holds whichever step it was built with
        self.use_contrastive_kernel = _contrastive.kernel_applicable(dev, self.vocab, k, C,
                                                                     self.dtype)
        # the history: bit copies of the hidden states the model produced (the
        # prompt's latent positions, then one row per committed step) and their
        # reciprocal norms; its length is sa_len
        rows = self.sa_cap or self.ca_cap
        self.hist = torch.zeros(self.groups, rows, C, dtype=self.dtype, device=dev)
        self.hist_rnorm = torch.zeros(self.groups, rows, dtype=torch.float32, device=dev)
        self.cand_prob = torch.zeros(B, dtype=torch.float32, device=dev)
        self.cand_src = torch.zeros(B, dtype=torch.int32, device=dev)
        self.alpha = torch.zeros(1, dtype=torch.float32, device=dev)
        self.done = torch.zeros(self.groups, dtype=torch.bool, device=dev)
        # row r: the token committed by step r; the last step's similarities and scores
        self.rec_tok = torch.zeros(rows + 1, self.groups, dtype=torch.long, device=dev)
        self.last_sim = torch.zeros(B, dtype=torch.float32, device=dev)
        self.last_score = torch.zeros(B, dtype=torch.float32, device=dev)
        self._reorder_bufs = [b for c in self.caches for b in (c.k_buf, c.v_buf)]
        self._reorder_counter = [0 if i == 0 else 1 for i, c in enumerate(self.caches)
                                 for _ in range(2)]
        self.reorder_table = None
        if self.use_contrastive_kernel:
            self.reorder_table = _beam.reorder_table(
                self._reorder_bufs, [0] * len(self._reorder_bufs), self._reorder_counter).to(dev)

    def _prefill_contrastive(self, prompt: torch.Tensor, prefix_len: int) -> torch.Tensor:
        """The contrastive middle of ``prefill``: the ``bsz`` prompts run replicated,
        then row 0's cache rows and logits are broadcast over its group (as
        ``_prefill_beams`` does, for the same reason) and the history is filled
        from row 0's latent hidden states. Returns the (batch, vocab) logits."""
        k, G = self.contrastive_k, self.groups
        if prompt.shape[0] != G:
            raise ValueError(f"contrastive prefill takes {G} prompts, got {prompt.shape[0]}")
        n0, n_sa = prompt.shape[1], prompt.shape[1] - prefix_len
        out = self.model(prompt.repeat_interleave(k, dim=0), prefix_len=prefix_len,
                         kv_cache=self.caches)
        for i, c in enumerate(self.caches):
            n = n0 if i == 0 else n_sa
            for buf in (c.k_buf, c.v_buf):
                v = buf.view(G, k, *buf.shape[1:])
                v[:, 1:, :n].copy_(v[:, :1, :n].expand(-1, k - 1, -1, -1))
        hs = out.last_hidden_state.reshape(G, k, n_sa, -1)[:, 0]
        self.hist[:, :n_sa].copy_(hs)
        self.hist_rnorm[:, :n_sa].copy_(_contrastive.recip_norm(hs))
        logits = out.logits[:, -1, :]
        logits = logits.view(G, k, -1)[:, :1].expand(-1, k, -1).reshape(G * k, -1)
        self.last_logits = logits[:, None, :]
        return logits

    def _propose_into_tok(self, logits: torch.Tensor):
        """tok, cand_prob <- the k candidates of row 0 of every group of the
        (batch, vocab) logits. One launch on the GPU."""
        k = self.contrastive_k
        if self.use_contrastive_kernel:
            _contrastive.propose_step(logits, self.tok.view(-1), self.cand_prob, k)
            return
        tok, prob = _contrastive.propose_reference(logits.view(self.groups, k, -1)[:, 0], k)
        self.tok.copy_(tok.reshape(-1, 1))
        self.cand_prob.copy_(prob.reshape(-1))

    def _contrastive_commit(self, h: torch.Tensor, logits: torch.Tensor):
        """One contrastive step from the (batch, C) candidate hidden states and
        their (batch, vocab) logits: record row ``step_idx``, done, the history
        row ``sa_len``, the next candidates and the copy of the winner's new KV
        row over its group. Three launches on the GPU."""
        k, G = self.contrastive_k, self.groups
        if self.use_contrastive_kernel:
            part = _contrastive.contrastive_sim(h, self.hist, self.hist_rnorm, self.sa_len, k)
            _contrastive.commit_step(
                logits, self.tok.view(-1), self.cand_prob, k, h=h, part=part, hist=self.hist,
                rnorm=self.hist_rnorm, hist_len=self.sa_len, done=self.done, src=self.cand_src,
                alpha=self.alpha, eos_fill=self.eos_fill, step=self.step_idx, rec=self.rec_tok,
                sim_out=self.last_sim, score_out=self.last_score)
            _contrastive.contrastive_copy(self.reorder_table, self.counters, self.cand_src, k,
                                          buffers=self._reorder_bufs)
            return
        sel, emitted, done, sim, score = _contrastive.contrastive_reference(
            h, self.hist, self.hist_rnorm, self.sa_len, self.tok.view(-1), self.cand_prob,
            self.done, self.alpha[0], self.eos_fill[0], self.eos_fill[1], k)
        rows = sel + torch.arange(G, device=self.device) * k
        self.rec_tok.index_copy_(0, self.step_idx, emitted[None])
        self.done.copy_(done)
        self.cand_src.copy_(sel.repeat_interleave(k))
        self.last_sim.copy_(sim.reshape(-1))
        self.last_score.copy_(score.reshape(-1))
        won = h.index_select(0, rows)
        at = self.sa_len.clamp(max=self.hist.shape[1] - 1)
        self.hist.index_copy_(1, at, won[:, None].to(self.hist.dtype))
        self.hist_rnorm.index_copy_(1, at, _contrastive.recip_norm(won)[:, None])
        tok, prob = _contrastive.propose_reference(logits.index_select(0, rows), k)
        self.tok.copy_(tok.reshape(-1, 1))
        self.cand_prob.copy_(prob.reshape(-1))
        _contrastive.copy_reference(
            self._reorder_bufs, [self.counters[ci:ci + 1] for ci in self._reorder_counter], sel, k)

    # ----------------------------------------------------------------- sampling

    def set_sampling(self, do_sample=_KEEP, temperature=_KEEP, top_k=_KEEP, top_p=_KEEP,
                     eos_token_id=_KEEP, pad_token_id=_KEEP, penalty_alpha=_KEEP):
        """Rewrite the sampling parameters between requests. ``do_sample``,
        ``temperature``, ``top_k`` and ``top_p`` take scalars or per-row
        ``(batch,)`` tensors; None switches top-k / top-p / EOS off. With the
        kernel the captured graph is reused as it is. The torch composition
        bakes the values into the graph, so there a change drops the graph and
        the next ``decode`` captures again. ``penalty_alpha`` (a contrastive
        decoder's) is a device buffer in both forms, like EOS and fill."""
        if penalty_alpha is not _KEEP:
            self.penalty_alpha = float(penalty_alpha)
        if self.contrastive_k:
            self.alpha.fill_(self.penalty_alpha)
        if do_sample is not _KEEP:
            self.do_sample = do_sample
        if temperature is not _KEEP:
            self.temperature = temperature
        if top_k is not _KEEP:
            self.top_k = top_k
        if top_p is not _KEEP:
            self.top_p = top_p
        if eos_token_id is not _KEEP:
            self.eos_token_id = eos_token_id
        if pad_token_id is not _KEEP:
            self.pad_token_id = pad_token_id
        for name, v in (("eos_token_id", self.eos_token_id), ("pad_token_id", self.pad_token_id)):
            if v is not None and not 0 <= int(v) < self.vocab:
                raise ValueError(f"{name}={v} outside the vocabulary [0, {self.vocab})")

        B, dev = self.batch, self.device
        self.p_do_sample.copy_(_sample.row_param(self.do_sample, B, torch.int32, dev, 0))
        self.p_temperature.copy_(_sample.row_param(self.temperature, B, torch.float32, dev, 1.0))
        self.p_top_k.copy_(_sample.row_param(self.top_k, B, torch.int32, dev, 0))
        self.p_top_p.copy_(_sample.row_param(self.top_p, B, torch.float32, dev, 1.0))
        eos = -1 if self.eos_token_id is None else int(self.eos_token_id)
        fill = self.pad_token_id if self.pad_token_id is not None else self.eos_token_id
        self._eos, self._fill = eos, 0 if fill is None else int(fill)
        self.eos_fill.copy_(torch.tensor([self._eos, self._fill], dtype=torch.long))
        ds = self.do_sample
        self._any_sample = bool(ds.any()) if isinstance(ds, torch.Tensor) else bool(ds)
        # the beam and the contrastive steps read eos_fill themselves
        if not self.use_kernel and self.num_beams == 1 and not self.contrastive_k:
            self._graph = None

    @property
    def finished(self) -> torch.Tensor:
        """(batch,) bool: rows that have emitted ``eos_token_id`` since the prefill
        ((bsz,) for a contrastive decoder: one flag per prompt)."""
        return self.done

    # ------------------------------------------------------------------ prefill

    @torch.no_grad()
    def prefill(self, prompt: torch.Tensor, prefix_len: int,
                generator: Optional[torch.Generator] = None,
                attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Run the normal host-driven cached forward over the prompt, seed the
        device counters/buffers, and return the first selected token (a
        contrastive decoder: the first (bsz, k) candidates).

        ``attention_mask`` (a ``ragged`` decoder only): (batch, n) with every row
        ``0…0 1…1`` and at least one 1, anything else raises ``ValueError``. The
        forward runs with ``pad_mask = ~attention_mask``, so positions are
        shifted and clamped as ``PerceiverAR.forward`` does.

        Sampling draws a fresh seed here, from ``generator`` when given and
        otherwise from torch's global generator, and restarts the draw index:
        equally seeded generators decode identical samples, and two prefills
        without one decode different samples."""
        for c in self.caches:
            c.disable_graph_append()
            c.reset()
            # store keys pre-rotated at their absolute positions: the decode
            # step then never touches cached rows again (no O(cache) re-rotate)
            c.pre_rotated = True
        n_ca, n_sa = prompt.shape[1], prompt.shape[1] - prefix_len
        pad_mask = self._left_pad_mask(prompt, attention_mask)
        if self.num_beams > 1:
            logits = self._prefill_beams(prompt, prefix_len)
        elif self.contrastive_k:
            logits = self._prefill_contrastive(prompt, prefix_len)
        else:
            logits = self.model(prompt, prefix_len=prefix_len, pad_mask=pad_mask,
                                kv_cache=self.caches).logits[:, -1, :]

        self.ca_len.fill_(n_ca)
        self.sa_len.fill_(n_sa)
        self.step_idx.fill_(0)
        self.draw_idx.fill_(0)
        self.done.zero_()
        if self.num_beams > 1:
            self._beam_select_into_tok(logits, rec_offset=0)
        elif self.contrastive_k:
            self._propose_into_tok(logits)
        else:
            self._generator = None if self.use_kernel else generator  # torch composition only
            if self.use_kernel:
                if self._any_sample:  # greedy draws nothing
                    gdev = generator.device if generator is not None else "cpu"
                    self.seed.fill_(int(torch.randint(0, 2 ** 62, (1,), generator=generator,
                                                      device=gdev).item()))
            elif generator is not None and self.use_graph and self._any_sample:
                raise RuntimeError("a generator on the captured-graph path needs the "
                                   "decode_select kernel (PERCEIVER_DECODE_SELECT=0 or an "
                                   "unsupported vocabulary)")
            self._select_into_tok(logits, record=False)
        self.draw_idx.fill_(1)

        self.ca_len_host = n_ca
        self.sa_len_host = n_sa
        self._steps_host = 0
        self.caches[0].enable_graph_append(self.ca_len)
        for c in self.caches[1:]:
            c.enable_graph_append(self.sa_len)
        if self.contrastive_k:
            return self.tok.view(self.groups, self.contrastive_k).clone()
        return self.tok.clone()

    def _left_pad_mask(self, prompt, attention_mask) -> Optional[torch.Tensor]:
        """Validate ``attention_mask``, store the pad counts in ``shift`` and
        return the forward's pad mask (None for a decoder that is not ragged)."""
        if not self.ragged:
            if attention_mask is not None and bool((attention_mask == 0).any()):
                raise ValueError("a padded attention_mask needs GraphedDecoder(ragged=True)")
            return None
        if attention_mask is None:
            self.shift.zero_()
            return torch.zeros(prompt.shape, dtype=torch.bool, device=prompt.device)
        live = attention_mask.to(prompt.device) != 0
        if live.shape != prompt.shape:
            raise ValueError(f"attention_mask has shape {tuple(live.shape)}, the prompt "
                             f"{tuple(prompt.shape)}")
        if not left_padded(live):
            raise ValueError("attention_mask must be left-padded (every row 0…0 1…1 with at "
                             "least one 1)")
        self.shift.copy_((~live).sum(dim=1))
        return ~live

    def _prefill_beams(self, prompt: torch.Tensor, prefix_len: int) -> torch.Tensor:
        """The beam middle of ``prefill``: the ``bsz`` prompts run replicated, then
        beam 0's cache rows and logits are broadcast over its group. A replicated
        batch through library GEMMs is not guaranteed bit-identical row to row,
        and reordering only the generated rows is exact only if the prompt rows
        are. Restarts the beam state and returns the (batch, vocab) logits."""
        nb, G = self.num_beams, self.groups
        if prompt.shape[0] != G:
            raise ValueError(f"beam prefill takes {G} prompts, got {prompt.shape[0]}")
        n0, prefix0 = prompt.shape[1], prefix_len
        out = self.model(prompt.repeat_interleave(nb, dim=0), prefix_len=prefix_len,
                         kv_cache=self.caches)
        for i, c in enumerate(self.caches):
            n = n0 if i == 0 else n0 - prefix0
            for buf in (c.k_buf, c.v_buf):
                v = buf.view(G, nb, *buf.shape[1:])
                v[:, 1:, :n].copy_(v[:, :1, :n].expand(-1, nb - 1, -1, -1))
        logits = out.logits[:, -1, :]
        logits = logits.view(G, nb, -1)[:, :1].expand(-1, nb, -1).reshape(G * nb, -1)
        self.last_logits = logits[:, None, :]

        self.gen_len.zero_()
        self.group_done.zero_()
        self.rec_all_done.zero_()
        start = torch.full((G, nb), -1e9, dtype=torch.float32)
        start[:, 0] = 0.0
        self.beam_scores.copy_(start.view(-1))
        if self.reorder_table is not None:
            # the rows a request generates start where its prompt ends
            row0 = torch.tensor([n0 if ci == 0 else n0 - prefix0
                                 for ci in self._reorder_counter], dtype=torch.long)
            self.reorder_table[:, 4].copy_(row0)
        return logits

    def _select_into_tok(self, logits: torch.Tensor, record: bool):
        """tok <- next token from (batch, vocab) logits, with the EOS fill and
        ``done`` update; ``record`` first stores the previous token at the step
        cursor of ``out_buf``. One kernel launch on the GPU."""
        if self.use_kernel:
            _sample.select_step(
                logits, self.p_do_sample, self.p_temperature, self.p_top_k, self.p_top_p,
                self.seed, self.draw_idx, tok=self.tok.view(-1),
                out_buf=self.out_buf if record else None,
                step=self.step_idx if record else None,
                done=self.done, eos_fill=self.eos_fill)
            return
        if record:
            self.out_buf.index_copy_(1, self.step_idx, self.tok)
        tok = self._select(logits.float())
        if self.eos_token_id is not None:
            tok = torch.where(self.done[:, None], torch.full_like(tok, self._fill), tok)
            self.done.logical_or_(tok.squeeze(-1) == self._eos)
        self.tok.copy_(tok)

    def _select(self, scores: torch.Tensor) -> torch.Tensor:
        """Greedy or Gumbel-max sampled token from (batch, vocab) fp32 scores:
        the torch composition, used off the GPU and as the A/B reference.
        Capture-safe: torch's CUDA Philox state is graph-aware, and the
        exponential_/log Gumbel trick avoids multinomial's sync."""
        greedy = scores.argmax(-1, keepdim=True)
        if not self._any_sample:
            return greedy
        T = _sample.row_param(self.temperature, self.batch, torch.float32, scores.device, 1.0)
        scaled = scores / T[:, None]
        if self.top_k is not None or self.top_p is not None:
            keep = _sample.keep_mask_reference(scores, T, self.top_k, self.top_p)
            scaled = scaled.masked_fill(~keep, float("-inf"))
        g = torch.empty_like(scaled).exponential_(generator=self._generator).log().neg_()
        drawn = (scaled + g).argmax(-1, keepdim=True)
        if isinstance(self.do_sample, torch.Tensor):
            return torch.where(self.p_do_sample[:, None] != 0, drawn, greedy)
        return drawn

    # --------------------------------------------------------------------- step

    def _step(self):
        """One single-token decode step, everything dynamic read from device
        buffers. Mirrors the cached branch of ``PerceiverAR.forward`` +
        ``CausalSequenceModel.forward`` (modules.py) with full-capacity masked
        attention instead of host-length views."""
        m = self.model
        if self.ragged:
            pos_q = (self.ca_len - self.shift).view(self.batch, 1)
        else:
            pos_q = self.ca_len.view(1, 1).expand(self.batch, 1)
        x, frq_q = m.input_adapter(self.tok, abs_pos=pos_q)

        # cross-attention: new token is the single latent; cached K/V at full
        # capacity, tail j > ca_len masked (the new token lands AT index ca_len).
        # Caches are pre-rotated, so BOTH rotary tables are just the current
        # position's row: q uses it directly, k uses it to rotate the new row
        # before it is appended.
        rot_now = RotaryPositionEmbedding(frq_q, right_align=True)
        if self.ragged:  # two device integers per row, no mask tensor
            ca_mask = KeyWindow(self.shift, self.ca_len)
        else:
            ca_mask = (self.ar_ca > self.ca_len).expand(self.batch, -1)
        ca_out = m.cross_attention(
            x,
            x_kv_prefix=x[:, :0],
            pad_mask=ca_mask,
            rot_pos_emb_q=rot_now,
            rot_pos_emb_k=rot_now,
            kv_cache=self.caches[0],
        )

        if self.ragged:
            sa_mask = KeyWindow(None, self.sa_len)
        else:
            sa_mask = (self.ar_sa > self.sa_len).expand(self.batch, -1)
        sa_out = m.self_attention(
            ca_out.last_hidden_state,
            pad_mask=sa_mask,
            rot_pos_emb=rot_now,
            kv_cache=list(self.caches[1:]),
        )

        h = sa_out.last_hidden_state
        if m.config.output_norm:
            h = m.out_norm(h)
        logits = m.output_adapter(h, txt_embedding=m.input_adapter.txt_embedding)

        # token selection + bookkeeping, all on-device: the graph is self-advancing
        self.last_logits = logits  # graph-pool tensor: valid until the next replay
        if self.num_beams > 1:
            self._beam_select_into_tok(logits[:, -1, :], rec_offset=1)
            self._beam_reorder()
        elif self.contrastive_k:
            self._contrastive_commit(h[:, -1, :], logits[:, -1, :])
        else:
            self._select_into_tok(logits[:, -1, :], record=True)
        self.counters.add_(1)  # cache lengths, step cursor and draw index together

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):  # allocator/dispatch warmup — real decode steps
                self._step()
                self.ca_len_host += 1
                self.sa_len_host += 1
        torch.cuda.current_stream().wait_stream(s)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self._step()

    @torch.no_grad()
    def decode(self, n: int, tokens: bool = True) -> Optional[torch.Tensor]:
        """Generate the next ``n`` tokens after ``prefill``; returns (batch, n)
        ((bsz, n) committed tokens for a contrastive decoder), or None with ``tokens=False`` (a beam caller that only wants ``best``
        spares the backtrack).
        May be called repeatedly after one prefill (``generate`` decodes in
        chunks to look at ``finished`` in between). The first call captures the
        step graph (2 warmup steps run eagerly and count toward ``n``); later
        calls are pure replays."""
        if n < 1:
            raise ValueError("decode() needs n >= 1")
        if self.ca_len_host + n > self.ca_cap or self.sa_len_host + n > self.sa_cap:
            raise RuntimeError("decode would overflow the KV cache capacity")
        done = 0
        if self.use_graph and self._graph is None:
            if n < 2:
                raise RuntimeError("first decode() call needs n >= 2 to capture")
            self._capture()
            done = 2
        for _ in range(n - done):
            if self.use_graph:
                self._graph.replay()
            else:
                self._step()
            self.ca_len_host += 1
            self.sa_len_host += 1
        # out_buf rows 0..n-1 hold the tokens EMITTED by each step's predecessor:
        # row i is the token fed INTO step i, i.e. the model's (i)'th generated
        # token counting the prefill argmax as the 0'th. Together with the final
        # self.tok this yields the n generated tokens after the prefill token.
        s0 = self._steps_host
        self._steps_host += n
        if not tokens:
            return None
        if self.num_beams > 1:
            # the current beams' last n tokens; a later step may still permute them
            return self.hypotheses()[:, s0 + 1:]
        if self.contrastive_k:
            return self.rec_tok[s0:s0 + n].t().contiguous()
        first = self.out_buf[:, s0 + 1:s0 + n]
        return torch.cat([first, self.tok], dim=1)


# ------------------------------------------------------------- request policy
# Which generate() request replays a captured graph, and which cached decoder
# serves it. ``model`` is the ``CausalSequenceModel`` backend throughout.

class GraphRoute(NamedTuple):
    """What ``graph_route`` grants a request."""

    batch: int    # rows of the decoder's caches (bsz * num_beams)
    bucket: int   # cross-attention cache capacity
    ragged: bool  # a left-padded request: GraphedDecoder(ragged=True)
    baked: bool   # torch selection: the sampling parameters are part of the graph


def left_padded(attention_mask: torch.Tensor) -> bool:
    """Whether every row of the (batch, n) mask is ``0…0 1…1`` with at least one
    1: the last position is live and no live position precedes a pad."""
    live = attention_mask != 0
    return bool(live[:, -1].all()) and bool((live[:, 1:] | ~live[:, :-1]).all())


def capacity_bucket(need: int, max_seq_len: int) -> int:
    """Cross-attention cache capacity for a request of ``need`` positions: the
    next power of two >= ``need`` (at least 2048), at most ``max_seq_len``. The
    graphed step reads the FULL (masked) cache every token, so the cache is
    sized to the request and not to the model (an 8192-context model would pay
    8192 dead rows for a 1k-token request)."""
    bucket = 2048
    while bucket < need:
        bucket *= 2
    return min(bucket, max_seq_len)


def fits_graph(model, seq_len: int, prefix_len: int, max_new_tokens: int,
               eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None) -> bool:
    """The shape half of ``graph_route``, the same for every mode: the capture
    takes 2 steps after the prefill token, every generated token stays within
    the latent-growth phase of the schedule (no prefix growth, no window
    slide), and EOS / pad ids lie inside the vocabulary, because the graphed
    step embeds the fill token where the host loop only writes it out."""
    vocab = model.config.vocab_size
    return (all(t is None or 0 <= t < vocab for t in (eos_token_id, pad_token_id))
            and max_new_tokens >= 3
            and (seq_len - prefix_len) + max_new_tokens <= model.max_latents
            and seq_len + max_new_tokens <= model.max_seq_len)


def graph_route(model, batch: int, seq_len: int, prefix_len: int, max_new_tokens: int,
                num_beams: int = 1, attention_mask: Optional[torch.Tensor] = None,
                eos_token_id: Optional[int] = None, pad_token_id: Optional[int] = None,
                top_p: Optional[float] = None,
                generator: Optional[torch.Generator] = None,
                contrastive_k: int = 0) -> Optional[GraphRoute]:
    """THE gate of the captured-graph decode path: the route of a ``generate``
    request, or None for one that keeps the host loop.

    Every mode needs a GPU model and ``fits_graph``. On top of that:

    - tokens (``num_beams == 1``): with the ``decode_select`` kernel every
      sampling configuration replays one graph. Without it
      (PERCEIVER_DECODE_SELECT=0, or a vocabulary it has no tier for) the torch
      selection bakes ``do_sample`` / ``temperature`` / ``top_k`` into the
      graph, and top-p, EOS and generator requests are refused.
    - a mask that holds zeros: only left-padded, with the select kernel and
      head dims that ``decode_attn`` takes in every attention layer. The
      decoder is ragged then; unpadded requests keep a decoder of their own.
    - beams: the beam kernels must apply (``2 <= num_beams <= 8``) and the mask
      must hold no zero.
    - contrastive search (``contrastive_k > 0``; ``generate`` sends only
      requests that do not sample): no zero in the mask, and the contrastive kernels must apply (``2 <= k <= 8``, bf16
      hidden states of a multiple of 8 channels, PERCEIVER_CONTRASTIVE_GRAPH
      not 0). The route's batch is ``batch * k``."""
    p = next(model.parameters())
    if p.device.type != "cuda" or not fits_graph(model, seq_len, prefix_len, max_new_tokens,
                                                 eos_token_id, pad_token_id):
        return None
    vocab = model.config.vocab_size
    padded = attention_mask is not None and bool((attention_mask == 0).any())
    bucket = capacity_bucket(seq_len + max_new_tokens, model.max_seq_len)
    if num_beams > 1:
        if padded or not _beam.kernel_applicable(p.device, vocab, num_beams):
            return None
        return GraphRoute(batch * num_beams, bucket, ragged=False, baked=False)
    if contrastive_k > 0:
        if padded or not _contrastive.kernel_applicable(
                p.device, vocab, contrastive_k, model.config.num_channels, p.dtype):
            return None
        return GraphRoute(batch * contrastive_k, bucket, ragged=False, baked=False)
    select_kernel = _sample.kernel_applicable(p.device, vocab)
    if not select_kernel and not (eos_token_id is None and top_p is None and generator is None):
        return None
    if padded and not (
            select_kernel
            and all(decode_attn_applicable(m.num_qk_channels // m.num_heads,
                                           m.num_v_channels // m.num_heads)
                    for m in model.modules() if isinstance(m, MultiHeadAttention))
            and left_padded(attention_mask)):
        return None
    return GraphRoute(batch, bucket, ragged=padded, baked=not select_kernel)


def decoder_for(owner, model, route: GraphRoute, num_beams: int = 1, do_sample=False,
                temperature=1.0, top_k=None, make=GraphedDecoder,
                contrastive_k: int = 0) -> GraphedDecoder:
    """The decoder (captured graph + caches) that serves ``route``, kept in the
    plain dict ``owner._graph_decoders``: repeated requests only pay prefill +
    replays. At most two are held, token and beam decoders alike, and the
    oldest goes first, which bounds the cache memory. ``make`` is
    ``GraphedDecoder`` except in tests. A contrastive request keys on its k
    (``penalty_alpha`` is a device buffer and no key).

    ``p.data_ptr()`` pins a cached graph to the current parameter storage:
    ``model.to(device/dtype)`` reallocates it, and a graph replaying against the
    old pointers would silently use stale weights (an in-place
    ``load_state_dict`` is fine, the graph holds parameter pointers)."""
    p = next(model.parameters())
    key = (route.batch, route.bucket, p.device, p.dtype, p.data_ptr(), num_beams, route.ragged,
           contrastive_k)
    if route.baked:
        key += (do_sample, float(temperature), top_k)
    cache = getattr(owner, "_graph_decoders", None)
    if cache is None:
        cache = owner._graph_decoders = {}
    gd = cache.get(key)
    if gd is None:
        if len(cache) >= 2:
            cache.pop(next(iter(cache)))
        gd = cache[key] = make(
            model, allocate_kv_cache(model, route.batch, device=p.device, dtype=p.dtype,
                                     ca_capacity=route.bucket),
            do_sample=do_sample, temperature=temperature, top_k=top_k, num_beams=num_beams,
            ragged=route.ragged, **({"contrastive_k": contrastive_k} if contrastive_k else {}))
    return gd


def replay(gd: GraphedDecoder, n: int, eos_token_id: Optional[int] = None,
           tokens: bool = True) -> Optional[torch.Tensor]:
    """Decode up to ``n`` tokens after ``gd.prefill``. Without EOS that is one
    ``decode(n)`` with no host synchronisation. With EOS the replays run in
    chunks of 16 with one look at ``finished`` between them (one sync per 16
    tokens) and stop once every row is done; the caller cuts the result where
    the host loop would have stopped. Returns (rows, <= n) tokens, one row per
    entry of ``finished`` (the batch, or the prompts of a contrastive decoder),
    or None with ``tokens=False``."""
    if eos_token_id is None:
        return gd.decode(n, tokens=tokens)
    chunks = [gd.tok.new_empty((gd.finished.shape[0], 0))]
    while n > 0 and not bool(gd.finished.all()):
        c = min(16, n)
        chunks.append(gd.decode(c, tokens=tokens))
        n -= c
    return torch.cat(chunks, dim=1) if tokens else None
