"""🤗 integration base: PreTrainedModel wrapper for causal Perceiver-AR models with
the sliding latent/prefix generation schedule, plus weight-copy utilities mapping
``transformers`` Perceiver checkpoints onto this library's modules.

Parity: reference perceiver/model/core/huggingface.py:21-230. The generation loop is
implemented natively (transformers 5.x removed the legacy list-of-tuples cache path
its GenerationMixin integration relied on): ``generate`` supports greedy, temperature/
top-k/top-p sampling and the grow-latents -> grow-prefix -> slide-window schedule with
self/cross cache truncation, with cached and uncached paths producing identical
tokens (the reference's equality contract).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import torch
import torch.nn as nn
from transformers import PreTrainedModel
from transformers.modeling_outputs import CausalLMOutputWithPast

from perceiver_amd.core import (
    CrossAttentionLayer,
    MLP,
    MultiHeadAttention,
    PerceiverDecoder,
    PerceiverEncoder,
    SelfAttentionLayer,
)
from perceiver_amd.core import graph_decode as _graph
from perceiver_amd.core.cache import StaticKVCache, allocate_kv_cache, cache_len
from perceiver_amd.core.modules import KVCache


# ----------------------------------------------------------------- param copying
def copy_param(src: nn.Parameter, tgt: nn.Parameter):
    with torch.no_grad():
        tgt.copy_(src)


def copy_params(src: nn.Module, tgt: nn.Module):
    tgt.load_state_dict(src.state_dict())


def copy_attention_params(src, tgt: MultiHeadAttention):
    if hasattr(tgt, "qkv_proj"):
        # merged projection (self-attention layers): write the q/k/v slices
        qk = tgt.num_qk_channels
        with torch.no_grad():
            tgt.qkv_proj.weight[:qk].copy_(src.attention.self.query.weight)
            tgt.qkv_proj.weight[qk: 2 * qk].copy_(src.attention.self.key.weight)
            tgt.qkv_proj.weight[2 * qk:].copy_(src.attention.self.value.weight)
            if tgt.qkv_proj.bias is not None:
                tgt.qkv_proj.bias[:qk].copy_(src.attention.self.query.bias)
                tgt.qkv_proj.bias[qk: 2 * qk].copy_(src.attention.self.key.bias)
                tgt.qkv_proj.bias[2 * qk:].copy_(src.attention.self.value.bias)
    else:
        copy_params(src.attention.self.query, tgt.q_proj)
        copy_params(src.attention.self.key, tgt.k_proj)
        copy_params(src.attention.self.value, tgt.v_proj)
    copy_params(src.attention.output.dense, tgt.o_proj)


def copy_mlp_params(src, tgt: MLP):
    copy_params(src.layernorm, tgt[0])
    copy_params(src.mlp.dense1, tgt[1])
    copy_params(src.mlp.dense2, tgt[3])


def copy_cross_attention_layer_params(src, tgt: CrossAttentionLayer, query_residual: bool):
    att_tgt = tgt[0].module if query_residual else tgt[0]
    mlp_tgt = tgt[1].module
    copy_params(src.attention.self.layernorm1, att_tgt.q_norm)
    copy_params(src.attention.self.layernorm2, att_tgt.kv_norm)
    copy_attention_params(src, att_tgt.attention)
    copy_mlp_params(src, mlp_tgt)


def copy_self_attention_layer_params(src, tgt: SelfAttentionLayer):
    att_tgt = tgt[0].module
    mlp_tgt = tgt[1].module
    copy_params(src.attention.self.layernorm1, att_tgt.norm)
    copy_attention_params(src, att_tgt.attention)
    copy_mlp_params(src, mlp_tgt)


def copy_self_attention_block_params(src: Sequence, tgt: Sequence):
    assert len(src) == len(tgt)
    for src_layer, tgt_layer in zip(src, tgt):
        copy_self_attention_layer_params(src_layer, tgt_layer)


def copy_latent_provider_params(src, tgt: PerceiverEncoder):
    copy_param(src.embeddings.latents, tgt.latent_provider._query)


def copy_classification_decoder_params(src, tgt: PerceiverDecoder, query_residual=True):
    copy_cross_attention_layer_params(
        src.decoder.decoder.decoding_cross_attention, tgt.cross_attn, query_residual=query_residual
    )
    copy_params(src.decoder.decoder.final_layer, tgt.output_adapter.linear)
    copy_param(src.decoder.decoder.output_position_encodings.position_embeddings,
               tgt.output_query_provider._query)


# ----------------------------------------------------------------- causal base
@dataclass
class PerceiverCausalSequenceModelOutput(CausalLMOutputWithPast):
    prefix_len: Optional[int] = None


class PerceiverCausalSequenceModel(PreTrainedModel):
    """Wraps a CausalSequenceModel backend for 🤗 inference. Subclasses set
    ``self.backend_model`` in __init__."""

    @classmethod
    def can_generate(cls) -> bool:
        # transformers gates generation plumbing (pipeline assistant fields,
        # generation_config) on this; our generate() is native, not
        # GenerationMixin, so the base-class heuristic misses it
        return True

    def forward(
        self,
        input_ids: torch.LongTensor,
        prefix_len: int,
        attention_mask: Optional[torch.FloatTensor] = None,
        past_key_values: Optional[List[KVCache]] = None,
        use_cache: Optional[bool] = None,
        labels: Optional[torch.LongTensor] = None,
        **kwargs: Any,
    ):
        if labels is not None:
            raise ValueError("Loss computation from labels not supported yet")
        pad_mask = None if attention_mask is None else ~attention_mask.type(torch.bool)
        if use_cache and past_key_values is None:
            past_key_values = []
        output = self.backend_model(input_ids, prefix_len=prefix_len, pad_mask=pad_mask,
                                    kv_cache=past_key_values)
        return PerceiverCausalSequenceModelOutput(
            logits=output.logits,
            hidden_states=(output.last_hidden_state,),
            past_key_values=output.kv_cache,
            prefix_len=prefix_len,
        )

    # -------------------------------------------------- cache maintenance
    def _reorder_cache(self, past_key_values, beam_idx):
        out = []
        for layer_past in past_key_values:
            if isinstance(layer_past, StaticKVCache):
                out.append(layer_past.index_select_batch(beam_idx.to(layer_past.k_buf.device)))
            else:
                out.append(tuple(t.index_select(0, beam_idx.to(t.device)) for t in layer_past))
        return out

    @staticmethod
    def _truncate_entry(entry, max_len):
        if isinstance(entry, StaticKVCache):
            entry.truncate_front_to(max_len)
            return entry
        k, v = entry
        return (k[:, -max_len:], v[:, -max_len:])

    def _truncate_cross_attention_past_key_values(self, past_key_values):
        max_ca_cache_len = self.backend_model.max_seq_len - 1
        ca_cache, *sa_cache = past_key_values
        return [self._truncate_entry(ca_cache, max_ca_cache_len)] + sa_cache

    def _truncate_self_attention_past_key_values(self, past_key_values):
        max_sa_cache_len = self.backend_model.max_latents - 1
        ca_cache, *sa_cache = past_key_values
        return [ca_cache] + [self._truncate_entry(e, max_sa_cache_len) for e in sa_cache]

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, **kwargs):
        """The sliding schedule: grow latents to max_latents, then grow the prefix to
        max_prefix_len, then slide the window (discarding the left-most prefix token).
        Kept API-compatible with the reference (core/huggingface.py:89-138)."""
        attention_mask = kwargs.get("attention_mask", None)
        use_cache = kwargs.get("use_cache", None)
        prefix_len = kwargs.get("prefix_len", None)

        has_cached = (past_key_values is not None and len(past_key_values) > 0
                      and cache_len(past_key_values[0]) > 0)
        if not has_cached:
            input_len = input_ids.shape[1]
        else:
            # contrastive-search workaround: derive input length from the cache
            input_len = cache_len(past_key_values[0]) + 1

        max_seq_len = self.backend_model.max_seq_len
        num_latents = input_len - prefix_len

        max_seq_len_exceeded = input_len > max_seq_len
        max_latents_exceeded = num_latents > self.backend_model.max_latents

        if max_latents_exceeded and prefix_len < self.backend_model.max_prefix_len:
            prefix_len += 1

        if has_cached:
            input_ids = input_ids[:, -1:]
        else:
            input_ids = input_ids[:, -max_seq_len:]

        if attention_mask is not None and attention_mask.shape[1] > max_seq_len:
            attention_mask = attention_mask[:, -max_seq_len:]

        if has_cached:
            if max_latents_exceeded:
                past_key_values = self._truncate_self_attention_past_key_values(past_key_values)
            if max_seq_len_exceeded:
                past_key_values = self._truncate_cross_attention_past_key_values(past_key_values)

        return {
            "input_ids": input_ids,
            "attention_mask": attention_mask,
            "past_key_values": past_key_values,
            "use_cache": use_cache,
            "prefix_len": prefix_len,
        }

    # -------------------------------------------------- generation
    @torch.no_grad()
    def generate(
        self,
        inputs: Optional[torch.Tensor] = None,
        input_ids: Optional[torch.Tensor] = None,
        num_latents: int = 1,
        max_new_tokens: int = 64,
        do_sample: bool = False,
        temperature: float = 1.0,
        top_k: Optional[int] = None,
        top_p: Optional[float] = None,
        use_cache: bool = True,
        static_cache: bool = True,
        attention_mask: Optional[torch.Tensor] = None,
        pad_token_id: Optional[int] = None,
        eos_token_id: Optional[int] = None,
        num_beams: int = 1,
        length_penalty: float = 1.0,
        penalty_alpha: Optional[float] = None,
        generator: Optional[torch.Generator] = None,
        **kwargs,
    ) -> torch.Tensor:
        """Native generation loop with the latent/prefix sliding schedule.

        ``num_latents``: initial number of latent positions assigned to the end of
        the prompt. Cached and uncached paths produce identical tokens.
        """
        if input_ids is None:
            input_ids = inputs
        if input_ids is None:
            raise ValueError("Either inputs or input_ids must be defined")

        seq_len = input_ids.shape[1]
        if not 0 < seq_len <= self.backend_model.max_seq_len:
            raise ValueError(
                f"Input sequence length out of valid range [1..{self.backend_model.max_seq_len}]"
            )
        if not 0 < num_latents <= self.backend_model.max_latents:
            raise ValueError(
                f"num_latents={num_latents} out of valid range [1..{self.backend_model.max_latents}]"
            )
        num_latents = min(seq_len, num_latents)
        prefix_len = seq_len - num_latents
        if prefix_len > self.backend_model.max_prefix_len:
            num_latents_min = num_latents + prefix_len - self.backend_model.max_prefix_len
            raise ValueError(
                f"For given sequence of length={seq_len}, num_latents must "
                f"be in range [{num_latents_min}..{self.backend_model.max_latents}]"
            )

        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if num_beams > 1:
            if use_cache and static_cache:
                out = self._beam_search_graphed(input_ids, attention_mask, prefix_len, num_beams,
                                                max_new_tokens, eos_token_id, pad_token_id,
                                                length_penalty)
                if out is not None:
                    return out
            return self._beam_search(input_ids, attention_mask, prefix_len, num_beams,
                                     max_new_tokens, eos_token_id, pad_token_id,
                                     length_penalty, use_cache, static_cache)
        if penalty_alpha is not None and penalty_alpha > 0 and top_k and top_k > 1 \
                and not do_sample:
            if use_cache and static_cache:
                out = self._contrastive_search_graphed(input_ids, attention_mask, prefix_len,
                                                       top_k, penalty_alpha, max_new_tokens,
                                                       eos_token_id, pad_token_id)
                if out is not None:
                    return out
            return self._contrastive_search(input_ids, attention_mask, prefix_len,
                                            top_k, penalty_alpha, max_new_tokens,
                                            eos_token_id, pad_token_id, use_cache,
                                            static_cache)
        done = torch.zeros(input_ids.shape[0], dtype=torch.bool, device=input_ids.device)
        past = None
        if use_cache and static_cache:
            # hipGraph fast path: one captured-graph replay per token for the
            # requests that graph_decode.graph_route admits
            route = _graph.graph_route(
                self.backend_model, input_ids.shape[0], seq_len, prefix_len, max_new_tokens,
                attention_mask=attention_mask, eos_token_id=eos_token_id,
                pad_token_id=pad_token_id, top_p=top_p, generator=generator)
            if route is not None:
                gd = _graph.decoder_for(self, self.backend_model, route, do_sample=do_sample,
                                        temperature=temperature, top_k=top_k)
                if not route.baked:
                    gd.set_sampling(do_sample=do_sample, temperature=temperature, top_k=top_k,
                                    top_p=top_p, eos_token_id=eos_token_id,
                                    pad_token_id=pad_token_id)
                first = gd.prefill(input_ids, prefix_len=prefix_len, generator=generator,
                                   attention_mask=attention_mask if route.ragged else None)
                new = torch.cat([first, _graph.replay(gd, max_new_tokens - 1, eos_token_id)],
                                dim=1)
                if eos_token_id is not None:  # cut where the host loop would have stopped
                    new = self._cut_at_all_done(new, eos_token_id)
                return torch.cat([input_ids, new], dim=1)

            # preallocated in-place cache: no per-step concat/realloc (K9)
            p = next(self.backend_model.parameters())
            past = allocate_kv_cache(self.backend_model, input_ids.shape[0],
                                     device=p.device, dtype=p.dtype)

        for _ in range(max_new_tokens):
            model_inputs = self.prepare_inputs_for_generation(
                input_ids, past_key_values=past, attention_mask=attention_mask,
                use_cache=use_cache, prefix_len=prefix_len,
            )
            out = self(**model_inputs)
            prefix_len = out.prefix_len
            past = out.past_key_values if use_cache else None

            logits = out.logits[:, -1, :].float()
            next_token = self._select_next(logits, do_sample, temperature, top_k, top_p, generator)
            if eos_token_id is not None:
                fill = pad_token_id if pad_token_id is not None else eos_token_id
                next_token = torch.where(done, torch.full_like(next_token, fill), next_token)
                done = done | (next_token == eos_token_id)

            input_ids = torch.cat([input_ids, next_token[:, None]], dim=1)
            attention_mask = torch.cat(
                [attention_mask, torch.ones_like(next_token[:, None])], dim=1
            )
            if eos_token_id is not None and bool(done.all()):
                break

        return input_ids

    @torch.no_grad()
    def _beam_search_graphed(self, input_ids, attention_mask, prefix_len, num_beams,
                             max_new_tokens, eos_token_id, pad_token_id, length_penalty):
        """Beam search on the captured decode graph. Returns None when
        ``graph_decode.graph_route`` refuses the request: the host loop
        ``_beam_search`` runs then.

        One decoder (captured graph + caches of ``bsz * num_beams`` rows) is kept
        per (bsz, num_beams, bucket); EOS and fill ids live in device memory, so
        requests that differ in them or in prompt length replay the same graph."""
        bsz, seq_len = input_ids.shape
        route = _graph.graph_route(
            self.backend_model, bsz, seq_len, prefix_len, max_new_tokens, num_beams=num_beams,
            attention_mask=attention_mask, eos_token_id=eos_token_id, pad_token_id=pad_token_id)
        if route is None:
            return None
        gd = _graph.decoder_for(self, self.backend_model, route, num_beams=num_beams)
        # the host loop's fill: the pad id, else EOS, else 0
        gd.set_sampling(eos_token_id=eos_token_id, pad_token_id=pad_token_id)
        gd.prefill(input_ids, prefix_len=prefix_len)
        _graph.replay(gd, max_new_tokens - 1, eos_token_id, tokens=False)
        # best() cuts the output where the host loop would have stopped
        tokens, _ = gd.best(length_penalty)
        return torch.cat([input_ids, tokens], dim=1)

    @torch.no_grad()
    def _beam_search(self, input_ids, attention_mask, prefix_len, num_beams,
                     max_new_tokens, eos_token_id, pad_token_id, length_penalty,
                     use_cache, static_cache):
        """Compact beam search over the sliding latent/prefix schedule: beams stay
        live until EOS (frozen beams propose only EOS at unchanged score); the
        highest length-penalized score per batch wins."""
        bsz, seq_len = input_ids.shape
        device = input_ids.device
        # expand to (bsz * num_beams)
        input_ids = input_ids.repeat_interleave(num_beams, dim=0)
        attention_mask = attention_mask.repeat_interleave(num_beams, dim=0)
        beam_scores = torch.full((bsz, num_beams), -1e9, device=device)
        beam_scores[:, 0] = 0.0
        done = torch.zeros(bsz * num_beams, dtype=torch.bool, device=device)
        gen_len = torch.zeros(bsz * num_beams, device=device)

        past = None
        if use_cache and static_cache:
            p = next(self.backend_model.parameters())
            past = allocate_kv_cache(self.backend_model, bsz * num_beams,
                                     device=p.device, dtype=p.dtype)

        fill = pad_token_id if pad_token_id is not None else (eos_token_id or 0)
        for _ in range(max_new_tokens):
            model_inputs = self.prepare_inputs_for_generation(
                input_ids, past_key_values=past, attention_mask=attention_mask,
                use_cache=use_cache, prefix_len=prefix_len,
            )
            out = self(**model_inputs)
            prefix_len = out.prefix_len
            past = out.past_key_values if use_cache else None

            logp = out.logits[:, -1, :].float().log_softmax(-1)   # (bsz*beams, V)
            vocab = logp.shape[-1]
            if eos_token_id is not None:
                # frozen beams propose only the fill token at unchanged score
                frozen = torch.zeros_like(logp)
                frozen[:] = -1e9
                frozen[:, fill] = 0.0
                logp = torch.where(done[:, None], frozen, logp)

            cand = beam_scores.view(-1, 1) + logp                 # (bsz*beams, V)
            cand = cand.view(bsz, num_beams * vocab)
            top_scores, top_idx = cand.topk(num_beams, dim=-1)    # (bsz, beams)
            src_beam = top_idx // vocab                            # (bsz, beams)
            next_tok = top_idx % vocab

            beam_idx = (src_beam + torch.arange(bsz, device=device)[:, None] * num_beams).view(-1)
            input_ids = input_ids.index_select(0, beam_idx)
            attention_mask = attention_mask.index_select(0, beam_idx)
            done = done.index_select(0, beam_idx)
            gen_len = gen_len.index_select(0, beam_idx)
            if past is not None:
                past = self._reorder_cache(past, beam_idx)

            next_tok = next_tok.view(-1)
            beam_scores = top_scores
            gen_len = gen_len + (~done).float()
            if eos_token_id is not None:
                done = done | (next_tok == eos_token_id)

            input_ids = torch.cat([input_ids, next_tok[:, None]], dim=1)
            attention_mask = torch.cat([attention_mask, torch.ones_like(next_tok[:, None])], dim=1)
            if eos_token_id is not None and bool(done.all()):
                break

        norm = gen_len.view(bsz, num_beams).clamp(min=1.0) ** length_penalty
        best = (beam_scores / norm).argmax(dim=-1)
        idx = best + torch.arange(bsz, device=device) * num_beams
        return input_ids.index_select(0, idx)

    @torch.no_grad()
    def _contrastive_search_graphed(self, input_ids, attention_mask, prefix_len, top_k,
                                    penalty_alpha, max_new_tokens, eos_token_id, pad_token_id):
        """Contrastive search on the captured decode graph. Returns None when
        ``graph_decode.graph_route`` refuses the request: the host loop
        ``_contrastive_search`` runs then.

        One decoder (captured graph + caches of ``bsz * top_k`` rows) is kept per
        (bsz, top_k, bucket); ``penalty_alpha``, EOS and fill ids live in device
        memory, so requests that differ in them or in prompt length replay the
        same graph."""
        bsz, seq_len = input_ids.shape
        route = _graph.graph_route(
            self.backend_model, bsz, seq_len, prefix_len, max_new_tokens,
            attention_mask=attention_mask, eos_token_id=eos_token_id, pad_token_id=pad_token_id,
            contrastive_k=top_k)
        if route is None:
            return None
        gd = _graph.decoder_for(self, self.backend_model, route, contrastive_k=top_k)
        # the host loop's fill: the pad id, else EOS, else 0
        gd.set_sampling(penalty_alpha=penalty_alpha, eos_token_id=eos_token_id,
                        pad_token_id=pad_token_id)
        gd.prefill(input_ids, prefix_len=prefix_len)
        new = _graph.replay(gd, max_new_tokens, eos_token_id)
        if eos_token_id is not None:  # cut where the host loop would have stopped
            new = self._cut_at_all_done(new, eos_token_id)
        return torch.cat([input_ids, new], dim=1)

    @torch.no_grad()
    def _contrastive_search(self, input_ids, attention_mask, prefix_len, top_k,
                            penalty_alpha, max_new_tokens, eos_token_id,
                            pad_token_id, use_cache, static_cache):
        """Contrastive search (Su et al. 2022, the 🤗 penalty_alpha decoding the
        reference inherits from GenerationMixin): each step scores the top-k
        candidates by (1-a)*p(v) - a*max_cos(h_v, previous hidden states) and
        commits the best. The candidate forward runs the batch expanded k-fold
        through the normal cached step, so the selected candidate's KV append is
        reused as the real step (one extra forward per token, not k).

        Perceiver-AR adaptation: only latent positions have output states, so the
        degeneration penalty compares against the latent tail of the prompt plus
        the generated tokens (prefix-only positions have no hidden state)."""
        if not use_cache:
            raise ValueError("contrastive search requires use_cache=True")
        bsz = input_ids.shape[0]
        device = input_ids.device
        k = top_k

        past = None
        if static_cache:
            p = next(self.backend_model.parameters())
            past = allocate_kv_cache(self.backend_model, bsz, device=p.device, dtype=p.dtype)

        # prompt pass: logits for step 0 + the latent hidden states as history
        model_inputs = self.prepare_inputs_for_generation(
            input_ids, past_key_values=past if past is not None else [],
            attention_mask=attention_mask, use_cache=True, prefix_len=prefix_len)
        out = self(**model_inputs)
        prefix_len = out.prefix_len
        past = out.past_key_values
        logits = out.logits[:, -1, :].float()
        hist = torch.nn.functional.normalize(out.hidden_states[-1].float(), dim=-1)

        done = torch.zeros(bsz, dtype=torch.bool, device=device)
        fill = pad_token_id if pad_token_id is not None else (eos_token_id or 0)
        rep = torch.arange(bsz, device=device).repeat_interleave(k)

        for _ in range(max_new_tokens):
            probs = logits.softmax(-1)
            top_p_vals, cand = probs.topk(k, dim=-1)             # (bsz, k)

            # expanded candidate step: k copies of every sequence, one per candidate
            past_k = self._reorder_cache(past, rep)
            ids_k = torch.cat([input_ids.index_select(0, rep), cand.view(-1, 1)], dim=1)
            mask_k = torch.cat([attention_mask.index_select(0, rep),
                                torch.ones(bsz * k, 1, dtype=attention_mask.dtype,
                                           device=device)], dim=1)
            model_inputs = self.prepare_inputs_for_generation(
                ids_k, past_key_values=past_k, attention_mask=mask_k,
                use_cache=True, prefix_len=prefix_len)
            out = self(**model_inputs)

            h_cand = torch.nn.functional.normalize(
                out.hidden_states[-1][:, -1, :].float(), dim=-1)  # (bsz*k, C)
            # max cosine similarity against each candidate's own history
            sim = torch.einsum("btc,bkc->bkt", hist,
                               h_cand.view(bsz, k, -1)).amax(-1)  # (bsz, k)
            score = (1.0 - penalty_alpha) * top_p_vals - penalty_alpha * sim
            sel = score.argmax(-1)                                # (bsz,)
            idx = torch.arange(bsz, device=device) * k + sel

            past = self._reorder_cache(out.past_key_values, idx)
            prefix_len = out.prefix_len
            logits = out.logits.index_select(0, idx)[:, -1, :].float()
            hist = torch.cat([hist, h_cand.index_select(0, idx)[:, None]], dim=1)

            next_token = cand.gather(-1, sel[:, None]).squeeze(-1)
            if eos_token_id is not None:
                next_token = torch.where(done, torch.full_like(next_token, fill), next_token)
                done = done | (next_token == eos_token_id)

            input_ids = torch.cat([input_ids, next_token[:, None]], dim=1)
            attention_mask = torch.cat([attention_mask,
                                        torch.ones_like(next_token[:, None])], dim=1)
            if eos_token_id is not None and bool(done.all()):
                break

        return input_ids

    @staticmethod
    def _cut_at_all_done(new_tokens: torch.Tensor, eos_token_id: int) -> torch.Tensor:
        """(batch, n) generated tokens cut after the first column by which every
        row has emitted EOS: the length at which the host loop breaks."""
        all_done = (new_tokens == eos_token_id).int().cummax(dim=1).values.bool().all(dim=0)
        if not bool(all_done.any()):
            return new_tokens
        return new_tokens[:, :int(all_done.int().argmax()) + 1]

    @staticmethod
    def _select_next(logits, do_sample, temperature, top_k, top_p, generator):
        if not do_sample:
            return logits.argmax(dim=-1)
        if temperature != 1.0:
            logits = logits / temperature
        if top_k is not None and top_k > 0:
            kth = torch.topk(logits, min(top_k, logits.shape[-1]))[0][..., -1, None]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        if top_p is not None and 0 < top_p < 1:
            # standard nucleus rule: keep the smallest prefix of the sorted
            # distribution whose mass exceeds top_p (shifted cumsum so the
            # token that crosses the threshold is still kept)
            sorted_logits, sorted_idx = torch.sort(logits, descending=True)
            cum = sorted_logits.softmax(-1).cumsum(-1)
            remove = cum > top_p
            remove[..., 1:] = remove[..., :-1].clone()
            remove[..., 0] = False
            scatter_mask = remove.scatter(-1, sorted_idx, remove)
            logits = logits.masked_fill(scatter_mask, float("-inf"))
        probs = logits.softmax(dim=-1)
        return torch.multinomial(probs, 1, generator=generator).squeeze(-1)
