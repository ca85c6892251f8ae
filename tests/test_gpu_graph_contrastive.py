"""Contrastive search on the captured-graph decode path:
GraphedDecoder(contrastive_k=...) replaying contrastive_sim + contrastive_commit +
contrastive_copy, and generate(penalty_alpha, top_k) taking it."""
import pytest
import torch

import _contrastive_ref as ref

from perceiver_amd.core import graph_decode
from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.hf_base import PerceiverCausalSequenceModel
from perceiver_amd.models.text.clm import CausalLanguageModel, CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops import contrastive as cs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K, ALPHA = 4, 0.6


def _cfg():
    return CausalLanguageModelConfig(vocab_size=61, max_seq_len=48, max_latents=16,
                                     num_channels=32, num_heads=4, num_self_attention_layers=2,
                                     cross_attention_dropout=0.0)


def _decoder(model, bsz, k=K, **kw):
    kw.setdefault("penalty_alpha", ALPHA)
    return GraphedDecoder(model, allocate_kv_cache(model, bsz * k, device=DEV,
                                                   dtype=torch.bfloat16), contrastive_k=k, **kw)


def _run(gd, prompt, n):
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=prompt.shape[1] - 1)
        assert first.shape == (prompt.shape[0], gd.contrastive_k)
        return gd.decode(n)


def _bits(t):
    return t.view(torch.int16)


def _assert_group_rows_identical(gd):
    for buf, ci in zip(gd._reorder_bufs, gd._reorder_counter):
        n = int(gd.counters[ci])
        v = _bits(buf).view(gd.groups, gd.contrastive_k, *buf.shape[1:])[:, :, :n]
        assert torch.equal(v, v[:, :1].expand_as(v))


def test_graph_replay_equals_the_eager_step():
    torch.manual_seed(0)
    model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    free = _run(_decoder(model, 2, use_graph=False), prompt, 10)
    eos = int(free[0, 3])  # prompt 0 stops early

    eager = _decoder(model, 2, use_graph=False, eos_token_id=eos)
    graph = _decoder(model, 2, use_graph=True, eos_token_id=eos)
    assert eager.use_contrastive_kernel and graph.use_contrastive_kernel
    # the eager decoder one step at a time: which candidate won each step
    with torch.no_grad():
        eager.prefill(prompt, prefix_len=29)
        cols, sels = [], []
        for _ in range(10):
            cols.append(eager.decode(1))
            sels.append(eager.cand_src.view(2, K)[:, 0].clone())
            _assert_group_rows_identical(eager)
    a, b = torch.cat(cols, dim=1), _run(graph, prompt, 10)
    assert graph._graph is not None and eager._graph is None
    assert a.shape == (2, 10) and torch.equal(a, b)
    assert (a >= 0).all() and (a < 61).all()
    assert bool(eager.finished[0]) and eager.finished.shape == (2,)
    assert (a[0, 3:] == eos).all()
    assert torch.equal(eager.finished, graph.finished)
    assert torch.equal(_bits(eager.hist), _bits(graph.hist))
    assert torch.equal(eager.hist_rnorm, graph.hist_rnorm)
    assert torch.equal(eager.tok, graph.tok) and torch.equal(eager.cand_prob, graph.cand_prob)
    assert torch.equal(eager.rec_tok, graph.rec_tok)
    for ce, cg in zip(eager.caches, graph.caches):
        assert torch.equal(_bits(ce.k_buf), _bits(cg.k_buf))
        assert torch.equal(_bits(ce.v_buf), _bits(cg.v_buf))
    # the invariant held while the copy had work to do: some step chose sel != 0
    assert bool((torch.stack(sels) != 0).any())
    _assert_group_rows_identical(graph)
    # the history: the prompt's one latent position, then one row per step
    assert int(graph.sa_len) == 11
    assert bool((graph.hist_rnorm[:, :11] > 0).all()) and bool((graph.hist_rnorm[:, 11:] == 0).all())


def test_kernels_equal_the_torch_composition(monkeypatch):
    n = 8
    inner = cs.contrastive_reference
    for seed in range(20):
        torch.manual_seed(100 + seed)
        model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
        prompt = torch.randint(0, 61, (2, 30), device=DEV)
        monkeypatch.setenv("PERCEIVER_CONTRASTIVE_GRAPH", "0")
        gaps, moved = [], []
        monkeypatch.setattr(graph_decode._contrastive, "contrastive_reference",
                            ref.oracle_spy(inner, gaps, moved))
        comp = _decoder(model, 2, use_graph=False)
        assert not comp.use_contrastive_kernel
        want = _run(comp, prompt, n)
        monkeypatch.setattr(graph_decode._contrastive, "contrastive_reference", inner)
        monkeypatch.delenv("PERCEIVER_CONTRASTIVE_GRAPH")
        # clear: >= 64x the score tolerance of these shapes, and no less than the
        # 1e-4 the oracle spy holds the composition to
        tol = ref.score_tolerance(ALPHA, 32, comp.last_logits[:, -1].float().cpu())
        if min(gaps) >= max(64 * tol, 1e-4):
            break
    assert min(gaps) >= max(64 * tol, 1e-4), "no seed gives a clear gap at every step"
    assert len(gaps) == 2 * n and any(moved)
    gd = _decoder(model, 2, use_graph=True)
    assert gd.use_contrastive_kernel
    got = _run(gd, prompt, n)
    print(f"smallest fp64 gap {min(gaps):.3e}, 64 x score tolerance {64 * tol:.3e}")
    assert torch.equal(got, want)
    assert torch.equal(_bits(gd.hist), _bits(comp.hist))
    r_err = float(((gd.hist_rnorm - comp.hist_rnorm).abs() * comp.hist_rnorm.clamp_min(1e-30).reciprocal()
                   )[:, :int(gd.sa_len)].max())
    assert r_err <= 2 * (32 + 4) * 2.0 ** -24
    _assert_group_rows_identical(comp)
    _assert_group_rows_identical(gd)


def _hf_model(seed):
    torch.manual_seed(seed)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(_cfg()))
    return model.to(DEV, torch.bfloat16).eval()


def _contrastive_decoders(model):
    return [gd for gd in getattr(model, "_graph_decoders", {}).values() if gd.contrastive_k]


def test_generate_takes_the_graph_path_and_reuses_it():
    model = _hf_model(2)
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    out = model.generate(input_ids=prompt, num_latents=1, max_new_tokens=10, top_k=K,
                         penalty_alpha=0.6)
    assert out.shape == (2, 40) and torch.equal(out[:, :30], prompt)
    assert (out >= 0).all() and (out < 61).all()
    (gd,) = _contrastive_decoders(model)
    assert gd.contrastive_k == K and gd.batch == 2 * K and gd._graph is not None
    graph = gd._graph
    # the decoder's own answer for the same request
    fresh = _decoder(model.backend_model, 2)
    assert torch.equal(out[:, 30:], _run(fresh, prompt, 10))

    # another prompt length, alpha, EOS and pad ids: the same captured graph
    shorter = torch.randint(0, 61, (2, 23), device=DEV)
    free = _run(_decoder(model.backend_model, 2, penalty_alpha=0.35), shorter, 10)
    eos = int(free[1, 4])
    again = model.generate(input_ids=shorter, num_latents=1, max_new_tokens=10, top_k=K,
                           penalty_alpha=0.35, eos_token_id=eos, pad_token_id=59)
    assert again.shape[0] == 2 and torch.equal(again[:, :23], shorter)
    assert _contrastive_decoders(model) == [gd] and gd._graph is graph
    assert abs(float(gd.alpha) - 0.35) < 1e-7 and gd.eos_fill.tolist() == [eos, 59]
    fresh = _decoder(model.backend_model, 2, penalty_alpha=0.35, eos_token_id=eos, pad_token_id=59)
    want = _run(fresh, shorter, 10)
    assert bool(gd.finished[1]) and (want[1, 5:] == 59).all()
    assert torch.equal(again[:, 23:], PerceiverCausalSequenceModel._cut_at_all_done(want, eos))


def test_tiny_alpha_equals_the_greedy_graph_decode():
    # the first seed whose greedy path keeps its best logit >= 8 bf16 ulps ahead
    # of the second at every step: the contrastive run sees the same logits
    # through a batch four times as large, and library GEMMs need not agree to
    # the last bit across batch sizes. With alpha -> 0 candidate 0 always wins,
    # so the rows the candidates come from are the greedy path's.
    new = 5
    for seed in range(60):
        model = _hf_model(10 + seed)
        prompt = torch.randint(0, 61, (2, 30), device=DEV)
        gd = _decoder(model.backend_model, 2, use_graph=False, penalty_alpha=1e-6)
        margin = float("inf")  # in bf16 ulps of the best logit
        with torch.no_grad():
            gd.prefill(prompt, prefix_len=29)
            for _ in range(new):
                rows = torch.arange(2, device=DEV) * K + gd.cand_src.view(2, K)[:, 0]
                top = gd.last_logits[rows, -1].float().topk(2).values
                ulp = torch.exp2(top[:, 0].abs().clamp_min(2.0 ** -100).log2().floor() - 7)
                margin = min(margin, float(((top[:, 0] - top[:, 1]) / ulp).min()))
                gd.decode(1)
        if margin >= 8:
            break
    assert margin >= 8, "no seed gives greedy decoding a clear margin"
    print(f"seed {10 + seed}: smallest greedy margin {margin:.1f} bf16 ulps")
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=new)
    greedy = model.generate(**kw)
    contrastive = model.generate(top_k=K, penalty_alpha=1e-6, **kw)
    assert len(_contrastive_decoders(model)) == 1 and len(model._graph_decoders) == 2
    assert torch.equal(greedy, contrastive)


def test_requests_outside_the_gate_take_the_host_loop(monkeypatch):
    model = _hf_model(4)
    calls = []
    inner = PerceiverCausalSequenceModel._contrastive_search

    def spy(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)

    monkeypatch.setattr(PerceiverCausalSequenceModel, "_contrastive_search", spy)
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=6, penalty_alpha=0.6)
    out = model.generate(top_k=9, **kw)
    assert out.shape == (2, 36) and len(calls) == 1
    mask = torch.ones_like(prompt)
    mask[0, :4] = 0
    out = model.generate(top_k=K, attention_mask=mask, **kw)
    assert out.shape == (2, 36) and len(calls) == 2
    monkeypatch.setenv("PERCEIVER_CONTRASTIVE_GRAPH", "0")
    out = model.generate(top_k=K, **kw)
    assert out.shape == (2, 36) and len(calls) == 3
    assert not _contrastive_decoders(model)
    monkeypatch.delenv("PERCEIVER_CONTRASTIVE_GRAPH")
    model.generate(top_k=K, **kw)
    assert len(calls) == 3 and len(_contrastive_decoders(model)) == 1
