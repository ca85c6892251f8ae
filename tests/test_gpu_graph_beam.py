"""Beam search on the captured-graph decode path: GraphedDecoder(num_beams=...)
replaying beam_select + beam_reorder, and generate(num_beams > 1) taking it."""
import pytest
import torch

from _beam_ref import candidates64, tolerance

from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.hf_base import PerceiverCausalSequenceModel
from perceiver_amd.models.text.clm import CausalLanguageModel, CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NB = 3


def _cfg():
    return CausalLanguageModelConfig(vocab_size=61, max_seq_len=48, max_latents=16,
                                     num_channels=32, num_heads=4, num_self_attention_layers=2,
                                     cross_attention_dropout=0.0)


def _decoder(model, bsz, nb=NB, **kw):
    return GraphedDecoder(model, allocate_kv_cache(model, bsz * nb, device=DEV,
                                                   dtype=torch.bfloat16), num_beams=nb, **kw)


def _run(gd, prompt, n):
    with torch.no_grad():
        gd.prefill(prompt, prefix_len=prompt.shape[1] - 1)
        gd.decode(n)
    return gd.hypotheses()


def _bits(t):
    return t.view(torch.int16)


def test_graph_replay_equals_the_eager_step():
    torch.manual_seed(0)
    model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    free = _run(_decoder(model, 2, use_graph=False), prompt, 10)
    eos = int(free[0, 3])  # some beam stops early

    eager = _decoder(model, 2, use_graph=False, eos_token_id=eos)
    graph = _decoder(model, 2, use_graph=True, eos_token_id=eos)
    assert eager.use_beam_kernel and graph.use_beam_kernel
    a, b = _run(eager, prompt, 10), _run(graph, prompt, 10)
    assert graph._graph is not None and eager._graph is None
    assert a.shape == (2 * NB, 11) and torch.equal(a, b)
    assert (a >= 0).all() and (a < 61).all()
    assert bool(eager.finished.any())
    assert torch.equal(eager.beam_scores, graph.beam_scores)
    assert torch.equal(eager.finished, graph.finished)
    assert torch.equal(eager.gen_len, graph.gen_len)
    assert torch.equal(eager.rec_all_done, graph.rec_all_done)
    for ce, cg in zip(eager.caches, graph.caches):
        assert torch.equal(_bits(ce.k_buf), _bits(cg.k_buf))
        assert torch.equal(_bits(ce.v_buf), _bits(cg.v_buf))
    # the beams did move: the reorder had work to do
    assert (eager.rec_parent[1:11].cpu() != torch.arange(NB).repeat(2).int()).any()
    ta, sa = eager.best(1.0)
    tb, sb = graph.best(1.0)
    assert torch.equal(ta, tb) and torch.equal(sa, sb)


def _composition_run(model, prompt, n):
    """The torch composition step by step: tokens, scores, the smallest gap
    between the NB'th and the next candidate over all steps, and the summed
    per-step tolerance of the scores."""
    gd = _decoder(model, prompt.shape[0], use_graph=False)
    assert not gd.use_beam_kernel
    gap, tol = float("inf"), 0.0

    def look(scores, done):
        nonlocal gap, tol
        x = gd.last_logits[:, -1, :].float().cpu()
        s, d = scores.cpu(), done.cpu()
        cand = candidates64(x, s, d, 0).view(prompt.shape[0], -1)
        top = cand.topk(NB + 1).values
        gap = min(gap, float((top[:, NB - 1] - top[:, NB]).min()))
        tol += tolerance(x, s, d, 0, rows=(s > -1e8) & ~d)

    with torch.no_grad():
        start = torch.full((prompt.shape[0], NB), -1e9)
        start[:, 0] = 0.0
        gd.prefill(prompt, prefix_len=prompt.shape[1] - 1)
        look(start.view(-1), torch.zeros(prompt.shape[0] * NB, dtype=torch.bool))
        for _ in range(n):
            scores, done = gd.beam_scores.clone(), gd.finished.clone()
            gd.decode(1)
            look(scores, done)
    return gd.hypotheses(), gd.beam_scores.clone(), gap, tol


def test_kernels_equal_the_torch_composition(monkeypatch):
    n = 8
    for seed in range(20):
        torch.manual_seed(100 + seed)
        model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
        prompt = torch.randint(0, 61, (2, 30), device=DEV)
        monkeypatch.setenv("PERCEIVER_BEAM_GRAPH", "0")
        want, want_scores, gap, tol = _composition_run(model, prompt, n)
        if gap >= 1e-4:
            break
    assert gap >= 1e-4, "no seed gives a clear gap at every step"
    monkeypatch.delenv("PERCEIVER_BEAM_GRAPH")
    gd = _decoder(model, 2, use_graph=True)
    assert gd.use_beam_kernel
    got = _run(gd, prompt, n)
    assert torch.equal(got, want)
    err = float((gd.beam_scores - want_scores).abs().max())
    print(f"gap={gap:.3e} summed tol={tol:.3e} max |score - composition| = {err:.3e}")
    assert err <= tol


def _hf_model(seed):
    torch.manual_seed(seed)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(_cfg()))
    return model.to(DEV, torch.bfloat16).eval()


def _beam_decoders(model):
    return [gd for gd in getattr(model, "_graph_decoders", {}).values() if gd.num_beams > 1]


def test_generate_takes_the_graph_path_and_reuses_it():
    model = _hf_model(2)
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    out = model.generate(input_ids=prompt, num_latents=1, max_new_tokens=10, num_beams=NB)
    assert out.shape == (2, 40) and torch.equal(out[:, :30], prompt)
    assert (out >= 0).all() and (out < 61).all()
    (gd,) = _beam_decoders(model)
    assert gd.num_beams == NB and gd.batch == 2 * NB and gd._graph is not None
    graph = gd._graph
    # the decoder's own answer for the same request
    fresh = _decoder(model.backend_model, 2)
    _run(fresh, prompt, 9)
    assert torch.equal(out[:, 30:], fresh.best(1.0)[0])

    # another prompt length, other EOS and pad ids: the same captured graph
    shorter = torch.randint(0, 61, (2, 23), device=DEV)
    again = model.generate(input_ids=shorter, num_latents=1, max_new_tokens=10, num_beams=NB,
                           eos_token_id=60, pad_token_id=59, length_penalty=0.5)
    assert again.shape[0] == 2 and torch.equal(again[:, :23], shorter)
    assert _beam_decoders(model) == [gd] and gd._graph is graph
    fresh = _decoder(model.backend_model, 2, eos_token_id=60, pad_token_id=59)
    _run(fresh, shorter, 9)
    assert torch.equal(again[:, 23:], fresh.best(0.5)[0])


def test_generate_with_eos_returns_the_host_loops_length(monkeypatch):
    model = _hf_model(3)
    prompt = torch.randint(0, 61, (1, 30), device=DEV)
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=14, num_beams=NB)
    model.generate(**kw)
    (gd,) = _beam_decoders(model)
    beams = gd.hypotheses()
    # a token the free run's beams are seen to emit: the most frequent one
    eos = int(beams.flatten().bincount(minlength=61).argmax())
    out = model.generate(eos_token_id=eos, **kw)
    assert _beam_decoders(model) == [gd]
    assert bool(gd.finished.any())
    new = out[0, 30:].tolist()
    if eos in new:  # after EOS only the fill id (EOS itself without a pad id) follows
        assert all(t == eos for t in new[new.index(eos):])
    # the cut is the first step at which every beam was done, else the full length
    stop = gd.rec_all_done[:gd._steps_host + 1].all(dim=1).int()
    want_len = int(stop.argmax()) + 1 if bool(stop.any()) else 14
    assert len(new) == want_len
    monkeypatch.setenv("PERCEIVER_BEAM_GRAPH", "0")
    host = model.generate(eos_token_id=eos, **kw)
    assert _beam_decoders(model) == [gd]  # the lever sends generate() to the host loop
    assert host.shape == out.shape


def test_requests_outside_the_gate_take_the_host_loop(monkeypatch):
    model = _hf_model(4)
    calls = []
    inner = PerceiverCausalSequenceModel._beam_search

    def spy(self, *a, **k):
        calls.append(1)
        return inner(self, *a, **k)

    monkeypatch.setattr(PerceiverCausalSequenceModel, "_beam_search", spy)
    prompt = torch.randint(0, 61, (2, 30), device=DEV)
    mask = torch.ones_like(prompt)
    mask[0, :4] = 0
    out = model.generate(input_ids=prompt, attention_mask=mask, num_latents=1, max_new_tokens=6,
                         num_beams=NB)
    assert out.shape == (2, 36) and len(calls) == 1
    out = model.generate(input_ids=prompt, num_latents=1, max_new_tokens=6, num_beams=9)
    assert out.shape == (2, 36) and len(calls) == 2
    assert not _beam_decoders(model)
    model.generate(input_ids=prompt, num_latents=1, max_new_tokens=6, num_beams=NB)
    assert len(calls) == 2 and len(_beam_decoders(model)) == 1
