"""Left-padded prompt batches on the captured decode graph:
GraphedDecoder(ragged=True) replaying the windowed decode_attn kernel, and
generate() admitting left-padded requests to it."""
import gc

import pytest
import torch

from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.hf_base import PerceiverCausalSequenceModel
from perceiver_amd.models.text.clm import CausalLanguageModel, CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops import decode_attn as da

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
V, N, LATENTS, STEPS = 61, 30, 7, 8
PREFIX = N - LATENTS


@pytest.fixture(autouse=True, scope="module")
def _collect_garbage_before_later_tests():
    """The models, decoders and captured graphs of this module hold GPU
    resources. Collect what is left of them here, in this process, and not in a
    worker process that a later test of the session forks."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _cfg(channels=32, heads=4):
    return CausalLanguageModelConfig(vocab_size=V, max_seq_len=48, max_latents=16,
                                     num_channels=channels, num_heads=heads,
                                     num_self_attention_layers=2, cross_attention_dropout=0.0)


def _hf_model(seed=0):
    torch.manual_seed(seed)
    return PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(_cfg())).to(
        DEV, torch.bfloat16).eval()


def _batch(pads, seed=1):
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(1, V, (len(pads), N), generator=g)
    mask = torch.ones(len(pads), N, dtype=torch.long)
    for b, p in enumerate(pads):
        prompt[b, :p] = 0
        mask[b, :p] = 0
    return prompt.to(DEV), mask.to(DEV)


def _decoder(model, bsz, **kw):
    return GraphedDecoder(model, allocate_kv_cache(model, bsz, device=DEV, dtype=torch.bfloat16),
                          **kw)


def _run(gd, prompt, mask, n=STEPS):
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=PREFIX, attention_mask=mask)
        return torch.cat([first, gd.decode(n)], dim=1)


def _bits(t):
    return t.view(torch.int16)


def _ragged_decoders(model):
    return [gd for gd in getattr(model, "_graph_decoders", {}).values() if gd.ragged]


@pytest.mark.parametrize("channels,heads", [(32, 4), (128, 2)], ids=["d8", "d64"])
def test_graph_replay_equals_the_eager_step(channels, heads):
    torch.manual_seed(0)
    model = CausalLanguageModel(_cfg(channels, heads)).to(DEV, torch.bfloat16).eval()
    eager = _decoder(model, 3, ragged=True, use_graph=False)
    graph = _decoder(model, 3, ragged=True, use_graph=True)
    captured = None
    for pads in ([0, 4, 11], [9, 0, PREFIX + 2]):
        prompt, mask = _batch(pads)
        a, b = _run(eager, prompt, mask), _run(graph, prompt, mask)
        assert graph._graph is not None and eager._graph is None
        # a later prefill rewrites shift and replays the same graph
        captured = captured or graph._graph
        assert graph._graph is captured
        assert torch.equal(graph.shift.cpu(), torch.tensor(pads))
        assert a.shape == (3, STEPS + 1) and torch.equal(a, b)
        assert (a >= 0).all() and (a < V).all()
        assert torch.equal(eager.finished, graph.finished)
        for ce, cg in zip(eager.caches, graph.caches):
            assert torch.equal(_bits(ce.k_buf), _bits(cg.k_buf))
            assert torch.equal(_bits(ce.v_buf), _bits(cg.v_buf))


def test_generate_takes_the_graph_path_for_left_padded_requests():
    model = _hf_model()
    prompt, mask = _batch([0, 4, 11])
    kw = dict(input_ids=prompt, attention_mask=mask, num_latents=LATENTS, max_new_tokens=6)
    out = model.generate(**kw)
    decoders = _ragged_decoders(model)
    assert len(decoders) == 1 and decoders[0]._graph is not None
    assert out.shape == (3, N + 6) and torch.equal(out[:, :N], prompt)
    assert (out[:, N:] >= 0).all() and (out[:, N:] < V).all()
    graph = decoders[0]._graph
    assert torch.equal(model.generate(**kw), out)
    assert _ragged_decoders(model) == decoders and decoders[0]._graph is graph
    # an unpadded request keeps a decoder of its own, which is not ragged
    model.generate(input_ids=prompt, num_latents=LATENTS, max_new_tokens=6)
    assert len(model._graph_decoders) == 2 and _ragged_decoders(model) == decoders


def test_requests_outside_the_gate_take_the_host_loop(monkeypatch):
    model = _hf_model()
    prefills, beams = [], []
    inner_prefill = GraphedDecoder.prefill
    inner_beam = PerceiverCausalSequenceModel._beam_search

    def spy_prefill(self, *a, **k):
        prefills.append(1)
        return inner_prefill(self, *a, **k)

    def spy_beam(self, *a, **k):
        beams.append(1)
        return inner_beam(self, *a, **k)

    monkeypatch.setattr(GraphedDecoder, "prefill", spy_prefill)
    monkeypatch.setattr(PerceiverCausalSequenceModel, "_beam_search", spy_beam)
    prompt, mask = _batch([0, 4, 11])
    right = torch.ones_like(mask)
    right[1, -3:] = 0
    holes = mask.clone()
    holes[2, 20] = 0
    dead = mask.clone()
    dead[1] = 0
    for bad in (right, holes, dead):
        out = model.generate(input_ids=prompt, attention_mask=bad, num_latents=LATENTS,
                             max_new_tokens=6)
        assert out.shape == (3, N + 6)
    assert not prefills and not getattr(model, "_graph_decoders", {})
    out = model.generate(input_ids=prompt, attention_mask=mask, num_latents=LATENTS,
                         max_new_tokens=6, num_beams=3)
    assert out.shape == (3, N + 6) and len(beams) == 1 and not prefills
    # the left-padded greedy request does take the decoder
    model.generate(input_ids=prompt, attention_mask=mask, num_latents=LATENTS, max_new_tokens=6)
    assert len(prefills) == 1


def test_lever_runs_the_mask_composition(monkeypatch):
    model = _hf_model()
    prompt, mask = _batch([0, 4, 11])
    kw = dict(input_ids=prompt, attention_mask=mask, num_latents=LATENTS, max_new_tokens=6)
    want = model.generate(**kw)

    composed, kernel = [], []
    inner_comp, inner_kernel = da.window_attention_composition, da.decode_attn

    def spy_comp(*a, **k):
        composed.append(1)
        return inner_comp(*a, **k)

    def spy_kernel(*a, **k):
        kernel.append(1)
        return inner_kernel(*a, **k)

    monkeypatch.setattr(da, "window_attention_composition", spy_comp)
    monkeypatch.setattr(da, "decode_attn", spy_kernel)
    monkeypatch.setenv("PERCEIVER_DECODE_ATTN", "0")
    other = _hf_model()  # same weights, no decoder yet
    got = other.generate(**kw)
    decoders = _ragged_decoders(other)
    assert len(decoders) == 1 and decoders[0]._graph is not None
    assert composed and not kernel
    assert got.shape == want.shape and torch.equal(got[:, :N], prompt)
    match = (got[:, N:] == want[:, N:]).float().mean().item()
    assert match >= 0.75, match


# The agreement test runs at a capacity of 512 and prompts of 300 tokens. At the
# capacity of 48 used above, today's decoder reads one 64-key tile exactly as the
# host-driven forward does, its logits are bit-equal to the host's, and a
# yardstick of 0.0 admits no kernel that orders its sums differently (measured
# there: standard decoder 0.0, ragged decoder 1.2e-4, one bf16 step of a logit).
# From 256 keys on the flash forward splits the key axis, the decoder over the
# capacity and the host over the live prefix, as on the flagship, and today's
# decoder shows the deviation the issue takes as the yardstick.
AG_N, AG_PREFIX = 300, 293


def _ag_model():
    torch.manual_seed(0)
    cfg = CausalLanguageModelConfig(vocab_size=V, max_seq_len=512, max_latents=16,
                                    num_channels=32, num_heads=4, num_self_attention_layers=2,
                                    cross_attention_dropout=0.0)
    return PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg)).to(
        DEV, torch.bfloat16).eval()


def _ag_batch(pads, seed):
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(1, V, (len(pads), AG_N), generator=g)
    mask = torch.ones(len(pads), AG_N, dtype=torch.long)
    for b, p in enumerate(pads):
        prompt[b, :p] = 0
        mask[b, :p] = 0
    return prompt.to(DEV), mask.to(DEV)


def _teacher_forced_gap(model, gd, prompt, mask):
    """(decoder tokens, per-row max |logit(decoder step) - logit(host-driven cached
    forward fed the decoder's tokens)|)."""
    b = prompt.shape[0]
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=AG_PREFIX, attention_mask=mask)
        toks, logits = [first], []
        for _ in range(STEPS):
            toks.append(gd.decode(1))
            logits.append(gd.last_logits[:, -1].float().clone())
        toks = torch.cat(toks, dim=1)

        kv = allocate_kv_cache(model, b, device=DEV, dtype=torch.bfloat16)
        am = None if mask is None else mask.clone()
        model(prompt, prefix_len=AG_PREFIX, pad_mask=None if am is None else am == 0, kv_cache=kv)
        gap = torch.zeros(b, device=DEV)
        for i in range(STEPS):
            if am is not None:
                am = torch.cat([am, torch.ones(b, 1, dtype=am.dtype, device=DEV)], dim=1)
            out = model(toks[:, i:i + 1], prefix_len=0, pad_mask=None if am is None else am == 0,
                        kv_cache=kv)
            gap = torch.maximum(gap, (out.logits[:, -1].float() - logits[i]).abs().amax(dim=-1))
    return toks, gap.cpu()


def test_agreement_with_the_host_loop():
    hf = _ag_model()
    model = hf.backend_model
    pads = [0, 40, 111, 250]
    prompt, mask = _ag_batch(pads, seed=1)
    full, _ = _ag_batch([0, 0, 0, 0], seed=2)
    # both decoders reach their split paths at this capacity
    from perceiver_amd.ops import hip

    assert hip.ext().flash_split_plan(4 * 4, 512, 64)[0] > 1
    assert hip.ext().decode_attn_plan(4, 4, 512, 8)[0] > 1

    # the yardstick: today's decoder on unpadded prompts against the same host forward
    _, base = _teacher_forced_gap(model, _decoder(model, 4, use_graph=False), full, None)
    toks, gap = _teacher_forced_gap(model, _decoder(model, 4, ragged=True, use_graph=False),
                                    prompt, mask)
    padded = gap[1:].max().item()
    print(f"teacher-forced max |dlogit|: padded rows of the ragged decoder {padded:.4e}, "
          f"unpadded prompts through the standard decoder {base.max().item():.4e}")

    with torch.no_grad():
        host = hf.generate(input_ids=prompt, attention_mask=mask, num_latents=AG_N - AG_PREFIX,
                           max_new_tokens=STEPS + 1, static_cache=False)[:, AG_N:]
        gd = _decoder(model, 4, ragged=True)
        graph = torch.cat([gd.prefill(prompt, prefix_len=AG_PREFIX, attention_mask=mask),
                           gd.decode(STEPS)], dim=1)
    assert gd._graph is not None
    assert torch.equal(graph, toks)  # the captured graph is the eager step measured above
    match = (graph == host).float().mean().item()
    assert match >= 0.75, f"ragged graph decode diverged from the host loop: {match:.2f}"
    assert padded <= 4.0 * base.max().item(), (padded, base.max().item())
