"""Sampling, EOS and seeds on the captured-graph decode path: GraphedDecoder
with device-resident sampling parameters, and generate() taking that path for
nucleus / EOS / seeded requests with one decoder per batch size."""
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

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _cfg(**kw):
    base = dict(vocab_size=61, max_seq_len=48, max_latents=16, num_channels=32,
                num_heads=4, num_self_attention_layers=2, cross_attention_dropout=0.0)
    base.update(kw)
    return CausalLanguageModelConfig(**base)


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _decoder(model, batch, **kw):
    return GraphedDecoder(model, allocate_kv_cache(model, batch, device=DEV,
                                                   dtype=torch.bfloat16), **kw)


def _run(gd, prompt, n, seed):
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=prompt.shape[1] - 1, generator=_gen(seed))
        return torch.cat([first, gd.decode(n)], dim=1), gd.finished.clone()


def test_graph_and_eager_steps_sample_identically():
    torch.manual_seed(0)
    model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
    prompt = torch.randint(0, 61, (4, 30), device=DEV)
    kw = dict(do_sample=True, top_k=8, top_p=0.9)

    # an EOS that row 0 is known to draw early with this seed
    free, _ = _run(_decoder(model, 4, use_graph=False, **kw), prompt, 10, seed=5)
    eos = int(free[0, 3])

    eager = _decoder(model, 4, use_graph=False, eos_token_id=eos, **kw)
    graph = _decoder(model, 4, use_graph=True, eos_token_id=eos, **kw)
    a, a_done = _run(eager, prompt, 10, seed=5)
    b, b_done = _run(graph, prompt, 10, seed=5)
    assert graph._graph is not None and eager._graph is None
    assert torch.equal(a, b)
    assert torch.equal(a_done, b_done)
    stop = free[0].tolist().index(eos)
    assert bool(a_done[0]) and (a[0, stop:] == eos).all()  # fill is EOS without a pad id
    assert torch.equal(a[0, :stop + 1], free[0, :stop + 1])  # same draws up to the stop
    assert (a >= 0).all() and (a < 61).all()

    # another seed decodes other samples, the same seed the same ones
    c, _ = _run(graph, prompt, 10, seed=6)
    d, _ = _run(graph, prompt, 10, seed=5)
    assert not torch.equal(c, b)
    assert torch.equal(d, b)


def test_set_sampling_reuses_the_captured_graph():
    torch.manual_seed(1)
    model = CausalLanguageModel(_cfg()).to(DEV, torch.bfloat16).eval()
    prompt = torch.randint(0, 61, (4, 30), device=DEV)
    gd = _decoder(model, 4, do_sample=True, temperature=1.5, top_k=8, top_p=0.9)
    sampled, _ = _run(gd, prompt, 8, seed=1)
    graph = gd._graph
    assert graph is not None

    gd.set_sampling(temperature=0.6, top_p=0.5)
    other, _ = _run(gd, prompt, 8, seed=1)
    assert gd._graph is graph
    assert (other >= 0).all() and (other < 61).all()

    # the rewritten buffers are what the replay reads: top_k=1 is greedy
    gd.set_sampling(do_sample=False)
    greedy, _ = _run(gd, prompt, 8, seed=1)
    gd.set_sampling(do_sample=True, temperature=2.0, top_k=1, top_p=None)
    top1, _ = _run(gd, prompt, 8, seed=1)
    assert gd._graph is graph
    assert torch.equal(top1, greedy)
    assert not torch.equal(sampled, greedy)

    # per-row parameters: rows 0-1 greedy, rows 2-3 sampled with the old settings
    ds = torch.tensor([False, False, True, True])
    gd.set_sampling(do_sample=ds, temperature=1.5, top_k=8, top_p=0.9)
    mixed, _ = _run(gd, prompt, 8, seed=1)
    assert gd._graph is graph
    assert torch.equal(mixed[:2], greedy[:2])
    assert torch.equal(mixed[2:], sampled[2:])


def _hf_model(seed):
    torch.manual_seed(seed)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(_cfg()))
    return model.to(DEV, torch.bfloat16).eval()


def test_generate_nucleus_eos_seed_replays_one_graph():
    model = _hf_model(2)
    prompt = torch.randint(0, 61, (4, 30), device=DEV)
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=12, do_sample=True,
              top_p=0.9, top_k=8)
    free = model.generate(generator=_gen(7), **kw)[:, 30:]
    eos = int(free[0, 2])

    out = model.generate(generator=_gen(7), eos_token_id=eos, **kw)
    decoders = model._graph_decoders
    assert len(decoders) == 1
    gd = next(iter(decoders.values()))
    graph = gd._graph
    assert graph is not None

    again = model.generate(generator=_gen(7), eos_token_id=eos, **kw)
    assert torch.equal(out, again)

    model.generate(generator=_gen(7), eos_token_id=eos, temperature=1.7,
                   **{**kw, "top_p": 0.5})
    assert len(model._graph_decoders) == 1
    assert next(iter(model._graph_decoders.values())) is gd and gd._graph is graph

    new = out[:, 30:]
    assert torch.equal(out[:, :30], prompt)
    stop = free[0].tolist().index(eos)
    assert torch.equal(new[0, :stop + 1], free[0, :stop + 1])
    # after a row's EOS only the fill id (EOS itself here) follows
    for row in new.tolist():
        if eos in row:
            assert all(t == eos for t in row[row.index(eos):])
    # the length is the host loop's: cut after the first column by which all rows are done
    assert new.shape == PerceiverCausalSequenceModel._cut_at_all_done(new, eos).shape
    hit = (new == eos).any(dim=1)
    if bool(hit.all()):
        assert not bool((new[:, :-1] == eos).any(dim=1).all())
    else:
        assert new.shape[1] == 12


def test_generate_cuts_at_the_first_all_done_column():
    model = _hf_model(3)
    prompt = torch.randint(0, 61, (1, 30), device=DEV)
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=14)
    free = model.generate(**kw)[0, 30:].tolist()
    # the token whose first occurrence comes latest: the longest run before the stop
    col = max(free.index(t) for t in set(free))
    out = model.generate(eos_token_id=free[col], pad_token_id=(free[col] + 1) % 61, **kw)
    assert out.shape[1] == 30 + col + 1
    assert out[0, 30:].tolist() == free[:col + 1]
    assert len(model._graph_decoders) == 1  # greedy and EOS requests share the decoder


def test_lever_puts_the_torch_composition_back(monkeypatch):
    monkeypatch.setenv("PERCEIVER_DECODE_SELECT", "0")
    model = _hf_model(4)
    prompt = torch.randint(0, 61, (4, 30), device=DEV)
    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=8, do_sample=True, top_k=8)
    # top-p / EOS / generator requests are the host loop's again
    out = model.generate(top_p=0.9, eos_token_id=3,
                         generator=torch.Generator(device=DEV).manual_seed(1), **kw)
    assert out.shape[0] == 4 and not getattr(model, "_graph_decoders", None)
    # plain sampling still replays a graph, on the torch selection
    model.generate(**kw)
    gd = next(iter(model._graph_decoders.values()))
    assert not gd.use_kernel and gd._graph is not None

    # the decoder's torch selection expresses top-p and EOS too, and captures
    gd = _decoder(model.backend_model, 4, do_sample=True, top_k=8, top_p=0.9, eos_token_id=3)
    with torch.no_grad():
        gd.prefill(prompt, prefix_len=29)
        toks = gd.decode(8)
    assert not gd.use_kernel and gd._graph is not None
    assert toks.shape == (4, 8) and (toks >= 0).all() and (toks < 61).all()
    for row, fin in zip(toks.tolist(), gd.finished.tolist()):
        if 3 in row[:-1]:
            assert fin and all(t == 3 for t in row[row.index(3):])
    # its parameters are constants of the capture: changing them drops the graph
    gd.set_sampling(top_p=0.5)
    assert gd._graph is None
