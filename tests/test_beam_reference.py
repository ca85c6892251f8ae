"""Beam search rules in plain torch (ops/beam.py::beam_select_reference) and the
beam GraphedDecoder's eager step on the CPU against generate()'s host loop."""
import pytest
import torch

from _beam_ref import tie_cases

from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.text.clm import CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops.beam import backtrack, beam_select_reference, reorder_table

VOCAB, SEQ, LAT = 60, 20, 8


def _host_step(logits, beam_scores, done, gen_len, nb, eos, fill):
    """One iteration of _beam_search's tail, as models/hf_base.py composes it."""
    bsz = logits.shape[0] // nb
    logp = logits.float().log_softmax(-1)
    vocab = logp.shape[-1]
    frozen = torch.zeros_like(logp)
    frozen[:] = -1e9
    frozen[:, fill] = 0.0
    logp = torch.where(done[:, None], frozen, logp)
    cand = (beam_scores.view(-1, 1) + logp).view(bsz, nb * vocab)
    top_scores, top_idx = cand.topk(nb, dim=-1)
    src, tok = top_idx // vocab, (top_idx % vocab).view(-1)
    rows = (src + torch.arange(bsz)[:, None] * nb).view(-1)
    done, gen_len = done.index_select(0, rows), gen_len.index_select(0, rows)
    gen_len = gen_len + (~done).float()
    done = done | (tok == eos)
    return src.view(-1), tok, top_scores.view(-1), done, gen_len


def test_reference_reproduces_one_host_loop_step():
    g = torch.Generator().manual_seed(0)
    nb, bsz, V, eos, fill = 3, 2, 37, 5, 9
    logits = torch.randn(bsz * nb, V, generator=g) * 3
    scores = -torch.rand(bsz * nb, generator=g) * 4
    done = torch.tensor([False, True, False, False, False, True])
    gen_len = torch.tensor([3, 2, 3, 3, 1, 3])
    want = _host_step(logits, scores.view(bsz, nb), done, gen_len.float(), nb, eos, fill)
    # no ties among the leading candidates: topk's order is then the rule's
    top = (scores[:, None] + logits.log_softmax(-1)).view(bsz, -1).topk(nb + 1).values
    assert (top[:, :-1] - top[:, 1:]).min() > 1e-5
    src, tok, new, ndone, nlen, all_done = beam_select_reference(
        logits, scores, done, gen_len, nb, eos, fill)
    assert torch.equal(src.long(), want[0]) and torch.equal(tok, want[1])
    torch.testing.assert_close(new, want[2], rtol=0, atol=2e-6)
    assert torch.equal(ndone, want[3]) and torch.equal(nlen.float(), want[4])
    assert torch.equal(all_done, ndone.view(bsz, nb).all(-1))


@pytest.mark.parametrize("name", ["identical_rows", "duplicates_in_a_row"])
def test_tie_rule(name):
    x, s, done, nb, eos, fill, want_src, want_tok = tie_cases()[name]
    src, tok, *_ = beam_select_reference(x, s, done, torch.zeros(len(s), dtype=torch.int32),
                                         nb, eos, fill)
    assert src.tolist() == want_src and tok.tolist() == want_tok


def test_frozen_rows_propose_only_the_fill_token():
    nb, V, eos, fill = 3, 19, 4, 7
    x = torch.randn(nb, V, generator=torch.Generator().manual_seed(1))
    scores = torch.tensor([-1.5, -0.25, -0.75])
    done = torch.tensor([False, True, True])
    gen_len = torch.tensor([5, 2, 3], dtype=torch.int32)
    src, tok, new, ndone, nlen, all_done = beam_select_reference(
        x, scores, done, gen_len, nb, eos, fill)
    # the two frozen beams stay, best first, at unchanged score and length
    assert src.tolist()[:2] == [1, 2] and tok.tolist()[:2] == [fill, fill]
    assert new.tolist()[:2] == [-0.25, -0.75]
    assert ndone.tolist()[:2] == [True, True] and nlen.tolist()[:2] == [2, 3]
    assert src[2] == 0 and nlen[2] == 6 and not bool(all_done[0])
    # every other token of a frozen row sits at score - 1e9
    only = beam_select_reference(x[1:2].repeat(2, 1), scores[1:2].repeat(2), done[1:],
                                 gen_len[1:], 2, eos, fill)
    assert only[1].tolist() == [fill, fill] and bool(only[5][0])


def test_backtrack_follows_the_parents():
    # two steps, one group of 3: step 1's beams come from beams (2, 0, 0)
    rec_tok = torch.tensor([[10, 11, 12], [20, 21, 22]])
    rec_parent = torch.tensor([[0, 0, 0], [2, 0, 0]], dtype=torch.int32)
    assert backtrack(rec_tok, rec_parent, 3, 2).tolist() == [[12, 20], [10, 21], [10, 22]]


def test_reorder_table_picks_the_unit_by_row_size():
    even = torch.zeros(2, 4, 32, dtype=torch.bfloat16)
    ragged = torch.zeros(2, 5, 13, dtype=torch.bfloat16)
    t = reorder_table([even, ragged], [1, 2], [0, 1])
    assert t.shape == (2, 6)
    assert t[0].tolist() == [even.data_ptr(), 4, 4, 16, 1, 0]
    assert t[1].tolist()[1:] == [5, 13, 2, 2, 1]
    with pytest.raises(ValueError):
        reorder_table([even[:, :, :8]], [0], [0])


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    cfg = CausalLanguageModelConfig(
        vocab_size=VOCAB, max_seq_len=SEQ, max_latents=LAT, num_channels=24, num_heads=4,
        num_self_attention_layers=2, cross_attention_dropout=0.0,
    )
    return PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg)).eval()


def _prompt(b, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, VOCAB, (b, n), generator=g)


def _sequence_score(model, ids, n0, prefix_len, eos):
    """Sum of log-probabilities of ids[n0:] up to and including the first EOS."""
    total = 0.0
    for t in range(n0, ids.shape[0]):
        logits = model(ids[None, :t], prefix_len=prefix_len).logits[0, -1]
        total += float(logits.float().log_softmax(-1)[ids[t]])
        if eos is not None and int(ids[t]) == eos:
            break
    return total


def _decode(model, prompt, nb, new, eos):
    bm = model.backend_model
    gd = GraphedDecoder(bm, allocate_kv_cache(bm, prompt.shape[0] * nb), use_graph=False,
                        num_beams=nb, eos_token_id=eos)
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=prompt.shape[1] - 4)
        assert first.shape == (prompt.shape[0] * nb, 1)
        left = new - 1
        while left > 0 and not bool(gd.finished.all()):
            rest = gd.decode(1)
            assert rest.shape == (prompt.shape[0] * nb, 1)
            left -= 1
    return gd


@pytest.mark.parametrize("with_eos", [False, True])
def test_cpu_beam_decoder_matches_the_host_loop(model, with_eos):
    nb, new = 3, 4
    prompt = _prompt(2, 10, seed=5)
    kw = dict(input_ids=prompt, num_latents=4, max_new_tokens=new, num_beams=nb)
    free = model.generate(**kw)
    eos = None
    if with_eos:
        # a token that the free run's winning beams emit before the end: some beam
        # reaches it, and prompt 0 stops early
        eos = int(free[0, 11])
    want = model.generate(eos_token_id=eos, **kw)
    gd = _decode(model, prompt, nb, new, eos)
    toks, scores = gd.best(1.0)
    got = torch.cat([prompt, toks], dim=1)
    assert got.shape == want.shape, (got, want)
    assert torch.equal(got, want)
    if with_eos:
        assert bool(gd.finished.any())
    with torch.no_grad():
        for b in range(2):
            ref = _sequence_score(model, want[b], 10, 6, eos)
            assert abs(float(scores[b]) - ref) < 1e-4, (b, float(scores[b]), ref)
    # every beam's history is as long as the steps taken, inside the vocabulary
    hyp = gd.hypotheses()
    assert hyp.shape[0] == 2 * nb and (hyp >= 0).all() and (hyp < VOCAB).all()


def test_best_cuts_after_the_first_all_done_step_and_applies_the_penalty(model):
    prompt = _prompt(2, 10, seed=5)
    gd = _decode(model, prompt, 3, 4, None)
    full, _ = gd.best(1.0)
    assert full.shape == (2, 4)
    # what beam_select records when every beam of every prompt is done at step 1
    gd.rec_all_done[1] = True
    cut, _ = gd.best(1.0)
    assert torch.equal(cut, full[:, :2])
    gd.rec_all_done[1, 0] = False  # one prompt still live: no stop
    assert gd.best(1.0)[0].shape == (2, 4)
    # length_penalty: score / clamp(gen_len, 1) ** penalty picks the hypothesis
    gd.beam_scores.copy_(torch.tensor([-4.0, -3.0, -9.0, -1.0, -2.0, -3.0]))
    gd.gen_len.copy_(torch.tensor([4, 1, 4, 1, 4, 4], dtype=torch.int32))
    assert gd.best(0.0)[1].tolist() == [-3.0, -1.0]
    assert gd.best(1.0)[1].tolist() == [-4.0, -2.0]


def test_num_beams_1_is_the_plain_decoder(model):
    bm = model.backend_model
    gd = GraphedDecoder(bm, allocate_kv_cache(bm, 2), use_graph=False, num_beams=1)
    assert gd.num_beams == 1 and not hasattr(gd, "beam_scores")
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 18), use_graph=False, num_beams=9)
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 4), use_graph=False, num_beams=3)
