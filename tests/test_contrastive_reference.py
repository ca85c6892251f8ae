"""Contrastive search rules in plain torch (ops/contrastive.py) against the fp64
oracle, the fp32 arithmetic of the kernels against the derived bounds at the
GPU cases' inputs, and the contrastive GraphedDecoder's eager step on the CPU
against generate()'s host loop."""
import pytest
import torch

import _contrastive_ref as ref

from perceiver_amd.core import graph_decode
from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.hf_base import PerceiverCausalSequenceModel
from perceiver_amd.models.text.clm import CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops import contrastive as cs

VOCAB, K, ALPHA, NEW, PROMPT, LATENTS = 61, 4, 0.6, 8, 10, 4


# ------------------------------------------------------- rules vs the oracle

def test_equal_logits_give_the_lowest_index_first():
    x = torch.full((1, 23), -3.0)
    x[0, [17, 4, 9]] = 2.0
    x[0, 20] = 2.5
    tok, prob = cs.propose_reference(x, 3)
    want_tok, want_p = ref.propose64(x[0], 3)
    assert tok[0].tolist() == want_tok == [20, 4, 9]
    assert (prob[0].double() - torch.tensor(want_p)).abs().max() <= ref.prob_tolerance(x)
    # NaN compares largest
    x[0, 11] = float("nan")
    assert cs.propose_reference(x, 2)[0][0].tolist() == ref.propose64(x[0], 2)[0] == [11, 20]


def _group(seed=0, C=32, k=4, cap=12, n=7):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(k, C, generator=g)
    hist = torch.randn(1, cap, C, generator=g)
    rnorm = cs.recip_norm(hist)
    tok = torch.arange(k) + 5
    return h, hist, rnorm, n, tok


def test_equal_scores_give_the_lowest_j():
    h, hist, rnorm, n, tok = _group()
    h[2] = h[1]                       # candidates 1 and 2: same state, same probability
    hist[0, :n] -= 2 * h[1]           # and far from the history: the best score, twice
    prob = torch.tensor([0.2, 0.3, 0.3, 0.1])
    done = torch.zeros(1, dtype=torch.bool)
    sel, emitted, ndone, sim, score = cs.contrastive_reference(
        h, hist, rnorm, n, tok, prob, done, ALPHA, -1, 0, 4)
    want = ref.step64(h, hist[0], n, tok, prob, False, ALPHA, -1, 0)
    assert float(score[0, 1]) == float(score[0, 2]) == float(score.max())
    assert int(sel) == want[0] == 1 and int(emitted) == want[1] == 6
    # a NaN score compares largest, the lowest j among several
    h[3, 0] = float("nan")
    sel = cs.contrastive_reference(h, hist, rnorm, n, tok, prob, done, ALPHA, -1, 0, 4)[0]
    assert int(sel) == ref.step64(h, hist[0], n, tok, prob, False, ALPHA, -1, 0)[0] == 3


def test_done_and_fill_bookkeeping():
    h, hist, rnorm, n, tok = _group(seed=1)
    h, hist, rnorm = h.repeat(2, 1), hist.repeat(2, 1, 1), rnorm.repeat(2, 1)
    prob = torch.tensor([0.4, 0.3, 0.2, 0.1]).repeat(2)
    toks = torch.cat([tok, tok])
    free = cs.contrastive_reference(h, hist, rnorm, n, toks, prob, torch.zeros(2, dtype=torch.bool),
                                    ALPHA, -1, 0, 4)
    eos = int(free[1][0])
    sel, emitted, done, *_ = cs.contrastive_reference(
        h, hist, rnorm, n, toks, prob, torch.tensor([False, True]), ALPHA, eos, 3, 4)
    assert emitted.tolist() == [eos, 3] and done.tolist() == [True, True]
    assert sel.tolist() == free[0].tolist()  # a done group keeps its real candidate
    # an empty history scores 0 similarity: the one deviation from amax
    sim = cs.contrastive_reference(h, hist, rnorm, 0, toks, prob, torch.zeros(2, dtype=torch.bool),
                                   ALPHA, -1, 0, 4)[3]
    assert sim.abs().max() == 0 and ref.sim64(h[:4], hist[0], 0).abs().max() == 0


# ---------------------------- the kernels' arithmetic at the GPU cases' inputs

def _kernel_arithmetic(h, hist, rnorm, k, *, normalise=True):
    """fp32 ``dot * r_t * r_j`` of every (group, row, candidate): (G, cap, k)."""
    G, cap, C = hist.shape
    dots = torch.einsum("gtc,gkc->gtk", hist.float(), h.float().view(G, k, C))
    v = dots * rnorm[:, :, None]
    if normalise:
        v = v * cs.recip_norm(h).view(G, 1, k)
    return v


def _sim_at(v, n, reduce="max", first=0):
    rows = v[:, first:n]
    return rows.amin(1) if reduce == "min" else rows.amax(1)


@pytest.mark.parametrize("cap", ref.SIM_CAPS)
@pytest.mark.parametrize("C", ref.SIM_CHANNELS)
def test_fp32_arithmetic_stays_inside_the_bound(C, cap):
    worst = 0.0
    for k in ref.SIM_K:
        h, hist, rnorm = ref.sim_inputs(C, k, cap)
        want = ref.sim_oracle_all(h, hist, k)
        got = _kernel_arithmetic(h, hist, rnorm, k).double()
        for n in ref.hist_lens(ref.SIM_GROUPS, cap, C):
            err = float((_sim_at(got, n) - _sim_at(want, n)).abs().max())
            worst = max(worst, err / ref.sim_bound(C))
        # the reference states the same arithmetic
        n = ref.hist_lens(ref.SIM_GROUPS, cap, C)[-2]
        sim = cs.sim_reference(h, hist, rnorm, n, k).double()
        assert float((sim - _sim_at(want, n)).abs().max()) <= ref.sim_bound(C)
    print(f"C={C} cap={cap}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0


def _planted(C=32, k=4, cap=16, n=9):
    """Candidate 0's nearest row is row 0, candidate 1's is row n - 1 (the last
    live one) and row n, just past the history, is a decoy that matches
    candidate 2. The candidates are far from unit length."""
    g = torch.Generator().manual_seed(7)
    h = (torch.randn(k, C, generator=g) * 5).bfloat16()
    hist = torch.randn(1, cap, C, generator=g)
    hist[0, 0] = h[0].float() * 1.5
    hist[0, n - 1] = h[1].float() * 0.7
    hist[0, n] = h[2].float() * 2.0
    hist = hist.bfloat16()
    return h, hist, cs.recip_norm(hist), n


def test_mutants_of_the_similarity_leave_the_bound():
    h, hist, rnorm, n = _planted()
    k, C = h.shape
    want = ref.sim64(h, hist[0], n)
    bound = ref.sim_bound(C)
    v = _kernel_arithmetic(h, hist, rnorm, k).double()
    assert float((_sim_at(v, n)[0] - want).abs().max()) <= bound
    mutants = {
        "min instead of max": _sim_at(v, n, reduce="min"),
        "history starts at row 1": _sim_at(v, n, first=1),
        "history ends one row early": _sim_at(v, n - 1),
        "history ends one row late": _sim_at(v, n + 1),
        "candidate not normalised": _sim_at(
            _kernel_arithmetic(h, hist, rnorm, k, normalise=False).double(), n),
    }
    for name, got in mutants.items():
        err = float((got[0] - want).abs().max())
        assert err >= 10 * bound, (name, err, bound)


def test_mutants_of_the_score_change_the_selection():
    h, hist, rnorm, n = _planted()
    k, C = h.shape
    tok = torch.arange(k)
    # a logit row whose top-k share of the mass is far from 1: renormalising
    # over the top k moves every probability
    x = torch.zeros(1, VOCAB)
    x[0, :k] = torch.tensor([1.0, 1.05, 0.9, 0.95])
    cand, prob = cs.propose_reference(x, k)
    want_tok, want_p = ref.propose64(x[0], k)
    assert cand[0].tolist() == want_tok
    tol = ref.prob_tolerance(x)
    assert float((prob[0].double() - torch.tensor(want_p)).abs().max()) <= tol
    renormalised = x[0, cand[0]].softmax(-1).double()
    assert float((renormalised - torch.tensor(want_p)).abs().max()) >= 10 * tol

    prob = prob[0][cand[0].argsort()]  # candidate j is token j
    done = torch.zeros(1, dtype=torch.bool)
    sel, *_, sim, score = cs.contrastive_reference(h, hist, rnorm, n, tok, prob, done, ALPHA,
                                                   -1, 0, k)
    want = ref.step64(h, hist[0], n, tok, prob, False, ALPHA, -1, 0)
    assert int(sel) == want[0]
    gap = want[4].sort(descending=True).values
    assert float(gap[0] - gap[1]) >= 64 * ref.score_tolerance(ALPHA, C, x)
    plus = (1.0 - ALPHA) * prob + ALPHA * sim[0]
    assert int(plus.argmax()) != want[0]


# --------------------------------------------- the CPU decoder vs the host loop

def _hf_model(seed):
    torch.manual_seed(seed)
    cfg = CausalLanguageModelConfig(
        vocab_size=VOCAB, max_seq_len=40, max_latents=16, num_channels=32, num_heads=4,
        num_self_attention_layers=2, cross_attention_dropout=0.0)
    return PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg)).eval()


def _decoder(model, bsz, **kw):
    bm = model.backend_model
    return GraphedDecoder(bm, allocate_kv_cache(bm, bsz * K), use_graph=False, contrastive_k=K,
                          penalty_alpha=ALPHA, **kw)


def _assert_group_rows_identical(gd):
    """The invariant: the k rows of a group hold bit-identical cache rows [0, len)."""
    for buf, ci in zip(gd._reorder_bufs, gd._reorder_counter):
        n = int(gd.counters[ci])
        v = buf.view(gd.groups, gd.contrastive_k, *buf.shape[1:])[:, :, :n]
        assert torch.equal(v, v[:, :1].expand_as(v))


def _decode(model, prompt, eos=None, look=None):
    """Prefill and NEW steps, one at a time; ``look(gd)`` after every step."""
    gd = _decoder(model, prompt.shape[0], eos_token_id=eos)
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=PROMPT - LATENTS)
        assert first.shape == (prompt.shape[0], K)
        _assert_group_rows_identical(gd)
        cols = []
        for _ in range(NEW):
            cols.append(gd.decode(1))
            assert cols[-1].shape == (prompt.shape[0], 1)
            _assert_group_rows_identical(gd)
            if look is not None:
                look(gd)
    return gd, torch.cat(cols, dim=1)


@pytest.fixture(scope="module")
def clear_gap_run():
    """The first seed whose fp64 score gap between the best and the second
    candidate is >= 1e-4 at every step, with the decoder's free run on it. The
    oracle scores every step from the very inputs the decoder's step saw."""
    inner = cs.contrastive_reference
    for seed in range(20):
        model = _hf_model(seed)
        prompt = torch.randint(0, VOCAB, (2, PROMPT), generator=torch.Generator().manual_seed(seed))
        gaps, moved = [], []

        spy = ref.oracle_spy(inner, gaps, moved)
        graph_decode._contrastive.contrastive_reference = spy
        try:
            gd, toks = _decode(model, prompt)
        finally:
            graph_decode._contrastive.contrastive_reference = inner
        if min(gaps) >= 1e-4:
            assert len(gaps) == 2 * NEW and any(moved)
            return model, prompt, toks
    raise AssertionError("no seed gives a clear gap at every step")


@pytest.mark.parametrize("with_eos", [False, True])
def test_cpu_contrastive_decoder_matches_the_host_loop(clear_gap_run, with_eos):
    model, prompt, free = clear_gap_run
    kw = dict(input_ids=prompt, num_latents=LATENTS, max_new_tokens=NEW, top_k=K,
              penalty_alpha=ALPHA)
    eos = None
    if with_eos:
        eos = int(free[0, 2])  # seen to occur: prompt 0 stops early
    want = model.generate(eos_token_id=eos, **kw)
    gd, toks = _decode(model, prompt, eos=eos)
    if with_eos:
        assert bool(gd.finished[0]) and gd.finished.shape == (2,)
        # after EOS only the fill id (EOS itself without a pad id) follows
        assert (toks[0, 2:] == eos).all()
        toks = PerceiverCausalSequenceModel._cut_at_all_done(toks, eos)
    else:
        assert torch.equal(toks, free)
    got = torch.cat([prompt, toks], dim=1)
    assert got.shape == want.shape, (got, want)
    assert torch.equal(got, want)
    assert (toks >= 0).all() and (toks < VOCAB).all()


def test_set_sampling_rewrites_alpha_eos_and_fill(clear_gap_run):
    model, prompt, free = clear_gap_run
    gd = _decoder(model, 2)
    gd.set_sampling(penalty_alpha=0.25, eos_token_id=7, pad_token_id=9)
    assert float(gd.alpha) == 0.25 and gd.eos_fill.tolist() == [7, 9]
    # a tiny alpha is greedy decoding
    gd.set_sampling(penalty_alpha=1e-6, eos_token_id=None, pad_token_id=None)
    with torch.no_grad():
        gd.prefill(prompt, prefix_len=PROMPT - LATENTS)
        toks = gd.decode(NEW)
    greedy = model.generate(input_ids=prompt, num_latents=LATENTS, max_new_tokens=NEW)
    assert torch.equal(toks, greedy[:, PROMPT:])


def test_contrastive_decoder_refuses_beams_padding_and_bad_k(clear_gap_run):
    bm = clear_gap_run[0].backend_model
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 8), use_graph=False, contrastive_k=4, ragged=True)
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 8), use_graph=False, contrastive_k=4, num_beams=2)
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 18), use_graph=False, contrastive_k=9)
    with pytest.raises(ValueError):
        GraphedDecoder(bm, allocate_kv_cache(bm, 7), use_graph=False, contrastive_k=3)
    gd = GraphedDecoder(bm, allocate_kv_cache(bm, 2), use_graph=False)
    assert gd.contrastive_k == 0 and not hasattr(gd, "hist")


def test_policy_keys_on_k_and_passes_the_keyword_only_when_set(clear_gap_run):
    import types
    bm, owner, built = clear_gap_run[0].backend_model, types.SimpleNamespace(), []

    def make(m, caches, **kw):
        built.append(kw)
        return object()

    route = graph_decode.GraphRoute(8, 2048, ragged=False, baked=False)
    a = graph_decode.decoder_for(owner, bm, route, make=make, contrastive_k=4)
    b = graph_decode.decoder_for(owner, bm, route, make=make, contrastive_k=2)
    assert a is not b and built[0]["contrastive_k"] == 4 and built[1]["contrastive_k"] == 2
    assert graph_decode.decoder_for(owner, bm, route, make=make, contrastive_k=4) is a
    graph_decode.decoder_for(owner, bm, route, make=make)
    assert "contrastive_k" not in built[-1] and len(built) == 3
    # off the GPU no request is routed to a graph
    assert graph_decode.graph_route(bm, 2, 10, 6, 8, contrastive_k=4) is None
    assert cs.in_range(61, 4, 32) and not cs.in_range(61, 9, 32) and not cs.in_range(61, 4, 36)
    assert not cs.in_range(3, 4, 32) and cs.in_range(32768, 8, 1280)
    assert cs.in_range(61, 8, ref.MAX_CHANNELS) and not cs.in_range(61, 8, ref.MAX_CHANNELS + 8)
