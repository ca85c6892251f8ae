"""CPU checks of the decode selection rules (ops/sample.py): the torch reference
of the kept set against the mask ``_select_next`` implies, its tie handling,
the kernel's host-side shape gate, and the EOS bookkeeping of the un-captured
GraphedDecoder against the host generation loop."""
import pytest
import torch

from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.hf_base import PerceiverCausalSequenceModel
from perceiver_amd.models.text.clm import CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops.sample import keep_mask_reference


def _cfg(**kw):
    base = dict(vocab_size=61, max_seq_len=48, max_latents=16, num_channels=32,
                num_heads=4, num_self_attention_layers=2, cross_attention_dropout=0.0)
    base.update(kw)
    return CausalLanguageModelConfig(**base)


def _boundary_margin(x, T, k, p):
    """Smallest |cumulative mass - p| over the sorted top-k set, in fp64."""
    sv = x.double().sort(descending=True).values
    if 0 < k < sv.numel():
        sv = sv[:k]
    w = torch.exp((sv - sv[0]) / T)
    cum = w.cumsum(0) / w.sum()
    return float((cum - p).abs().min())


def _tie_free_rows(V, T, k, p, rows=4):
    """Distinct fp32 logits whose nucleus boundary is clear of p by 1e-4, so the
    fp32 softmax of _select_next and the fp64 reference cannot disagree."""
    out, seed = [], 0
    while len(out) < rows:
        g = torch.Generator().manual_seed(1000 * V + seed)
        seed += 1
        x = torch.randn(V, generator=g) * 2.0
        if x.unique().numel() != V:
            continue
        if p is not None and _boundary_margin(x, T, k, p) < 1e-4:
            continue
        out.append(x)
    return torch.stack(out)


def _select_next_mask(logits, T, k, p, monkeypatch):
    """The kept set of _select_next: the non-zero entries of the distribution it
    hands to multinomial (the -inf positions before its softmax)."""
    seen = {}

    def fake_multinomial(probs, n, generator=None):
        seen["probs"] = probs
        return probs.argmax(-1, keepdim=True)

    monkeypatch.setattr(torch, "multinomial", fake_multinomial)
    PerceiverCausalSequenceModel._select_next(logits, True, T, k, p, None)
    return seen["probs"] > 0


@pytest.mark.parametrize("V", [61, 262])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_keep_mask_reference_matches_select_next(V, T, monkeypatch):
    for k in (0, 1, 7, V):
        for p in (None, 0.3, 0.9):
            x = _tie_free_rows(V, T, k, p)
            want = _select_next_mask(x, T, k, p, monkeypatch)
            got = keep_mask_reference(x, T, k, p)
            assert torch.equal(got, want), (V, T, k, p)
            # per-row tensors mean the same as scalars
            got_t = keep_mask_reference(x, torch.full((4,), T), torch.full((4,), k),
                                        torch.full((4,), 1.0 if p is None else p))
            assert torch.equal(got_t, want), (V, T, k, p)


def test_keep_mask_reference_keeps_ties_together():
    x = torch.full((1, 12), -3.0)
    x[0, [2, 9]] = 5.0
    x[0, [0, 4, 11]] = 3.0
    x[0, 6] = 1.0
    # the 3rd largest is one of three tied 3.0s: all of them stay
    m = keep_mask_reference(x, 1.0, 3, None)
    assert m[0].nonzero().flatten().tolist() == [0, 2, 4, 9, 11]

    w = torch.exp(x[0].double() - 5.0)
    two_top = float(w[[2, 9]].sum() / w.sum())
    one_top = two_top / 2
    # boundary inside the tied maxima: both stay (nothing is strictly above
    # them), and the 3.0s go together (the mass above them exceeds top_p)
    m = keep_mask_reference(x, 1.0, 0, (one_top + two_top) / 2)
    assert m[0].nonzero().flatten().tolist() == [2, 9]
    # boundary inside the tied 3.0s: the mass above them is within top_p, so
    # all three stay; 1.0 has more than top_p above it
    five = float(w[[0, 2, 4, 9, 11]].sum() / w.sum())
    m = keep_mask_reference(x, 1.0, 0, (two_top + five) / 2)
    assert m[0].nonzero().flatten().tolist() == [0, 2, 4, 9, 11]
    # and top-p renormalises over the top-k set
    m = keep_mask_reference(x, 1.0, 2, 0.999999)
    assert m[0].nonzero().flatten().tolist() == [2, 9]


def test_decode_select_applicable_gate():
    from perceiver_amd.ops import hip

    try:
        ext = hip.ext()
    except (ImportError, RuntimeError):
        pytest.skip("in-tree extension not built")
    for v in (1, 61, 1024, 1025, 32768):
        assert ext.decode_select_applicable(v), v
    for v in (0, 32769):
        assert not ext.decode_select_applicable(v), v


def test_uncaptured_decoder_with_eos_matches_host_loop():
    torch.manual_seed(0)
    backend_cfg = _cfg(abs_pos_emb=False)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(backend_cfg)).eval()
    backend = model.backend_model
    prompt = torch.randint(0, 61, (3, 30))
    n_new = 10

    free = model.generate(input_ids=prompt, num_latents=1, max_new_tokens=n_new,
                          static_cache=False)[:, 30:]
    # an EOS some row reaches early and (to exercise fill + cut) not as its last token
    eos = int(free[0, 2])
    pad = (eos + 1) % 61
    host = model.generate(input_ids=prompt, num_latents=1, max_new_tokens=n_new,
                          static_cache=False, eos_token_id=eos, pad_token_id=pad)[:, 30:]
    assert (host[0, 3:] == pad).all()  # the case does stop a row early

    gd = GraphedDecoder(backend, allocate_kv_cache(backend, 3), use_graph=False,
                        eos_token_id=eos, pad_token_id=pad)
    first = gd.prefill(prompt, prefix_len=29)
    # two decode calls after one prefill, as generate() chunks them
    toks = torch.cat([first, gd.decode(4), gd.decode(n_new - 5)], dim=1)
    want_done = (host == eos).any(dim=1) if host.shape[1] == n_new else None
    cut = PerceiverCausalSequenceModel._cut_at_all_done(toks, eos)
    assert torch.equal(cut, host)
    if want_done is not None:
        assert torch.equal(gd.finished, want_done)
    assert gd.finished[0]
