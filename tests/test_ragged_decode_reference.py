"""CPU (fp32) checks of GraphedDecoder(ragged=True): the un-captured step over
per-row key windows against the host generation loop with a left-padded
attention mask, each row against its unpadded self, and the mask validation."""
import functools

import pytest
import torch

from perceiver_amd.core.cache import allocate_kv_cache
from perceiver_amd.core.graph_decode import GraphedDecoder
from perceiver_amd.models.text.clm import CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.ops.sample import keep_mask_reference

V, N, LATENTS, STEPS = 61, 30, 7, 8
PREFIX = N - LATENTS
PADS = [0, 4, 11]


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    cfg = CausalLanguageModelConfig(
        vocab_size=V, max_seq_len=48, max_latents=16, num_channels=32, num_heads=4,
        num_self_attention_layers=2, cross_attention_dropout=0.0, abs_pos_emb=False)
    return PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg)).eval()


def _batch(pads, seed=1):
    g = torch.Generator().manual_seed(seed)
    prompt = torch.randint(1, V, (len(pads), N), generator=g)
    mask = torch.ones(len(pads), N, dtype=torch.long)
    for b, p in enumerate(pads):
        prompt[b, :p] = 0
        mask[b, :p] = 0
    return prompt, mask


def _decode_with_logits(gd, first, steps):
    """Tokens (B, 1 + steps) and the logits (steps, B, V) behind tokens 1.."""
    toks, logits = [first], []
    for _ in range(steps):
        toks.append(gd.decode(1))
        logits.append(gd.last_logits[:, -1].clone())
    return torch.cat(toks, dim=1), torch.stack(logits)


def _ragged(pads, **kw):
    backend = _model().backend_model
    prompt, mask = _batch(pads)
    gd = GraphedDecoder(backend, allocate_kv_cache(backend, len(pads)), use_graph=False,
                        ragged=True, **kw)
    return gd, prompt, mask


@pytest.mark.parametrize("pads", [PADS, [0, 4, PREFIX + 2]],
                         ids=["pads_in_prefix", "pad_count_above_prefix_len"])
def test_greedy_equals_host_loop(pads):
    gd, prompt, mask = _ragged(pads)
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=PREFIX, attention_mask=mask)
        toks = torch.cat([first, gd.decode(STEPS)], dim=1)
        host = _model().generate(input_ids=prompt, attention_mask=mask, num_latents=LATENTS,
                                 max_new_tokens=STEPS + 1, static_cache=True)
    assert torch.equal(gd.shift, torch.tensor(pads))
    assert torch.equal(host[:, :N], prompt)
    assert torch.equal(toks, host[:, N:])


def test_seeded_top_k_sampling_follows_host_loop_rules():
    """The decoder's draws are its own (Gumbel-max), so the sampled stream is
    checked teacher-forced: fed the decoder's tokens, the host-driven cached
    forward with the padded mask must imply the same kept set at every step
    (keep_mask_reference), and every drawn token must lie in it."""
    top_k, T = 5, 1.3
    gd, prompt, mask = _ragged(PADS, do_sample=True, temperature=T, top_k=top_k)
    backend = _model().backend_model
    with torch.no_grad():
        first = gd.prefill(prompt, prefix_len=PREFIX, attention_mask=mask,
                           generator=torch.Generator().manual_seed(5))
        toks, logits = _decode_with_logits(gd, first, STEPS)
        gd.prefill(prompt, prefix_len=PREFIX, attention_mask=mask,
                   generator=torch.Generator().manual_seed(5))
        again = gd.decode(STEPS)
        assert torch.equal(again, toks[:, 1:])  # equal seeds, equal samples

        kv = allocate_kv_cache(backend, len(PADS))
        am = mask.clone()
        out = backend(prompt, prefix_len=PREFIX, pad_mask=am == 0, kv_cache=kv)
        keep = keep_mask_reference(out.logits[:, -1], T, top_k, None)
        assert keep.gather(1, toks[:, :1]).all()
        for i in range(STEPS):
            am = torch.cat([am, torch.ones(len(PADS), 1, dtype=am.dtype)], dim=1)
            out = backend(toks[:, i:i + 1], prefix_len=0, pad_mask=am == 0, kv_cache=kv)
            host_logits = out.logits[:, -1]
            torch.testing.assert_close(logits[i], host_logits, rtol=1e-4, atol=1e-5)
            keep = keep_mask_reference(host_logits, T, top_k, None)
            assert torch.equal(keep, keep_mask_reference(logits[i], T, top_k, None)), i
            assert keep.gather(1, toks[:, i + 1:i + 2]).all(), i
    assert toks.unique().numel() > 3  # it does sample


def _alone(prompt_row, prefix_len):
    """Tokens and logits of one unpadded prompt in a standard decoder of batch 1."""
    backend = _model().backend_model
    gd = GraphedDecoder(backend, allocate_kv_cache(backend, 1), use_graph=False)
    first = gd.prefill(prompt_row[None], prefix_len=prefix_len)
    return _decode_with_logits(gd, first, STEPS)


def test_each_row_equals_its_unpadded_self():
    backend = _model().backend_model
    with torch.no_grad():
        # the yardstick: the same comparison between two unpadded batch sizes
        full, _ = _batch([0, 0, 0], seed=2)
        gd3 = GraphedDecoder(backend, allocate_kv_cache(backend, 3), use_graph=False)
        t3, l3 = _decode_with_logits(gd3, gd3.prefill(full, prefix_len=PREFIX), STEPS)
        noise = 0.0
        for b in range(3):
            t1, l1 = _alone(full[b], PREFIX)
            assert torch.equal(t1[0], t3[b])
            noise = max(noise, float((l1[:, 0] - l3[:, b]).abs().max()))
        tol = max(4.0 * noise, 1e-5)

        gd, prompt, mask = _ragged(PADS)
        toks, logits = _decode_with_logits(
            gd, gd.prefill(prompt, prefix_len=PREFIX, attention_mask=mask), STEPS)

        # the row without padding against the same prompt in an unpadded decoder
        gdu = GraphedDecoder(backend, allocate_kv_cache(backend, 1), use_graph=False)
        tu = torch.cat([gdu.prefill(prompt[:1], prefix_len=PREFIX), gdu.decode(STEPS)], dim=1)
        assert torch.equal(tu[0], toks[0])

        worst = 0.0
        for b, pad in enumerate(PADS):
            t1, l1 = _alone(prompt[b, pad:], PREFIX - pad)
            assert torch.equal(t1[0], toks[b]), b
            worst = max(worst, float((l1[:, 0] - logits[:, b]).abs().max()))
    print(f"padded row vs unpadded self: max |dlogit| {worst:.3e}; batch-size noise "
          f"{noise:.3e}, tolerance {tol:.3e}")
    assert worst <= tol


def test_invalid_masks_and_beams_raise():
    gd, prompt, mask = _ragged(PADS)
    right = torch.ones_like(mask)
    right[1, -3:] = 0
    holes = mask.clone()
    holes[2, 20] = 0
    dead = mask.clone()
    dead[1] = 0
    for bad in (right, holes, dead):
        with pytest.raises(ValueError, match="left-padded"):
            gd.prefill(prompt, prefix_len=PREFIX, attention_mask=bad)
    backend = _model().backend_model
    with pytest.raises(ValueError, match="ragged"):
        GraphedDecoder(backend, allocate_kv_cache(backend, 4), use_graph=False, ragged=True,
                       num_beams=2)
    # a standard decoder does not take a padded mask
    std = GraphedDecoder(backend, allocate_kv_cache(backend, 3), use_graph=False)
    with pytest.raises(ValueError, match="ragged"):
        std.prefill(prompt, prefix_len=PREFIX, attention_mask=mask)
    # and a ragged decoder still serves an unpadded request
    with torch.no_grad():
        a = gd.prefill(prompt, prefix_len=PREFIX)
        b = std.prefill(prompt, prefix_len=PREFIX)
    assert torch.equal(a, b) and int(gd.shift.sum()) == 0
