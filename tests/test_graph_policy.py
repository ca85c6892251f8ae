"""CPU checks of the request policy of the captured-graph decode path
(core/graph_decode.py): the left-pad predicate, the capacity bucket, the shape
half of the gate and the decoder lookup. The device half of the gate needs a
GPU and is covered by the tests/test_gpu_graph_*.py files."""
import functools
import types

import pytest
import torch

from perceiver_amd.core import graph_decode as gd
from perceiver_amd.models.text.clm import CausalLanguageModel, CausalLanguageModelConfig

V = 61


@functools.lru_cache(maxsize=None)
def _model():
    torch.manual_seed(0)
    return CausalLanguageModel(CausalLanguageModelConfig(
        vocab_size=V, max_seq_len=64, max_latents=16, num_channels=32, num_heads=4,
        num_self_attention_layers=1, cross_attention_dropout=0.0)).eval()


def _mask(*rows):
    return torch.tensor([[int(c) for c in r] for r in rows])


@pytest.mark.parametrize("rows,want", [
    (("00011111", "11111111", "00000001"), True),
    (("11111111",) * 3, True),
    (("00011111", "11111000", "11111111"), False),  # right padding
    (("00011111", "11101111", "11111111"), False),  # a hole
    (("00011111", "00000000", "11111111"), False),  # an all-zero row
    (("00011111", "11111111", "00111110"), False),  # a row ending in 0
], ids=["left", "ones", "right", "hole", "dead_row", "ends_in_0"])
def test_left_padded(rows, want):
    mask = _mask(*rows)
    assert mask.shape == (3, 8)
    assert gd.left_padded(mask) is want
    assert gd.left_padded(mask.bool()) is want


@pytest.mark.parametrize("need,max_seq_len,want", [
    (1, 8192, 2048), (2048, 8192, 2048), (2049, 8192, 4096), (4097, 8192, 8192),
    (1, 3000, 2048), (2048, 3000, 2048), (2049, 3000, 3000), (4097, 3000, 3000),
])
def test_capacity_bucket(need, max_seq_len, want):
    assert gd.capacity_bucket(need, max_seq_len) == want


@pytest.mark.parametrize("seq_len,prefix_len,new,eos,want", [
    (30, 23, 2, None, False),   # the capture alone takes 2 steps after the prefill token
    (30, 23, 3, None, True),
    (30, 23, 9, None, True),    # latents + new = 16
    (30, 23, 10, None, False),  # 17: the schedule would grow the prefix
    (61, 60, 3, None, True),    # seq_len + new = 64
    (62, 60, 3, None, False),   # 65: the window would slide
    (30, 23, 3, V - 1, True),
    (30, 23, 3, V, False),      # the step would embed an id outside the vocabulary
])
def test_shape_half_of_the_gate(seq_len, prefix_len, new, eos, want):
    model = _model()
    assert (model.max_latents, model.max_seq_len) == (16, 64)
    assert gd.fits_graph(model, seq_len, prefix_len, new, eos_token_id=eos) is want
    assert gd.fits_graph(model, seq_len, prefix_len, new, pad_token_id=eos) is want
    # off the GPU no request is routed to a graph, whatever its shape
    assert gd.graph_route(model, 2, seq_len, prefix_len, new, eos_token_id=eos) is None


def test_decoder_lookup_evicts_the_oldest_of_two():
    model, owner, built = _model(), types.SimpleNamespace(), []

    def make(m, caches, **kw):
        built.append(caches[0].k_buf.shape[:2])  # (batch, capacity clamped to max_seq_len)
        return object()

    def lookup(batch, **kw):
        route = gd.GraphRoute(batch, 2048, ragged=False, baked=False)
        return gd.decoder_for(owner, model, route, make=make, **kw)

    a, b = lookup(1), lookup(2)
    assert list(owner._graph_decoders.values()) == [a, b] and built == [(1, 64), (2, 64)]
    # a repeated key builds nothing; sampling parameters that are not baked in are no key
    assert lookup(1) is a and lookup(2, do_sample=True, top_k=5) is b and len(built) == 2
    c = lookup(3)
    assert list(owner._graph_decoders.values()) == [b, c] and len(built) == 3
    assert lookup(1) is not a  # evicted, first in first out: built again, b goes
    assert list(owner._graph_decoders.values())[0] is c and len(built) == 4


def test_decoder_key_separates_storage_beams_padding_and_baked_sampling():
    model, owner, built = _model(), types.SimpleNamespace(), []

    def make(m, caches, **kw):
        built.append(kw)
        return object()

    def lookup(route, **kw):
        return gd.decoder_for(owner, model, route, make=make, **kw)

    plain = gd.GraphRoute(2, 2048, ragged=False, baked=False)
    first = lookup(plain)
    keys = list(owner._graph_decoders)
    p = next(model.parameters())
    assert p.data_ptr() in keys[0]
    # reallocated parameter storage (what model.to() does) is a new key
    old = p.data
    p.data = old.clone()
    try:
        assert lookup(plain) is not first
        assert p.data_ptr() in list(owner._graph_decoders)[-1] and len(built) == 2
    finally:
        p.data = old
    assert lookup(plain) is first and len(built) == 2
    for route, kw in ((plain._replace(ragged=True), {}),
                      (plain._replace(batch=6), {"num_beams": 3}),
                      (plain._replace(bucket=4096), {}),
                      (plain._replace(baked=True), {"do_sample": True, "top_k": 5}),
                      (plain._replace(baked=True), {"do_sample": True, "top_k": 6})):
        n = len(built)
        fresh = lookup(route, **kw)
        assert len(built) == n + 1 and lookup(route, **kw) is fresh and len(built) == n + 1
    assert built[-1] == dict(do_sample=True, temperature=1.0, top_k=6, num_beams=1, ragged=False)
