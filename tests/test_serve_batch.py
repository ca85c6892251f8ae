"""Serving endpoint /generate_batch: prompts of different lengths, left-padded
into one generate() call, must read like the same prompts served one by one."""
import pytest
import torch
from fastapi.testclient import TestClient
from transformers import PerceiverTokenizer

from perceiver_amd.models.text.clm import CausalLanguageModelConfig
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)
from perceiver_amd.serve import create_app

PROMPTS = ["a quick brown fox jumps over", "hello world", "the lazy dog sleeps"]


@pytest.fixture(scope="module")
def served():
    torch.manual_seed(0)
    cfg = CausalLanguageModelConfig(vocab_size=262, max_seq_len=128, max_latents=32,
                                    num_channels=32, num_heads=4,
                                    num_self_attention_layers=2,
                                    cross_attention_dropout=0.0)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg)).eval()
    return model, TestClient(create_app(model, PerceiverTokenizer()))


def test_batch_equals_the_prompts_served_alone(served, monkeypatch):
    model, client = served
    calls = []
    real = model.generate

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(model, "generate", spy)
    # 64 latents requested: clamped to the shortest prompt (11 byte tokens)
    req = {"prompts": PROMPTS, "max_new_tokens": 8, "num_latents": 64}
    r = client.post("/generate_batch", json=req)
    assert r.status_code == 200, r.text
    assert len(calls) == 1  # one generate() call for the batch
    assert calls[0]["num_latents"] == len("hello world")
    mask = calls[0]["attention_mask"]
    assert mask.shape == (3, len(PROMPTS[0])) and mask.sum(1).tolist() == [len(p) for p in PROMPTS]
    assert bool(mask[:, -1].all())  # left-padded
    results = r.json()["results"]
    assert len(results) == 3
    for prompt, got in zip(PROMPTS, results):
        alone = client.post("/generate", json={"prompt": prompt, "max_new_tokens": 8,
                                               "num_latents": calls[0]["num_latents"]})
        assert alone.status_code == 200
        assert got["text"] == alone.json()["text"], prompt
        assert got["prompt_tokens"] == len(prompt)  # byte tokenizer
        assert got["generated_tokens"] == 8


def test_single_prompt_batch(served):
    _, client = served
    r = client.post("/generate_batch", json={"prompts": ["hello"], "max_new_tokens": 4,
                                             "num_latents": 2})
    alone = client.post("/generate", json={"prompt": "hello", "max_new_tokens": 4,
                                           "num_latents": 2})
    assert r.status_code == 200
    assert r.json()["results"][0] == alone.json()


def test_empty_prompt_is_400(served):
    _, client = served
    r = client.post("/generate_batch", json={"prompts": ["fine", ""], "max_new_tokens": 4})
    assert r.status_code == 400


def test_prompt_count_limits_are_422(served):
    _, client = served
    assert client.post("/generate_batch", json={"prompts": ["x"] * 65}).status_code == 422
    assert client.post("/generate_batch", json={"prompts": []}).status_code == 422
