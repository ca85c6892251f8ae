"""Measurements of the windowed decode attention (profiles/r09_decode_attn.md), the two
arms of every comparison alternating inside one process:

- micro: one decode_attn launch against mask + flash_fwd (+ merge) at the flagship
  step's shapes (B 32, H 8, D 128), device events, median of 7 rounds of 200 launches;
- decoders: GraphedDecoder(ragged=True) at pad 0 against the standard decoder on the
  benchmark's shape, 128 graph replays after a prefill;
- end to end: generate() for a 32-row left-padded batch (pad counts spread over 0..512,
  2048-token rows, 64 new tokens) on the graph path against the host loop.

Usage: python tools/bench_decode_attn.py [--out FILE.json]
Prints one JSON line per measurement.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

import torch

from perceiver_amd.ops import hip
from perceiver_amd.ops import decode_attn as da

DEV = torch.device("cuda:0")
ext = hip.ext()
OUT = {}


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / iters  # us


def ab(fa, fb, iters=200, rounds=7):
    for _ in range(20):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(rounds):
        a.append(timed(fa, iters))
        b.append(timed(fb, iters))
    return a, b


def med(x):
    return statistics.median(x)


def micro():
    B, H, D = 32, 8, 128
    rows = []
    g = torch.Generator().manual_seed(0)
    for label, cap, live, pad_hi in [("CA", 8192, 7168, 0), ("CA", 8192, 2048, 0),
                                      ("SA", 1024, 1, 0), ("SA", 1024, 16, 0), ("SA", 1024, 512, 0),
                                      ("CA", 8192, 7168, 1024), ("CA", 8192, 2048, 1024),
                                      ("SA", 1024, 512, 1024)]:
        kb = (torch.randn(B, cap, H * D, generator=g) * 0.3).bfloat16().to(DEV)
        vb = torch.randn(B, cap, H * D, generator=g).bfloat16().to(DEV)
        k = kb.view(B, cap, H, D).transpose(1, 2)
        v = vb.view(B, cap, H, D).transpose(1, 2)
        q = (torch.randn(B, H, 1, D, generator=g) * 0.3).bfloat16().to(DEV)
        if pad_hi:
            lo = torch.linspace(0, min(pad_hi, live - 1), B).long().to(DEV)
        else:
            lo = torch.zeros(B, dtype=torch.long, device=DEV)
        hi = torch.full((1,), live - 1, dtype=torch.long, device=DEV)
        ar = torch.arange(cap, device=DEV).unsqueeze(0)
        n_live = (hi - lo + 1).clamp(min=0).sum().item()

        def arm_kernel():
            return ext.decode_attn(q, k, v, lo, hi)

        if pad_hi:
            def arm_flash():
                mask = (ar < lo[:, None]) | (ar > hi)
                return ext.flash_fwd(q, k, v, mask, False, 0.0, 0)[0]
        else:
            def arm_flash():
                mask = (ar > hi).expand(B, -1)
                return ext.flash_fwd(q, k, v, mask, False, 0.0, 0)[0]

        o1, o2 = arm_kernel(), arm_flash()
        diff = (o1.float() - o2.float()).abs().max().item()
        a, b = ab(arm_kernel, arm_flash)
        live_bytes = n_live * H * D * 2 * 2
        cap_bytes = B * cap * H * D * 2 * 2
        row = dict(layer=label, cap=cap, live=live, pad_max=pad_hi,
                   nsplit=ext.decode_attn_plan(B, H, cap, D)[0],
                   kernel_us=med(a), kernel_min=min(a), kernel_max=max(a),
                   flash_us=med(b), flash_min=min(b), flash_max=max(b),
                   kernel_TBps_live=live_bytes / med(a) / 1e6,
                   flash_TBps_live=live_bytes / med(b) / 1e6,
                   flash_TBps_cap=cap_bytes / med(b) / 1e6, max_abs_diff=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del kb, vb
    OUT["micro"] = rows


def flagship():
    from perceiver_amd.models.flagship import clm_flagship
    from perceiver_amd.models.text.clm import CausalLanguageModel
    torch.manual_seed(0)
    cfg = clm_flagship()
    return cfg, CausalLanguageModel(cfg).to(DEV).to(torch.bfloat16).eval()


def decoders(cfg, model):
    """Standard against ragged decoder at pad 0 on the benchmark's shape."""
    from perceiver_amd.core.cache import allocate_kv_cache
    from perceiver_amd.core.graph_decode import GraphedDecoder
    B = 32
    n = cfg.max_seq_len - cfg.max_latents
    g = torch.Generator().manual_seed(0)
    prompt = torch.randint(0, cfg.vocab_size, (B, n), generator=g).to(DEV)
    gds = {}
    for name, kw in (("standard", {}), ("ragged", {"ragged": True})):
        gd = GraphedDecoder(model, allocate_kv_cache(model, B, device=DEV, dtype=torch.bfloat16), **kw)
        with torch.no_grad():
            gd.prefill(prompt, prefix_len=n - 1)
            gd.decode(8)
        gds[name] = gd
    res = {k: [] for k in gds}
    toks = {}
    for r in range(5):
        for name, gd in gds.items():
            with torch.no_grad():
                gd.prefill(prompt, prefix_len=n - 1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks[name] = gd.decode(128)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            res[name].append(B * 128 / dt)
    agree = (toks["standard"] == toks["ragged"]).float().mean().item()
    OUT["decoders_pad0"] = {k: dict(tok_s_median=med(v), tok_s_min=min(v), tok_s_max=max(v))
                            for k, v in res.items()}
    OUT["decoders_pad0"]["token_agreement"] = agree
    print(json.dumps(OUT["decoders_pad0"]), flush=True)
    del gds


def end_to_end(cfg, model):
    from perceiver_amd.models.text.clm_hf import (PerceiverCausalLanguageModel,
                                                  PerceiverCausalLanguageModelConfig)
    from perceiver_amd.core import graph_decode
    hf = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg))
    hf.backend_model = model
    hf.eval()
    B, n, new = 32, 2048, 64
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(1, cfg.vocab_size, (B, n), generator=g)
    mask = torch.ones(B, n, dtype=torch.long)
    pads = torch.linspace(0, 512, B).long().tolist()
    for b, p in enumerate(pads):
        prompt[b, :p] = 0
        mask[b, :p] = 0
    prompt, mask = prompt.to(DEV), mask.to(DEV)
    kw = dict(input_ids=prompt, attention_mask=mask, num_latents=512, max_new_tokens=new)
    inner = graph_decode.graph_route

    def run(graph):
        # the host arm refuses EVERY request, padded or not: hf_base looks the gate up per call
        graph_decode.graph_route = inner if graph else (lambda *a, **k: None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = hf.generate(**kw)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    run(True)  # capture
    res = {"graph": [], "host": []}
    outs = {}
    for r in range(3):
        for name in ("graph", "host"):
            outs[name], dt = run(name == "graph")
            res[name].append(B * new / dt)
    graph_decode.graph_route = inner
    agree = (outs["graph"][:, n:] == outs["host"][:, n:]).float().mean().item()
    OUT["end_to_end"] = {k: dict(tok_s_median=med(v), tok_s_min=min(v), tok_s_max=max(v))
                         for k, v in res.items()}
    OUT["end_to_end"]["token_agreement"] = agree
    OUT["end_to_end"]["ragged_decoders"] = len([g_ for g_ in hf._graph_decoders.values() if g_.ragged])
    print(json.dumps(OUT["end_to_end"]), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write every result to this JSON file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    micro()
    cfg, model = flagship()
    decoders(cfg, model)
    end_to_end(cfg, model)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(OUT, f, indent=1)
