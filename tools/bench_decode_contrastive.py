"""Times generate(penalty_alpha=..., top_k=...) for a serving-style request on the
flagship CLM: 7168-token prompts, 64 new tokens, no EOS.

Usage: python tools/bench_decode_contrastive.py [--batch 8] [--top-k 4] [--new-tokens 64]
       python tools/bench_decode_contrastive.py --sim-launch [--batch 32] [--cap 1024]
Prints one JSON line; "path" says whether the request replayed the captured
decode graph or ran the host-driven loop (PERCEIVER_CONTRASTIVE_GRAPH=0 forces
the latter; run it in a process of its own for the parent's behaviour, since a
process that has served a graph request keeps that decoder's caches allocated).
--sim-launch times one contrastive_sim launch at a full history against a plain
bf16 add that moves the same bytes, alternating, in one run.
"""
import argparse
import json
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

import torch

from perceiver_amd.models.flagship import clm_flagship
from perceiver_amd.models.text.clm_hf import (
    PerceiverCausalLanguageModel,
    PerceiverCausalLanguageModelConfig,
)


def _time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def sim_launch(args, dev):
    from perceiver_amd.ops import contrastive as cs

    G, k, cap, C = args.batch, args.top_k, args.cap, args.channels
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    h = torch.randn(G * k, C, generator=g).to(dev, torch.bfloat16)
    hist = torch.randn(G, cap, C, generator=g).to(dev, torch.bfloat16)
    rnorm = cs.recip_norm(hist)
    n = torch.tensor([cap], dtype=torch.long, device=dev)
    # the sweep reads the history and its norms once; the add a + b -> c moves
    # three operands, so each holds a third of those bytes
    moved = hist.numel() * 2 + rnorm.numel() * 4
    third = moved // 3 // 2  # bf16 elements per operand
    x, y = (torch.randn(third, device=dev).bfloat16() for _ in range(2))
    out = torch.empty_like(x)
    nsplit, granule = cs.plan(G, cap, C)

    def sim():
        cs.contrastive_sim(h, hist, rnorm, n, k)

    def add():
        torch.add(x, y, out=out)

    for _ in range(20):
        sim()
        add()
    torch.cuda.synchronize()
    sims, adds = [], []
    for _ in range(args.requests):
        sims.append(_time_us(sim, 50))
        adds.append(_time_us(add, 50))
    sims.sort()
    adds.sort()
    ms, ma = sims[len(sims) // 2], adds[len(adds) // 2]
    print(json.dumps({
        "metric": "contrastive_sim_launch_us", "value": round(ms, 1), "unit": "us", "groups": G,
        "k": k, "cap": cap, "channels": C, "nsplit": nsplit, "bytes": moved,
        "us_min_max": [round(sims[0], 1), round(sims[-1], 1)], "tb_per_s": round(moved / ms / 1e6, 2),
        "bf16_add_same_bytes_us": round(ma, 1),
        "bf16_add_us_min_max": [round(adds[0], 1), round(adds[-1], 1)],
        "bf16_add_tb_per_s": round(third * 2 * 3 / ma / 1e6, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--penalty-alpha", type=float, default=0.6)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--requests", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--sim-launch", action="store_true",
                    help="time one contrastive_sim launch at --batch groups x --cap x --channels")
    ap.add_argument("--cap", type=int, default=1024)
    ap.add_argument("--channels", type=int, default=1280)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    if args.sim_launch:
        return sim_launch(args, dev)
    cfg = clm_flagship()
    torch.manual_seed(args.seed)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg))
    model = model.to(dev, torch.bfloat16).eval()
    prompt_len = cfg.max_seq_len - cfg.max_latents
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    prompts = [torch.randint(0, cfg.vocab_size, (args.batch, prompt_len), generator=g).to(dev)
               for _ in range(args.warmup + args.requests)]

    def request(i):
        return model.generate(input_ids=prompts[i], num_latents=1, max_new_tokens=args.new_tokens,
                              top_k=args.top_k, penalty_alpha=args.penalty_alpha)

    def graphed():
        return [gd for gd in getattr(model, "_graph_decoders", {}).values()
                if getattr(gd, "contrastive_k", 0)]

    def measure():
        """Median and spread of --requests requests after --warmup; one JSON line."""
        for i in range(args.warmup):
            request(i)
        torch.cuda.synchronize()
        times, produced = [], 0
        for i in range(args.requests):
            t0 = time.perf_counter()
            res = request(args.warmup + i)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            produced += args.batch * (res.shape[1] - prompt_len)
        times.sort()
        median = times[len(times) // 2]
        new_tokens = produced / args.requests / args.batch
        print(json.dumps({
            "metric": "generate_tok_per_s_clm_contrastive",
            "value": round(args.batch * new_tokens / median, 1), "unit": "tok/s",
            "batch": args.batch, "top_k": args.top_k, "penalty_alpha": args.penalty_alpha,
            "new_tokens_per_request": new_tokens, "ms_per_request_median": round(median * 1e3, 2),
            "ms_per_request_min_max": [round(times[0] * 1e3, 2), round(times[-1] * 1e3, 2)],
            "path": "graph" if graphed() else "host-loop",
        }), flush=True)

    measure()


if __name__ == "__main__":
    main()
