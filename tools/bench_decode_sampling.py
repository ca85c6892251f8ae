"""Times generate() for a serving-style request on the flagship CLM: nucleus
sampling with top-k, a seed and an EOS id the random-weight model rarely emits.

Usage: python tools/bench_decode_sampling.py [--batch 32] [--new-tokens 64]
Prints one JSON line; "path" says whether the request replayed the captured
decode graph or ran the host-driven loop.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--requests", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--greedy", action="store_true", help="greedy request without EOS instead")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    cfg = clm_flagship()
    torch.manual_seed(args.seed)
    model = PerceiverCausalLanguageModel(PerceiverCausalLanguageModelConfig(cfg))
    model = model.to(dev, torch.bfloat16).eval()
    prompt_len = cfg.max_seq_len - cfg.max_latents
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    prompt = torch.randint(0, cfg.vocab_size, (args.batch, prompt_len), generator=g).to(dev)

    # the rarest next token after the prompt: far outside any top-40 set
    with torch.no_grad():
        out = model.backend_model(prompt, prefix_len=prompt_len - 1)
    eos = int(out.logits[:, -1].float().mean(0).argmin())
    del out

    kw = dict(input_ids=prompt, num_latents=1, max_new_tokens=args.new_tokens)
    if not args.greedy:
        kw.update(do_sample=True, top_p=0.9, top_k=40, eos_token_id=eos)

    def request(i):
        gen = None if args.greedy else torch.Generator(device=dev).manual_seed(args.seed + i)
        return model.generate(generator=gen, **kw)

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
        "metric": "generate_tok_per_s_clm_nucleus_eos" if not args.greedy
        else "generate_tok_per_s_clm_greedy",
        "value": round(args.batch * new_tokens / median, 1), "unit": "tok/s",
        "batch": args.batch, "new_tokens_per_request": new_tokens, "eos_token_id": eos,
        "ms_per_request_median": round(median * 1e3, 2),
        "ms_per_request_min_max": [round(times[0] * 1e3, 2), round(times[-1] * 1e3, 2)],
        "path": "graph" if getattr(model, "_graph_decoders", None) else "host-loop",
    }))


if __name__ == "__main__":
    main()
