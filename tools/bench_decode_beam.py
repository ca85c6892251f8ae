"""Times generate(num_beams=...) for a serving-style request on the flagship CLM:
7168-token prompts, 64 new tokens, no EOS.

Usage: python tools/bench_decode_beam.py [--batch 8] [--num-beams 4] [--new-tokens 64]
       python tools/bench_decode_beam.py --select-launch [--vocab 32768] [--num-beams 8]
Prints one JSON line; "path" says whether the request replayed the captured
decode graph or ran the host-driven loop (PERCEIVER_BEAM_GRAPH=0 forces the
latter). --select-launch times one beam_select launch instead.
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


def select_launch(args, dev):
    from perceiver_amd.ops import hip

    nb, V, G = args.num_beams, args.vocab, args.batch
    B = G * nb
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    logits = (torch.randn(B, V, generator=g) * 3).to(dev, torch.bfloat16)
    st = [torch.zeros(B, device=dev), torch.zeros(B, dtype=torch.bool, device=dev),
          torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.long, device=dev),
          torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(G, dtype=torch.bool, device=dev),
          torch.tensor([-1, 0], device=dev)]

    def launch():
        st[0].zero_()
        hip.ext().beam_select(logits, *st, nb)

    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(50):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st[0].zero_()
        a.record()
        hip.ext().beam_select(logits, *st, nb)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    print(json.dumps({"metric": "beam_select_launch_us", "value": round(times[len(times) // 2], 1),
                      "unit": "us", "vocab": V, "num_beams": nb, "groups": G, "dtype": "bf16",
                      "us_min_max": [round(times[0], 1), round(times[-1], 1)]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--num-beams", type=int, default=4)
    ap.add_argument("--new-tokens", type=int, default=64)
    ap.add_argument("--requests", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=17)
    ap.add_argument("--select-launch", action="store_true",
                    help="time one beam_select launch at --vocab x --num-beams instead")
    ap.add_argument("--vocab", type=int, default=32768)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    if args.select_launch:
        return select_launch(args, dev)
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
                              num_beams=args.num_beams)

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
    beam = [gd for gd in getattr(model, "_graph_decoders", {}).values()
            if getattr(gd, "num_beams", 1) > 1]
    print(json.dumps({
        "metric": "generate_tok_per_s_clm_beam", "value": round(args.batch * new_tokens / median, 1),
        "unit": "tok/s", "batch": args.batch, "num_beams": args.num_beams,
        "new_tokens_per_request": new_tokens, "ms_per_request_median": round(median * 1e3, 2),
        "ms_per_request_min_max": [round(times[0] * 1e3, 2), round(times[-1] * 1e3, 2)],
        "path": "graph" if beam else "host-loop",
    }))


if __name__ == "__main__":
    main()
