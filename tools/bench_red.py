"""Microbench for the row kernels: LN forward/backward, their residual-fused forms
next to the pair of kernels each replaces, and colsum, at the MLM/img shapes.

A plain bf16 ``a + b`` of the same shape is the roofline stand-in: every row gives
the median of ``--repeats`` timings, the max-min spread, the effective TB/s over
the bytes the op must move, and that bandwidth as a share of the add's.
"""
import argparse
import pathlib
import statistics
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

import torch

from perceiver_amd.ops import hip as hip_ops


def bench(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1000  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=8, help="timings per row (median, spread)")
    args = ap.parse_args()

    ext = hip_ops.ext()
    dev = torch.device("cuda")
    has_fused = hasattr(ext, "add_ln_fwd")
    for rows, C in [(16384, 1280), (65536, 768), (32768, 1024)]:
        x = torch.randn(rows, C, device=dev, dtype=torch.bfloat16)
        h = torch.randn(rows, C, device=dev, dtype=torch.bfloat16)
        dy = torch.randn(rows, C, device=dev, dtype=torch.bfloat16)
        ds = torch.randn(rows, C, device=dev, dtype=torch.bfloat16)
        w = torch.randn(C, device=dev, dtype=torch.bfloat16)
        b = torch.randn(C, device=dev, dtype=torch.bfloat16)
        y, mean, rstd = ext.ln_fwd(x, w, b, 1e-5)
        one_pass = rows * C * 2 / 1e12  # TB per bf16 pass over the tensor

        def add_then(fn):
            def run():
                fn(h + x)
            return run

        # (label, passes over the tensor that the op must make, callable)
        cases = [
            ("add (roofline stand-in)", 3, lambda: h + x),
            ("ln_fwd", 2, lambda: ext.ln_fwd(x, w, b, 1e-5)),
            ("add + ln_fwd", 5, add_then(lambda s: ext.ln_fwd(s, w, b, 1e-5))),
            ("ln_bwd dx-only", 3, lambda: ext.ln_bwd(dy, x, w, mean, rstd, False)),
            ("ln_bwd dx-only + add", 6,
             lambda: ext.ln_bwd(dy, x, w, mean, rstd, False)[0] + ds),
            ("ln_bwd dw/db", 3, lambda: ext.ln_bwd(dy, x, w, mean, rstd, True)),
            ("ln_bwd dw/db + add", 6, lambda: ext.ln_bwd(dy, x, w, mean, rstd, True)[0] + ds),
            ("colsum", 1, lambda: ext.colsum_bf16(dy)),
        ]
        if has_fused:
            cases[3:3] = [("add_ln_fwd (fused)", 4, lambda: ext.add_ln_fwd(h, x, w, b, 1e-5))]
            cases[6:6] = [("ln_bwd dx-only with ds (fused)", 4,
                           lambda: ext.ln_bwd(dy, x, w, mean, rstd, False, ds))]
            cases[9:9] = [("ln_bwd dw/db with ds (fused)", 4,
                           lambda: ext.ln_bwd(dy, x, w, mean, rstd, True, ds))]

        print(f"rows={rows} C={C} ({one_pass * 1e6:.1f} MB per pass, "
              f"median of {args.repeats}, spread = max - min)")
        add_tbs = None
        for label, passes, fn in cases:
            times = [bench(fn) for _ in range(args.repeats)]
            med = statistics.median(times)
            tbs = passes * one_pass / (med / 1e6)
            if add_tbs is None:
                add_tbs = tbs
            print(f"  {label:32s} {med:7.2f} us  spread {max(times) - min(times):5.2f}  "
                  f"{passes} passes  {tbs:5.2f} TB/s  {100 * tbs / add_tbs:5.1f}% of add")


if __name__ == "__main__":
    main()
