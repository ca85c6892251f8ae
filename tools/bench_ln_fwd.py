"""A/B of ln_fwd / add_ln_fwd between builds of the extension.

    python tools/bench_ln_fwd.py --lib old=/path/to/parent/_perceiver_hip.so --lib new=

Every library is timed in fresh child processes of its own (two builds export the
same symbols, so they cannot share a process), the libraries alternating, --rounds
processes each. An empty path means the in-tree build. A timed window is as many
calls as fill --window seconds (device events around it, the count taken from a
200-call probe), a process reports the median of --repeats windows per call and
shape, and the table gives every process's median, their median and their max - min
spread. Each child also reports the relative rstd error on a row of 64.0 with one
64.5, which tells a one-pass variance from a centred one.
"""
import argparse
import importlib.util
import json
import pathlib
import statistics
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
SHAPES = [(16384, 1280), (16384, 2048), (65536, 768)]


def child(path, window, repeats):
    import torch

    spec = importlib.util.spec_from_file_location("_perceiver_hip", path)
    ext = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ext)
    assert torch.cuda.is_available(), "bench_ln_fwd needs a GPU"
    out = {}
    x = torch.full((4, 1280), 64.0)
    x[:, 5] = 64.5
    ones = torch.ones(1280).bfloat16().cuda()
    rstd = ext.ln_fwd(x.bfloat16().cuda(), ones, None, 1e-5)[2]
    ref = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5)
    out["one-off rstd rel err"] = float(((rstd.cpu().double() - ref).abs() / ref).max())

    def timed(call, iters):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            call()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1000.0 / iters  # us per call

    for rows, C in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(rows + C)
        x = torch.randn(rows, C, generator=g).bfloat16().cuda()
        h = torch.randn(rows, C, generator=g).bfloat16().cuda()
        w = (torch.randn(C, generator=g).abs() + 0.5).bfloat16().cuda()
        b = torch.randn(C, generator=g).bfloat16().cuda()
        calls = {"ln_fwd": lambda: ext.ln_fwd(x, w, b, 1e-5),
                 "add_ln_fwd": lambda: ext.add_ln_fwd(h, x, w, b, 1e-5)}
        for name, call in calls.items():
            timed(call, 200)  # warm-up
            iters = max(200, int(window * 1e6 / timed(call, 200)))
            out[f"{name} {rows}x{C}"] = statistics.median(timed(call, iters)
                                                          for _ in range(repeats))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--rounds", type=int, default=3, help="processes per library")
    ap.add_argument("--window", type=float, default=0.4, help="seconds per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="windows per process")
    ap.add_argument("--json", default=None, help="also write the table here")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.window, args.repeats)
    libs = dict(item.split("=", 1) for item in (args.lib or ["tree="]))
    default = ROOT / "perceiver_amd" / "ops" / "_perceiver_hip.so"
    runs = {name: [] for name in libs}
    for _ in range(args.rounds):
        for name, path in libs.items():
            done = subprocess.run(
                [sys.executable, __file__, "--child", path or str(default), "--window",
                 str(args.window), "--repeats", str(args.repeats)],
                capture_output=True, text=True, timeout=600)
            if done.returncode != 0:
                print(done.stdout[-2000:], done.stderr[-2000:])
                return done.returncode
            line = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs[name].append(json.loads(line[7:]))
    table = {}
    for key in next(iter(runs.values()))[0]:
        table[key] = {}
        for name, rs in runs.items():
            vals = [r[key] for r in rs]
            table[key][name] = {"per_process": vals, "median": statistics.median(vals),
                                "spread": max(vals) - min(vals)}
        print(key, json.dumps(table[key]), flush=True)
    if args.json:
        pathlib.Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.json).write_text(json.dumps(table, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
