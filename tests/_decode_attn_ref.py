"""Shared oracle for the windowed decode attention tests
(test_decode_attn_oracle.py on the CPU, test_gpu_decode_attn.py on the GPU).

Inputs, the fp64 reference and the derived bound come from _attention_ref.py.
Added here: boundary-sensitive inputs (a window that is off by one key at
either end moves the output far outside the bound), a CPU emulation of the
kernel's numerics, Python copies of the host-side plan and gate, and the case
table. Nothing here touches a GPU.
"""
from __future__ import annotations

import functools

import torch

from _attention_ref import make_qkv, reference, tol, worst_ratio  # noqa: F401

EMPTY_LSE = -1e30


# ---------------------------------------------------------------- host rules
# Python copies of decode_attn_plan / decode_attn_applicable in
# csrc/decode_attn.hip; test_decode_attn_oracle.py holds them against the
# package and the built extension.

def plan(b, h, cap, d):
    """(nsplit, row granule): splits aim at ~512 workgroups, a slice of the
    capacity keeps at least 32 keys per partial of the merge (32 * nsplit^2 <=
    cap), at most 32; a wave's load covers 64 / pow2ceil(d / 8) rows."""
    lanes = 1
    while lanes * 8 < d:
        lanes *= 2
    blocks = b * h
    by_cap = 1
    while 32 * (by_cap + 1) ** 2 <= cap:
        by_cap += 1
    nsplit = 1 if blocks >= 512 else min(512 // blocks + 1, by_cap, 32)
    return nsplit, 64 // lanes


def applicable(d, dv):
    return d % 8 == 0 and dv % 8 == 0 and 8 <= d <= 128 and 8 <= dv <= 128


# ---------------------------------------------------------------- cases
# shape (B, H, cap, D, Dv); lo / hi per row, inclusive; nsplit: the slice count
# the case was written to reach.

CASES = {
    "small_unsplit": {"shape": (3, 2, 48, 16, 16), "lo": [0, 5, 47], "hi": [30, 30, 47],
                      "nsplit": 1},
    "d64_split8": {"shape": (3, 2, 2048, 64, 64), "lo": [1, 63, 65], "hi": [1500, 700, 66],
                   "nsplit": 8},
    "d128_split8": {"shape": (2, 4, 2048, 128, 128), "lo": [64, 300], "hi": [2046, 1000],
                    "nsplit": 8},
    "d32_dv64_split4": {"shape": (2, 2, 512, 32, 64), "lo": [3, 100], "hi": [400, 101],
                        "nsplit": 4},
}


def window_lengths(name):
    """Window lengths around the granule and the slice edges of a case."""
    b, h, cap, d, _ = CASES[name]["shape"]
    nsplit, g = plan(b, h, cap, d)
    return sorted({n for n in (1, 2, g - 1, g, g + 1, nsplit * g - 1, nsplit * g + 1, cap)
                   if 1 <= n <= cap})


def all_cases():
    """(name, n): n None is the table's own windows, else every row's window has n keys."""
    out = []
    for name in sorted(CASES):
        out.append((name, None))
        out.extend((name, n) for n in window_lengths(name))
    return out


def case_id(c):
    return c[0] if c[1] is None else f"{c[0]}-n{c[1]}"


def windows(name, n=None):
    """(lo, hi) int64 (B,) tensors of a case."""
    case = CASES[name]
    cap = case["shape"][2]
    lo = torch.tensor(case["lo"], dtype=torch.long)
    if n is None:
        return lo, torch.tensor(case["hi"], dtype=torch.long)
    lo = torch.minimum(lo, torch.full_like(lo, cap - n))
    return lo, lo + n - 1


def window_pad(lo, hi, b, cap):
    """(B, cap) bool, True = outside the window, as the issue states the mask."""
    j = torch.arange(cap)[None, :]
    lo = torch.zeros(b, dtype=torch.long) if lo is None else lo.expand(b)
    return (j < lo[:, None]) | (j > hi.expand(b)[:, None])


def plant_boundary_keys(q, k, lo, hi):
    """Replace the keys at lo-1, lo, hi, hi+1 of each row by q * 8 / |q|^2: their
    score is ~8 against a raw score std of 3, so a window that is off by one at
    either end gains or loses a dominant key."""
    cap = k.shape[2]
    qf = q.float()[:, :, 0, :]
    strong = (qf * (8.0 / qf.pow(2).sum(-1, keepdim=True))).bfloat16()
    k = k.clone()
    for b in range(k.shape[0]):
        for j in (int(lo[b]) - 1, int(lo[b]), int(hi[b]), int(hi[b]) + 1):
            if 0 <= j < cap:
                k[b, :, j, :] = strong[b]
    return k


@functools.lru_cache(maxsize=None)
def case_data(name, n=None):
    """(q, k, v, lo, hi, (out, lse, P, absPV)) of a case; computed once, shared
    and never written to."""
    b, h, cap, d, dv = CASES[name]["shape"]
    lo, hi = windows(name, n)
    q, k, v = make_qkv((b, h, 1, cap, d, dv), score_std=3.0,
                       seed=100 + sorted(CASES).index(name))
    k = plant_boundary_keys(q, k, lo, hi)
    with torch.no_grad():
        ref = reference(q, k, v, window_pad(lo, hi, b, cap))
    return q, k, v, lo, hi, ref


# ---------------------------------------------------------------- emulation

def emulate(q, k, v, lo, hi, nsplit, granule):
    """CPU emulation of the kernel's numerics: bf16 inputs, fp32 scores, fp32
    softmax with unrounded P, one normalised fp32 partial per slice (slices of
    ceil(n / nsplit) keys rounded up to the granule, counted from lo), merged by
    logsumexp weights in split order, bf16 output. Ends clamped into [0, cap);
    hi < lo gives zeros."""
    b, h, cap, _ = k.shape
    dv = v.shape[-1]
    qf, kf, vf = q.float(), k.float(), v.float()
    scores = (qf @ kf.transpose(-2, -1))[:, :, 0, :]  # (B, H, cap)
    out = torch.zeros(b, h, 1, dv)
    for bi in range(b):
        lo_raw = 0 if lo is None else int(lo.reshape(-1)[bi if lo.numel() > 1 else 0])
        hi_raw = int(hi.reshape(-1)[bi if hi.numel() > 1 else 0])
        if hi_raw < lo_raw:
            continue
        lo_c, hi_c = min(max(lo_raw, 0), cap - 1), min(max(hi_raw, 0), cap - 1)
        n = hi_c - lo_c + 1
        per = -(-n // nsplit)
        per = -(-per // granule) * granule
        parts, lses = [], []
        for sp in range(nsplit):
            beg, end = lo_c + min(n, sp * per), lo_c + min(n, (sp + 1) * per)
            if beg >= end:
                parts.append(torch.zeros(h, dv))
                lses.append(torch.full((h,), EMPTY_LSE))
                continue
            s = scores[bi, :, beg:end]
            m = s.amax(dim=-1)
            p = torch.exp(s - m[:, None])
            l = p.sum(dim=-1)
            parts.append((p[:, None, :] @ vf[bi, :, beg:end, :])[:, 0, :] / l[:, None])
            lses.append(m + torch.log(l))
        o_st, lse_st = torch.stack(parts), torch.stack(lses)
        mx = lse_st.amax(dim=0)
        w = torch.where(lse_st > 0.5 * EMPTY_LSE, torch.exp(lse_st - mx), torch.zeros(()))
        out[bi, :, 0, :] = (w[..., None] * o_st).sum(dim=0) / w.sum(dim=0)[:, None]
    return out.bfloat16()


MUTANTS = {"lo-1": (-1, 0), "lo+1": (1, 0), "hi-1": (0, -1), "hi+1": (0, 1)}
