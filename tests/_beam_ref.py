"""Shared pieces of the beam-search tests: the constructed tie cases and the
fp64 statement of the candidate rule with the tolerance derived from it."""
import math

import torch


def tie_cases():
    """name -> (logits, scores, done, nb, eos, fill, want_src, want_tok); the
    answer needs no arithmetic."""
    V, vstar = 23, 11
    row = torch.zeros(V)
    row[vstar] = 4.0
    same = (row.repeat(4, 1), torch.zeros(4), torch.zeros(4, dtype=torch.bool), 4, -1, 0,
            [0, 1, 2, 3], [vstar] * 4)
    # duplicated logits inside a row: the lowest token first; row 1 is out of reach
    x = torch.full((2, V), -3.0)
    x[0, [17, 4, 9]] = 2.0
    dup = (x, torch.tensor([0.0, -50.0]), torch.zeros(2, dtype=torch.bool), 2, -1, 0,
           [0, 0], [4, 9])
    return {"identical_rows": same, "duplicates_in_a_row": dup}


def _candidates(x, scores, done, fill, dtype):
    logp = x.to(dtype).log_softmax(-1)
    frozen = torch.full_like(logp, -1e9)
    frozen[:, fill] = 0.0
    return scores.to(dtype)[:, None] + torch.where(done[:, None], frozen, logp)


def candidates64(x, scores, done, fill):
    """(B, V) fp64 candidates of the rules in ops/beam.py."""
    return _candidates(x.float(), scores, done, fill, torch.float64)


def ulp32(v: float) -> float:
    """One fp32 unit in the last place at magnitude |v|."""
    return 2.0 ** (math.floor(math.log2(max(abs(v), 2.0 ** -126))) - 23)


def tolerance(x, scores, done, fill, rows=None):
    """4x the largest deviation of torch's own fp32 ``s + log_softmax(x)`` from
    the fp64 candidates on the same inputs, floored at one fp32 ulp of the
    largest |candidate|: the kernel may order its reduction and evaluate exp and
    log differently from torch, but nothing wider than fp32 rounding. ``rows``
    restricts both terms to those rows (the live rows: a frozen row's -1e9
    candidates alone put the floor at 64)."""
    ref = candidates64(x, scores, done, fill)
    own = _candidates(x.float(), scores, done, fill, torch.float32).double()
    if rows is not None:
        ref, own = ref[rows], own[rows]
    return max(4.0 * float((own - ref).abs().max()), ulp32(float(ref.abs().max())))
