"""Shared oracle for the attention path tests (test_attention_oracle.py on the
CPU, test_gpu_attention_paths.py on the GPU).

Holds the inputs, the fp64 reference, the derived error bound, a CPU emulation
of the kernels' numerics (with switchable defects, so the bound is shown to
catch them), Python copies of the host-side routing rules, and the case table.
Nothing here touches a GPU.
"""
from __future__ import annotations

import functools
import math

import torch

FLT_MAX = torch.finfo(torch.float32).max

# |lse - lse_ref| bound: an fp32 sum of up to 4096 terms is off by at most
# ~4096 * 2^-24 = 2.4e-4 relative, which is the absolute error of its log;
# 4x margin gives 2^-10.
LSE_TOL = 2.0 ** -10

# the project's gradient criterion (max abs error / max |ref|), see
# _assert_grads_close in test_gpu_kernels.py
GRAD_REL = 5e-2


# ---------------------------------------------------------------- inputs

def make_qkv(shape, score_std=3.0, seed=0):
    """bf16 (q, k, v) for shape (B, H, Nq, Lk, D, Dv) from a CPU generator.

    Raw scores q.k have std ~= score_std, so attention is peaked and a lost
    tile or split moves the output (at std 1 it is nearly uniform and hides
    them). Rounded to bf16 first: reference and kernel see identical inputs."""
    b, h, nq, lk, d, dv = shape
    g = torch.Generator(device="cpu").manual_seed(seed)
    scale = math.sqrt(score_std) * d ** -0.25
    q = torch.randn(b, h, nq, d, generator=g) * scale
    k = torch.randn(b, h, lk, d, generator=g) * scale
    v = torch.randn(b, h, lk, dv, generator=g)
    return q.bfloat16(), k.bfloat16(), v.bfloat16()


def make_dout(shape, seed=0):
    b, h, nq, _, _, dv = shape
    g = torch.Generator(device="cpu").manual_seed(seed + 1000)
    return torch.randn(b, h, nq, dv, generator=g).bfloat16()


def build_mask(pad, causal, nq, lk):
    """(B|1, 1, Nq, Lk) bool, True = masked; None when nothing is masked."""
    mask = None
    if pad is not None:
        mask = pad[:, None, None, :].expand(-1, 1, nq, lk)
    if causal:
        cm = torch.ones(nq, lk, dtype=torch.bool).triu(lk - nq + 1)[None, None]
        mask = cm if mask is None else mask | cm
    return mask


# ---------------------------------------------------------------- reference

def reference(q, k, v, pad=None, causal=False, keep=None, p=0.0):
    """fp64 attention with eager_attention's semantics (masked_fill(-finfo.max),
    so fully masked rows come out uniform). Differentiable.

    Returns (out, lse, P, absPV): lse is the logsumexp of the masked scores
    before dropout (what the kernels store), P the probabilities before
    dropout, absPV = P @ |v|. keep (bool, broadcastable to P) and p apply
    dropout to out only: out = (P * keep / (1 - p)) @ v."""
    qd, kd, vd = q.double(), k.double(), v.double()
    scores = qd @ kd.transpose(-2, -1)
    mask = build_mask(pad, causal, q.shape[-2], k.shape[-2])
    if mask is not None:
        scores = scores.masked_fill(mask, -torch.finfo(scores.dtype).max)
    lse = torch.logsumexp(scores, dim=-1)
    probs = scores.softmax(dim=-1)
    pe = probs if keep is None else probs * keep.double() / (1.0 - p)
    return pe @ vd, lse, probs, probs @ vd.abs()


def tol(out_ref, abs_pv, p=0.0):
    """Elementwise bound on |out - out_ref|, derived and not tuned.

    The kernels round twice to bf16, each with relative error 2^-9: P before
    the P.V MFMA (moves out by at most 2^-9 * P@|v|) and the output itself
    (2^-9 * |out|). Each gets a factor 2 of margin. Dropout scales both by
    1/(1-p). The fp32 accumulation and __expf terms are three orders of
    magnitude smaller; 1e-5 covers them."""
    return 2.0 ** -8 * (out_ref.abs() + abs_pv) / (1.0 - p) + 1e-5


def worst_ratio(got, want, bound):
    return ((got.double() - want.double()).abs() / bound).max().item()


def live_rows(pad, shape):
    """(B, 1, Nq) bool: rows with at least one unpadded key (their lse is real)."""
    b, _, nq, lk, _, _ = shape
    if pad is None:
        return torch.ones(b, 1, nq, dtype=torch.bool)
    return (~pad.all(dim=1))[:, None, None].expand(b, 1, nq)


# ---------------------------------------------------------------- emulation

def emulate(q, k, v, mask, tile=64, chunk=None,
            skip_tile=None, skip_split=None, equal_weights=False):
    """CPU emulation of the forward kernels' numerics: bf16 inputs, fp32
    scores, tile-wise online softmax in fp32, P rounded to bf16 before P.V,
    KV splits of `chunk` keys merged by logsumexp weights, bf16 output.

    Returns (out bf16, lse fp32).

    Defects, for showing that the bound catches them: skip_tile drops the tile
    starting at key skip_tile * tile, skip_split drops that split from the
    merge, equal_weights merges the splits with weight 1 each."""
    qf, kf, vf = q.float(), k.float(), v.float()
    lk = k.shape[-2]
    s_all = qf @ kf.transpose(-2, -1)
    if mask is not None:
        s_all = s_all.masked_fill(mask, -FLT_MAX)
    chunk = lk if chunk is None else chunk
    nsplit = (lk + chunk - 1) // chunk
    rows = s_all.shape[:-1]
    parts, lses, counts = [], [], []
    for sp in range(nsplit):
        lo, hi = sp * chunk, min(lk, (sp + 1) * chunk)
        m = torch.full(rows, -math.inf)
        l = torch.zeros(rows)
        o = torch.zeros(*rows, v.shape[-1])
        for kv0 in range(lo, hi, tile):
            if skip_tile is not None and kv0 == skip_tile * tile:
                continue
            s = s_all[..., kv0:min(kv0 + tile, hi)]
            m_new = torch.maximum(m, s.amax(dim=-1))
            alpha = torch.exp(m - m_new)
            pr = torch.exp(s - m_new[..., None])
            l = l * alpha + pr.sum(dim=-1)
            o = o * alpha[..., None] + pr.bfloat16().float() @ vf[..., kv0:min(kv0 + tile, hi), :]
            m = m_new
        live = l > 0
        part = torch.where(live[..., None], o / l.clamp_min(1e-37)[..., None], torch.zeros(()))
        lse = torch.where(live, m + torch.log(l.clamp_min(1e-37)), torch.full((), -1e30))
        parts.append(part)
        lses.append(lse)
        counts.append(float(hi - lo))
    if nsplit == 1:
        return parts[0].bfloat16(), lses[0]

    o_st, lse_st = torch.stack(parts), torch.stack(lses)
    mx = lse_st.amax(dim=0).clamp_min(-1e30)
    w = torch.exp(lse_st - mx)
    # rows masked in every split: weight the splits by their key counts
    dead = mx <= -1e29
    cnt = torch.tensor(counts).view(-1, *([1] * len(rows)))
    w = torch.where(dead, torch.where(lse_st < -0.5 * FLT_MAX, cnt, torch.zeros(())), w)
    if skip_split is not None:
        w[skip_split] = 0.0
    if equal_weights:
        w = torch.ones_like(w)
    wsum = w.sum(dim=0)
    out = (w[..., None] * o_st).sum(dim=0) / wsum.clamp_min(1e-37)[..., None]
    lse = torch.where(dead, torch.full((), -FLT_MAX), mx + torch.log(wsum.clamp_min(1e-37)))
    return out.bfloat16(), lse


# ---------------------------------------------------------------- routing
# Python copies of the host-side rules in csrc/attn_common.h, flash_fwd.hip,
# flash_fwd_pipe.hip and flash_bwd.hip. test_attention_oracle.py holds them
# against the built extension.

KVBLK = 64
PIPE_QBLK = 128
PIPE_TEMPLATES = [(32, 32), (32, 64), (32, 96), (32, 128), (32, 160),
                  (64, 64), (64, 128), (128, 128)]


def plan_split(blocks, length, tile):
    """(nsplit, chunk) of a length-long reduction axis over gridDim.z."""
    if blocks < 512 and length > 4 * tile:
        want = 512 // blocks + 1
        max_split = (length + 4 * tile - 1) // (4 * tile)
        n = min(want, max_split, 32)
        tiles = (length + tile - 1) // tile
        chunk = (tiles + n - 1) // n * tile
        return (length + chunk - 1) // chunk, chunk
    return 1, length


def pipe_applicable(d, dv, nq):
    return nq >= PIPE_QBLK and (d, dv) in PIPE_TEMPLATES


def _cdiv(a, b):
    return (a + b - 1) // b


def fwd_blocks(shape):
    """(uses the pipelined kernel, workgroups in the unsplit forward grid)."""
    b, h, nq, _, d, dv = shape
    if pipe_applicable(d, dv, nq):
        return True, _cdiv(nq, PIPE_QBLK) * b * h
    # v3: the QH = 2 templates (D <= 128) have 128-row workgroups, the rest 64
    qblk = 128 if (d <= 32 and dv <= 160) or (d <= 128 and dv <= 128) else 64
    return False, _cdiv(nq, qblk) * b * h


def bwd_template(d, dv):
    """(dq tile, dq q rows per workgroup, dkv tile, dkv keys per workgroup)."""
    if d <= 32 and dv <= 160 or d <= 64 and dv <= 64:
        return 64, 128, 64, 64
    if d <= 128 and dv <= 128:
        return 64, 128, 32, 64
    if d <= 160 and dv <= 160:
        return 64, 64, 32, 64
    return 32, 64, 32, 64


def route(shape, causal, plan=plan_split, pipe=pipe_applicable):
    """{'pipe', 'fwd', 'dq', 'dkv'}: forward kernel and the three (nsplit,
    chunk) plans for this problem. plan/pipe default to the Python copies; the
    GPU tests pass the extension's flash_split_plan / flash_fwd_pipe_applicable."""
    b, h, nq, lk, d, dv = shape
    use_pipe = bool(pipe(d, dv, nq))
    assert use_pipe == fwd_blocks(shape)[0]
    dq_tile, dq_qblk, dkv_tile, dkv_kblk = bwd_template(d, dv)
    return {
        "pipe": use_pipe,
        "fwd": tuple(plan(fwd_blocks(shape)[1], lk, KVBLK)),
        "dq": tuple(plan(_cdiv(nq, dq_qblk) * b * h, lk, dq_tile)),
        # causal keeps the whole query axis in dkv
        "dkv": (1, nq) if causal else tuple(plan(_cdiv(lk, dkv_kblk) * b * h, nq, dkv_tile)),
    }


# ---------------------------------------------------------------- cases
# shape (B, H, Nq, Lk, D, Dv); pad: (batch, first key, one past last key)
# spans; route: what the case exists to reach. The smallest shapes that still
# take each path.

def _case(shape, pad=(), causal=False, **route_):
    return {"shape": shape, "pad": tuple(pad), "causal": causal, "route": route_}


CASES = {
    # v3 forward KV-split + pad: b0's pad crosses the split boundary, b1's
    # second split is entirely masked. Also dq KV-split + pad (case 7).
    "v3_split_pad": _case((2, 1, 40, 330, 32, 160), [(0, 100, 260), (1, 192, 330)],
                          pipe=False, fwd=(2, 192), dq=(2, 192), dkv=(1, 40)),
    # decode over a cache: last split entirely masked, the third partly
    "v3_decode_cache": _case((2, 4, 1, 1000, 64, 64), [(0, 700, 1000), (1, 700, 1000)],
                             pipe=False, fwd=(4, 256)),
    "v3_split_causal": _case((1, 1, 96, 400, 48, 48), causal=True, pipe=False, fwd=(2, 256)),
    # causal with empty splits: query block 0 ends at key 192 (splits 1, 2
    # empty), block 1 at 320 (split 2 empty). Also dq KV-split + causal (case 6).
    "pipe_split_causal": _case((1, 1, 512, 576, 64, 64), causal=True,
                               pipe=True, fwd=(3, 192), dq=(3, 192), dkv=(1, 512)),
    # ragged last split; b0 loses two whole splits, b1's first split is all
    # masked (m = -FLT_MAX, then recovered by a later tile)
    "pipe_split_pad": _case((2, 1, 128, 2100, 32, 96), [(0, 300, 1100), (1, 0, 256)],
                            pipe=True, fwd=(9, 256)),
    # dkv Q-split + pad with a ragged last split (case 8)
    "dkv_qsplit_pad": _case((2, 1, 600, 70, 32, 64), [(0, 50, 70)],
                            pipe=True, fwd=(1, 70), dq=(1, 70), dkv=(3, 256)),
    # fully masked rows: the last batch element has every key padded
    "dead_unsplit": _case((2, 2, 40, 100, 32, 64), [(0, 60, 100), (1, 0, 100)],
                          pipe=False, fwd=(1, 100), dq=(1, 100), dkv=(1, 40)),
    "dead_pipe_split": _case((3, 1, 128, 2100, 32, 96),
                             [(0, 300, 1100), (1, 0, 256), (2, 0, 2100)],
                             pipe=True, fwd=(9, 256)),
    "dead_v3_split": _case((3, 1, 40, 330, 32, 160),
                           [(0, 100, 260), (1, 192, 330), (2, 0, 330)],
                           pipe=False, fwd=(2, 192), dq=(2, 192), dkv=(1, 40)),
}

# the batch element whose keys are all padded
DEAD_BATCH = {"dead_unsplit": 1, "dead_pipe_split": 2, "dead_v3_split": 2}


def make_pad(case):
    b, _, _, lk, _, _ = case["shape"]
    if not case["pad"]:
        return None
    pad = torch.zeros(b, lk, dtype=torch.bool)
    for bi, lo, hi in case["pad"]:
        pad[bi, lo:hi] = True
    return pad


def check_route(case, got):
    """got: route(...) of the case's shape; every entry the case names must match."""
    for key, want in case["route"].items():
        assert got[key] == want, f"route {key}: got {got[key]}, case needs {want}"


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(q, k, v, pad, (out, lse, P, absPV)) of a case; computed once, shared,
    and never written to."""
    case = CASES[name]
    q, k, v = make_qkv(case["shape"], seed=sorted(CASES).index(name))
    pad = make_pad(case)
    with torch.no_grad():
        ref = reference(q, k, v, pad, case["causal"])
    return q, k, v, pad, ref


@functools.lru_cache(maxsize=None)
def case_grads(name, zero_dead_dout=False):
    """(dout, (dq, dk, dv)) of a case: fp64 autograd through reference().
    zero_dead_dout zeroes dout on the fully padded batch element first."""
    case = CASES[name]
    q, k, v, pad, _ = case_data(name)
    dout = make_dout(case["shape"], seed=sorted(CASES).index(name))
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    out = reference(qd, kd, vd, pad, case["causal"])[0]
    g = dout.double()
    if zero_dead_dout:
        g = g.clone()
        g[DEAD_BATCH[name]] = 0.0
    out.backward(g)
    return dout, (qd.grad, kd.grad, vd.grad)
