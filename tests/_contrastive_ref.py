"""Shared pieces of the contrastive-search tests: the fp64 oracle of the rules in
ops/contrastive.py, the derived tolerances, and the inputs of the kernel cases
(the CPU tests hold an fp32 emulation of the kernel's arithmetic to the same
bounds at the same inputs the GPU tests use)."""
import math

import torch

EPS = 1e-12


# ------------------------------------------------------------------- the oracle

def _key(v: float):
    """Sort key of (value descending, NaN largest)."""
    return (0, 0.0) if math.isnan(v) else (1, -v)


def propose64(x: torch.Tensor, k: int):
    """One logit row (V,): the k largest tokens by (raw fp32 logit descending,
    index ascending) and their full-softmax probabilities in fp64."""
    xf = x.float()
    vals = xf.tolist()
    order = sorted(range(len(vals)), key=lambda v: (_key(vals[v]), v))[:k]
    xd = xf.double()
    e = (xd - xd.max()).exp()
    p = e / e.sum()
    return order, [float(p[v]) for v in order]


def cosines64(h: torch.Tensor, hist: torch.Tensor) -> torch.Tensor:
    """(cap, k) fp64 cosines of every history row against every candidate, each
    vector normalised by max(||.||, 1e-12) before the dot."""
    hn = h.double()
    hn = hn / hn.norm(dim=-1, keepdim=True).clamp_min(EPS)
    tn = hist.double()
    tn = tn / tn.norm(dim=-1, keepdim=True).clamp_min(EPS)
    return tn @ hn.t()


def sim64(h: torch.Tensor, hist: torch.Tensor, n: int) -> torch.Tensor:
    """(k,) max cosine of the candidates (k, C) over history rows [0, n) of
    (cap, C); NaN propagates; 0 with no rows."""
    n = max(0, min(int(n), hist.shape[0]))
    if n == 0:
        return torch.zeros(h.shape[0], dtype=torch.float64)
    return cosines64(h, hist[:n]).amax(0)


def step64(h, hist, n, tok, prob, done, alpha, eos, fill):
    """One group's step: (sel, emitted, done', sim, score) from the candidates'
    hidden states (k, C), the history (cap, C) with n live rows, the candidate
    tokens / probabilities (k,), and the group's done flag."""
    sim = sim64(h, hist, n)
    score = (1.0 - float(alpha)) * prob.double() - float(alpha) * sim
    vals = score.tolist()
    sel = min(range(len(vals)), key=lambda j: (_key(vals[j]), j))
    emitted = int(fill) if done else int(tok[sel])
    return sel, emitted, bool(done) or emitted == int(eos), sim, score


def oracle_spy(inner, gaps, moved):
    """``contrastive_reference`` wrapped: every call is scored by the oracle from
    the very inputs the step saw. ``gaps`` takes each group's fp64 gap between
    the best and the second score, ``moved`` whether the oracle's ``sel`` is not
    0; where the gap is >= 1e-4 the reference must select what the oracle does."""
    def spy(h, hist, rnorm, hist_len, tok, prob, done, alpha, eos, fill, k, **kw):
        out = inner(h, hist, rnorm, hist_len, tok, prob, done, alpha, eos, fill, k, **kw)
        hc, tc, pc = h.cpu(), tok.cpu(), prob.cpu()
        for g in range(hist.shape[0]):
            want = step64(hc[g * k:(g + 1) * k], hist[g].cpu(), int(hist_len),
                          tc[g * k:(g + 1) * k], pc[g * k:(g + 1) * k],
                          bool(done[g]), float(alpha), int(eos), int(fill))
            top = want[4].sort(descending=True).values
            gaps.append(float(top[0] - top[1]))
            moved.append(want[0] != 0)
            if gaps[-1] >= 1e-4:
                assert int(out[0][g]) == want[0]
        return out
    return spy


# ------------------------------------------------------------------- tolerances

def ulp32(v: float) -> float:
    """One fp32 unit in the last place at magnitude |v|."""
    return 2.0 ** (math.floor(math.log2(max(abs(v), 2.0 ** -126))) - 23)


def sim_bound(C: int) -> float:
    """Absolute bound on sim: an fp32 dot of C products errs by at most
    C * 2^-24 * ||a|| ||b|| (Cauchy-Schwarz), each of the two reciprocal norms
    carries at most (C + 4) * 2^-24 relative error (sum of squares, square
    root, reciprocal), and ||a|| ||b|| r_t r_j is about 1."""
    return (3 * C + 16) * 2.0 ** -24


def prob_tolerance(x: torch.Tensor) -> float:
    """4x torch's own largest fp32 deviation from the fp64 softmax on the same
    rows, floored at one fp32 ulp of the largest probability."""
    xf = x.float()
    ref = xf.double().softmax(-1)
    own = xf.softmax(-1).double()
    return max(4.0 * float((own - ref).abs().max()), ulp32(float(ref.max())))


def score_tolerance(alpha: float, C: int, x: torch.Tensor) -> float:
    """Tolerance of (1 - a) p - a sim from those of p and sim, plus the three
    fp32 roundings of the expression itself (|score| <= 1)."""
    return (1.0 - alpha) * prob_tolerance(x) + alpha * sim_bound(C) + 3 * 2.0 ** -24


# -------------------------------------------------------------- kernel cases

SIM_CHANNELS = (8, 32, 40, 520, 1280)
MAX_CHANNELS = 4088  # the widest rows the kernels take: 8 slots fill 64 KiB of LDS
SIM_K = (2, 3, 8)
SIM_CAPS = (16, 1024)
SIM_GROUPS = 2


def plan_twin(G: int, cap: int, C: int):
    """(nsplit, row granule) as contrastive_plan states them."""
    lanes = 1
    while lanes < (C + 7) // 8:
        lanes *= 2
    lanes = min(lanes, 64)
    if G >= 512:
        return 1, 64 // lanes
    return min(-(-512 // G), max(1, cap // 64), 32), 64 // lanes


def slice_rows(n: int, nsplit: int, granule: int) -> int:
    per = -(-n // nsplit)
    return -(-per // granule) * granule


def hist_lens(G: int, cap: int, C: int):
    """1, 2, the row granule and its neighbours, the lengths around which the
    slices grow by a granule, every slice edge at full capacity and its
    neighbours, and the capacity."""
    nsplit, granule = plan_twin(G, cap, C)
    lens = {1, 2, granule - 1, granule, granule + 1, cap}
    full = nsplit * granule
    lens |= {full - 1, full, full + 1}
    per = slice_rows(cap, nsplit, granule)
    for s in range(1, nsplit):
        lens |= {s * per - 1, s * per, s * per + 1}
    return sorted(n for n in lens if 1 <= n <= cap)


def sim_inputs(C: int, k: int, cap: int, seed: int = 0, G: int = SIM_GROUPS):
    """bf16 candidates (G * k, C) and history (G, cap, C) with the history's fp32
    reciprocal norms. A third of the history rows lean towards a candidate, so
    the maxima are not all alike and sit at scattered positions."""
    g = torch.Generator().manual_seed(1000 * C + 10 * k + cap + seed)
    h = (torch.randn(G * k, C, generator=g) * 1.7).bfloat16()
    hist = torch.randn(G, cap, C, generator=g)
    lean = torch.rand(G, cap, generator=g) < 1 / 3
    which = torch.randint(0, k, (G, cap), generator=g)
    mix = torch.rand(G, cap, 1, generator=g) * 1.5
    toward = h.float().view(G, k, C).gather(1, which[:, :, None].expand(-1, -1, C))
    hist = torch.where(lean[:, :, None], hist + mix * toward, hist)
    hist = (hist * (0.25 + 3 * torch.rand(G, cap, 1, generator=g))).bfloat16()
    rnorm = 1.0 / hist.float().norm(dim=-1).clamp_min(EPS)
    return h, hist, rnorm


def sim_oracle_all(h, hist, k):
    """(G, cap, k) fp64 cosines of the case: sim at length n is [:, :n].amax(1)."""
    G = hist.shape[0]
    return torch.stack([cosines64(h.view(G, k, -1)[g], hist[g]) for g in range(G)])


COMMIT_VOCABS = (61, 262, 1500, 32768)
