"""Shared oracle for the pointwise, column-sum and AdamW kernel tests
(test_pointwise_oracle.py on the CPU, test_gpu_pointwise.py on the GPU).

Holds the inputs, the fp64 references, the derived error bounds, CPU emulations
of the kernels' fp32 arithmetic (with switchable defects, so each bound is
shown to catch them) and the case tables. Nothing here touches a GPU.

Conventions: U = 2^-8 is one bf16 rounding as docs/kernels.md writes it for
attention (2^-9 with a factor 2). bf16 keeps 8 significant bits, so just above
a power of two a round-to-nearest is off by almost 2^-8 relative: the factor
is the rounding's own worst case, not slack, and measured ratios reach 0.996.
F32 = 2^-24 is one fp32 rounding. References are fp64, computed from the bf16/fp32 values the kernel
receives. Every bound's docstring counts the roundings it allows.
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

U = 2.0 ** -8
F32 = 2.0 ** -24

# grid cap of the grid-stride elementwise kernels (gelu_bias, adamw, dropout_add)
ELEMENTWISE_BLOCK_CAP = 2048
ELEMENTWISE_THREADS = 256


def worst_ratio(got, want, bound):
    """max |got - want| / bound; a zero bound with a zero error counts as 0."""
    err = (got.double() - want.double()).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return ratio.max().item() if ratio.numel() else 0.0


# ================================================================= GELU

INV_SQRT2 = 0.70710678118654752440
INV_SQRT2PI = 0.39894228040143267794

# Worst |erf_fast - erf| of the fp32 emulation over every finite bf16 v = x + b
# (argument v / sqrt 2), measured by test_pointwise_oracle: 5.0e-7 — the
# 1.5e-7 of the A&S 7.1.26 polynomial plus fp32 cancellation in
# 1 - poly*t*exp. The factor 2 is for __expf / __frcp_rn, which the emulation
# replaces by correctly rounded operations.
EPS_ERF_MEASURED = 5.1e-7
EPS_ERF = 2.0 * EPS_ERF_MEASURED

# Worst |gelu_grad_f - gelu'| of the fp32 emulation over the same set: 2.7e-7,
# doubled for the same reason.
EPS_GRAD_MEASURED = 2.7e-7
EPS_GRAD = 2.0 * EPS_GRAD_MEASURED


@functools.lru_cache(maxsize=None)
def all_finite_bf16():
    """(128, 512) bf16 holding every bf16 bit pattern once, NaN and inf
    patterns replaced by 0. Shared; never written to."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16).clone()
    x[~torch.isfinite(x.float())] = 0
    return x.reshape(128, 512)


def gelu_ref(v):
    """fp64 exact-erf GELU; erfc form, so the negative tail does not cancel."""
    v = v.double()
    return 0.5 * v * torch.special.erfc(-v * INV_SQRT2)


def gelu_grad_ref(v):
    v = v.double()
    return 0.5 * torch.special.erfc(-v * INV_SQRT2) + v * INV_SQRT2PI * torch.exp(-0.5 * v * v)


def gelu_pre(x, b):
    """fp32 v = x + b exactly as the kernel forms it (one fp32 add of two bf16)."""
    v = x.float()
    if b is not None:
        v = v + b.float()
    return v


def gelu_fwd_bound(v):
    """|y - ref| <= U*|ref| + 0.5*|v|*EPS_ERF + 1e-7, v = x + b in fp32.

    Roundings: the bf16 output (U); erf_fast is off
    by at most EPS_ERF absolute, which y = 0.5*v*(1 + erf) scales by 0.5*|v|;
    the three fp32 multiplies/adds around it are 3 * 2^-24 relative and sit
    with the bf16 subnormal flush in the 1e-7."""
    return U * gelu_ref(v).abs() + 0.5 * v.double().abs() * EPS_ERF + 1e-7


def gelu_bwd_bound(v, dy):
    """|dx - ref| <= U*|ref| + |dy|*EPS_GRAD, ref = dy * gelu'(v).

    Roundings: the bf16 output (U); gelu_grad_f = cdf + v*pdf is off by at
    most EPS_GRAD absolute (erf_fast's error halved, __expf in the pdf, three
    fp32 operations), which the product with dy scales by |dy|."""
    ref = dy.double() * gelu_grad_ref(v)
    return U * ref.abs() + dy.double().abs() * EPS_GRAD


def erf_fast_emul(x):
    """common.h erf_fast in torch fp32, operation by operation (no FMA)."""
    assert x.dtype == torch.float32
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    ax = x.abs()
    t = 1.0 / (1.0 + f(0.3275911) * ax)
    poly = f(1.061405429) * t - f(1.453152027)
    poly = poly * t + f(1.421413741)
    poly = poly * t - f(0.284496736)
    poly = poly * t + f(0.254829592)
    e = 1.0 - poly * t * torch.exp(-ax * ax)
    return torch.copysign(e, x)


def gelu_tanh(v):
    """The tanh approximation, the defect the old 2e-2 tolerance let through."""
    v = v.double()
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def gelu_fwd_emul(x, b=None, defect=None):
    """gelu_bias_fwd in fp32, bf16 out. x (rows, C) bf16, b (C) bf16 or None.
    defect: 'tanh', 'bias_shift8' (bias from column c + 8), 'no_bias'."""
    if defect == "no_bias":
        b = None
    elif defect == "bias_shift8" and b is not None:
        b = torch.roll(b, -8)
    v = gelu_pre(x, b)
    if defect == "tanh":
        return gelu_tanh(v).float().bfloat16()
    k = torch.tensor(INV_SQRT2, dtype=torch.float32)
    return (0.5 * v * (1.0 + erf_fast_emul(v * k))).bfloat16()


def gelu_grad_emul_f32(v):
    """common.h gelu_grad_f in fp32 (before the product with dy)."""
    k = torch.tensor(INV_SQRT2, dtype=torch.float32)
    kp = torch.tensor(INV_SQRT2PI, dtype=torch.float32)
    cdf = 0.5 * (1.0 + erf_fast_emul(v * k))
    pdf = kp * torch.exp(-0.5 * v * v)
    return cdf, v * pdf


def gelu_bwd_emul(x, b, dy, defect=None):
    """gelu_bias_bwd in fp32, bf16 out. defect: 'no_xpdf' drops the x*pdf term."""
    v = gelu_pre(x, b)
    cdf, xpdf = gelu_grad_emul_f32(v)
    grad = cdf if defect == "no_xpdf" else cdf + xpdf
    return (dy.float() * grad).bfloat16()


def gelu_bias_case(rows, C, seed=0):
    """(x, b): x ~ N(0, 2) bf16, b[c] = c/4 - C/8 — distinct and exact in bf16,
    so a wrong column moves v by at least 0.25."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(rows, C, generator=g) * 2.0).bfloat16()
    b = (torch.arange(C, dtype=torch.float32) / 4 - C / 8).bfloat16()
    assert torch.equal(b.float(), torch.arange(C, dtype=torch.float32) / 4 - C / 8)
    return x, b


# rows of the bias-indexing cases; (58260, 72) is the second grid-stride trip
GELU_BIAS_SHAPES = [(33, 8), (33, 24), (33, 72)]
GELU_STRIDE_SHAPE = (58260, 72)


# ================================================================= dropout

def rng_hash(seed, bh, i, j):
    """common.h rng_hash in numpy uint32; i, j arrays (or scalars)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        x = np.uint32(seed & 0xFFFFFFFF) + np.uint32(seed >> 32) * np.uint32(0x9E3779B9)
        x = x + np.uint32(bh) * np.uint32(0x85EBCA6B) \
            + np.asarray(i).astype(np.uint32) * np.uint32(0xC2B2AE35) \
            + np.asarray(j).astype(np.uint32) * np.uint32(0x27D4EB2F)
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def dropout_thresh(p):
    """uint32(float32(p) * 2^32), as dropout_add.hip computes it."""
    return int(float(np.float32(p)) * 4294967296.0)


def dropout_inv_keep(p):
    """fp32 1 / (1 - float(p)), as the launcher computes it."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


@functools.lru_cache(maxsize=64)
def dropout_draws(seed, n):
    """uint32 draw of every element of an n-element tensor: element 8i + e of
    granule i draws rng_hash(seed, 0, i, e) (i < 2^31; the i >= 2^31 branch
    would need a 32 GB tensor and is not covered)."""
    assert n % 8 == 0 and n // 8 < 2 ** 31
    i = np.repeat(np.arange(n // 8, dtype=np.uint32), 8)
    e = np.tile(np.arange(8, dtype=np.uint32), n // 8)
    return rng_hash(seed, 0, i, e)


def dropout_keep(seed, p, n):
    """bool (n,) tensor: the emulated keep mask."""
    return torch.from_numpy(dropout_draws(seed, n) >= np.uint32(dropout_thresh(p)))


DROPOUT_SEEDS = [0, 1, 777, 2 ** 40 + 5, 2 ** 62 - 1]
DROPOUT_PS = [0.1, 0.25, 0.5, 0.9]
DROPOUT_N = 2 ** 20


def dropout_stats(mask_of, seed, p, n):
    """Every statistic the issue names, as {name: (value, expected, limit)};
    mask_of(seed, p, n) -> bool (n,) tensor. sigma = sqrt(p(1-p)/n)."""
    sigma = math.sqrt(p * (1 - p) / n)
    keep_p = 1.0 - dropout_thresh(p) / 2.0 ** 32
    m = mask_of(seed, p, n)
    md = m.double()
    out = {"keep": (md.mean().item(), keep_p, 5 * sigma)}
    agree = p * p + (1 - p) * (1 - p)
    for name, other in (("next_seed", seed + 1), ("high_word", seed ^ 2 ** 32)):
        out[name] = ((m == mask_of(other, p, n)).double().mean().item(), agree, 5 * sigma)
    c = md - md.mean()
    var = (c * c).mean()
    for lag in (1, 8, 64):
        out[f"lag{lag}"] = (((c[:-lag] * c[lag:]).mean() / var).item(), 0.0, 5 / math.sqrt(n))
    return out


def dropout_value_bound(ref):
    """|out - ref| <= U*|ref| + 1e-7 where the mask keeps, ref = x*inv_keep + r
    in fp64 with the fp32 inv_keep. Roundings: the bf16 output (U); the fp32
    multiply and add (or one FMA) are 2 * 2^-24 of |x*inv_keep| + |ref| and sit
    in the 1e-7 for the O(1) inputs the test uses."""
    return U * ref.abs() + 1e-7


# ================================================================= colsum

COLSUM_WPB = 4
COLSUM_EXACT_ROWS = [1, 3, 4, 5, 1023, 1024, 1025, 8224, 40000]
COLSUM_EXACT_C = [1, 7, 8, 9, 64, 65, 511, 512, 513, 1030, 1537, 2047, 2048]
COLSUM_EXACT_SHAPES = sorted(
    {(r, c) for r in COLSUM_EXACT_ROWS for c in (7, 65, 1030)}
    | {(r, c) for r in (5, 1025) for c in COLSUM_EXACT_C})
COLSUM_RANDOM_SHAPE = (1025, 1030)
# block counts the exact cases exist to reach: one wave per row below the
# 256-block floor, the first count above the floor, the 1024-block cap
COLSUM_BLOCKS = {1025: 256, 8224: 257, 40000: 1024}


def reduction_blocks(rows, waves_per_block=COLSUM_WPB, cap=1024):
    """Python copy of row_common.h reduction_blocks."""
    nblocks = min(max(rows // 32, 256), cap)
    return min(nblocks, (rows + waves_per_block - 1) // waves_per_block)


def colsum_nparts(rows):
    return reduction_blocks(rows) * COLSUM_WPB


@functools.lru_cache(maxsize=None)
def colsum_exact_case(rows, C):
    """(x bf16, bf16 of the int64 column sum). Integers in [-8, 8]: i.i.d. in
    [-6, 6] plus a row-dependent r % 5 - 2, so no two neighbouring rows are
    alike. Every fp32 partial sum is exact in any order (|sum| <= 8 * 40000 <
    2^24), so the kernel's result has to equal bf16(sum) bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(rows * 4099 + C)
    x = torch.randint(-6, 7, (rows, C), generator=g)
    x = x + (torch.arange(rows)[:, None] % 5 - 2)
    assert x.abs().max() <= 8
    want = x.sum(0).float().bfloat16()  # int64 -> fp32 is exact below 2^24
    return x.bfloat16(), want


def colsum_random_case(rows, C, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(rows, C, generator=g) * 0.5).bfloat16()


def colsum_depth(rows, nparts):
    """Length of one column's fp32 summation chain, see colsum_bound."""
    return -(-rows // nparts) + -(-nparts // 16) + 16


def colsum_bound(x, nparts=None):
    """|got - ref| <= U*|ref| + depth * 2^-24 * sum_r |x[r, c]|, ref the fp64
    column sum of the bf16 input.

    Roundings: the bf16 output (U). The fp32 summation chain of one column is
    ceil(rows/nparts) adds in the wave's register, ceil(nparts/16) adds in a
    finalize thread and 16 adds across the finalize rows; each add rounds a
    partial sum of magnitude <= sum|x| by 2^-24."""
    rows = x.shape[0]
    nparts = colsum_nparts(rows) if nparts is None else nparts
    depth = colsum_depth(rows, nparts)
    xd = x.double()
    return U * xd.sum(0).abs() + depth * F32 * xd.abs().sum(0)


def colsum_emul(x, nparts=None, drop_row=None, double_row=None):
    """The kernel's summation order in fp32: wave p owns rows p, p + nparts, ..;
    finalize thread y sums parts y, y + 16, ..; then the 16 rows in order.
    Defects: drop_row is left out, double_row is counted twice."""
    rows, C = x.shape
    nparts = colsum_nparts(rows) if nparts is None else nparts
    xf = x.float()
    order = list(range(rows))
    if drop_row is not None:
        order.remove(drop_row)
    if double_row is not None:
        order.append(double_row)
    part = torch.zeros(nparts, C)
    for r in order:  # ascending per wave, as the grid-stride loop visits them
        part[r % nparts] += xf[r]
    fin = torch.zeros(16, C)
    for p in range(nparts):
        fin[p % 16] += part[p]
    total = torch.zeros(C)
    for y in range(16):
        total = total + fin[y]
    return total.bfloat16()


# ================================================================= AdamW

ADAMW_NS = [1, 3, 4, 5, 7, 1023, ELEMENTWISE_BLOCK_CAP * ELEMENTWISE_THREADS * 4 + 5]
ADAMW_STEPS = [1, 2, 3, 10, 1000, 100000]
ADAMW_LR_WD = [(1e-3, 0.0), (1e-2, 0.1)]
ADAMW_BETAS = [(0.9, 0.999), (0.8, 0.95)]
ADAMW_EPS = 1e-8

# fp32 operations between (m', v') and the update lr/bc1 * m' / denom, each one
# rounding of 2^-24 relative to the update: sqrtf, the rounding of inv_bc2, the
# product with it, the rounding of eps, the add of eps (denominator: 5); the
# rounding of lr/bc1 and the product with m' (numerator: 2); the division (1).
# The eps rounding and the three on sqrt(v') * inv_bc2 act on different addends,
# so at most seven apply to any one update; the eighth is the share of the
# final FMA's rounding that falls on the update.
ADAMW_K = 8


@functools.lru_cache(maxsize=None)
def adamw_inputs(n, seed=0):
    """(p, m, v, g) fp32: m random, v = random^2, g log-uniform in [1e-8, 1e4]
    with random sign; every 7th element has g = 0 and v = 0 (denom = eps).
    Shared; never written to."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.randn(n, generator=gen).square()
    mag = torch.exp(torch.rand(n, generator=gen).double() * math.log(1e12) + math.log(1e-8))
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = (mag * sign).float()
    zero = torch.arange(n) % 7 == 3
    g[zero] = 0.0
    v[zero] = 0.0
    return p, m, v, g


def adamw_scalars(lr, beta1, beta2, wd, step):
    """The host scalars in double: (lr/bc1, 1/sqrt(bc2), 1 - lr*wd)."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return lr / bc1, 1.0 / math.sqrt(bc2), 1.0 - lr * wd


def adamw_moments_ref(m, v, g, beta1, beta2):
    """fp64 m' = m + (1-b1)(g - m), v' = b2 v + (1-b2) g^2."""
    m, v, g = m.double(), v.double(), g.double()
    return m + (1.0 - beta1) * (g - m), beta2 * v + (1.0 - beta2) * g * g


def adamw_param_ref(p, m_new, v_new, lr, beta1, beta2, eps, wd, step):
    """fp64 (p', update) of the header formula from given m', v':
    p' = p (1 - lr wd) - lr/bc1 * m' / (sqrt(v') / sqrt(bc2) + eps)."""
    step_size, inv_bc2, wd_factor = adamw_scalars(lr, beta1, beta2, wd, step)
    update = step_size * m_new.double() / (v_new.double().sqrt() * inv_bc2 + eps)
    return p.double() * wd_factor - update, update


def adamw_m_bound(m, g):
    """|m' - ref| <= 4 * 2^-24 * (|m| + |g|): the rounding of 1 - b1, the
    subtraction g - m, the product and the add, each <= 2^-24 * (|m| + |g|)."""
    return 4 * F32 * (m.double().abs() + g.double().abs())


def adamw_v_bound(v_ref):
    """|v' - ref| <= 4 * 2^-24 * ref. b2*v carries the rounding of b2 and of
    the product, (1-b2)*g*g the rounding of 1 - b2 and two products; both are
    non-negative, so the add's rounding on top makes (1 + 2^-24)^4 at most."""
    return 4 * F32 * v_ref


def adamw_p_bound(p, update_ref):
    """|p' - ref| <= 2^-23 * |p| + ADAMW_K * 2^-24 * |update_ref|, ref evaluated
    in fp64 from the m', v' the kernel produced (they have their own bounds).

    p * (1 - lr wd) - update is one FMA: the rounding of 1 - lr*wd and the
    FMA's own, each <= 2^-24 * |p| (the FMA's share on the update is counted
    in ADAMW_K). The scalar factors lr/bc1, 1/sqrt(bc2) and 1 - lr*wd get one
    fp32 rounding of their double value and no more."""
    return 2 * F32 * p.double().abs() + ADAMW_K * F32 * update_ref.abs()


def adamw_emul(p, m, v, g, lr, beta1, beta2, eps, wd, step, defect=None, host="double"):
    """adamw_kernel in torch fp32. host: 'double' computes the scalar factors in
    double and rounds each once; 'powf' is the fp32 powf launcher. Defects:
    'no_wd', 'no_bc1', 'no_bc2', 'eps_inside' ((sqrt(v) + eps) * inv_bc2),
    'eps_1e-3'. Returns (p', m', v')."""
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    step_size, inv_bc2, wd_factor = adamw_scalars(lr, beta1, beta2, wd, step)
    if host == "powf":
        b1, b2 = np.float32(beta1), np.float32(beta2)
        bc1 = np.float32(1) - np.power(b1, np.float32(step), dtype=np.float32)
        bc2 = np.float32(1) - np.power(b2, np.float32(step), dtype=np.float32)
        step_size = float(np.float32(lr) / bc1)
        inv_bc2 = float(np.float32(1) / np.sqrt(bc2))
        wd_factor = float(np.float32(1) - np.float32(lr * wd))
    if defect == "no_wd":
        wd_factor = 1.0
    if defect == "no_bc1":
        step_size = lr
    if defect == "no_bc2":
        inv_bc2 = 1.0
    if defect == "eps_1e-3":
        eps = 1e-3
    m_new = m + f(1.0 - beta1) * (g - m)
    v_new = f(beta2) * v + f(1.0 - beta2) * g * g
    if defect == "eps_inside":
        denom = (v_new.sqrt() + f(eps)) * f(inv_bc2)
    else:
        denom = v_new.sqrt() * f(inv_bc2) + f(eps)
    update = f(step_size) * m_new / denom
    p_new = (p.double() * float(f(wd_factor)) - update.double()).float()  # FMA
    return p_new, m_new, v_new


MASTER_SHAPES = [(37,), (100, 64), (8, 8, 8), (3,)]
MASTER_STEPS = 5
MASTER_HP = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
# fp32 roundings between the bf16 gradients and a clipped fp32 gradient: the
# squares (1), torch's norm reduction (a chain of at most 24 adds: vector
# lanes, a per-thread strip and a log2(n) tree), halved by the square root,
# the root itself, + 1e-6, the division and the final product: (1 + 24)/2 + 4,
# rounded up to 20.
CLIP_ROUNDINGS = 20


def master_inputs(seed=0):
    """(weights, per-step gradients): bf16 tensors of MASTER_SHAPES."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    w = [torch.randn(*s, generator=gen).bfloat16() for s in MASTER_SHAPES]
    gs = [[torch.randn(*s, generator=gen).bfloat16() for s in MASTER_SHAPES]
          for _ in range(MASTER_STEPS)]
    return w, gs


def master_reference(w, gs, max_grad_norm=0.0):
    """fp64 AdamW over the flat concatenation, fed the same bf16 gradients, with
    the error bounds of master, m and v accumulated over the steps.

    Returns (p, m, v, bound_p, bound_m, bound_v), all flat fp64. Per step the
    local bounds are adamw_m_bound, adamw_v_bound and adamw_p_bound; errors
    already present propagate with factor <= 1 into m (a convex combination),
    v (b2 < 1) and p (1 - lr wd < 1), an error dm in m' moves the update by
    step_size * dm / denom, a relative error dv/v in v' by at most half of it.
    Clipping adds CLIP_ROUNDINGS * 2^-24 * |g| to the gradient's error."""
    lr, (b1, b2), eps, wd = (MASTER_HP["lr"], MASTER_HP["betas"], MASTER_HP["eps"],
                             MASTER_HP["weight_decay"])
    p = torch.cat([t.flatten() for t in w]).double()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    ep, em, ev = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    for t, grads in enumerate(gs, start=1):
        g = torch.cat([t_.flatten() for t_ in grads]).double()
        eg = torch.zeros_like(g)
        if max_grad_norm > 0:
            g = g * min(max_grad_norm / (g.norm().item() + 1e-6), 1.0)
            eg = CLIP_ROUNDINGS * F32 * g.abs()
        # local bounds are taken at the fp32 inputs, which differ from the
        # fp64 ones by the accumulated bounds: add those before scaling
        em = em + (1.0 - b1) * eg + 4 * F32 * (m.abs() + em + g.abs() + eg)
        ev = ev + (1.0 - b2) * (2 * g.abs() + eg) * eg
        m, v = adamw_moments_ref(m, v, g, b1, b2)
        ev = ev + 4 * F32 * (v + ev)
        p_new, update = adamw_param_ref(p, m, v, lr, b1, b2, eps, wd, t)
        step_size, inv_bc2, _ = adamw_scalars(lr, b1, b2, wd, t)
        v_lo = (v - ev).clamp_min(0.0)
        denom_lo = v_lo.sqrt() * inv_bc2 + eps
        moved = step_size * em / denom_lo + (update.abs() + step_size * em / denom_lo) \
            * 0.5 * ev / v_lo.clamp_min(1e-300)
        ep = ep + moved + 2 * F32 * (p.abs() + ep) + ADAMW_K * F32 * (update.abs() + moved)
        p = p_new
    return p, m, v, ep, em, ev


# ================================================================= rotary

TWO_PI = 2.0 * math.pi
# absolute error of the hardware sine/cosine on a reduced argument; the
# starting value of the issue, see docs/kernels.md for the measurement
DELTA_HW = 2.0 ** -20


def rotary_delta(f):
    """delta(f) = 1.5 * 2^-24 * |f| + DELTA_HW: the angle error of the fast
    sine. f / 2pi is formed by one fp32 multiply (2^-24 * |f| in radians), the
    fp32 constant 1/2pi is itself off by at most 2^-25 relative (0.5 * 2^-24 *
    |f|), the hardware sine adds DELTA_HW absolute."""
    return 1.5 * F32 * f.double().abs() + DELTA_HW


def frequency_table(positions, rot):
    """(B, N, rot) fp32 table as core.position.FrequencyPositionEncoding builds
    it: pos * 10000^(-2i/rot), each entry repeated twice."""
    inv_freq = 1.0 / (10000 ** (torch.arange(0, rot, 2).float() / rot))
    return (positions.float().unsqueeze(-1) * inv_freq).repeat_interleave(2, dim=-1)


def _rot_parts(t, frq, rot):
    td = t.double()
    e, o = td[..., 0:rot:2], td[..., 1:rot:2]
    f = frq.double()[:, None, :, 0::2]  # (FB, 1, N, rot/2), entry 2i of each pair
    return td, e, o, f


def rotary_ref(t, frq, rot, neg_sin=False):
    """fp64 rotation of the first rot channels of t (B, H, N, D) by the table
    frq (FB, N, rot), interleaved pairs (2i, 2i+1); neg_sin is the transpose."""
    td, e, o, f = _rot_parts(t, frq, rot)
    cs, sn = torch.cos(f), torch.sin(f)
    if neg_sin:
        sn = -sn
    out = td.clone()
    out[..., 0:rot:2] = e * cs - o * sn
    out[..., 1:rot:2] = o * cs + e * sn
    return out


def rotary_bound(t, frq, rot, ref):
    """|out - ref| <= U*|ref| + (|t_e| + |t_o|) * delta(f) on the rotated span,
    0 (bit-equal) on the pass-through channels.

    Roundings: the bf16 output (U); cos and sin are each off by at most
    delta(f) and multiply t_e and t_o; the two fp32 products and the add are
    3 * 2^-24 and inside U's margin."""
    td, e, o, f = _rot_parts(t, frq, rot)
    amp = (e.abs() + o.abs()) * rotary_delta(f)
    bound = torch.zeros_like(td)
    bound[..., 0:rot:2] = amp
    bound[..., 1:rot:2] = amp
    bound[..., :rot] += U * ref[..., :rot].abs()
    return bound


def rotary_roundtrip_bound(t, frq, rot):
    """Bound on |R^T(R t) - t| after two kernel passes: (|t_e| + |t_o|) * (2U +
    4 delta(f)), |t| of the issue's 2u|t| read as the pair's |t_e| + |t_o| (a
    channel's error comes from both channels of its pair). The first pass
    leaves |e1| <= U|y| + (|t_e| + |t_o|) delta per channel; the second mixes
    the pair's two errors with weights cos, sin (cos^2 + sin^2 = 1) and adds
    its own. delta: (2 + sqrt2) <= 4. U: two roundings of typical size; the
    chain's worst case, (1 + sqrt2) U, needs both roundings of a pair at their
    maximum, aligned, at a 45 degree angle, and is not what the issue sets."""
    td, e, o, f = _rot_parts(t, frq, rot)
    amp = (e.abs() + o.abs()) * (2 * U + 4 * rotary_delta(f))
    bound = torch.zeros_like(td)
    bound[..., 0:rot:2] = amp
    bound[..., 1:rot:2] = amp
    return bound


def rotary_emul(t, frq, rot, neg_sin=False, defect=None, reduce=True):
    """rotary_kernel in fp32, bf16 out: r = fl(f * fl(1/2pi)), its fraction
    (exact), then sine and cosine of 2 pi r rounded to fp32. reduce=False
    models a sine that returns sin 0, cos 1 beyond 256 revolutions.
    Defects: 'flip_sin', 'half_split' (pairs (i, i + rot/2))."""
    tf = t.float()
    f = frq.float()[:, None, :, 0::2]
    r = f * torch.tensor(1.0 / TWO_PI, dtype=torch.float32)
    if reduce:
        r = r - torch.floor(r)
    ang = r.double() * TWO_PI
    sn, cs = torch.sin(ang).float(), torch.cos(ang).float()
    if not reduce:
        far = r.abs() > 256
        sn = torch.where(far, torch.zeros_like(sn), sn)
        cs = torch.where(far, torch.ones_like(cs), cs)
    if neg_sin != (defect == "flip_sin"):
        sn = -sn
    out = tf.clone()
    if defect == "half_split":
        h = rot // 2
        e, o = tf[..., :h], tf[..., h:rot]
        out[..., :h] = e * cs - o * sn
        out[..., h:rot] = o * cs + e * sn
    else:
        e, o = tf[..., 0:rot:2], tf[..., 1:rot:2]
        out[..., 0:rot:2] = e * cs - o * sn
        out[..., 1:rot:2] = o * cs + e * sn
    return out.bfloat16()


def rotary_case(name, seed=0):
    """(t bf16 (B,H,N,D), frq fp32 (FB,N,rot), rot) of a named case; the GPU
    tests build the strided variants from these."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen).bfloat16()
    if name in ("far64", "far128"):
        # right_align-style slice of a 0..8191 table: the last 16 rows
        rot = 64 if name == "far64" else 128
        table = frequency_table(torch.arange(8192)[None], rot)
        return rnd(2, 2, 16, 128), table[:, -16:, :], rot
    if name == "shifted":
        # FB = B with a different left-pad shift per batch element
        pos = (torch.arange(40)[None] - torch.tensor([[0], [7], [33]])).clamp(min=0)
        return rnd(3, 2, 40, 64), frequency_table(pos, 32), 32
    if name == "rot0":
        return rnd(2, 2, 5, 32), torch.zeros(1, 5, 0), 0
    if name == "rot_full":
        return rnd(2, 2, 5, 32), frequency_table(torch.arange(100, 105)[None], 32), 32
    if name == "odd_d":
        return rnd(2, 3, 5, 33), frequency_table(torch.arange(5)[None], 16), 16
    if name == "one_row":
        return rnd(2, 2, 1, 64), frequency_table(torch.tensor([[6143]]), 32), 32
    raise KeyError(name)


ROTARY_CASES = ["far64", "far128", "shifted", "rot0", "rot_full", "odd_d", "one_row"]


# ================================================================= transpose

TRANSPOSE_SHAPES = [(1, 1), (8, 8), (63, 65), (65, 63), (1, 129), (129, 1), (64, 71), (200, 7)]


def transpose_input(n, k):
    """(n, k) bf16 with a distinct bit pattern per element (arange as bf16
    bits, offset so the values are ordinary finite numbers)."""
    bits = (torch.arange(n * k, dtype=torch.int32) + 0x3000).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(n, k).clone()
