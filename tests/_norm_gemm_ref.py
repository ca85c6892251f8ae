"""Shared oracle for the LayerNorm and GEMM kernel tests
(test_norm_gemm_oracle.py on the CPU, test_gpu_layer_norm_bounds.py and
test_gpu_gemm_bounds.py on the GPU).

Holds the input families, the fp64 references, the derived error bounds and CPU
emulations of the kernels' fp32 arithmetic with switchable defects. Nothing
here touches a GPU. Conventions are those of _pointwise_ref.py: U = 2^-8 is one
bf16 rounding, F32 = 2^-24 one fp32 rounding, references are fp64 computed from
the bf16 / fp32 values the kernel receives (for ln_bwd that includes the mean
and rstd it is handed), and every bound's docstring counts its roundings. No
constant in a bound comes from a GPU run.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from _pointwise_ref import (F32, U, colsum_bound, colsum_depth, gelu_fwd_bound, gelu_pre,  # noqa: F401
                            gelu_ref, reduction_blocks, worst_ratio)

f32 = np.float32

# ================================================================= LayerNorm

LN_EPS = 1e-5
LN_WPB = 4        # waves (rows in flight) per block, layer_norm.hip
LN_MAXC = 2048    # row_common.h ROW_MAXC

# shapes of test_gpu_add_layer_norm.py plus a ragged four-chunk row
LN_SHAPES = [(1, 768), (5, 8), (37, 322), (259, 768), (2051, 1280), (1030, 2048), (33, 2047)]

# blocks of the fused backward's reduction grid at those row counts
LN_SHAPE_BLOCKS = {1: 1, 5: 2, 37: 10, 259: 65, 2051: 256, 1030: 256, 33: 9}

LN_EXACT_ROWS = [1, 3, 4, 5, 1023, 1024, 1025, 4097, 8224]
LN_EXACT_C = [8, 322, 1030, 2048]
# block counts the exact cases exist to reach: fewer rows than waves, one row
# per wave on the 256-block floor, a wave's second and ragged last trip, the
# first count above the floor
LN_EXACT_BLOCKS = {1: 1, 3: 1, 4: 1, 5: 2, 1023: 256, 1024: 256, 1025: 256, 4097: 256, 8224: 257}


def ln_chunks(C):
    return -(-C // 512)


def ln_chain(C):
    """Length of a row reduction's fp32 chain: a lane adds its 8 * CHUNKS
    elements in turn, then the six butterfly stages."""
    return 8 * ln_chunks(C) + 6


def _gen(rows, C, seed):
    return torch.Generator(device="cpu").manual_seed(seed * 1000003 + rows * 4099 + C)


def fam_normal(rows, C, seed=0):
    return torch.randn(rows, C, generator=_gen(rows, C, seed)).bfloat16()


def fam_offset100(rows, C, seed=0):
    return (torch.randn(rows, C, generator=_gen(rows, C, seed)) + 100.0).bfloat16()


def fam_offset1000(rows, C, seed=0):
    return (torch.randn(rows, C, generator=_gen(rows, C, seed)) * 8.0 + 1000.0).bfloat16()


def fam_one_off(rows, C, seed=0):
    """All 64.0, one element 64.5 per row, at a different column per row."""
    x = torch.full((rows, C), 64.0)
    col = (torch.arange(rows) * 7 + 3 + seed) % C
    x[torch.arange(rows), col] = 64.5
    return x.bfloat16()


def fam_two_valued(rows, C, seed=0):
    pick = torch.rand(rows, C, generator=_gen(rows, C, seed)) < 0.5
    return torch.where(pick, 64.0, 64.5).bfloat16()


def fam_constant(rows, C, seed=0):
    return torch.full((rows, C), 64.0).bfloat16()


def fam_tiny(rows, C, seed=0):
    return (torch.randn(rows, C, generator=_gen(rows, C, seed)) * 1e-3).bfloat16()


def fam_huge(rows, C, seed=0):
    return (torch.randn(rows, C, generator=_gen(rows, C, seed)) * 1e4).bfloat16()


LN_FAMILIES = {
    "normal": fam_normal,          # N(0, 1)
    "offset100": fam_offset100,    # N(100, 1)
    "offset1000": fam_offset1000,  # N(1000, 8)
    "one_off": fam_one_off,        # 64.0 with one 64.5 per row
    "two_valued": fam_two_valued,  # {64.0, 64.5} at random
    "constant": fam_constant,      # 64.0
    "tiny": fam_tiny,              # 1e-3 N(0, 1): eps dominates the variance
    "huge": fam_huge,              # 1e4 N(0, 1)
}
# the families on which sumsq / C - mean^2 loses its digits
LN_CANCELLING = ("offset100", "one_off", "two_valued")


@functools.lru_cache(maxsize=None)
def ln_params(C, seed=0):
    """(w, b) bf16: w = |N(0, 1)| + 0.5, b ~ N(0, 1); i.i.d. draws, so w[c + 8]
    in place of w[c] shows. Shared; never written to."""
    g = torch.Generator(device="cpu").manual_seed(seed * 7919 + C)
    w = (torch.randn(C, generator=g).abs() + 0.5).bfloat16()
    b = torch.randn(C, generator=g).bfloat16()
    return w, b


@functools.lru_cache(maxsize=None)
def ln_case(family, rows, C, seed=0):
    """(x, dy) bf16 of a family at a shape. Shared; never written to."""
    x = LN_FAMILIES[family](rows, C, seed)
    g = torch.Generator(device="cpu").manual_seed(seed * 31 + rows * 4099 + C + 17)
    dy = torch.randn(rows, C, generator=g).bfloat16()
    return x, dy


def ln_split_sum(s, seed=0):
    """(h, x) bf16 with bf16(h + x) == s bit for bit: h is s with its low four
    mantissa bits cleared, x the exact remainder (at most four bits wide)."""
    bits = s.view(torch.int16)
    h = (bits & ~0xF).view(torch.bfloat16)
    x = (s.float() - h.float()).bfloat16()
    assert torch.equal((h.float() + x.float()).bfloat16().view(torch.int16), bits)
    return h.clone(), x


# ---- references

def ln_stats_ref(x, eps=LN_EPS):
    """fp64 (mean, var, rstd) per row; eps as the kernel holds it, in fp32."""
    xd = x.double()
    mean = xd.mean(1)
    var = ((xd - mean[:, None]) ** 2).mean(1)
    return mean, var, 1.0 / torch.sqrt(var + float(f32(eps)))


def ln_y_ref(x, w, b, eps=LN_EPS):
    """(y, xhat * w) in fp64 from the fp64 statistics."""
    mean, _, rstd = ln_stats_ref(x, eps)
    xw = (x.double() - mean[:, None]) * rstd[:, None] * w.double()
    return (xw + b.double() if b is not None else xw), xw


def ln_bwd_terms(dy, x, w, mean, rstd):
    """fp64 (g, xhat, s1, s2) from the mean / rstd the kernel was handed."""
    g = dy.double() * w.double()
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    return g, xh, g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)


def ln_dx_ref(dy, x, w, mean, rstd):
    g, xh, s1, s2 = ln_bwd_terms(dy, x, w, mean, rstd)
    return rstd.double()[:, None] * (g - s1 - xh * s2)


def ln_dwdb_ref(dy, x, mean, rstd):
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    return (dy.double() * xh).sum(0), dy.double().sum(0)


# ---- bounds

def ln_mean_bound(x):
    """|mean - ref| <= (chain + 2) * 2^-24 * mean|x| per row.

    Roundings: chain adds of the row sum, each rounding a partial sum of
    magnitude <= sum|x|; the division by C; one more for the conversion of C
    and the first add, which round nothing today and keep the count safe
    against a reordering of the lane's run."""
    C = x.shape[1]
    return (ln_chain(C) + 2) * F32 * x.double().abs().mean(1)


def ln_rstd_rel_bound(x, eps=LN_EPS):
    """|rstd - ref| / ref <= (0.5 * (chain + 6) + 2) * 2^-24
                             + 0.5 * mean_bound^2 / (var + eps) per row.

    The variance is the centred sum of squares. Roundings, relative to var +
    eps: x - mean counts twice (it is squared), the square, the chain adds of
    non-negative terms, the division by C, the fp32 rounding of eps and the add
    of eps: chain + 6, halved by the power -1/2. rsqrtf is the hardware
    reciprocal square root, one ulp = 2 * 2^-24. The kernel centres on its own
    fp32 mean m~: sum (x - m~)^2 = sum (x - m)^2 + C (m~ - m)^2 exactly (the
    cross term vanishes), so the mean's error enters in second order only.

    A bound that described sumsq / C - mean^2 would carry chain * 2^-24 *
    mean^2 / (var + eps) instead; that is not what is asserted here."""
    C = x.shape[1]
    _, var, _ = ln_stats_ref(x, eps)
    second = 0.5 * ln_mean_bound(x) ** 2 / (var + float(f32(eps)))
    return (0.5 * (ln_chain(C) + 6) + 2) * F32 + second


def ln_y_bound(x, w, b, eps=LN_EPS):
    """|y - ref| <= U * |ref| + (rstd_rel + 3 * 2^-24) * |xhat * w|
                    + 2^-24 * (|xhat * w| + |b|) + mean_bound * rstd * |w|.

    Roundings: the bf16 output (U). x - mean, the product with rstd and the
    product with w are one fp32 rounding each and rstd carries rstd_rel, all
    relative to |xhat * w|; the add of b rounds |xhat * w + b| <= |xhat * w| +
    |b| once. The mean's own error moves every xhat of the row by mean_bound *
    rstd whatever |xhat| is, so it cannot ride on |xhat * w| and has its own
    term."""
    ref, xw = ln_y_ref(x, w, b, eps)
    _, _, rstd = ln_stats_ref(x, eps)
    rel = ln_rstd_rel_bound(x, eps)[:, None] + 3 * F32
    babs = b.double().abs() if b is not None else 0.0
    shift = (ln_mean_bound(x) * rstd)[:, None] * w.double().abs()
    return U * ref.abs() + rel * xw.abs() + F32 * (xw.abs() + babs) + shift


LN_DX_K = 10  # see ln_dx_bound


def ln_dx_bound(dy, x, w, mean, rstd):
    """|dx - ref| <= U * |ref| + (chain + 10) * 2^-24 * rstd *
                     (|g| + mean|g| + |xhat| * mean|g * xhat|), g = dy * w.

    dx = rstd * (g - s1 - xhat * s2) is a difference of three terms, so the
    fp32 part scales with the sum of their magnitudes. The longest count is the
    third term's: xhat (2: the subtraction and the product), s2 = mean(g *
    xhat) (g 1, xhat 2, the product 1, chain adds, the division 1), xhat * s2
    (1), the subtraction (1), the product with rstd (1): chain + 10. The second
    term needs chain + 5, the first 4."""
    C = x.shape[1]
    g, xh, _, _ = ln_bwd_terms(dy, x, w, mean, rstd)
    mag = g.abs() + g.abs().mean(1, keepdim=True) + xh.abs() * (g * xh).abs().mean(1, keepdim=True)
    ref = ln_dx_ref(dy, x, w, mean, rstd)
    return U * ref.abs() + (ln_chain(C) + LN_DX_K) * F32 * rstd.double().abs()[:, None] * mag


def ln_reduction_depth(rows, nblocks):
    """ceil(rows / (4 nblocks)) adds in a wave's registers, 3 across the block's
    four LDS slots, ceil(nblocks / 16) in a finalize thread, 16 across the
    finalize rows (the colsum_bound chain with the block combine added). The
    first add of each of the three accumulating stages is to a zero and exact;
    those three pay for the three roundings inside a dw term (x - mean, the
    product with rstd, the product with dy)."""
    return -(-rows // (LN_WPB * nblocks)) + 3 + -(-nblocks // 16) + 16


def ln_dwdb_bound(terms, nblocks):
    """|got - ref| <= U * |ref| + depth * 2^-24 * sum_r |terms[r, c]|, terms
    the fp64 addends (dy * xhat for dw, dy for db): colsum_bound's form with
    ln_reduction_depth."""
    depth = ln_reduction_depth(terms.shape[0], nblocks)
    return U * terms.sum(0).abs() + depth * F32 * terms.abs().sum(0)


def ln_fwd_ratios(x, w, b, y, mean, rstd, eps=LN_EPS):
    """Worst error / bound of (mean, rstd, y) as ln_fwd returned them; all on the CPU."""
    mean_ref, _, rstd_ref = ln_stats_ref(x, eps)
    return (worst_ratio(mean, mean_ref, ln_mean_bound(x)),
            worst_ratio(rstd, rstd_ref, ln_rstd_rel_bound(x, eps) * rstd_ref),
            worst_ratio(y, ln_y_ref(x, w, b, eps)[0], ln_y_bound(x, w, b, eps)))


def ln_bwd_ratios(dy, x, w, mean, rstd, dx=None, dw=None, db=None):
    """Worst error / bound of whichever of (dx, dw, db) ln_bwd returned, against
    the fp64 reference from the mean / rstd it was handed; all on the CPU."""
    out = []
    if dx is not None:
        out.append(worst_ratio(dx, ln_dx_ref(dy, x, w, mean, rstd),
                               ln_dx_bound(dy, x, w, mean, rstd)))
    if dw is not None:
        nblocks = reduction_blocks(x.shape[0], LN_WPB)
        xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        dw_ref, db_ref = ln_dwdb_ref(dy, x, mean, rstd)
        out.append(worst_ratio(dw, dw_ref, ln_dwdb_bound(dy.double() * xh, nblocks)))
        out.append(worst_ratio(db, db_ref, ln_dwdb_bound(dy.double(), nblocks)))
    return tuple(out)


# ---- emulations (numpy fp32, the kernel's lane-and-chunk layout)

def _lanes(a, C):
    """(rows, C) fp32 -> (rows, CHUNKS, 64, 8) zero padded, and the in-range mask."""
    rows, chunks = a.shape[0], ln_chunks(C)
    pad = np.zeros((rows, chunks * 512), f32)
    pad[:, :C] = a
    mask = np.zeros((rows, chunks * 512), bool)
    mask[:, :C] = True
    shape = (rows, chunks, 64, 8)
    return pad.reshape(shape), mask.reshape(shape)


def wave_sum_emul(lanes):
    """lanes (rows, 64) fp32 -> lane 0 of the xor butterfly, masks 1, 2, .., 32."""
    v = lanes.astype(f32)
    idx = np.arange(64)
    m = 1
    while m < 64:
        v = (v + v[:, idx ^ m]).astype(f32)
        m <<= 1
    return v[:, 0]


def _row_sum_emul(vals, mask):
    """Per-lane run over chunks and elements in the kernel's order (adding the
    padding's zeros is exact), then the butterfly."""
    acc = np.zeros((vals.shape[0], 64), f32)
    for i in range(vals.shape[1]):
        for e in range(8):
            acc = (acc + np.where(mask[:, i, :, e], vals[:, i, :, e], f32(0))).astype(f32)
    return wave_sum_emul(acc)


def ln_fwd_emul(x, w, b, eps=LN_EPS, defect=None):
    """ln_fwd_kernel in fp32 (no FMA): returns (y bf16, mean fp32, rstd fp32).

    Defects: 'one_pass' (the variance as sumsq / C - mean^2, clamped at 0: the
    formula before the fix), 'var_cm1' (variance over C - 1), 'eps_outside'
    (1 / (sqrt(var) + eps)), 'w_shift8' (w from column c + 8 in the ragged
    granule), 'no_bias'."""
    rows, C = x.shape
    xf = x.float().numpy()
    vals, mask = _lanes(xf, C)
    epsf, Cf = f32(eps), f32(C)
    mean = (_row_sum_emul(vals, mask) / Cf).astype(f32)
    if defect == "one_pass":
        sumsq = _row_sum_emul((vals * vals).astype(f32), mask)
        var = ((sumsq / Cf).astype(f32) - (mean * mean).astype(f32)).astype(f32)
        var = np.maximum(var, f32(0))
    else:
        d = (vals - mean[:, None, None, None]).astype(f32)
        var = (_row_sum_emul((d * d).astype(f32), mask)
               / (f32(C - 1) if defect == "var_cm1" else Cf)).astype(f32)
    if defect == "eps_outside":
        rstd = (f32(1) / (np.sqrt(var, dtype=f32) + epsf).astype(f32)).astype(f32)
    else:
        rstd = (f32(1) / np.sqrt((var + epsf).astype(f32), dtype=f32)).astype(f32)
    wf = w.float().numpy()
    if defect == "w_shift8" and C % 8:
        wf = wf.copy()
        c0 = C - C % 8
        wf[c0:] = w.float().numpy()[(np.arange(c0, C) + 8) % C]
    o = (((xf - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32) * wf).astype(f32)
    if b is not None and defect != "no_bias":
        o = (o + b.float().numpy()).astype(f32)
    return torch.from_numpy(o).bfloat16(), torch.from_numpy(mean), torch.from_numpy(rstd)


def ln_dx_emul(dy, x, w, mean, rstd, defect=None):
    """The dx arithmetic of both backward kernels in fp32 (no FMA), bf16 out.
    Defects: 'no_s2' (dx without the xhat * s2 term), 's1_512' (s1 summed over
    the first 512 columns only)."""
    rows, C = x.shape
    m, r = mean.numpy().astype(f32)[:, None], rstd.numpy().astype(f32)[:, None]
    g = (dy.float().numpy() * w.float().numpy()).astype(f32)
    xh = ((x.float().numpy() - m).astype(f32) * r).astype(f32)
    gl, mask = _lanes(g, C)
    xl, _ = _lanes(xh, C)
    m1 = mask.copy()
    if defect == "s1_512":
        m1[:, 1:] = False
    Cf = f32(C)
    s1 = (_row_sum_emul(gl, m1) / Cf).astype(f32)[:, None]
    s2 = (_row_sum_emul((gl * xl).astype(f32), mask) / Cf).astype(f32)[:, None]
    t = (g - s1).astype(f32)
    if defect != "no_s2":
        t = (t - (xh * s2).astype(f32)).astype(f32)
    return torch.from_numpy((r * t).astype(f32)).bfloat16()


def ln_reduce_emul(terms, nblocks, drop_row=None, double_row=None):
    """The fused backward's column reduction of fp32 addends terms (rows, C):
    wave p of nblocks * 4 owns rows p, p + nwaves, .. in ascending order; the
    block sums its four slots in wave order; finalize thread y sums blocks y,
    y + 16, ..; then the 16 finalize rows in order. bf16 out.
    Defects: drop_row is left out, double_row counted twice."""
    rows, C = terms.shape
    nw = nblocks * LN_WPB
    t = terms.astype(f32).copy()
    if drop_row is not None:
        t[drop_row] = 0  # adding a zero is exact: the same as skipping the row
    trips = -(-rows // nw)
    pad = np.zeros((trips * nw, C), f32)
    pad[:rows] = t
    pad = pad.reshape(trips, nw, C)
    part = np.zeros((nw, C), f32)
    for k in range(trips):
        part = (part + pad[k]).astype(f32)
    if double_row is not None:
        part[double_row % nw] = (part[double_row % nw] + t[double_row]).astype(f32)
    part = part.reshape(nblocks, LN_WPB, C)
    blk = part[:, 0]
    for v in range(1, LN_WPB):
        blk = (blk + part[:, v]).astype(f32)
    ftrips = -(-nblocks // 16)
    fpad = np.zeros((ftrips * 16, C), f32)
    fpad[:nblocks] = blk
    fpad = fpad.reshape(ftrips, 16, C)
    fin = np.zeros((16, C), f32)
    for k in range(ftrips):
        fin = (fin + fpad[k]).astype(f32)
    total = np.zeros(C, f32)
    for y in range(16):
        total = (total + fin[y]).astype(f32)
    return torch.from_numpy(total).bfloat16()


def ln_dwdb_terms_emul(dy, x, mean, rstd, defect=None):
    """fp32 (dy * xhat, dy) addends as the fused kernel forms them.
    Defect: 'dw_from_x' multiplies dy with x in place of xhat."""
    m, r = mean.numpy().astype(f32)[:, None], rstd.numpy().astype(f32)[:, None]
    d = dy.float().numpy()
    xf = x.float().numpy()
    xh = xf if defect == "dw_from_x" else ((xf - m).astype(f32) * r).astype(f32)
    return (d * xh).astype(f32), d


def ln_exact_case(rows, C):
    """(dy, x, ds, w, dw, db): dy and x integers in [-8, 8] (i.i.d. in [-6, 6]
    plus a row-dependent shift, so no two neighbouring rows are alike), to be
    run with mean = 0 and rstd = 1 planted so that xhat = x. Every partial sum
    of dy * x stays below 64 * 8224 < 2^24 and is exact in any order: dw has
    to equal bf16(sum dy * x) and db bf16(sum dy) bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(rows * 4099 + C + 5)
    shift = torch.arange(rows)[:, None] % 5 - 2
    dy = torch.randint(-6, 7, (rows, C), generator=g) + shift
    x = torch.randint(-6, 7, (rows, C), generator=g) - shift
    assert dy.abs().max() <= 8 and x.abs().max() <= 8
    w = (torch.randn(C, generator=g).abs() + 0.5).bfloat16()
    ds = (x * 3 - 1).bfloat16()  # any bf16 values: ds only picks the kernel arm here
    dw = (dy * x).sum(0).float().bfloat16()  # int64 -> fp32 exact below 2^24
    db = dy.sum(0).float().bfloat16()
    return dy.bfloat16(), x.bfloat16(), ds, w, dw, db


# ================================================================= GEMM

GEMM_BM, GEMM_BK = 256, 64
WGRAD_STEP = 64


def gemm_tile_width(M, N):
    """Python-side copy of gemm_bt.hip pick_bn (the launcher's choice is not
    exposed; a change there has to be made here too): the tile width with fewer idle
    slots in the last round of 256 CUs, the tie to 160."""
    def waste(bn):
        if N % bn:
            return 1 << 60
        g = (M // GEMM_BM) * (N // bn)
        return -(-g // 256) * 256 - g
    return 160 if waste(160) <= waste(128) else 128


def gemm_ref(x, w, b=None):
    y = x.double() @ w.double().t()
    return y + b.double() if b is not None else y


def gemm_bound(x, w, b=None, K=None, ref=None):
    """|y - ref| <= U * |ref| + 2 * (K + 2) * 2^-24 * (|x| @ |w|^T + |b|).

    Roundings: the bf16 output (U). The products of two bf16 are exact in
    fp32; a sum of K of them in fp32 rounds at most K - 1 times, the bias add
    once and two more are kept for the accumulator hand-over between MFMAs,
    each at most 2^-24 of |x| @ |w|^T + |b|. K is the length of the reduction
    (M for the weight gradient, plus nsplit for its slab sum). The factor 2 is
    for the MFMA's internal summation order and rounding mode, which the
    hardware guides do not specify (a truncating adder doubles a rounding)."""
    K = x.shape[1] if K is None else K
    ref = gemm_ref(x, w, b) if ref is None else ref
    mag = x.double().abs() @ w.double().abs().t()
    if b is not None:
        mag = mag + b.double().abs()
    return U * ref.abs() + 2 * (K + 2) * F32 * mag


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


@functools.lru_cache(maxsize=None)
def gemm_exact_case(M, N, K):
    """(x, w, b, y, y_nobias) of the exact family: integer x and w in [-4, 4],
    integer bias in [-8, 8]. |partial sum| <= 16 K + 8 < 2^24 in any order, so
    the output has to be bf16(int64 result) bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(M * 1009 + N * 31 + K)
    x, w, b = _ints(g, -4, 4, M, K), _ints(g, -4, 4, N, K), _ints(g, -8, 8, N)
    assert 16 * K + 8 < 2 ** 24
    acc = x.double() @ w.double().t()  # exact: integers below 2^53
    return (x.bfloat16(), w.bfloat16(), b.bfloat16(),
            (acc + b).float().bfloat16(), acc.float().bfloat16())


def gemm_random_case(M, N, K, seed=0):
    """As tests/test_gpu_gemm.py draws them: x ~ N(0, 1), w ~ 0.05 N(0, 1), b ~ N(0, 1)."""
    g = torch.Generator(device="cpu").manual_seed(seed * 77 + M + N * 3 + K * 7)
    return (torch.randn(M, K, generator=g).bfloat16(),
            (torch.randn(N, K, generator=g) * 0.05).bfloat16(),
            torch.randn(N, generator=g).bfloat16())


def _neighbour(t, g):
    """bf16 values up to two ulps away from t (same sign, t away from 0)."""
    step = torch.randint(-2, 3, t.shape, generator=g).to(torch.int16)
    return (t.view(torch.int16) + step).view(torch.bfloat16)


def gemm_cancelling_case(M, N, K, seed=0):
    """(x, w, None): columns of w come in pairs (a, -a) against x columns that
    are equal up to two bf16 ulps, so that |ref| is about 1e-3 of |x| @ |w|^T
    and the fp32 term of the bound binds, not U * |ref|."""
    g = torch.Generator(device="cpu").manual_seed(seed * 77 + M + N * 3 + K * 7 + 1)
    x = (torch.randn(M, K, generator=g).abs() + 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g) * 0.05).bfloat16()
    x[:, 1::2] = _neighbour(x[:, 0::2].contiguous(), g)
    w[:, 1::2] = -w[:, 0::2]
    return x, w, None


def gemm_cancelling_bias_case(M, N, K, seed=0):
    """(x, w, b): positive x and w, so that acc = |x| @ |w|^T, and b =
    -bf16(acc[0]) on the even columns. Row 0 of x is repeated every 37th row:
    there y = acc - bf16(acc), at most half a bf16 ulp of acc, which a bias
    added after the bf16 rounding turns into 0."""
    g = torch.Generator(device="cpu").manual_seed(seed * 77 + M + N * 3 + K * 7 + 2)
    x = (torch.randn(M, K, generator=g).abs() + 0.5).bfloat16()
    w = (torch.randn(N, K, generator=g).abs() * 0.05 + 0.01).bfloat16()
    x[::37] = x[0]
    acc0 = x[0].double() @ w.double().t()
    b = torch.zeros(N)
    b[0::2] = -acc0.float().bfloat16().float()[0::2]
    return x, w, b.bfloat16()


GEMM_FAMILIES = {"random": gemm_random_case, "cancelling": gemm_cancelling_case,
                 "cancelling_bias": gemm_cancelling_bias_case}

# gemm_bt exact cases: every kt_total % 3, the three-tile minimum and a peeled
# loop of two trips at M = 256; both tile widths, alone and several side by side
GEMM_EXACT_K = [192, 256, 320, 384, 576]
GEMM_EXACT_N = {128: 128, 160: 160, 480: 160, 640: 128}  # N -> expected tile width
GEMM_BIG = (4864, 1792, 192)  # 19 x 14 = 266 workgroups of 256 x 128
GEMM_BOUND_SHAPES = [(512, 256, 320), (512, 480, 384)]
GELU_SHAPES = [(256, 256, 192), (256, 480, 256)]  # tile 128, tile 160


def gemm_emul(x, w, b=None, defect=None):
    """gemm_bt_kernel in fp32: the accumulator takes one 32-wide MFMA block of
    K after another (the block's own sum in torch's fp32 order), the bias joins
    in fp32, one bf16 rounding. Returns (y, pre): pre is the bf16 accumulator
    without bias, the GELU variant's first output.
    Defects: 'drop_last_tile' (the last 64 of K left out), 'double_tile' (the
    second K-tile counted twice), 'bias_after_round' (bf16(bf16(acc) + b))."""
    xf, wf = x.float(), w.float()
    K = x.shape[1]
    blocks = list(range(0, K, 32))
    if defect == "drop_last_tile":
        blocks = blocks[:-2]
    if defect == "double_tile":
        blocks = blocks + [64, 96]
    acc = torch.zeros(x.shape[0], w.shape[0])
    for k0 in blocks:
        acc = acc + xf[:, k0:k0 + 32] @ wf[:, k0:k0 + 32].t()
    pre = acc.bfloat16()
    if b is None:
        return pre, pre
    if defect == "bias_after_round":
        return (pre.float() + b.float()).bfloat16(), pre
    return (acc + b.float()).bfloat16(), pre


def gelu_out_emul(pre, b, defect=None):
    """The GELU epilogue in fp64 from the bf16 pre (the erf polynomial has its
    own test in test_pointwise_oracle). Defect: 'no_bias'."""
    v = gelu_pre(pre, None if defect == "no_bias" else b)
    return gelu_ref(v).float().bfloat16()


# ---- weight gradient

# (M, N, K, tile_k, nsplit, rows_per_split): the pinned plans of
# tests/test_gpu_wgrad.py and one whose last split is a single 64-row step
# behind longer ones
WGRAD_CASES = [
    (64, 256, 128, 128, 1, 64),
    (320, 512, 384, 128, 5, 64),
    (320, 512, 768, 128, 3, 128),
    (1088, 512, 768, 128, 6, 192),
    (2048, 1792, 1280, 256, 7, 320),
]
WGRAD_BOUND_CASES = [WGRAD_CASES[3], WGRAD_CASES[1]]


def wgrad_ref(dy, x):
    return dy.double().t() @ x.double(), dy.double().sum(0)


def wgrad_bound(dy, x, nsplit):
    """gemm_bound with the reduction length M + nsplit (the slab sum adds
    nsplit - 1 roundings) on dw = dy^T @ x."""
    return gemm_bound(dy.t(), x.t(), K=dy.shape[0] + nsplit)


def wgrad_db_bound(dy, nsplit, rows_per_split):
    """colsum_bound with the chain of the fused sum. A column's M rows are
    summed in 8 * nsplit parts: per split the four lane groups of a fragment
    times the two halves of a packed bf16 pair, each adding rows_per_split / 8
    values in turn. The parts meet in 1 add (the pair), 2 shuffles and nsplit
    adds of the finalize kernel: rows_per_split / 8 + 3 + nsplit in all.
    colsum_bound counts ceil(M / nparts) + ceil(nparts / 16) + 16 for nparts
    parts; nparts is the largest count up to 8 * nsplit at which that is no
    shorter than the chain just counted."""
    M = dy.shape[0]
    chain = rows_per_split // 8 + 3 + nsplit
    nparts = 8 * nsplit
    while nparts > 1 and colsum_depth(M, nparts) < chain:
        nparts -= 1
    assert colsum_depth(M, nparts) >= chain
    return colsum_bound(dy, nparts=nparts)


@functools.lru_cache(maxsize=None)
def wgrad_exact_case(M, N, K):
    """(dy, x, dw, db): integers in [-4, 4]; |partial| <= 16 M < 2^24."""
    g = torch.Generator(device="cpu").manual_seed(M * 1013 + N * 37 + K)
    dy, x = _ints(g, -4, 4, M, N), _ints(g, -4, 4, M, K)
    assert 16 * M < 2 ** 24
    dw = dy.double().t() @ x.double()  # exact: integers below 2^53
    return dy.bfloat16(), x.bfloat16(), dw.float().bfloat16(), dy.sum(0).float().bfloat16()


def wgrad_random_case(M, N, K, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed * 79 + M + N * 3 + K * 7)
    return (torch.randn(M, N, generator=g).bfloat16(),
            (torch.randn(M, K, generator=g) * 0.05).bfloat16())


def wgrad_cancelling_case(M, N, K, rows_per_split, seed=0):
    """(dy, x): positive dy and x in the even splits; every row of an odd
    split mirrors the row one split earlier with dy negated and x up to two
    bf16 ulps away; rows without a partner have dy = 0. The fp32 slabs are
    then large and opposite, |dw| about 1e-3 of |dy|^T @ |x|: the fp32 term of
    the bound binds, and a slab rounded to bf16 before the sum shows."""
    g = torch.Generator(device="cpu").manual_seed(seed * 79 + M + N * 3 + K * 7 + 1)
    dy = (torch.randn(M, N, generator=g).abs() + 0.5).bfloat16()
    x = (torch.randn(M, K, generator=g).abs() * 0.05 + 0.01).bfloat16()
    r = rows_per_split
    for s in range(0, -(-M // r), 2):
        lo, mid, hi = s * r, min((s + 1) * r, M), min((s + 2) * r, M)
        n = hi - mid
        dy[mid:hi] = -dy[lo:lo + n]
        x[mid:hi] = _neighbour(x[lo:lo + n].contiguous(), g)
        dy[lo + n:mid] = 0
    return dy, x


def wgrad_emul(dy, x, nsplit, rows_per_split, defect=None):
    """gemm_wgrad in fp32: per split the accumulator takes one 32-row MFMA
    block after another, the finalize kernel sums the slabs in split order and
    rounds once. Returns (dw, db) bf16. Defects: 'bf16_slabs' (each slab
    rounded to bf16 before the sum), 'drop_last_split'."""
    dyf, xf = dy.float(), x.float()
    M = dy.shape[0]
    dw = torch.zeros(dy.shape[1], x.shape[1])
    db = torch.zeros(dy.shape[1])
    splits = range(nsplit - 1 if defect == "drop_last_split" else nsplit)
    for s in splits:
        lo, hi = s * rows_per_split, min(M, (s + 1) * rows_per_split)
        acc = torch.zeros_like(dw)
        dacc = torch.zeros_like(db)
        for m0 in range(lo, hi, 32):
            acc = acc + dyf[m0:m0 + 32].t() @ xf[m0:m0 + 32]
            dacc = dacc + dyf[m0:m0 + 32].sum(0)
        if defect == "bf16_slabs":
            acc = acc.bfloat16().float()
        dw = dw + acc
        db = db + dacc
    return dw.bfloat16(), db.bfloat16()
