"""CPU tests of the LayerNorm / GEMM oracle (tests/_norm_gemm_ref.py).

They show, without a GPU, that every derived bound is one the kernels'
arithmetic can meet (an fp32 emulation with the kernel's lane-and-chunk layout
and xor butterfly stays inside it at every GPU case's shape and every input
family) and one that catches the defects the GPU tests exist for (each named
mutant lands >= 10x outside it on a family named here). The one-pass variance
mutant is the regression test of the variance fix in ln_fwd_kernel: far outside
on the offset and near-constant families, inside on N(0, 1), which is why
N(0, 1)-only tests never saw it.
"""
import pytest
import torch

import _norm_gemm_ref as R

# every shape of the GPU tests, and a three-chunk ragged row
EMUL_SHAPES = R.LN_SHAPES + [(9, 1030)]
# the mutants are decided at few rows: the rows of a family are alike
SMALL_SHAPES = sorted({(min(rows, 9), C) for rows, C in EMUL_SHAPES})


def _fwd_ratios(family, rows, C, with_bias=True, defect=None):
    x, _ = R.ln_case(family, rows, C)
    w, b = R.ln_params(C)
    b = b if with_bias else None
    y, mean, rstd = R.ln_fwd_emul(x, w, b, defect=defect)
    mean_ref, _, rstd_ref = R.ln_stats_ref(x)
    y_ref, _ = R.ln_y_ref(x, w, b)
    return (R.worst_ratio(mean, mean_ref, R.ln_mean_bound(x)),
            R.worst_ratio(rstd, rstd_ref, R.ln_rstd_rel_bound(x) * rstd_ref),
            R.worst_ratio(y, y_ref, R.ln_y_bound(x, w, b)))


# ----------------------------------------------------------------- LayerNorm forward

@pytest.mark.parametrize("family", list(R.LN_FAMILIES))
def test_ln_fwd_emulation_stays_inside_the_bounds(family):
    for rows, C in EMUL_SHAPES:
        for with_bias in (True, False):
            ratios = _fwd_ratios(family, rows, C, with_bias)
            assert max(ratios) <= 1.0, (family, rows, C, with_bias, ratios)


def test_ln_fwd_emulation_on_constant_rows_is_exact():
    for rows, C in EMUL_SHAPES:
        x, _ = R.ln_case("constant", rows, C)
        w, b = R.ln_params(C)
        y, mean, rstd = R.ln_fwd_emul(x, w, b)
        assert torch.equal(mean, torch.full((rows,), 64.0))
        assert torch.equal(y.view(torch.int16), b.expand(rows, C).contiguous().view(torch.int16))
        y0, _, _ = R.ln_fwd_emul(x, w, None)
        assert not y0.view(torch.int16).any()  # +0 everywhere


def test_one_pass_variance_is_far_outside_on_offset_rows_and_inside_on_n01():
    """Finding 1: sumsq / C - mean^2 in fp32."""
    shapes = [(9, 322), (9, 768), (9, 1280), (9, 2048)]
    for family in R.LN_CANCELLING:
        rstd = max(_fwd_ratios(family, r, C, defect="one_pass")[1] for r, C in shapes)
        yy = max(_fwd_ratios(family, r, C, defect="one_pass")[2] for r, C in shapes)
        print(f"one-pass variance, {family}: rstd error / bound {rstd:.3g}, y {yy:.3g}")
        assert rstd >= 10.0, (family, rstd)
        # on N(100, 1) the rstd error is 2e-4 relative, below y's own bf16
        # rounding; the near-constant rows get y itself wrong by a factor
        assert family == "offset100" or yy >= 10.0, (family, yy)
    for r, C in shapes:
        assert max(_fwd_ratios("normal", r, C, defect="one_pass")) <= 1.0


@pytest.mark.parametrize("defect,family,which", [
    ("var_cm1", "normal", 1),      # rstd off by 1 / 2C
    ("eps_outside", "tiny", 1),    # eps dominates the variance
    ("w_shift8", "normal", 2),     # the ragged granule of C = 322 / 1030 / 2047
    ("no_bias", "normal", 2),
])
def test_ln_fwd_mutants_land_outside(defect, family, which):
    worst = max(_fwd_ratios(family, r, C, defect=defect)[which] for r, C in SMALL_SHAPES)
    assert worst >= 10.0, worst
    if defect == "var_cm1":  # at every width, the widest included
        assert _fwd_ratios(family, 9, 2048, defect=defect)[1] >= 10.0


def test_split_sum_reproduces_the_family_row():
    for family in R.LN_FAMILIES:
        s, _ = R.ln_case(family, 9, 322)
        h, x = R.ln_split_sum(s)
        assert torch.equal((h.float() + x.float()).bfloat16().view(torch.int16),
                           s.view(torch.int16))
    assert R.ln_split_sum(R.ln_case("two_valued", 9, 322)[0])[1].any()


# ----------------------------------------------------------------- LayerNorm backward

def _stats(family, x, planted):
    """The statistics ln_bwd is handed: the forward emulation's own, or planted
    ones (a mean and rstd that belong to no row)."""
    rows = x.shape[0]
    if planted:
        return (torch.linspace(-0.5, 0.5, rows, dtype=torch.float32),
                torch.linspace(0.5, 2.0, rows, dtype=torch.float32))
    _, mean, rstd = R.ln_fwd_emul(x, *R.ln_params(x.shape[1]))
    return mean, rstd


def _dx_ratio(family, rows, C, planted=False, defect=None):
    x, dy = R.ln_case(family, rows, C)
    w, _ = R.ln_params(C)
    mean, rstd = _stats(family, x, planted)
    return R.worst_ratio(R.ln_dx_emul(dy, x, w, mean, rstd, defect=defect),
                         R.ln_dx_ref(dy, x, w, mean, rstd), R.ln_dx_bound(dy, x, w, mean, rstd))


def _dwdb_ratios(family, rows, C, planted=False, defect=None, **rowdefect):
    x, dy = R.ln_case(family, rows, C)
    mean, rstd = _stats(family, x, planted)
    nblocks = R.reduction_blocks(rows, R.LN_WPB)
    tw, tb = R.ln_dwdb_terms_emul(dy, x, mean, rstd, defect=defect)
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    ref_w, ref_b = R.ln_dwdb_ref(dy, x, mean, rstd)
    return (R.worst_ratio(R.ln_reduce_emul(tw, nblocks, **rowdefect), ref_w,
                          R.ln_dwdb_bound(dy.double() * xh, nblocks)),
            R.worst_ratio(R.ln_reduce_emul(tb, nblocks, **rowdefect), ref_b,
                          R.ln_dwdb_bound(dy.double(), nblocks)))


@pytest.mark.parametrize("family", list(R.LN_FAMILIES))
def test_ln_bwd_emulation_stays_inside_the_bounds(family):
    for rows, C in EMUL_SHAPES:
        for planted in (False, True):
            r = _dx_ratio(family, rows, C, planted)
            assert r <= 1.0, (family, rows, C, planted, r)
            rw, rb = _dwdb_ratios(family, rows, C, planted)
            assert max(rw, rb) <= 1.0, (family, rows, C, planted, rw, rb)


@pytest.mark.parametrize("rows,C", [(2051, 322), (1030, 8)])
def test_ln_dwdb_emulation_at_many_rows(rows, C):
    # more rows than waves in the reduction grid: the register chain, and the
    # finalize chain over 256 blocks
    for family in ("normal", "offset100"):
        assert max(_dwdb_ratios(family, rows, C)) <= 1.0


@pytest.mark.parametrize("defect", ["no_s2", "s1_512"])
def test_ln_dx_mutants_land_outside(defect):
    shapes = [(9, 768), (9, 1280), (9, 2047)]  # s1_512 needs a second chunk
    worst = max(_dx_ratio("normal", r, C, defect=defect) for r, C in shapes)
    assert worst >= 10.0, worst


def test_ln_dwdb_mutants_land_outside():
    # dw from x in place of xhat: on rows that are not already normalised
    assert _dwdb_ratios("offset100", 37, 322, defect="dw_from_x")[0] >= 10.0
    for rows, C in ((37, 322), (2051, 322)):
        for row in (0, rows - 1):
            assert min(_dwdb_ratios("normal", rows, C, drop_row=row)) >= 10.0
            assert min(_dwdb_ratios("normal", rows, C, double_row=row)) >= 10.0


def test_reduction_blocks_names_the_exact_cases_routes():
    for rows, blocks in R.LN_EXACT_BLOCKS.items():
        assert R.reduction_blocks(rows, R.LN_WPB) == blocks
    assert set(R.LN_EXACT_BLOCKS) == set(R.LN_EXACT_ROWS)
    for rows, _ in R.LN_SHAPES:
        assert R.reduction_blocks(rows, R.LN_WPB) == R.LN_SHAPE_BLOCKS[rows]
    # a wave's second trip starts at 1025 rows, a ragged last one at 4097
    assert 4 * 256 < 1025 and 4097 % (4 * 256) == 1


@pytest.mark.parametrize("rows,C", [(5, 8), (1025, 322), (4097, 8)])
def test_ln_exact_case_emulation_is_exact(rows, C):
    dy, x, _, _, dw, db = R.ln_exact_case(rows, C)
    mean, rstd = torch.zeros(rows), torch.ones(rows)
    nblocks = R.reduction_blocks(rows, R.LN_WPB)
    tw, tb = R.ln_dwdb_terms_emul(dy, x, mean, rstd)
    assert torch.equal(R.ln_reduce_emul(tw, nblocks), dw)
    assert torch.equal(R.ln_reduce_emul(tb, nblocks), db)
    lost = R.ln_reduce_emul(tw, nblocks, drop_row=rows - 1)
    twice = R.ln_reduce_emul(tw, nblocks, double_row=rows - 1)
    assert not torch.equal(lost, dw) and not torch.equal(twice, dw)


def test_derived_ln_bounds_are_below_the_old_tolerances():
    """On the N(0, 1) inputs of the older tests in test_gpu_kernels.py the derived
    y and dx bounds are the smaller ones elementwise (old: y atol = rtol = 3e-2, dx
    5e-2). The old assertions stay all the same; this only shows that the new
    ones ask more there."""
    for rows, C in [(400, 512), (400, 322), (37, 1540), (3, 2048), (259, 768)]:
        x, dy = R.ln_case("normal", rows, C)
        w, b = R.ln_params(C)
        y_ref, _ = R.ln_y_ref(x, w, b)
        assert (R.ln_y_bound(x, w, b) < 3e-2 + 3e-2 * y_ref.abs()).all()
        _, mean, rstd = R.ln_fwd_emul(x, w, b)
        dx_ref = R.ln_dx_ref(dy, x, w, mean, rstd)
        assert (R.ln_dx_bound(dy, x, w, mean, rstd) < 5e-2 + 5e-2 * dx_ref.abs()).all()
        # dw/db: U * |ref| exceeds the old 0.04 * mean|ref| + 0.08 where |ref| > 20,
        # so neither of the two is the smaller one everywhere


# ----------------------------------------------------------------- GEMM

def _gemm_ratio(family, M, N, K, defect=None):
    x, w, b = R.GEMM_FAMILIES[family](M, N, K)
    y, _ = R.gemm_emul(x, w, b, defect=defect)
    return R.worst_ratio(y, R.gemm_ref(x, w, b), R.gemm_bound(x, w, b))


@pytest.mark.parametrize("M,N,K", R.GEMM_BOUND_SHAPES)
def test_gemm_emulation_stays_inside_the_bound(M, N, K):
    for family in R.GEMM_FAMILIES:
        r = _gemm_ratio(family, M, N, K)
        assert r <= 1.0, (family, r)
    x, w, b = R.gemm_random_case(M, N, K)
    y, _ = R.gemm_emul(x, w, None)
    assert R.worst_ratio(y, R.gemm_ref(x, w), R.gemm_bound(x, w)) <= 1.0


def test_gemm_cancelling_family_makes_the_fp32_term_bind():
    for M, N, K in R.GEMM_BOUND_SHAPES:
        x, w, _ = R.gemm_cancelling_case(M, N, K)
        ref = R.gemm_ref(x, w)
        mag = x.double().abs() @ w.double().abs().t()
        assert ref.abs().median() < 2e-3 * mag.median()
        fp32_term = 2 * (K + 2) * R.F32 * mag
        assert (fp32_term > R.U * ref.abs()).double().mean() > 0.9


def test_gemm_exact_family_emulation_is_exact():
    for K in R.GEMM_EXACT_K:
        x, w, b, y, y0 = R.gemm_exact_case(256, 160, K)
        assert torch.equal(R.gemm_emul(x, w, b)[0], y)
        assert torch.equal(R.gemm_emul(x, w, None)[0], y0)
        assert torch.equal(R.gemm_emul(x, w, b)[1], y0)  # pre ignores the bias
        for defect in ("drop_last_tile", "double_tile"):
            assert not torch.equal(R.gemm_emul(x, w, b, defect=defect)[0], y)


def test_gemm_tile_widths_and_the_second_round():
    for N, bn in R.GEMM_EXACT_N.items():
        assert R.gemm_tile_width(256, N) == bn
    M, N, K = R.GEMM_BIG
    bn = R.gemm_tile_width(M, N)
    blocks = (M // 256) * (N // bn)
    assert (bn, blocks, blocks % 8) == (128, 266, 2)
    assert [R.gemm_tile_width(M, N) for M, N, _ in R.GELU_SHAPES] == [128, 160]
    assert [R.gemm_tile_width(M, N) for M, N, _ in R.GEMM_BOUND_SHAPES] == [128, 160]


@pytest.mark.parametrize("defect,family", [
    ("drop_last_tile", "random"), ("double_tile", "random"),
    ("drop_last_tile", "cancelling"), ("bias_after_round", "cancelling_bias"),
])
def test_gemm_mutants_land_outside(defect, family):
    worst = max(_gemm_ratio(family, M, N, K, defect) for M, N, K in R.GEMM_BOUND_SHAPES)
    assert worst >= 10.0, worst


def test_gelu_from_pre_without_the_bias_lands_outside():
    for M, N, K in R.GELU_SHAPES:
        x, w, b = R.gemm_random_case(M, N, K)
        _, pre = R.gemm_emul(x, w, b)
        v = R.gelu_pre(pre, b)
        ref, bound = R.gelu_ref(v), R.gelu_fwd_bound(v)
        assert R.worst_ratio(R.gelu_out_emul(pre, b), ref, bound) <= 1.0
        assert R.worst_ratio(R.gelu_out_emul(pre, b, defect="no_bias"), ref, bound) >= 10.0


# ----------------------------------------------------------------- weight gradient

def _wgrad_ratios(family, case, defect=None):
    M, N, K, _, nsplit, rps = case
    dy, x = (R.wgrad_random_case(M, N, K) if family == "random"
             else R.wgrad_cancelling_case(M, N, K, rps))
    dw, db = R.wgrad_emul(dy, x, nsplit, rps, defect=defect)
    ref_w, ref_b = R.wgrad_ref(dy, x)
    return (R.worst_ratio(dw, ref_w, R.wgrad_bound(dy, x, nsplit)),
            R.worst_ratio(db, ref_b, R.wgrad_db_bound(dy, nsplit, rps)))


@pytest.mark.parametrize("case", R.WGRAD_BOUND_CASES)
def test_wgrad_emulation_stays_inside_the_bounds(case):
    for family in ("random", "cancelling"):
        ratios = _wgrad_ratios(family, case)
        assert max(ratios) <= 1.0, (family, ratios)


def test_wgrad_exact_family_emulation_is_exact():
    for M, N, K, _, nsplit, rps in R.WGRAD_CASES[:4]:
        dy, x, dw, db = R.wgrad_exact_case(M, N, K)
        got = R.wgrad_emul(dy, x, nsplit, rps)
        assert torch.equal(got[0], dw) and torch.equal(got[1], db)
    for M, _, _, _, nsplit, rps in R.WGRAD_CASES:  # 8 * nsplit parts cover the chain as they are
        assert R.colsum_depth(M, 8 * nsplit) >= rps // 8 + 3 + nsplit


def test_wgrad_mutants_land_outside():
    for case in R.WGRAD_BOUND_CASES:
        assert _wgrad_ratios("cancelling", case, defect="bf16_slabs")[0] >= 10.0, case
    # the last, shorter split dropped: (1088, ..) ends in a 128-row split
    rw, rb = _wgrad_ratios("random", R.WGRAD_CASES[3], defect="drop_last_split")
    assert rw >= 10.0 and rb >= 10.0, (rw, rb)
    # bf16 slabs hide on the random family, which is why the cancelling one exists
    assert _wgrad_ratios("random", R.WGRAD_CASES[3], defect="bf16_slabs")[0] < 10.0
