"""CPU tests of the pointwise oracle (tests/_pointwise_ref.py).

They show, without a GPU, that every derived bound is one the kernels'
arithmetic can meet (an fp32 emulation of it stays inside the bound at the
inputs of every GPU case) and one that catches the defects the GPU tests exist
for (each named mutant lands >= 10x outside it on at least one case), that the
measured constants in the bounds are what the emulation shows, and that the
emulated dropout hash has the statistics the GPU mask is held to.
"""
import math

import pytest
import torch

import _pointwise_ref as R


# ----------------------------------------------------------------- GELU

def _gelu_cases():
    yield "exhaustive", R.all_finite_bf16(), None
    for rows, C in R.GELU_BIAS_SHAPES + [R.GELU_STRIDE_SHAPE]:
        x, b = R.gelu_bias_case(rows, C)
        yield f"{rows}x{C}", x, b


def _dy_like(x, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(x.shape, generator=g).bfloat16()


def test_eps_erf_and_eps_grad_are_the_measured_values():
    v = R.all_finite_bf16().float()
    k = torch.tensor(R.INV_SQRT2, dtype=torch.float32)
    erf_err = (R.erf_fast_emul(v * k).double()
               - torch.special.erf(v.double() * R.INV_SQRT2)).abs().max().item()
    cdf, xpdf = R.gelu_grad_emul_f32(v)
    grad_err = ((cdf + xpdf).double() - R.gelu_grad_ref(v)).abs().max().item()
    print(f"eps_erf measured {erf_err:.3e}, eps_grad measured {grad_err:.3e}")
    assert 0.9 * R.EPS_ERF_MEASURED <= erf_err <= R.EPS_ERF_MEASURED
    assert 0.9 * R.EPS_GRAD_MEASURED <= grad_err <= R.EPS_GRAD_MEASURED


def test_gelu_emulation_stays_inside_the_bounds():
    for name, x, b in _gelu_cases():
        v = R.gelu_pre(x, b)
        fwd = R.worst_ratio(R.gelu_fwd_emul(x, b), R.gelu_ref(v), R.gelu_fwd_bound(v))
        assert fwd <= 1.0, (name, fwd)
        for dy in (torch.ones_like(x), _dy_like(x)):
            ref = dy.double() * R.gelu_grad_ref(v)
            bwd = R.worst_ratio(R.gelu_bwd_emul(x, b, dy), ref, R.gelu_bwd_bound(v, dy))
            assert bwd <= 1.0, (name, bwd)


def test_gelu_emulation_sign_and_identity_tails():
    x = R.all_finite_bf16()
    v, y = x.float(), R.gelu_fwd_emul(x).float()
    assert (y[v < 0] <= 0).all()
    assert torch.equal(y[v >= 8], v[v >= 8])
    # a zero bias changes no bit, except at x = -0 (-0 + 0 = +0 in IEEE)
    yb = R.gelu_fwd_emul(x).view(torch.int16)
    y0b = R.gelu_fwd_emul(x, torch.zeros(512).bfloat16()).view(torch.int16)
    neg_zero = x.view(torch.int16) == -0x8000
    assert torch.equal(yb[~neg_zero], y0b[~neg_zero])
    assert yb[neg_zero].item() == -0x8000 and y0b[neg_zero].item() == 0


@pytest.mark.parametrize("defect", ["tanh", "bias_shift8", "no_bias"])
def test_gelu_forward_mutants_land_outside(defect):
    worst = 0.0
    for name, x, b in _gelu_cases():
        if name.endswith("x72") and name != "33x72":
            continue  # the small cases decide; spare the 4M-element one
        v = R.gelu_pre(x, b)
        worst = max(worst, R.worst_ratio(R.gelu_fwd_emul(x, b, defect=defect), R.gelu_ref(v),
                                         R.gelu_fwd_bound(v)))
    assert worst >= 10.0, worst


def test_gelu_backward_mutant_lands_outside():
    x = R.all_finite_bf16()
    v, dy = x.float(), torch.ones_like(x)
    ratio = R.worst_ratio(R.gelu_bwd_emul(x, None, dy, defect="no_xpdf"),
                          dy.double() * R.gelu_grad_ref(v), R.gelu_bwd_bound(v, dy))
    assert ratio >= 10.0, ratio


# ----------------------------------------------------------------- dropout

def test_rng_hash_known_values():
    # the mixing steps written out by hand for one input, so that a typo in
    # the numpy port cannot hide behind a matching typo in a second port
    seed, i, e = 2 ** 40 + 5, 3, 2
    x = (5 + (2 ** 8) * 0x9E3779B9 + i * 0xC2B2AE35 + e * 0x27D4EB2F) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    assert int(R.rng_hash(seed, 0, i, e)) == x
    assert int(R.dropout_draws(seed, 32)[8 * i + e]) == x


def test_dropout_threshold_and_scale():
    assert R.dropout_thresh(0.5) == 2 ** 31
    assert R.dropout_thresh(0.25) == 2 ** 30
    # 0.1 is not exact in fp32: the threshold follows float32(p)
    assert R.dropout_thresh(0.1) == int(0.10000000149011612 * 2 ** 32)
    assert R.dropout_inv_keep(0.5) == 2.0


@pytest.mark.parametrize("p", R.DROPOUT_PS)
def test_dropout_value_emulation_stays_inside_the_bound(p):
    g = torch.Generator(device="cpu").manual_seed(3)  # test_gpu_pointwise's inputs
    x = torch.randn(2 ** 16, generator=g).bfloat16()
    r = torch.randn(2 ** 16, generator=g).bfloat16()
    inv_keep = R.dropout_inv_keep(p)
    out = (x.float() * torch.tensor(inv_keep, dtype=torch.float32) + r.float()).bfloat16()
    ref = x.double() * inv_keep + r.double()
    assert R.worst_ratio(out, ref, R.dropout_value_bound(ref)) <= 1.0
    # the scale left out, the defect of a mask applied without 1 / (1 - p)
    unscaled = (x.float() + r.float()).bfloat16()
    assert R.worst_ratio(unscaled, ref, R.dropout_value_bound(ref)) >= 10.0


@pytest.mark.parametrize("p", R.DROPOUT_PS)
@pytest.mark.parametrize("seed", R.DROPOUT_SEEDS)
def test_emulated_mask_statistics(seed, p):
    for name, (value, want, limit) in R.dropout_stats(R.dropout_keep, seed, p, R.DROPOUT_N).items():
        assert abs(value - want) <= limit, (name, seed, p, value, want, limit)


# ----------------------------------------------------------------- colsum

def test_reduction_blocks_names_the_colsum_routes():
    for rows, blocks in R.COLSUM_BLOCKS.items():
        assert R.reduction_blocks(rows) == blocks
    # at most one row per wave up to 1024 rows; 1025 is the first second trip
    assert all(R.colsum_nparts(r) >= r for r in (1, 3, 4, 5, 1023, 1024))
    assert R.colsum_nparts(1025) == 1024


@pytest.mark.parametrize("rows,C", [(5, 7), (1025, 65), (1025, 1030)])
def test_colsum_emulation_is_exact_on_the_integer_cases(rows, C):
    x, want = R.colsum_exact_case(rows, C)
    assert torch.equal(R.colsum_emul(x), want)
    # a dropped and a doubled row both show, and differ from each other
    lost, twice = R.colsum_emul(x, drop_row=rows - 1), R.colsum_emul(x, double_row=rows - 1)
    assert not torch.equal(lost, want) and not torch.equal(twice, want)
    assert not torch.equal(lost, twice)


def test_colsum_random_case_emulation_and_mutants():
    x = R.colsum_random_case(*R.COLSUM_RANDOM_SHAPE)
    ref, bound = x.double().sum(0), R.colsum_bound(x)
    assert R.worst_ratio(R.colsum_emul(x), ref, bound) <= 1.0
    rows = x.shape[0]
    for row in (0, rows - 1):
        assert R.worst_ratio(R.colsum_emul(x, drop_row=row), ref, bound) >= 10.0
        assert R.worst_ratio(R.colsum_emul(x, double_row=row), ref, bound) >= 10.0
    # the old atol = 4.0 let an all-zero result through at (3, 2048)
    x3 = R.colsum_random_case(3, 2048)
    assert R.worst_ratio(torch.zeros(2048), x3.double().sum(0), R.colsum_bound(x3)) >= 10.0


@pytest.mark.parametrize("rows,C", [(401408, 261), (16384, 1792), (1000, 7), (3, 2048),
                                    (130, 1030)])
def test_colsum_bound_is_tighter_than_the_old_tolerance(rows, C):
    # shapes of test_gpu_kernels.test_colsum_matches_torch_sum; old: 4.0 + 1e-2 |ref|
    g = torch.Generator(device="cpu").manual_seed(0)
    x = (torch.randn(min(rows, 4096), C, generator=g) * 0.5).bfloat16()
    # relative part: U < 1e-2; absolute part, sum|x| scaled up from a 4096-row sample
    nparts = R.colsum_nparts(rows)
    depth = -(-rows // nparts) + -(-nparts // 16) + 16
    absolute = depth * R.F32 * (rows / x.shape[0]) * x.double().abs().sum(0)
    assert R.U < 1e-2 and (absolute < 4.0).all(), absolute.max().item()


# ----------------------------------------------------------------- AdamW

def _adamw_grid():
    for step in R.ADAMW_STEPS:
        for lr, wd in R.ADAMW_LR_WD:
            for betas in R.ADAMW_BETAS:
                yield step, lr, wd, betas


def _adamw_ratios(n, step, lr, wd, betas, **kw):
    p, m, v, g = R.adamw_inputs(n)
    b1, b2 = betas
    p_new, m_new, v_new = R.adamw_emul(p, m, v, g, lr, b1, b2, R.ADAMW_EPS, wd, step, **kw)
    m_ref, v_ref = R.adamw_moments_ref(m, v, g, b1, b2)
    p_ref, upd = R.adamw_param_ref(p, m_new, v_new, lr, b1, b2, R.ADAMW_EPS, wd, step)
    return (R.worst_ratio(p_new, p_ref, R.adamw_p_bound(p, upd)),
            R.worst_ratio(m_new, m_ref, R.adamw_m_bound(m, g)),
            R.worst_ratio(v_new, v_ref, R.adamw_v_bound(v_ref)))


def test_adamw_emulation_stays_inside_the_bounds():
    for n in (7, 1023):
        for step, lr, wd, betas in _adamw_grid():
            ratios = _adamw_ratios(n, step, lr, wd, betas)
            assert max(ratios) <= 1.0, (n, step, lr, wd, betas, ratios)


def test_adamw_fp32_powf_launcher_is_outside_the_bound():
    """The finding: bias corrections from fp32 powf miss the one-rounding
    clause in the early steps, double-precision host scalars meet it."""
    worst = {step: max(_adamw_ratios(1023, step, lr, wd, betas, host="powf")[0]
                       for lr, wd in R.ADAMW_LR_WD for betas in R.ADAMW_BETAS)
             for step in R.ADAMW_STEPS}
    print("powf launcher, worst |p' - ref| / bound per step:", worst)
    assert worst[2] > 1.0, worst


@pytest.mark.parametrize("defect", ["no_wd", "no_bc1", "no_bc2", "eps_inside", "eps_1e-3"])
def test_adamw_mutants_land_outside(defect):
    worst = max(_adamw_ratios(1023, step, lr, wd, betas, defect=defect)[0]
                for step, lr, wd, betas in _adamw_grid())
    assert worst >= 10.0, worst


def test_master_reference_bounds_are_small_and_finite():
    w, gs = R.master_inputs()
    for clip in (0.0, 0.5):
        p, m, v, ep, em, ev = R.master_reference(w, gs, clip)
        assert all(torch.isfinite(t).all() for t in (p, m, v, ep, em, ev))
        # accumulated over 5 steps the bounds stay at fp32 rounding level: far
        # below what a wrong hyperparameter moves (1e-2 * lr at the least)
        assert ep.max() < 1e-5 and (em <= 1e-5).all() and (ev <= 1e-5 * (1 + v)).all()


# ----------------------------------------------------------------- rotary

def test_fast_sine_costs_less_than_the_output_rounding():
    """The criterion that must hold in any case: delta(f) <= U/2 at position
    8192, channel 0 (f = 8192), beyond every shipped sequence length."""
    assert R.rotary_delta(torch.tensor(8192.0)).item() <= R.U / 2


@pytest.mark.parametrize("name", R.ROTARY_CASES)
@pytest.mark.parametrize("neg_sin", [False, True])
def test_rotary_emulation_stays_inside_the_bound(name, neg_sin):
    t, frq, rot = R.rotary_case(name)
    ref = R.rotary_ref(t, frq, rot, neg_sin)
    out = R.rotary_emul(t, frq, rot, neg_sin)
    assert R.worst_ratio(out, ref, R.rotary_bound(t, frq, rot, ref)) <= 1.0
    assert torch.equal(out[..., rot:], t[..., rot:])
    back = R.rotary_emul(out, frq, rot, not neg_sin)
    assert R.worst_ratio(back, t, R.rotary_roundtrip_bound(t, frq, rot)) <= 1.0


@pytest.mark.parametrize("defect", ["flip_sin", "half_split"])
def test_rotary_mutants_land_outside(defect):
    worst = 0.0
    for name in ("far64", "shifted", "rot_full"):
        t, frq, rot = R.rotary_case(name)
        ref = R.rotary_ref(t, frq, rot)
        worst = max(worst, R.worst_ratio(R.rotary_emul(t, frq, rot, defect=defect), ref,
                                         R.rotary_bound(t, frq, rot, ref)))
    assert worst >= 10.0, worst


def test_unreduced_fast_sine_lands_outside():
    # a sine that gives up beyond 256 revolutions (f > 1608) fails the large
    # position cases by far
    t, frq, rot = R.rotary_case("far64")
    ref = R.rotary_ref(t, frq, rot)
    ratio = R.worst_ratio(R.rotary_emul(t, frq, rot, reduce=False), ref,
                          R.rotary_bound(t, frq, rot, ref))
    assert ratio >= 10.0, ratio


# ----------------------------------------------------------------- transpose

def test_transpose_inputs_are_distinct_and_finite():
    for n, k in R.TRANSPOSE_SHAPES:
        x = R.transpose_input(n, k)
        assert torch.isfinite(x.float()).all()
        assert x.view(torch.int16).flatten().unique().numel() == n * k
        assert math.prod(x.shape) == n * k
