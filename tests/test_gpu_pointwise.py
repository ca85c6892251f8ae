"""GPU tests of the pointwise, column-sum and AdamW kernels against the fp64
oracle in tests/_pointwise_ref.py: gelu_bias, dropout_add, colsum_bf16,
adamw_step / MasterAdamW, rotary_apply, transpose_bf16.

Every bound is a function of _pointwise_ref with its roundings counted in the
docstring; test_pointwise_oracle.py shows on the CPU that the kernels'
arithmetic can meet each of them and that the defects these tests exist for
cannot. Each test prints its worst |got - ref| / bound before it asserts.
"""
import pytest
import torch

import _pointwise_ref as R

pytestmark = pytest.mark.gpu


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _ratio(name, got, want, bound):
    r = R.worst_ratio(got.cpu(), want, bound)
    print(f"{name}: worst |got - ref| / bound = {r:.4f}")
    return r


# ----------------------------------------------------------------- GELU

def test_gelu_exhaustive_bf16():
    x = R.all_finite_bf16()
    xg = x.cuda()
    v = x.float()
    y = _ext().gelu_bias_fwd(xg, None)
    y0 = _ext().gelu_bias_fwd(xg, torch.zeros(512, dtype=torch.bfloat16, device="cuda"))
    # b = 0 changes no bit of y, except at x = -0: IEEE gives -0 + 0 = +0, and
    # gelu keeps the sign of each zero
    yb, y0b = y.view(torch.int16).cpu(), y0.view(torch.int16).cpu()
    neg_zero = x.view(torch.int16) == -0x8000
    assert neg_zero.sum() == 1
    assert torch.equal(yb[~neg_zero], y0b[~neg_zero])
    assert yb[neg_zero].item() == -0x8000 and y0b[neg_zero].item() == 0
    yc = y.cpu()
    assert _ratio("gelu fwd exhaustive", yc, R.gelu_ref(v), R.gelu_fwd_bound(v)) <= 1.0
    assert (yc.float()[v < 0] <= 0).all()
    assert torch.equal(yc.float()[v >= 8], v[v >= 8])

    g = torch.Generator(device="cpu").manual_seed(1)
    for name, dy in (("ones", torch.ones_like(x)),
                     ("random", torch.randn(x.shape, generator=g).bfloat16())):
        dx = _ext().gelu_bias_bwd(xg, None, dy.cuda())
        ref = dy.double() * R.gelu_grad_ref(v)
        assert _ratio(f"gelu bwd exhaustive dy={name}", dx, ref, R.gelu_bwd_bound(v, dy)) <= 1.0


@pytest.mark.parametrize("rows,C", R.GELU_BIAS_SHAPES + [R.GELU_STRIDE_SHAPE])
def test_gelu_bias_indexing(rows, C):
    if (rows, C) == R.GELU_STRIDE_SHAPE:
        # more granules than the capped grid has threads: the loop's second trip
        assert rows * C > R.ELEMENTWISE_BLOCK_CAP * R.ELEMENTWISE_THREADS * 8
    x, b = R.gelu_bias_case(rows, C)
    v = R.gelu_pre(x, b)
    y = _ext().gelu_bias_fwd(x.cuda(), b.cuda())
    assert _ratio(f"gelu fwd {rows}x{C}", y, R.gelu_ref(v), R.gelu_fwd_bound(v)) <= 1.0
    g = torch.Generator(device="cpu").manual_seed(2)
    dy = torch.randn(x.shape, generator=g).bfloat16()
    dx = _ext().gelu_bias_bwd(x.cuda(), b.cuda(), dy.cuda())
    ref = dy.double() * R.gelu_grad_ref(v)
    assert _ratio(f"gelu bwd {rows}x{C}", dx, ref, R.gelu_bwd_bound(v, dy)) <= 1.0


def test_gelu_rejects_ragged_rows_and_takes_empty_input():
    x = torch.zeros(4, 12, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        _ext().gelu_bias_fwd(x, None)
    with pytest.raises(RuntimeError):
        _ext().gelu_bias_bwd(x, None, x)
    empty = torch.zeros(0, 16, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    assert _ext().gelu_bias_fwd(empty, bias).shape == (0, 16)
    assert _ext().gelu_bias_bwd(empty, bias, empty).shape == (0, 16)


# ----------------------------------------------------------------- dropout

def _gpu_mask(seed, p, n):
    ones = torch.ones(n, dtype=torch.bfloat16, device="cuda")
    return (_ext().dropout_add_fwd(ones, torch.zeros_like(ones), p, seed) != 0).cpu()


@pytest.mark.parametrize("n", [8, R.DROPOUT_N])
def test_dropout_mask_equals_the_hash_emulation(n):
    for seed in R.DROPOUT_SEEDS:
        for p in R.DROPOUT_PS:
            fwd = _gpu_mask(seed, p, n)
            assert torch.equal(fwd, R.dropout_keep(seed, p, n)), (seed, p)
            ones = torch.ones(n, dtype=torch.bfloat16, device="cuda")
            bwd = (_ext().dropout_add_bwd(ones, p, seed) != 0).cpu()
            assert torch.equal(bwd, fwd), (seed, p)  # one mask, no tolerated disagreement


@pytest.mark.parametrize("p", R.DROPOUT_PS)
def test_dropout_values(p):
    n, seed = 2 ** 16, 2 ** 40 + 5
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(n, generator=g).bfloat16()
    r = torch.randn(n, generator=g).bfloat16()
    dy = torch.randn(n, generator=g).bfloat16()
    keep = _gpu_mask(seed, p, n)
    inv_keep = R.dropout_inv_keep(p)

    out = _ext().dropout_add_fwd(x.cuda(), r.cuda(), p, seed).cpu()
    assert torch.equal(out[~keep].view(torch.int16), r[~keep].view(torch.int16))
    ref = x.double() * inv_keep + r.double()
    assert _ratio(f"dropout_add fwd p={p}", out[keep], ref[keep],
                  R.dropout_value_bound(ref[keep])) <= 1.0

    dx = _ext().dropout_add_bwd(dy.cuda(), p, seed).cpu()
    assert (dx[~keep] == 0).all()
    ref = dy.double() * inv_keep
    assert _ratio(f"dropout_add bwd p={p}", dx[keep], ref[keep], R.U * ref[keep].abs()) <= 1.0


@pytest.mark.parametrize("p", R.DROPOUT_PS)
def test_dropout_mask_statistics(p):
    for seed in R.DROPOUT_SEEDS:
        for name, (value, want, limit) in R.dropout_stats(_gpu_mask, seed, p, R.DROPOUT_N).items():
            assert abs(value - want) <= limit, (name, seed, p, value, want, limit)


# ----------------------------------------------------------------- colsum

@pytest.mark.parametrize("rows,C", R.COLSUM_EXACT_SHAPES)
def test_colsum_exact_on_small_integers(rows, C):
    if rows in R.COLSUM_BLOCKS:
        # the launch this row count exists to reach (row_common.h reduction_blocks)
        nblocks = min(max(rows // 32, 256), 1024)
        nblocks = min(nblocks, (rows + R.COLSUM_WPB - 1) // R.COLSUM_WPB)
        assert nblocks == R.COLSUM_BLOCKS[rows] == R.reduction_blocks(rows)
    x, want = R.colsum_exact_case(rows, C)
    got = _ext().colsum_bf16(x.cuda()).cpu()
    assert got.dtype == torch.bfloat16 and got.shape == (C,)
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()


def test_colsum_random_values():
    x = R.colsum_random_case(*R.COLSUM_RANDOM_SHAPE)
    got = _ext().colsum_bf16(x.cuda())
    assert _ratio("colsum (1025, 1030)", got, x.double().sum(0), R.colsum_bound(x)) <= 1.0


def test_colsum_rejects_wide_rows_and_sums_no_rows_to_zero():
    with pytest.raises(RuntimeError):
        _ext().colsum_bf16(torch.zeros(4, 2049, dtype=torch.bfloat16, device="cuda"))
    got = _ext().colsum_bf16(torch.zeros(0, 40, dtype=torch.bfloat16, device="cuda"))
    assert got.shape == (40,) and got.dtype == torch.bfloat16 and (got == 0).all()


# ----------------------------------------------------------------- AdamW

def adamw_direct_ratios(n, step, lr, wd, betas):
    """Worst |got - ref| / bound of (p', m', v') for one direct adamw_step call."""
    p, m, v, g = R.adamw_inputs(n)
    b1, b2 = betas
    pg, mg, vg, gg = p.cuda(), m.cuda(), v.cuda(), g.cuda()
    _ext().adamw_step(pg, mg, vg, gg, lr, b1, b2, R.ADAMW_EPS, wd, step)
    assert torch.equal(gg.cpu(), g)  # the gradient is read only
    m_ref, v_ref = R.adamw_moments_ref(m, v, g, b1, b2)
    # p' against the formula evaluated in fp64 at the m', v' the kernel wrote
    p_ref, upd = R.adamw_param_ref(p, mg.cpu(), vg.cpu(), lr, b1, b2, R.ADAMW_EPS, wd, step)
    return (R.worst_ratio(pg.cpu(), p_ref, R.adamw_p_bound(p, upd)),
            R.worst_ratio(mg.cpu(), m_ref, R.adamw_m_bound(m, g)),
            R.worst_ratio(vg.cpu(), v_ref, R.adamw_v_bound(v_ref)))


@pytest.mark.parametrize("n", R.ADAMW_NS)
def test_adamw_step_direct(n):
    if n == R.ADAMW_NS[-1]:
        # a second grid-stride trip of the float4 loop plus the scalar tail
        assert n > R.ELEMENTWISE_BLOCK_CAP * R.ELEMENTWISE_THREADS * 4 and n % 4 != 0
        grid = [(2, lr, wd, betas) for lr, wd in R.ADAMW_LR_WD for betas in R.ADAMW_BETAS]
        grid.append((1000, 1e-3, 0.0, R.ADAMW_BETAS[1]))
    else:
        grid = [(step, lr, wd, betas) for step in R.ADAMW_STEPS for lr, wd in R.ADAMW_LR_WD
                for betas in R.ADAMW_BETAS]
    worst = {}
    for step, lr, wd, betas in grid:
        rp, rm, rv = adamw_direct_ratios(n, step, lr, wd, betas)
        worst[step] = tuple(max(a, b) for a, b in zip(worst.get(step, (0, 0, 0)), (rp, rm, rv)))
    print(f"adamw_step n={n}: worst (p', m', v') / bound per step: {worst}")
    assert all(max(r) <= 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("max_grad_norm", [0.0, 0.5])
def test_master_adamw_fused_path(max_grad_norm):
    from perceiver_amd.train.optim import MasterAdamW

    w, gs = R.master_inputs()
    params = [torch.nn.Parameter(t.cuda()) for t in w]
    opt = MasterAdamW(params, max_grad_norm=max_grad_norm, **R.MASTER_HP)
    for grads in gs:
        for prm, g in zip(params, grads):
            prm.grad = g.cuda()
        opt.step()
    p_ref, m_ref, v_ref, ep, em, ev = R.master_reference(w, gs, max_grad_norm)
    fl = opt.state_dict()["fused_flat"][0]
    assert fl["step"] == R.MASTER_STEPS
    assert fl["master"].dtype == torch.float32 and fl["master"].numel() == p_ref.numel()
    assert _ratio("MasterAdamW master", fl["master"], p_ref, ep) <= 1.0
    assert _ratio("MasterAdamW m", fl["m"], m_ref, em) <= 1.0
    assert _ratio("MasterAdamW v", fl["v"], v_ref, ev) <= 1.0
    flat = torch.cat([prm.detach().flatten() for prm in params])
    assert torch.equal(flat.view(torch.int16), fl["master"].bfloat16().view(torch.int16))


# ----------------------------------------------------------------- rotary

@pytest.mark.parametrize("name", R.ROTARY_CASES)
def test_rotary_against_fp64(name):
    t, frq, rot = R.rotary_case(name)
    tg = t.cuda()
    fg = frq.cuda()
    if name.startswith("far"):
        # the slice of the long table itself: a storage offset on frq
        table = R.frequency_table(torch.arange(8192)[None], rot).cuda()
        fg = table[:, -16:, :]
        assert fg.storage_offset() > 0 and torch.equal(fg.cpu(), frq)
    for neg_sin in (False, True):
        ref = R.rotary_ref(t, frq, rot, neg_sin)
        out = _ext().rotary_apply(tg, fg, rot, neg_sin)
        assert out.shape == t.shape and out.is_contiguous()
        assert _ratio(f"rotary {name} neg_sin={neg_sin}", out, ref,
                      R.rotary_bound(t, frq, rot, ref)) <= 1.0
        assert torch.equal(out[..., rot:].cpu().view(torch.int16),
                           t[..., rot:].contiguous().view(torch.int16))
    back = _ext().rotary_apply(_ext().rotary_apply(tg, fg, rot, False), fg, rot, True)
    assert _ratio(f"rotary {name} round trip", back, t,
                  R.rotary_roundtrip_bound(t, frq, rot)) <= 1.0


def test_rotary_strided_inputs_are_bit_equal_to_contiguous():
    t, frq, rot = R.rotary_case("shifted")  # (3, 2, 40, 64), FB = B
    b, h, n, d = t.shape
    tg, fg = t.cuda(), frq.cuda()
    want = _ext().rotary_apply(tg, fg, rot, False)

    def same(view):
        assert view.shape == tg.shape and torch.equal(view, tg)
        got = _ext().rotary_apply(view, fg, rot, False)
        return torch.equal(got.view(torch.int16), want.view(torch.int16))

    # head-transposed view of a (B, N, H, D) buffer
    bnhd = tg.transpose(1, 2).contiguous()
    view = bnhd.transpose(1, 2)
    assert not view.is_contiguous() and same(view)
    # prefix of a longer cache: row and head strides of the cache
    cache = torch.zeros(b, h, n + 24, d + 16, dtype=torch.bfloat16, device="cuda")
    cache[:, :, :n, :d] = tg
    view = cache[:, :, :n, :d]
    assert view.stride() != tg.stride() and view.stride(3) == 1 and same(view)
    # last-dim stride 2: the contiguous() fallback
    wide = torch.zeros(b, h, n, 2 * d, dtype=torch.bfloat16, device="cuda")
    wide[..., ::2] = tg
    view = wide[..., ::2]
    assert view.stride(3) == 2 and same(view)


def test_rotary_table_batch_forms():
    t, frq, rot = R.rotary_case("shifted")
    tg = t.cuda()
    # FB = 1 and its stride-0 expansion to B give the same bits
    one = frq[:1].cuda()
    ref = R.rotary_ref(t, frq[:1], rot)
    got_one = _ext().rotary_apply(tg, one, rot, False)
    assert _ratio("rotary FB=1", got_one, ref, R.rotary_bound(t, frq[:1], rot, ref)) <= 1.0
    expanded = one.expand(t.shape[0], -1, -1)
    assert expanded.stride(0) == 0
    got_exp = _ext().rotary_apply(tg, expanded, rot, False)
    assert torch.equal(got_exp.view(torch.int16), got_one.view(torch.int16))
    # FB = B: each batch element is rotated by its own row of the table
    got_b = _ext().rotary_apply(tg, frq.cuda(), rot, False)
    assert torch.equal(got_b[0].view(torch.int16), got_one[0].view(torch.int16))
    assert not torch.equal(got_b[1], got_one[1]) and not torch.equal(got_b[2], got_one[2])


def test_rotary_empty_input():
    t = torch.zeros(2, 2, 0, 32, dtype=torch.bfloat16, device="cuda")
    frq = torch.zeros(1, 0, 16, device="cuda")
    assert _ext().rotary_apply(t, frq, 16, False).shape == (2, 2, 0, 32)


# ----------------------------------------------------------------- transpose

@pytest.mark.parametrize("n,k", R.TRANSPOSE_SHAPES)
def test_transpose_moves_every_element(n, k):
    x = R.transpose_input(n, k)
    got = _ext().transpose_bf16(x.cuda()).cpu()
    assert got.shape == (k, n) and got.is_contiguous()
    assert torch.equal(got.view(torch.int16), x.t().contiguous().view(torch.int16))


@pytest.mark.parametrize("n,k", [(0, 16), (16, 0)])
def test_transpose_empty(n, k):
    x = torch.zeros(n, k, dtype=torch.bfloat16, device="cuda")
    got = _ext().transpose_bf16(x)
    assert got.shape == (k, n) and got.numel() == 0
