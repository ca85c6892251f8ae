"""Residual add + LayerNorm in one pass (add_ln_fwd, ln_bwd with a residual
gradient ds, AddLayerNormFn) against the kernels and the torch adds they replace.

The contracts are bit-equalities: s against torch's `h + x`; y/mean/rstd against
`ln_fwd(s)`; `d = bf16(dx) + ds` against `ln_bwd(...)[0] + ds` of the same build.
dw/db may change their summation order with the grid and are held to the derived
bound of tests/_norm_gemm_ref.py, next to the older `_dwdb_ok` tolerance.
"""
import pytest
import torch

import _norm_gemm_ref as NG

pytestmark = pytest.mark.gpu

EPS = 1e-5

# (rows, C)
SHAPES = [
    (1, 768),      # a single row
    (5, 8),        # a single granule
    (37, 322),     # ragged last granule, rows only 4-byte aligned
    (259, 768),    # rows not a multiple of the 4 waves per block
    (2051, 1280),  # flagship width: third chunk half empty; more rows than waves in the
                   # reduction grid, every wave takes several rows, ragged last pass
    (1030, 2048),  # four full chunks
    (0, 768),      # empty
]


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


_CACHE = {}


def _inputs(rows, C):
    """bf16 h, x, dy, ds, w, b on the GPU; made once per shape and never modified."""
    key = (rows, C)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(rows * 4099 + C)

        def rnd(*shape):
            return torch.randn(*shape, generator=g).bfloat16().cuda()

        _CACHE[key] = dict(
            h=rnd(rows, C), x=rnd(rows, C), dy=rnd(rows, C), ds=rnd(rows, C),
            w=(torch.randn(C, generator=g).abs() + 0.5).bfloat16().cuda(), b=rnd(C),
        )
    return _CACHE[key]


def _dwdb_ok(got, want):
    """The older LayerNorm dw/db tolerance of tests/test_gpu_kernels.py, kept next
    to the derived bound where the inputs are at hand (it is the only check of
    the module-level gradients in the chain test)."""
    scale = want.abs().mean().clamp(min=1.0)
    err = (got.float() - want.float()).abs().max().item()
    assert err < 0.04 * float(scale) + 0.08, (err, float(scale))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _assert_bit_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    diff = int((_bits(got) != _bits(want)).sum())
    assert diff == 0, f"{what}: {diff} of {got.numel()} elements differ"


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_add_ln_fwd_equals_add_then_ln_fwd(rows, C, with_bias):
    t = _inputs(rows, C)
    b = t["b"] if with_bias else None
    s, y, mean, rstd = _ext().add_ln_fwd(t["h"], t["x"], t["w"], b, EPS)
    _assert_bit_equal(s, t["h"] + t["x"], "s")
    y_ref, mean_ref, rstd_ref = _ext().ln_fwd(s, t["w"], b, EPS)
    _assert_bit_equal(y, y_ref, "y")
    _assert_bit_equal(mean, mean_ref, "mean")
    _assert_bit_equal(rstd, rstd_ref, "rstd")


@pytest.mark.parametrize("needs_dwdb", [False, True])
@pytest.mark.parametrize("rows,C", SHAPES)
def test_ln_bwd_with_ds_equals_ln_bwd_then_add(rows, C, needs_dwdb):
    t = _inputs(rows, C)
    ext = _ext()
    s = t["h"] + t["x"]
    _, mean, rstd = ext.ln_fwd(s, t["w"], t["b"], EPS)

    dx, dw, db = ext.ln_bwd(t["dy"], s, t["w"], mean, rstd, needs_dwdb)
    # without ds the entry point is what it was, positionally and by keyword
    dx_kw = ext.ln_bwd(t["dy"], s, t["w"], mean, rstd, needs_dwdb, ds=None)[0]
    _assert_bit_equal(dx_kw, dx, "dx with ds=None")

    d, dw_ds, db_ds = ext.ln_bwd(t["dy"], s, t["w"], mean, rstd, needs_dwdb, t["ds"])
    _assert_bit_equal(d, dx + t["ds"], "d")

    if rows == 0:  # the empty case returns zero dw/db whether asked or not
        for g in (dw, db, dw_ds, db_ds):
            assert g.shape == (C,) and not g.any()
        return
    if not needs_dwdb:
        assert dw is None and db is None and dw_ds is None and db_ds is None
        return
    sf = s.float().requires_grad_()
    wf = t["w"].float().requires_grad_()
    bf = t["b"].float().requires_grad_()
    torch.nn.functional.layer_norm(sf, (C,), wf, bf, EPS).backward(t["dy"].float())
    cpu = [v.cpu() for v in (t["dy"], s, t["w"], mean, rstd)]
    for got_w, got_b in ((dw, db), (dw_ds, db_ds)):
        assert got_w.shape == (C,) and got_b.shape == (C,)
        _dwdb_ok(got_w, wf.grad)
        _dwdb_ok(got_b, bf.grad)
        # the derived bound of tests/_norm_gemm_ref.py, from the statistics handed in
        ratios = NG.ln_bwd_ratios(*cpu, dx.cpu(), got_w.cpu(), got_b.cpu())
        assert max(ratios) <= 1.0, ratios


def _chain(fused, x0, norms, linears):
    """Three residual blocks x + linear(LN(x)); the sum of each block is formed in
    the next block's LayerNorm (fused) or by a torch add in front of it."""
    from perceiver_amd.ops.norm import add_layer_norm

    h, s = None, x0
    for ln, lin in zip(norms, linears):
        if fused:
            s, y = add_layer_norm(ln, h, s)
        else:
            s = s if h is None else h + s
            y = ln(s)
        h = lin(y)
    return h + s


def test_add_layer_norm_chain_matches_unfused_composition():
    from perceiver_amd.ops.norm import LayerNorm

    B, N, C = 3, 50, 322
    g = torch.Generator(device="cpu").manual_seed(7)
    norms = [LayerNorm(C).cuda().bfloat16() for _ in range(3)]
    linears = [torch.nn.Linear(C, C).cuda().bfloat16() for _ in range(3)]
    with torch.no_grad():
        for ln in norms:
            ln.weight.copy_(torch.randn(C, generator=g).abs() + 0.5)
            ln.bias.copy_(torch.randn(C, generator=g))
        for lin in linears:
            lin.weight.copy_(torch.randn(C, C, generator=g) * C ** -0.5)
            lin.bias.copy_(torch.randn(C, generator=g) * 0.1)
    x = torch.randn(B, N, C, generator=g).bfloat16().cuda()
    dout = torch.randn(B, N, C, generator=g).bfloat16().cuda()
    params = [p for m in norms + linears for p in m.parameters()]

    results = {}
    for fused in (False, True):
        x0 = x.clone().requires_grad_()
        for p in params:
            p.grad = None
        out = _chain(fused, x0, norms, linears)
        out.backward(dout)
        results[fused] = (out.detach(), x0.grad, [p.grad for p in params])

    out_u, dx_u, grads_u = results[False]
    out_f, dx_f, grads_f = results[True]
    _assert_bit_equal(out_f, out_u, "output")
    _assert_bit_equal(dx_f, dx_u, "input gradient")
    ln_params = {id(p) for ln in norms for p in ln.parameters()}
    for p, gf, gu in zip(params, grads_f, grads_u):
        if id(p) in ln_params:
            _dwdb_ok(gf, gu)
        else:
            _assert_bit_equal(gf, gu, "linear gradient")


def test_add_layer_norm_backward_with_an_unused_output():
    """Either incoming gradient may be absent: only the shortcut, or only the
    normalised output, reaches the loss."""
    from perceiver_amd.ops.norm import LayerNorm, add_layer_norm

    t = _inputs(259, 768)
    ln = LayerNorm(768).cuda().bfloat16()
    for use_s, use_y in ((True, False), (False, True)):
        h = t["h"].clone().requires_grad_()
        x = t["x"].clone().requires_grad_()
        s, y = add_layer_norm(ln, h, x)
        ((s if use_s else y) * t["dy"]).sum().backward()

        h_ref = t["h"].clone().requires_grad_()
        x_ref = t["x"].clone().requires_grad_()
        s_ref = h_ref + x_ref
        ((s_ref if use_s else ln(s_ref)) * t["dy"]).sum().backward()
        _assert_bit_equal(h.grad, h_ref.grad, "dh")
        _assert_bit_equal(x.grad, x_ref.grad, "dx")
