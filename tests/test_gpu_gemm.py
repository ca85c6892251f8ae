"""GPU parity tests for the deep-pipeline custom GEMM (y = x @ w^T + b).

Covers every K-tail path of the ring scheduler (kt_total % 3 in {0,1,2}),
bias/no-bias, and the real flagship projection shapes. Reference is fp32
torch.matmul of the same operands (the kernel accumulates in fp32, so the
bf16-rounded outputs must match the fp32 reference to bf16 resolution).
"""
import pytest
import torch

import _norm_gemm_ref as NG

pytestmark = pytest.mark.gpu


def _ref(x, w, b):
    y = x.float() @ w.float().t()
    if b is not None:
        y = y + b.float()
    return y.to(torch.bfloat16)


@pytest.mark.parametrize(
    "M,N,K",
    [
        (512, 256, 192),    # kt_total=3: pure tail
        (512, 128, 256),    # kt_total=4: tail 1
        (512, 256, 320),    # kt_total=5: tail 2
        (512, 128, 384),    # kt_total=6: peeled + tail 3
        (2048, 1280, 1280),  # flagship self-attn projection shape class
        (2048, 256, 768),    # encoder cross-attn kv projection class
        (1536, 2816, 1280),
    ],
)
@pytest.mark.parametrize("bias", [True, False])
def test_gemm_bt_parity(M, N, K, bias):
    from perceiver_amd.ops import hip as hip_ops

    ext = hip_ops.ext()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
    w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05
    b = torch.randn(N, device=dev, dtype=torch.bfloat16) if bias else None
    assert ext.gemm_bt_applicable(M, N, K)
    y = ext.gemm_bt(x, w, b)
    ref = _ref(x, w, b)
    err = (y.float() - ref.float()).abs()
    scale = ref.float().abs().clamp_min(1.0)
    assert (err / scale).max().item() < 2e-2, (err.max().item(), (err / scale).max().item())
    # exact-match rate against the fp32-then-round reference should be high
    match = (y == ref).float().mean().item()
    assert match > 0.98, match
    # the derived bound of tests/_norm_gemm_ref.py against fp64
    xc, wc, bc = x.cpu(), w.cpu(), None if b is None else b.cpu()
    ratio = NG.worst_ratio(y.cpu(), NG.gemm_ref(xc, wc, bc), NG.gemm_bound(xc, wc, bc))
    assert ratio <= 1.0, ratio


def test_perceiver_linear_dgrad_routes_custom():
    """PerceiverLinear backward (custom dgrad GEMM + colsum db) matches a
    plain fp32 F.linear autograd reference."""
    from perceiver_amd.ops.linear import PerceiverLinear

    torch.manual_seed(1)
    dev = torch.device("cuda")
    lin = PerceiverLinear(1280, 1280, bias=True).to(dev, torch.bfloat16)
    x = torch.randn(8192, 1280, device=dev, dtype=torch.bfloat16, requires_grad=True)
    y = lin(x)
    dy = torch.randn_like(y)
    y.backward(dy)

    xr = x.detach().float().requires_grad_(True)
    wr = lin.weight.detach().float().requires_grad_(True)
    br = lin.bias.detach().float().requires_grad_(True)
    yr = torch.nn.functional.linear(xr, wr, br)
    yr.backward(dy.float())

    for got, ref in [(x.grad, xr.grad), (lin.weight.grad, wr.grad), (lin.bias.grad, br.grad)]:
        err = (got.float() - ref).abs()
        scale = ref.abs().clamp_min(1.0)
        assert (err / scale).max().item() < 3e-2


def test_linear_gelu_fused_matches_reference():
    """Fused GEMM+bias+GELU vs the unfused bf16 path (F.linear + GeluBias).

    The unfused path is the numerics contract: both recompute gelu' from the
    bf16-rounded pre-activation, so they must agree to accumulation-order
    noise. (A pure fp32 reference is only a sanity bound on the output — the
    bf16 pre-activation shifts gelu' systematically, and column sums of that
    shift are visible in dw for the unfused path exactly as much.)"""
    from perceiver_amd.ops.gelu import GeluBias, LinearGeluBias

    torch.manual_seed(2)
    dev = torch.device("cuda")
    M, N, K = 2048, 1792, 1280
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05).requires_grad_(True)
    b = torch.randn(N, device=dev, dtype=torch.bfloat16, requires_grad=True)
    y = LinearGeluBias.apply(x, w, b)
    dy = torch.randn_like(y)
    y.backward(dy)

    xr = x.detach().clone().requires_grad_(True)
    wr = w.detach().clone().requires_grad_(True)
    br = b.detach().clone().requires_grad_(True)
    hr = torch.nn.functional.linear(xr, wr)
    yr = GeluBias.apply(hr.contiguous(), br)
    yr.backward(dy)

    # output sanity vs fp32 as well
    yf = torch.nn.functional.gelu(
        torch.nn.functional.linear(x.detach().float(), w.detach().float(), b.detach().float()))
    err_f = ((y.float() - yf).abs() / yf.abs().clamp_min(1.0)).max().item()
    assert err_f < 2e-2, err_f

    for got, ref, tol in [(y, yr, 1e-2), (x.grad, xr.grad, 1e-2),
                          (w.grad, wr.grad, 2e-2), (b.grad, br.grad, 2e-2)]:
        err = (got.float() - ref.float()).abs()
        scale = ref.float().abs().clamp_min(1.0)
        assert (err / scale).max().item() < tol, (err / scale).max().item()


def test_gemm_bt_bn160_path():
    """N divisible by 160 routes the exact-fill tile and stays correct."""
    from perceiver_amd.ops import hip as hip_ops

    ext = hip_ops.ext()
    torch.manual_seed(3)
    dev = torch.device("cuda")
    for M, N, K in [(512, 1280, 1280), (256, 160, 192), (512, 480, 320)]:
        x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05
        b = torch.randn(N, device=dev, dtype=torch.bfloat16)
        y = ext.gemm_bt(x, w, b)
        ref = _ref(x, w, b)
        match = (y == ref).float().mean().item()
        assert match > 0.98, (M, N, K, match)
        # 20 workgroups of 256x128 waste fewer slots of a round than 16 of 256x160,
        # so (512, 1280) takes the 128 tile; the other two can only take 160
        assert NG.gemm_tile_width(M, N) == (128 if N == 1280 else 160)
        ratio = NG.worst_ratio(y.cpu(), NG.gemm_ref(x.cpu(), w.cpu(), b.cpu()),
                               NG.gemm_bound(x.cpu(), w.cpu(), b.cpu()))
        assert ratio <= 1.0, (M, N, K, ratio)


def test_transpose_bf16():
    from perceiver_amd.ops import hip as hip_ops

    ext = hip_ops.ext()
    torch.manual_seed(4)
    dev = torch.device("cuda")
    for N, K in [(1280, 1280), (1792, 1280), (100, 37), (64, 64), (2816, 1280)]:
        x = torch.randn(N, K, device=dev, dtype=torch.bfloat16)
        assert torch.equal(ext.transpose_bf16(x), x.t().contiguous())


def test_gemm_bt_rejects_bad_shapes():
    from perceiver_amd.ops import hip as hip_ops

    ext = hip_ops.ext()
    assert not ext.gemm_bt_applicable(100, 128, 192)   # M not /256
    assert not ext.gemm_bt_applicable(256, 100, 192)   # N not /128
    assert not ext.gemm_bt_applicable(256, 128, 100)   # K not /64
    assert not ext.gemm_bt_applicable(256, 128, 128)   # K too short for the ring
