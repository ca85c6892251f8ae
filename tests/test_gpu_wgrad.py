"""GPU parity tests for the split-K weight-gradient GEMM with fused bias sums.

    dw[n,k] = sum_m dy[m,n] * x[m,k]        db[n] = sum_m dy[m,n]

Reference: fp32 torch of the same operands, rounded once to bf16 (the kernel
accumulates in fp32 and rounds once). Shapes are the smallest that reach each
path: one tile / one split, several tiles in both directions with N != K,
several splits with a shorter last split, one K-step per split, and both
output tiles (256x128 and 256x256).
"""
import pytest
import torch

import _norm_gemm_ref as NG

pytestmark = pytest.mark.gpu

K_STEP = 64


def _ext():
    from perceiver_amd.ops import hip as hip_ops

    return hip_ops.ext()


def _check_dw(dw, dy, x):
    # bounds of tests/test_gpu_gemm.py::test_gemm_bt_parity
    ref = (dy.float().t() @ x.float()).to(torch.bfloat16)
    assert dw.shape == ref.shape and dw.dtype == torch.bfloat16
    err = (dw.float() - ref.float()).abs()
    scale = ref.float().abs().clamp_min(1.0)
    assert (err / scale).max().item() < 2e-2, (err.max().item(), (err / scale).max().item())
    match = (dw == ref).float().mean().item()
    assert match > 0.98, match
    # the derived bound of tests/_norm_gemm_ref.py against fp64
    nsplit = _ext().wgrad_plan(dy.shape[0], dy.shape[1], x.shape[1])[2]
    ratio = NG.worst_ratio(dw.cpu(), NG.wgrad_ref(dy.cpu(), x.cpu())[0],
                           NG.wgrad_bound(dy.cpu(), x.cpu(), nsplit))
    assert ratio <= 1.0, ratio


def _check_db(db, dy, x):
    # bounds of tests/test_gpu_kernels.py::test_colsum_matches_torch_sum
    want = dy.float().sum(0).bfloat16().float()
    assert db.dtype == torch.bfloat16 and db.shape == want.shape
    torch.testing.assert_close(db.float(), want, atol=4.0, rtol=1e-2)
    # colsum_bound with the chain of the fused sum (tests/_norm_gemm_ref.py);
    # x only says which plan the launch used
    _, _, nsplit, rows = _ext().wgrad_plan(dy.shape[0], dy.shape[1], x.shape[1])
    ratio = NG.worst_ratio(db.cpu(), dy.cpu().double().sum(0),
                           NG.wgrad_db_bound(dy.cpu(), nsplit, rows))
    assert ratio <= 1.0, ratio


# (M, N, K, tile_k, nsplit, rows_per_split) — the plan is pinned so a planner
# change cannot silently move a case off the path it is here to cover
CASES = [
    (64, 256, 128, 128, 1, 64),       # one split, one tile, one K-step
    (320, 512, 384, 128, 5, 64),      # 2 x 3 tiles (N != K), one K-step per split
    (320, 512, 768, 128, 3, 128),     # 2 x 6 tiles, last split shorter (64 rows)
    (1088, 512, 768, 128, 6, 192),    # several steps per split, last split 128 rows
    (2048, 1792, 1280, 256, 7, 320),  # 256x256 tile, 7 x 5 tiles, last split 128 rows
]


@pytest.mark.parametrize("M,N,K,tile_k,nsplit,rows", CASES)
@pytest.mark.parametrize("want_db", [True, False])
def test_gemm_wgrad_parity(M, N, K, tile_k, nsplit, rows, want_db):
    ext = _ext()
    assert ext.gemm_wgrad_applicable(M, N, K)
    assert tuple(ext.wgrad_plan(M, N, K)) == (256, tile_k, nsplit, rows)
    torch.manual_seed(0)
    dev = torch.device("cuda")
    dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16) * 0.05
    out = ext.gemm_wgrad(dy, x, want_db)
    assert len(out) == (2 if want_db else 1)
    _check_dw(out[0], dy, x)
    if want_db:
        _check_db(out[1], dy, x)


def test_gemm_wgrad_is_deterministic():
    ext = _ext()
    torch.manual_seed(1)
    dev = torch.device("cuda")
    dy = torch.randn(1088, 512, device=dev, dtype=torch.bfloat16)
    x = torch.randn(1088, 768, device=dev, dtype=torch.bfloat16) * 0.05
    a = ext.gemm_wgrad(dy, x, True)
    b = ext.gemm_wgrad(dy, x, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_gemm_wgrad_rejects_bad_shapes():
    ext = _ext()
    dev = torch.device("cuda")
    dy = torch.zeros(96, 256, device=dev, dtype=torch.bfloat16)
    x = torch.zeros(96, 128, device=dev, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        ext.gemm_wgrad(dy, x, True)


def test_wrapper_takes_non_contiguous_dy():
    """dy reaching the autograd wrapper as a transposed view."""
    from perceiver_amd.ops.linear import _ColsumLinearFn

    torch.manual_seed(2)
    dev = torch.device("cuda")
    M, N, K = 320, 512, 384
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16) * 0.05
    w = (torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05).requires_grad_(True)
    b = torch.zeros(N, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(N, M, device=dev, dtype=torch.bfloat16).t()
    assert not dy.is_contiguous()
    y = _ColsumLinearFn.apply(x, w, b)
    y.backward(dy)
    _check_dw(w.grad, dy.contiguous(), x)
    _check_db(b.grad, dy.contiguous(), x)


def _grads(make_out, params, dy):
    for p in params:
        p.grad = None
    make_out().backward(dy)
    return [p.grad.clone() for p in params]


def _assert_close_bf16_paths(got, ref, tol):
    # tolerances of test_linear_gelu_fused_matches_reference (two bf16 paths)
    err = (got.float() - ref.float()).abs()
    scale = ref.float().abs().clamp_min(1.0)
    assert (err / scale).max().item() < tol, (err / scale).max().item()


def test_perceiver_linear_wgrad_matches_lever_off(monkeypatch):
    from perceiver_amd.ops import linear
    from perceiver_amd.ops.linear import PerceiverLinear

    torch.manual_seed(3)
    dev = torch.device("cuda")
    M, N, K = PerceiverLinear._MIN_ROWS, 256, 256
    lin = PerceiverLinear(K, N, bias=True).to(dev, torch.bfloat16)
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
    params = [x, lin.weight, lin.bias]
    assert _ext().gemm_wgrad_applicable(M, N, K)
    monkeypatch.setattr(linear, "_WGRAD", True)
    new = _grads(lambda: lin(x), params, dy)
    monkeypatch.setattr(linear, "_WGRAD", False)
    old = _grads(lambda: lin(x), params, dy)
    for got, ref, tol in zip(new, old, (1e-2, 2e-2, 2e-2)):
        _assert_close_bf16_paths(got, ref, tol)
    _check_dw(new[1], dy, x.detach())
    _check_db(new[2], dy, x.detach())


def test_linear_gelu_bias_wgrad_matches_lever_off(monkeypatch):
    from perceiver_amd.ops import linear
    from perceiver_amd.ops.gelu import LinearGeluBias

    torch.manual_seed(4)
    dev = torch.device("cuda")
    M, N, K = 8192, 256, 256
    x = torch.randn(M, K, device=dev, dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn(N, K, device=dev, dtype=torch.bfloat16) * 0.05).requires_grad_(True)
    b = torch.randn(N, device=dev, dtype=torch.bfloat16, requires_grad=True)
    dy = torch.randn(M, N, device=dev, dtype=torch.bfloat16)
    params = [x, w, b]
    monkeypatch.setattr(linear, "_WGRAD", True)
    new = _grads(lambda: LinearGeluBias.apply(x, w, b), params, dy)
    monkeypatch.setattr(linear, "_WGRAD", False)
    old = _grads(lambda: LinearGeluBias.apply(x, w, b), params, dy)
    for got, ref, tol in zip(new, old, (1e-2, 2e-2, 2e-2)):
        _assert_close_bf16_paths(got, ref, tol)
