"""GPU tests of gemm_bt, gemm_bt_gelu and gemm_wgrad against the fp64 oracle in
tests/_norm_gemm_ref.py.

The exact family (small integers, every partial sum below 2^24) pins the result
bit for bit on every K-tail path of the ring, both tile widths, a grid of more
than 256 workgroups that is no multiple of 8, and every pinned split plan of
the weight gradient. The random and the cancelling families hold the kernels
to |y - ref| <= U |ref| + 2 (K + 2) 2^-24 (|x| @ |w|^T + |b|); on the
cancelling ones the fp32 term binds. test_norm_gemm_oracle.py shows on the CPU
that the kernels' arithmetic can meet the bounds and that the defects these
tests exist for cannot. Each test prints its worst |got - ref| / bound.
"""
import pytest
import torch

import _norm_gemm_ref as R

pytestmark = pytest.mark.gpu


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _ratio(name, got, want, bound):
    r = R.worst_ratio(got.cpu(), want, bound)
    print(f"{name}: worst |got - ref| / bound = {r:.4f}")
    return r


def _bits_equal(got, want):
    return torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def _cuda(t):
    return None if t is None else t.cuda()


# ----------------------------------------------------------------- gemm_bt

def _exact_gemm(M, N, K):
    x, w, b, y, y0 = R.gemm_exact_case(M, N, K)
    assert _ext().gemm_bt_applicable(M, N, K)
    assert _bits_equal(_ext().gemm_bt(x.cuda(), w.cuda(), b.cuda()), y), (M, N, K, "bias")
    assert _bits_equal(_ext().gemm_bt(x.cuda(), w.cuda(), None), y0), (M, N, K, "no bias")


@pytest.mark.parametrize("K", R.GEMM_EXACT_K)
def test_gemm_bt_exact_on_every_k_tail(K):
    # kt_total = 3, 4, 5, 6, 9: the three-tile minimum, every kt_total % 3, a
    # peeled loop of two trips
    assert [k // R.GEMM_BK for k in R.GEMM_EXACT_K] == [3, 4, 5, 6, 9]
    for N in (128, 160):
        _exact_gemm(256, N, K)


@pytest.mark.parametrize("N,tile", sorted(R.GEMM_EXACT_N.items()))
def test_gemm_bt_exact_at_both_tile_widths(N, tile):
    # the Python-side copy of pick_bn against the table; the launcher's own
    # choice is not exposed
    assert R.gemm_tile_width(256, N) == tile
    _exact_gemm(256, N, 320)


def test_gemm_bt_exact_on_a_second_round_and_the_ragged_xcd_remap():
    M, N, K = R.GEMM_BIG
    tile = R.gemm_tile_width(M, N)  # Python-side copy of pick_bn
    blocks = (M // R.GEMM_BM) * (N // tile)
    assert (tile, blocks, blocks % 8) == (128, 266, 2)
    _exact_gemm(M, N, K)


@pytest.mark.parametrize("family", list(R.GEMM_FAMILIES))
@pytest.mark.parametrize("M,N,K", R.GEMM_BOUND_SHAPES)
def test_gemm_bt_within_the_bound(M, N, K, family):
    x, w, b = R.GEMM_FAMILIES[family](M, N, K)
    biases = [b] if family != "random" else [b, None]
    for bias in biases:
        y = _ext().gemm_bt(x.cuda(), w.cuda(), _cuda(bias))
        assert _ratio(f"gemm_bt {family} {M}x{N}x{K} bias={bias is not None}", y,
                      R.gemm_ref(x, w, bias), R.gemm_bound(x, w, bias)) <= 1.0


# ----------------------------------------------------------------- gemm_bt_gelu

@pytest.mark.parametrize("M,N,K", R.GELU_SHAPES)
def test_gemm_bt_gelu_pre_and_gelu(M, N, K):
    # exact family: pre is the bias-free result whatever the bias argument is
    x, w, b, _, y0 = R.gemm_exact_case(M, N, K)
    for bias in (b, None):
        pre, gel = _ext().gemm_bt_gelu(x.cuda(), w.cuda(), _cuda(bias))
        assert _bits_equal(pre, y0), (M, N, K, bias is not None)
        v = R.gelu_pre(y0, bias)
        assert _ratio(f"gemm_bt_gelu exact {M}x{N}x{K} gelu bias={bias is not None}", gel,
                      R.gelu_ref(v), R.gelu_fwd_bound(v)) <= 1.0
    # random family: pre under the GEMM bound, gelu under gelu_fwd_bound of the
    # pre the kernel returned
    x, w, b = R.gemm_random_case(M, N, K)
    ref, bound = R.gemm_ref(x, w), R.gemm_bound(x, w)
    pres = []
    for bias in (b, None):
        pre, gel = _ext().gemm_bt_gelu(x.cuda(), w.cuda(), _cuda(bias))
        tag = f"gemm_bt_gelu random {M}x{N}x{K} bias={bias is not None}"
        assert _ratio(f"{tag} pre", pre, ref, bound) <= 1.0
        v = R.gelu_pre(pre.cpu(), bias)
        assert _ratio(f"{tag} gelu", gel, R.gelu_ref(v), R.gelu_fwd_bound(v)) <= 1.0
        pres.append(pre.cpu())
    assert _bits_equal(pres[0], pres[1])
    assert _bits_equal(_ext().gemm_bt(x.cuda(), w.cuda(), None), pres[0])


# ----------------------------------------------------------------- gemm_wgrad

# the last split is a single 64-row step behind four of three steps
WGRAD_SHORT_LAST = (832, 512, 768, 128, 5, 192)


def _assert_plan(M, N, K, tile_k, nsplit, rows):
    assert _ext().gemm_wgrad_applicable(M, N, K)
    assert tuple(_ext().wgrad_plan(M, N, K)) == (256, tile_k, nsplit, rows)


@pytest.mark.parametrize("M,N,K,tile_k,nsplit,rows", R.WGRAD_CASES + [WGRAD_SHORT_LAST])
def test_gemm_wgrad_exact_at_the_pinned_plans(M, N, K, tile_k, nsplit, rows):
    _assert_plan(M, N, K, tile_k, nsplit, rows)
    if (M, N, K) == WGRAD_SHORT_LAST[:3]:
        assert M - (nsplit - 1) * rows == 64 and rows > 64
    dy, x, dw, db = R.wgrad_exact_case(M, N, K)
    got_w, got_b = _ext().gemm_wgrad(dy.cuda(), x.cuda(), True)
    assert _bits_equal(got_w, dw) and _bits_equal(got_b, db)
    only_w, = _ext().gemm_wgrad(dy.cuda(), x.cuda(), False)
    assert _bits_equal(only_w, dw)


@pytest.mark.parametrize("family", ["random", "cancelling"])
@pytest.mark.parametrize("M,N,K,tile_k,nsplit,rows", R.WGRAD_BOUND_CASES)
def test_gemm_wgrad_within_the_bound(M, N, K, tile_k, nsplit, rows, family):
    _assert_plan(M, N, K, tile_k, nsplit, rows)
    dy, x = (R.wgrad_random_case(M, N, K) if family == "random"
             else R.wgrad_cancelling_case(M, N, K, rows))
    ref_w, ref_b = R.wgrad_ref(dy, x)
    dw, db = _ext().gemm_wgrad(dy.cuda(), x.cuda(), True)
    tag = f"gemm_wgrad {family} {M}x{N}x{K}"
    assert _ratio(f"{tag} dw", dw, ref_w, R.wgrad_bound(dy, x, nsplit)) <= 1.0
    assert _ratio(f"{tag} db", db, ref_b, R.wgrad_db_bound(dy, nsplit, rows)) <= 1.0
    only_w, = _ext().gemm_wgrad(dy.cuda(), x.cuda(), False)
    assert _bits_equal(only_w, dw.cpu())  # want_db changes no bit of dw
