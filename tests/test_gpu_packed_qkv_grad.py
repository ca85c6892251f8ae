"""flash_bwd writing dq/dk/dv as the column slices of one packed (B, N, 2*qk + v)
gradient buffer, and the self-attention path built on it: bit-equal to the three
separate gradients and to the split + concat path."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _split_heads(t, H):
    b, n, _ = t.shape
    return t.view(b, n, H, -1).transpose(1, 2)


_CACHE = {}


def _problem(B, H, N, qk, vc, p):
    """Head views of a merged qkv activation as the module makes them, the flash
    forward's results and a dout; made once per case and never modified."""
    key = (B, H, N, qk, vc, p)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(N * 31 + qk)
        qkv = torch.randn(B, N, 2 * qk + vc, generator=g).bfloat16().cuda()
        q, k, v = (_split_heads(t, H) for t in qkv.split([qk, qk, vc], dim=-1))
        q = q * (qk // H) ** -0.5
        seed = 1234 if p > 0 else 0
        out, lse = _ext().flash_fwd(q, k, v, None, False, p, seed)
        dout = torch.randn(B, H, N, vc // H, generator=g).bfloat16().cuda()
        _CACHE[key] = (q, k, v, out, lse, dout, seed)
    return _CACHE[key]


def _plans(B, H, N):
    """(dq, dkv) gridDim.z of the <32,160> and <64,64> tiers: 128-query dq blocks,
    64-key dkv blocks, 64-row tiles on the split axis."""
    ext = _ext()
    dq = ext.flash_split_plan(-(-N // 128) * B * H, N, 64)[0]
    dkv = ext.flash_split_plan(-(-N // 64) * B * H, N, 64)[0]
    return dq, dkv


@pytest.mark.parametrize("B,H,N,qk,vc,p,split", [
    (2, 8, 200, 256, 1280, 0.0, False),  # the <32,160> tier; N ragged against 64/128-row tiles
    (2, 8, 200, 256, 1280, 0.1, False),  # with dropout, same seed on both sides
    (2, 4, 200, 256, 256, 0.0, False),   # the D = 64 tier
    (1, 8, 600, 256, 1280, 0.0, True),   # dq KV-split and dkv Q-split: fp32 partials copied in
    (1, 8, 600, 256, 1280, 0.1, True),
])
def test_packed_slices_equal_separate_gradients(B, H, N, qk, vc, p, split):
    dq_split, dkv_split = _plans(B, H, N)
    assert (dq_split > 1 and dkv_split > 1) == split and (dq_split > 1 or dkv_split > 1) == split
    q, k, v, out, lse, dout, seed = _problem(B, H, N, qk, vc, p)
    ext = _ext()
    dq, dk, dv = ext.flash_bwd(dout, q, k, v, out, lse, None, False, p, seed)

    # NaN bits in the buffer: a column the kernels leave unwritten shows
    buf = torch.full((B, N, 2 * qk + vc), float("nan"), dtype=torch.bfloat16, device="cuda")
    pq, pk, pv = ext.flash_bwd(dout, q, k, v, out, lse, None, False, p, seed, buf)
    for got, want, c0, width in ((pq, dq, 0, qk), (pk, dk, qk, qk), (pv, dv, 2 * qk, vc)):
        assert got.shape == want.shape
        assert torch.equal(got, want)
        merged = want.transpose(1, 2).reshape(B, N, width)
        assert torch.equal(buf[..., c0:c0 + width], merged)
        assert got.data_ptr() == buf[..., c0:c0 + width].data_ptr()


def test_packed_buffer_is_refused_on_the_padded_tier():
    ext = _ext()
    assert ext.flash_bwd_packs_qkv_grad(32, 160) and ext.flash_bwd_packs_qkv_grad(64, 64)
    assert not ext.flash_bwd_packs_qkv_grad(261, 261)


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_self_attention_gradients_equal_with_lever_on_and_off(monkeypatch, dropout):
    from perceiver_amd.core.modules import MultiHeadAttention
    from perceiver_amd.ops import flash

    torch.manual_seed(0)
    mha = MultiHeadAttention(
        num_heads=8, num_q_input_channels=128, num_kv_input_channels=128,
        num_qk_channels=256, num_v_channels=1280, dropout=dropout, merged_qkv=True,
    ).cuda().bfloat16()
    mha.train()
    x = torch.randn(2, 200, 128, device="cuda").bfloat16()
    dout = torch.randn(2, 200, 128, device="cuda").bfloat16()

    taken = []
    real_apply = flash.PackedQKVFlashAttention.apply
    monkeypatch.setattr(flash, "packed_qkv_attention",
                        lambda *a, **kw: (taken.append(1), real_apply(*a, **kw))[1])

    results = {}
    for lever in ("1", "0"):
        monkeypatch.setenv("PERCEIVER_PACKED_QKV_GRAD", lever)
        mha.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_()
        torch.manual_seed(5)  # the dropout seed is drawn from the global generator
        out = mha(xin, xin).last_hidden_state
        out.backward(dout)
        results[lever] = (out.detach(), xin.grad, mha.qkv_proj.weight.grad.clone(),
                          mha.qkv_proj.bias.grad.clone())
        assert len(taken) == 1  # on: the packed path ran; off: it did not run again
    for a, b in zip(results["1"], results["0"]):
        assert torch.equal(a, b)
