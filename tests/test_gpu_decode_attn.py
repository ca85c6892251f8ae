"""GPU tests of the windowed single-query attention kernel (decode_attn).

Every oracle case first asserts the slice count it was written to reach through
the extension's decode_attn_plan, then holds the kernel to the fp64 reference
under the bound derived in tests/_attention_ref.py. test_decode_attn_oracle.py
shows on the CPU that this bound catches a window that is off by one key at
either end. The exactness properties (empty and clamped windows, layouts,
neighbour independence, offset invariance, determinism) are bit comparisons.
"""
import gc

import pytest
import torch

import _decode_attn_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(autouse=True, scope="module")
def _collect_garbage_before_later_tests():
    """The tensors of this module hold GPU memory. Collect what is left of them here, in this process, and not in a
    worker process that a later test of the session forks."""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _run(q, k, v, lo, hi):
    return _ext().decode_attn(q, k, v, lo, hi)


def _case_on_device(name, n=None):
    q, k, v, lo, hi, ref = R.case_data(name, n)
    return _dev(q, k, v, lo, hi) + (ref,)


@pytest.mark.parametrize("case", R.all_cases(), ids=R.case_id)
def test_case_matches_reference(case):
    name = case[0]
    b, h, cap, d, _ = R.CASES[name]["shape"]
    nsplit, granule = _ext().decode_attn_plan(b, h, cap, d)
    assert nsplit == R.CASES[name]["nsplit"]
    assert (nsplit, granule) == R.plan(b, h, cap, d)
    q, k, v, lo, hi, (out_ref, _, _, abs_pv) = _case_on_device(*case)
    out = _run(q, k, v, lo, hi).cpu()
    assert out.shape == out_ref.shape and torch.isfinite(out.float()).all()
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    print(f"{R.case_id(case)}: error/tol {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_output_is_a_view_of_merged_heads_memory():
    q, k, v, lo, hi, _ = _case_on_device("small_unsplit")
    out = _run(q, k, v, lo, hi)
    b, h, _, dv = out.shape
    assert out.transpose(1, 2).is_contiguous()
    assert out.transpose(1, 2).reshape(b, 1, h * dv).data_ptr() == out.data_ptr()


@pytest.mark.parametrize("name", ["small_unsplit", "d64_split8"])
def test_empty_window_gives_zeros(name):
    q, k, v, lo, hi, _ = _case_on_device(name)
    hi2 = hi.clone()
    hi2[1] = lo[1] - 1
    out = _run(q, k, v, lo, hi2)
    assert torch.count_nonzero(out[1]) == 0
    want = _run(q, k, v, lo, hi)
    assert torch.equal(out[0], want[0]) and torch.equal(out[2], want[2])


@pytest.mark.parametrize("name", ["small_unsplit", "d64_split8"])
def test_garbage_counters_are_clamped(name):
    q, k, v, lo, hi, _ = _case_on_device(name)
    cap = k.shape[2]
    lo_bad = torch.tensor([-5, -(1 << 40), int(lo[2])], device=DEV)
    hi_bad = torch.tensor([cap, (1 << 40), cap + 7], device=DEV)
    out = _run(q, k, v, lo_bad, hi_bad)
    torch.cuda.synchronize()
    want = _run(q, k, v, torch.tensor([0, 0, int(lo[2])], device=DEV),
                torch.full((3,), cap - 1, device=DEV))
    assert torch.equal(out, want)


@pytest.mark.parametrize("name", ["small_unsplit", "d128_split8", "d32_dv64_split4"])
def test_model_layouts_equal_contiguous_copies(name):
    q, k, v, lo, hi, _ = _case_on_device(name)
    b, h, cap, d = k.shape
    dv = v.shape[-1]
    want = _run(q, k, v, lo, hi)
    # head-transposed views of (B, cap, H * D) cache buffers
    k_buf = k.transpose(1, 2).reshape(b, cap, h * d).contiguous()
    v_buf = v.transpose(1, 2).reshape(b, cap, h * dv).contiguous()
    k_view = k_buf.view(b, cap, h, d).transpose(1, 2)
    v_view = v_buf.view(b, cap, h, dv).transpose(1, 2)
    assert not k_view.is_contiguous()
    assert torch.equal(_run(q, k_view, v_view, lo, hi), want)
    # batch-stride-0 q, and one-element lo / hi against B elements
    q0 = q[:1].expand(b, -1, -1, -1)
    assert q0.stride(0) == 0
    lo1, hi1 = lo[:1].clone(), hi[:1].clone()
    got = _run(q0, k_view, v_view, lo1, hi1)
    assert torch.equal(got, _run(q0.contiguous(), k, v, lo1.expand(b).contiguous(),
                                 hi1.expand(b).contiguous()))
    # lo absent means 0
    zero = torch.zeros(b, dtype=torch.long, device=DEV)
    assert torch.equal(_run(q, k_view, v_view, None, hi), _run(q, k, v, zero, hi))


@pytest.mark.parametrize("name", ["small_unsplit", "d64_split8"])
def test_row_is_independent_of_its_neighbours(name):
    q, k, v, lo, hi, _ = _case_on_device(name)
    want = _run(q, k, v, lo, hi)
    q2, k2, v2, lo2, hi2 = q.clone(), k.clone(), v.clone(), lo.clone(), hi.clone()
    for t in (q2, k2, v2):
        t[0].mul_(-0.5)
        t[2].add_(1.0)
    lo2[0], hi2[0] = 2, 3
    lo2[2], hi2[2] = 0, k.shape[2] - 1
    assert torch.equal(_run(q2, k2, v2, lo2, hi2)[1], want[1])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_offset_invariance(name):
    """A row's keys moved to offset 0 of another buffer of the same capacity,
    with lo = 0, give the same bits."""
    q, k, v, lo, hi, _ = _case_on_device(name)
    want = _run(q, k, v, lo, hi)
    g = torch.Generator(device="cpu").manual_seed(7)
    k2 = torch.randn(k.shape, generator=g).bfloat16().to(DEV)
    v2 = torch.randn(v.shape, generator=g).bfloat16().to(DEV)
    n = hi - lo + 1
    for b in range(k.shape[0]):
        nb, l0 = int(n[b]), int(lo[b])
        k2[b, :, :nb] = k[b, :, l0:l0 + nb]
        v2[b, :, :nb] = v[b, :, l0:l0 + nb]
    got = _run(q, k2, v2, torch.zeros_like(lo), n - 1)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", ["small_unsplit", "d128_split8"])
def test_two_runs_are_bit_equal(name):
    q, k, v, lo, hi, _ = _case_on_device(name)
    assert torch.equal(_run(q, k, v, lo, hi), _run(q, k, v, lo, hi))


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_against_flash_fwd_with_the_equivalent_mask(name):
    q, k, v, lo, hi, (out_ref, _, _, abs_pv) = _case_on_device(name)
    pad = R.window_pad(lo.cpu(), hi.cpu(), k.shape[0], k.shape[2]).to(DEV)
    flash, _ = _ext().flash_fwd(q, k, v, pad, False, 0.0, 0)
    got = _run(q, k, v, lo, hi)
    ratio = R.worst_ratio(got.cpu(), flash.cpu(), 2.0 * R.tol(out_ref, abs_pv))
    print(f"{name}: |decode_attn - flash_fwd| / (sum of the two bounds) {ratio:.3f}")
    assert ratio <= 1.0, ratio


def test_routing_and_lever(monkeypatch):
    from perceiver_amd.ops import decode_attn as da
    from perceiver_amd.ops.attention import scaled_dot_attention

    q, k, v, lo, hi, (out_ref, _, _, abs_pv) = _case_on_device("d64_split8")
    assert da.kernel_applicable(q, k, v)
    routed = scaled_dot_attention(q, k, v, pad_mask=da.KeyWindow(lo, hi), causal=True)
    assert torch.equal(routed, _run(q, k, v, lo, hi))
    # a plain tensor mask is today's path
    pad = R.window_pad(lo.cpu(), hi.cpu(), k.shape[0], k.shape[2]).to(DEV)
    flash, _ = _ext().flash_fwd(q, k, v, pad, True, 0.0, 0)
    assert torch.equal(scaled_dot_attention(q, k, v, pad_mask=pad, causal=True), flash)
    # the lever sends the window through the mask composition
    monkeypatch.setenv("PERCEIVER_DECODE_ATTN", "0")
    assert not da.kernel_applicable(q, k, v)
    composed = scaled_dot_attention(q, k, v, pad_mask=da.KeyWindow(lo, hi), causal=True)
    assert torch.equal(composed, flash)
    assert R.worst_ratio(composed.cpu(), out_ref, R.tol(out_ref, abs_pv)) <= 1.0
