"""CPU tests of the windowed decode attention oracle (tests/_decode_attn_ref.py).

Without a GPU they show that the derived bound of _attention_ref.tol() is one
the kernel's numerics meet (a CPU emulation of them stays inside it at every
GPU case), that it catches a window that is off by one key at either end (each
of the four mutants lands >= 10x outside it), that the Python copies of the
host-side plan and gate agree with the package and the built extension, and
that the mask composition and the KeyWindow routing compute the window.
"""
import pytest
import torch

import _decode_attn_ref as R
from perceiver_amd.ops import decode_attn as da
from perceiver_amd.ops.attention import eager_attention, scaled_dot_attention

ALL = R.all_cases()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_python_plan_reaches_the_case_slices(name):
    case = R.CASES[name]
    b, h, cap, d, _ = case["shape"]
    assert R.plan(b, h, cap, d)[0] == case["nsplit"]


def test_plan_bounds():
    assert R.plan(3, 2, 48, 16) == (1, 32)
    assert R.plan(3, 2, 2048, 64)[0] > 1
    assert R.plan(1, 1, 1 << 20, 128) == (32, 4)
    assert R.plan(64, 8, 8192, 128)[0] == 1  # B*H fills the chip
    for blocks in (1, 2, 6, 100, 511, 512, 4096):
        for cap in (1, 48, 255, 256, 1024, 8192, 1 << 20):
            n, g = R.plan(blocks, 1, cap, 64)
            assert 1 <= n <= 32 and g == 8


def test_python_copies_match_package_and_extension():
    args = [(b, h, cap, d) for b in (1, 2, 3, 32, 64) for h in (1, 2, 4, 8, 16)
            for cap in (1, 48, 255, 256, 512, 1024, 2048, 8192, 100000)
            for d in range(8, 129, 8)]
    for a in args:
        assert da.decode_attn_plan(*a) == R.plan(*a), a
    dims = [(d, dv) for d in range(0, 145, 4) for dv in range(0, 145, 4)]
    for d, dv in dims:
        assert da.decode_attn_applicable(d, dv) == R.applicable(d, dv), (d, dv)

    from perceiver_amd.ops import hip

    try:
        ext = hip.ext()
    except (ImportError, RuntimeError):
        pytest.skip("in-tree extension not built")
    for a in args:
        assert tuple(ext.decode_attn_plan(*a)) == R.plan(*a), a
    for d, dv in dims:
        assert bool(ext.decode_attn_applicable(d, dv)) == R.applicable(d, dv), (d, dv)


def _emulate(name, n=None, dlo=0, dhi=0):
    q, k, v, lo, hi, _ = R.case_data(name, n)
    b, h, cap, d, _ = R.CASES[name]["shape"]
    return R.emulate(q, k, v, lo + dlo, hi + dhi, *R.plan(b, h, cap, d))


@pytest.mark.parametrize("case", ALL, ids=R.case_id)
def test_emulation_stays_inside_the_bound(case):
    _, _, _, _, _, (out_ref, _, _, abs_pv) = R.case_data(*case)
    out = _emulate(*case)
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    print(f"{R.case_id(case)}: emulation error/tol {ratio:.3f}")
    assert torch.isfinite(out.float()).all()
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("mutant", sorted(R.MUTANTS))
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_bound_catches_an_off_by_one_window(name, mutant):
    _, _, _, _, _, (out_ref, _, _, abs_pv) = R.case_data(name)
    out = _emulate(name, None, *R.MUTANTS[mutant])
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    print(f"{name}: window {mutant} lands at {ratio:.1f}x the bound")
    assert ratio >= 10.0, ratio


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_composition_computes_the_window(name):
    q, k, v, lo, hi, (out_ref, _, _, abs_pv) = R.case_data(name)
    out = da.decode_attn(q.float(), k.float(), v.float(), lo, hi)
    assert R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv)) <= 1.0
    routed = scaled_dot_attention(q.float(), k.float(), v.float(),
                                  pad_mask=da.KeyWindow(lo, hi), causal=True)
    assert torch.equal(routed, out)
    pad = R.window_pad(lo, hi, q.shape[0], k.shape[2])
    assert torch.equal(out, eager_attention(q.float(), k.float(), v.float(), pad_mask=pad))


def test_composition_clamps_and_zeroes_empty_windows():
    q, k, v, _, _, _ = R.case_data("small_unsplit")
    q, k, v = q.float(), k.float(), v.float()
    cap = k.shape[2]
    lo = torch.tensor([-7, 5, 40])
    hi = torch.tensor([30, cap + 100, 39])  # row 2 is empty
    out = da.decode_attn(q, k, v, lo, hi)
    want = da.decode_attn(q, k, v, torch.tensor([0, 5, 0]), torch.tensor([30, cap - 1, 0]))
    assert torch.equal(out[:2], want[:2])
    assert torch.count_nonzero(out[2]) == 0
    # lo absent means 0; one element serves every row
    a = da.decode_attn(q, k, v, None, torch.tensor([30]))
    b = da.decode_attn(q, k, v, torch.zeros(3, dtype=torch.long), torch.tensor([30, 30, 30]))
    assert torch.equal(a, b)


def test_tensor_pad_mask_is_untouched():
    q, k, v, lo, hi, _ = R.case_data("small_unsplit")
    pad = R.window_pad(lo, hi, q.shape[0], k.shape[2])
    got = scaled_dot_attention(q.float(), k.float(), v.float(), pad_mask=pad)
    assert torch.equal(got, eager_attention(q.float(), k.float(), v.float(), pad_mask=pad))
