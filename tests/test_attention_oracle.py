"""CPU tests of the attention oracle (tests/_attention_ref.py).

They show, without a GPU, that the derived bound is one the kernels' numerics
can meet (a CPU emulation of those numerics stays inside it at every case
shape) and one that catches the defects the GPU tests exist for (a skipped
tile, a skipped split, a mis-weighted merge land >= 10x outside it), and that
the Python copy of the split planner names the routes in the case table.
"""
import pytest
import torch

import _attention_ref as R

FWD_CASES = sorted(R.CASES)


def _emulate(name, **defect):
    case = R.CASES[name]
    q, k, v, pad, _ = R.case_data(name)
    nq, lk = case["shape"][2], case["shape"][3]
    got = R.route(case["shape"], case["causal"])
    nsplit, chunk = got["fwd"]
    return R.emulate(q, k, v, R.build_mask(pad, case["causal"], nq, lk), tile=R.KVBLK,
                     chunk=chunk if nsplit > 1 else None, **defect)


@pytest.mark.parametrize("name", FWD_CASES)
def test_python_plan_names_the_case_route(name):
    case = R.CASES[name]
    R.check_route(case, R.route(case["shape"], case["causal"]))


def test_python_plan_matches_extension():
    from perceiver_amd.ops import hip

    try:
        ext = hip.ext()
    except (ImportError, RuntimeError):
        pytest.skip("in-tree extension not built")
    for blocks in (1, 2, 3, 4, 8, 10, 12, 18, 64, 511, 512, 1280):
        for length in (1, 40, 70, 100, 256, 257, 330, 400, 576, 600, 1000, 2100, 4096, 182528):
            for tile in (32, 64):
                assert tuple(ext.flash_split_plan(blocks, length, tile)) == \
                    R.plan_split(blocks, length, tile), (blocks, length, tile)
    for d in range(16, 177, 16):
        for dv in range(16, 177, 16):
            for nq in (1, 127, 128, 600):
                assert bool(ext.flash_fwd_pipe_applicable(d, dv, nq)) == \
                    R.pipe_applicable(d, dv, nq), (d, dv, nq)
    for name, case in R.CASES.items():
        got = R.route(case["shape"], case["causal"], plan=ext.flash_split_plan,
                      pipe=ext.flash_fwd_pipe_applicable)
        assert got == R.route(case["shape"], case["causal"]), name


@pytest.mark.parametrize("name", FWD_CASES)
def test_emulation_stays_inside_the_bound(name):
    case = R.CASES[name]
    _, _, _, pad, (out_ref, lse_ref, _, abs_pv) = R.case_data(name)
    out, lse = _emulate(name)
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    live = R.live_rows(pad, case["shape"]).expand_as(lse)
    lse_err = (lse.double() - lse_ref)[live].abs().max().item()
    print(f"{name}: emulation error/tol {ratio:.3f}, lse error {lse_err:.2e}")
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    assert ratio <= 1.0, ratio
    assert lse_err <= R.LSE_TOL, lse_err


@pytest.mark.parametrize("name", FWD_CASES)
def test_bound_catches_a_skipped_tile(name):
    _, _, _, _, (out_ref, _, _, abs_pv) = R.case_data(name)
    out, _ = _emulate(name, skip_tile=0)
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    print(f"{name}: skipped tile lands at {ratio:.0f}x the bound")
    assert ratio >= 10.0, ratio


SPLIT_CASES = [n for n in FWD_CASES if R.CASES[n]["route"]["fwd"][0] > 1]


@pytest.mark.parametrize("defect", [{"skip_split": 0}, {"equal_weights": True}],
                         ids=["skipped_split", "equal_weights"])
@pytest.mark.parametrize("name", SPLIT_CASES)
def test_bound_catches_a_bad_merge(name, defect):
    _, _, _, _, (out_ref, _, _, abs_pv) = R.case_data(name)
    out, _ = _emulate(name, **defect)
    ratio = R.worst_ratio(out, out_ref, R.tol(out_ref, abs_pv))
    print(f"{name}: {defect} lands at {ratio:.0f}x the bound")
    assert ratio >= 10.0, ratio


@pytest.mark.parametrize("name", sorted(R.DEAD_BATCH))
def test_reference_and_emulation_average_v_on_fully_masked_rows(name):
    case = R.CASES[name]
    _, _, v, _, (out_ref, _, _, abs_pv) = R.case_data(name)
    b = R.DEAD_BATCH[name]
    mean_v = v[b].double().mean(dim=-2, keepdim=True).expand_as(out_ref[b])
    assert torch.allclose(out_ref[b], mean_v, atol=1e-12)
    out, lse = _emulate(name)
    assert R.worst_ratio(out[b], mean_v, R.tol(out_ref, abs_pv)[b]) <= 1.0
    assert torch.isfinite(lse[b]).all(), case
