"""beam_select kernel against an fp64 reference of the rules in ops/beam.py:
validity of the returned candidates within a tolerance derived from torch's own
fp32 error, exact selection on inputs with a clear gap, the constructed tie
cases, and the done / gen_len bookkeeping."""
import pytest
import torch

from _beam_ref import candidates64, tie_cases, tolerance

from perceiver_amd.ops import hip
from perceiver_amd.ops.beam import beam_select_reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EOS, FILL = 3, 5
CASES = [(262, 4, 3), (389, 3, 2), (61, 8, 1), (1500, 8, 2), (32768, 2, 1)]


def _inputs(V, nb, bsz, dtype, seed, with_done):
    """x is the [:, -1, :] view of a (B, 3, V) tensor: a strided, unaligned row."""
    g = torch.Generator().manual_seed(1000003 * V + 131 * nb + seed)
    B = bsz * nb
    full = (torch.randn(B, 3, V, generator=g) * 3.0).to(dtype)
    scores = -torch.rand(B, generator=g) * 5.0
    gen_len = torch.randint(0, 9, (B,), generator=g, dtype=torch.int32)
    done = torch.zeros(B, dtype=torch.bool)
    if with_done:
        done[1::3] = True  # every group of 2..8 rows mixes live and frozen beams
    return full, scores, done, gen_len


def _launch(full, scores, done, gen_len, nb, eos=EOS, fill=FILL):
    view = full.to(DEV)[:, -1, :]
    assert not view.is_contiguous() or full.shape[0] == 1
    B = view.shape[0]
    st = dict(score=scores.clone().to(DEV), done=done.clone().to(DEV),
              gen_len=gen_len.clone().to(DEV),
              tok=torch.full((B,), -1, dtype=torch.long, device=DEV),
              src=torch.full((B,), -1, dtype=torch.int32, device=DEV),
              all_done=torch.zeros(B // nb, dtype=torch.bool, device=DEV))
    hip.ext().beam_select(view, st["score"], st["done"], st["gen_len"], st["tok"], st["src"],
                          st["all_done"], torch.tensor([eos, fill], device=DEV), nb)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in st.items()}


def _check_bookkeeping(out, done, gen_len, nb, eos):
    """done' and gen_len' follow exactly from the returned (src, tok)."""
    B = done.numel()
    rows = out["src"].long() + (torch.arange(B) // nb) * nb
    was = done[rows]
    assert torch.equal(out["done"], was | (out["tok"] == eos))
    assert torch.equal(out["gen_len"], gen_len[rows] + (~was).int())
    assert torch.equal(out["all_done"], out["done"].view(-1, nb).all(-1))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,nb,bsz", CASES)
def test_returned_candidates_are_valid(V, nb, bsz, dtype):
    full, scores, done, gen_len = _inputs(V, nb, bsz, dtype, 0, with_done=True)
    x = full[:, -1, :]
    out = _launch(full, scores, done, gen_len, nb)
    B = bsz * nb
    src, tok = out["src"].long(), out["tok"]
    assert ((src >= 0) & (src < nb)).all() and ((tok >= 0) & (tok < V)).all()
    rows = src + (torch.arange(B) // nb) * nb
    ref = candidates64(x, scores, done, FILL)
    # the issue's tolerance (its floor is an ulp of the -1e9 candidates here)
    # and the one of the live rows alone, which binds every live candidate
    tol_all = tolerance(x, scores, done, FILL)
    tol_live = tolerance(x, scores, done, FILL, rows=~done)
    got = out["score"].double()
    at = ref[rows, tok]
    print(f"V={V} nb={nb} {dtype}: tol_all={tol_all:.3e} tol_live={tol_live:.3e} "
          f"max |score - ref| = {float((got - at).abs().max()):.3e}")
    assert (got - at).abs().max() <= tol_all
    live = (~done[rows]) & (at > -1e8)
    assert live.any()
    assert (got - at)[live].abs().max() <= tol_live
    # distinct candidates, best first
    flat = (rows * V + tok).view(bsz, nb)
    assert all(len(set(r)) == nb for r in flat.tolist())
    assert (got.view(bsz, nb)[:, 1:] <= got.view(bsz, nb)[:, :-1]).all()
    # nothing that was left out beats the smallest returned candidate
    rest = ref.clone()
    rest[rows, tok] = float("-inf")
    left = rest.view(bsz, nb * V).max(-1).values
    smallest = at.view(bsz, nb).min(-1).values
    tol = torch.where(smallest > -1e8, tol_live, tol_all)
    assert (left <= smallest + tol).all(), (left, smallest)
    _check_bookkeeping(out, done, gen_len, nb, EOS)


def _gap_inputs(V, nb, bsz, dtype):
    """The first seed whose fp64 reference has a gap of at least 64 tol between
    consecutive entries of every group's top nb + 1."""
    for seed in range(1, 200):
        full, scores, done, gen_len = _inputs(V, nb, bsz, dtype, seed, with_done=False)
        x = full[:, -1, :]
        tol = tolerance(x, scores, done, FILL)
        top = candidates64(x, scores, done, FILL).view(bsz, nb * V).topk(nb + 1).values
        if float((top[:, :-1] - top[:, 1:]).min()) >= 64 * tol:
            return full, scores, done, gen_len, tol
    raise AssertionError(f"no seed gives a clear gap at V={V}, nb={nb}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V,nb,bsz", CASES)
def test_exact_selection_on_clear_gaps(V, nb, bsz, dtype):
    full, scores, done, gen_len, tol = _gap_inputs(V, nb, bsz, dtype)
    x = full[:, -1, :]
    ref = candidates64(x, scores, done, FILL).view(bsz, nb * V)
    top = ref.topk(nb + 1)
    assert float((top.values[:, :-1] - top.values[:, 1:]).min()) >= 64 * tol  # precondition
    want_src = (top.indices[:, :nb] // V).reshape(-1)
    want_tok = (top.indices[:, :nb] % V).reshape(-1)
    out = _launch(full, scores, done, gen_len, nb)
    assert torch.equal(out["src"].long(), want_src)
    assert torch.equal(out["tok"], want_tok)
    assert (out["score"].double() - top.values[:, :nb].reshape(-1)).abs().max() <= tol
    # the whole step equals the fp64 statement of the rules
    w = beam_select_reference(x.float(), scores, done, gen_len, nb, EOS, FILL, dtype=torch.float64)
    assert torch.equal(out["src"], w[0]) and torch.equal(out["tok"], w[1])
    assert torch.equal(out["done"], w[3]) and torch.equal(out["gen_len"], w[4])
    assert torch.equal(out["all_done"], w[5])
    _check_bookkeeping(out, done, gen_len, nb, EOS)
    # two runs agree bit for bit
    again = _launch(full, scores, done, gen_len, nb)
    assert all(torch.equal(out[k], again[k]) for k in out)


@pytest.mark.parametrize("name", ["identical_rows", "duplicates_in_a_row"])
def test_tie_rule(name):
    x, s, done, nb, eos, fill, want_src, want_tok = tie_cases()[name]
    full = x[:, None, :].repeat(1, 3, 1).contiguous()
    out = _launch(full, s, done, torch.zeros(len(s), dtype=torch.int32), nb, eos=eos, fill=fill)
    assert out["src"].tolist() == want_src and out["tok"].tolist() == want_tok
    if name == "identical_rows":  # identical rows give identical bits
        assert len(set(out["score"].tolist())) == 1


def test_frozen_groups_nan_rows_and_the_record():
    nb, V, bsz = 3, 61, 2
    B = nb * bsz
    full, scores, done, gen_len = _inputs(V, nb, bsz, torch.float32, 7, with_done=False)
    done[:3] = True                    # group 0: every beam frozen
    full[4, -1, 20] = float("nan")     # group 1: a NaN compares largest
    view = full.to(DEV)[:, -1, :]
    st = dict(score=scores.clone().to(DEV), done=done.clone().to(DEV),
              gen_len=gen_len.clone().to(DEV), tok=torch.zeros(B, dtype=torch.long, device=DEV),
              src=torch.zeros(B, dtype=torch.int32, device=DEV),
              all_done=torch.zeros(bsz, dtype=torch.bool, device=DEV))
    rec_tok = torch.full((4, B), -1, dtype=torch.long, device=DEV)
    rec_parent = torch.full((4, B), -1, dtype=torch.int32, device=DEV)
    rec_all = torch.zeros(4, bsz, dtype=torch.bool, device=DEV)
    hip.ext().beam_select(view, st["score"], st["done"], st["gen_len"], st["tok"], st["src"],
                          st["all_done"], torch.tensor([EOS, FILL], device=DEV), nb,
                          step=torch.tensor([1], device=DEV), rec_offset=1, rec_tok=rec_tok,
                          rec_parent=rec_parent, rec_all_done=rec_all)
    out = {k: v.cpu() for k, v in st.items()}
    # frozen beams keep score and length and propose the fill token, best first
    order = scores[:3].argsort(descending=True)
    assert out["src"][:3].tolist() == order.tolist() and out["tok"][:3].tolist() == [FILL] * 3
    assert torch.equal(out["score"][:3], scores[:3][order])
    assert torch.equal(out["gen_len"][:3], gen_len[:3][order])
    assert out["all_done"].tolist() == [True, False]
    # the NaN row's candidates are all NaN and come first, lowest index first
    assert out["src"][3:].tolist() == [1, 1, 1] and out["tok"][3:].tolist() == [0, 1, 2]
    assert out["score"][3:].isnan().all()
    # the record lands in row step + offset and nowhere else
    assert torch.equal(rec_tok[2].cpu(), out["tok"]) and torch.equal(rec_parent[2].cpu(), out["src"])
    assert rec_all[2].cpu().tolist() == [True, False]
    assert (rec_tok[[0, 1, 3]] == -1).all() and (rec_parent[[0, 1, 3]] == -1).all()
    _check_bookkeeping(out, done, gen_len, nb, EOS)
