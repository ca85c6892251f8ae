"""decode_select kernel against the torch reference of ops/sample.py: the kept
set (exact), greedy ties, the sampled distribution and the decode bookkeeping."""
import math

import pytest
import torch

from perceiver_amd.ops.sample import keep_mask, keep_mask_reference, select_tokens

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# per-row mixed parameters of the kept-set cases: (temperature, top_k, top_p);
# top_k 0 and top_p 1.0 are "off", and 10**6 is a top_k >= V
ROW_PARAMS = [(1.0, 0, 0.9), (0.7, 20, 0.5), (2.0, 7, 1.0), (0.5, 0, 0.3), (1.3, 10 ** 6, 0.8)]


def _above_mass(x, T, k):
    """fp64, per token of the top-k set: normalised mass of strictly larger logits."""
    sv = x.double().sort(descending=True).values
    if 0 < k < sv.numel():
        sv = sv[sv >= sv[k - 1]]
    w = torch.exp((sv - sv[0]) / T)
    excl = w.cumsum(0) - w
    first = torch.ones_like(sv, dtype=torch.bool)
    first[1:] = sv[1:] != sv[:-1]
    above = torch.where(first, excl, torch.zeros_like(excl)).cummax(0).values
    return above / w.sum()


def _boundary_margin(x, T, k, p):
    """Distance of top_p from the cumulative mass just before and just after the
    nucleus boundary (the nearest values on either side are the minimum)."""
    if not 0 < p < 1:
        return 1.0
    return float((_above_mass(x, T, k) - p).abs().min())


def _rows(V, dtype, scale=3.0, params=None, distinct=True):
    """(5, V) logits, chosen on the CPU by seed so that every row's nucleus
    boundary is at least 1e-4 clear of its top_p in fp64. fp32 rows are
    permutations of distinct values; bf16 rows have plenty of ties."""
    params = params or ROW_PARAMS
    for seed in range(500):
        g = torch.Generator().manual_seed(7919 * V + seed)
        x = (torch.randn(len(params), V, generator=g) * scale).to(dtype)
        if distinct and dtype == torch.float32 and any(r.unique().numel() != V for r in x):
            continue
        if all(_boundary_margin(r.float(), T, k, p) >= 1e-4
               for r, (T, k, p) in zip(x, params)):
            return x
    raise AssertionError(f"no seed gives a clear nucleus boundary at V={V}")


def _params(device, params=None):
    params = params or ROW_PARAMS
    T = torch.tensor([p[0] for p in params], dtype=torch.float32, device=device)
    k = torch.tensor([p[1] for p in params], dtype=torch.long, device=device)
    p = torch.tensor([p[2] for p in params], dtype=torch.float32, device=device)
    return T, k, p


@pytest.mark.parametrize("V", [61, 70, 262, 1024, 1025, 4099])
def test_kept_set_exact_fp32(V):
    x = _rows(V, torch.float32)
    for r, (T, k, p) in zip(x, ROW_PARAMS):
        assert _boundary_margin(r, T, k, p) >= 1e-4
    want = keep_mask_reference(x, *_params("cpu"))
    got = keep_mask(x.to(DEV), *_params(DEV))
    assert got.dtype == torch.bool and got.shape == (len(ROW_PARAMS), V)
    for row in range(len(ROW_PARAMS)):
        assert torch.equal(got[row].cpu(), want[row]), (V, row, ROW_PARAMS[row])
    # the cases are not vacuous: every row drops something and keeps something
    assert (want.sum(-1) < V)[:4].all() and (want.sum(-1) > 0).all()


def test_kept_set_exact_bf16_ties():
    x = _rows(262, torch.bfloat16, scale=2.0)
    assert all(r.unique().numel() < 262 for r in x)  # ties are there
    want = keep_mask_reference(x.float(), *_params("cpu"))
    got = keep_mask(x.to(DEV), *_params(DEV))
    for row in range(len(ROW_PARAMS)):
        assert torch.equal(got[row].cpu(), want[row]), (row, ROW_PARAMS[row])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [70, 262, 1025])
def test_greedy_lowest_index_wins_ties(dtype, V):
    B = 130  # more rows than one block of the wave tier holds
    g = torch.Generator().manual_seed(V)
    x = torch.randn(B, 3, V, generator=g).to(dtype)
    last = x[:, -1]  # strided view: row stride 3 * V
    pos = torch.randint(0, V, (B, 3), generator=g)
    top = last.float().max() + 1.0
    last.scatter_(1, pos, torch.full((B, 3), float(top)).to(dtype))  # duplicate maxima
    want = last.float().argmax(-1)
    assert torch.equal(want, pos.min(-1).values)
    xg = x.to(DEV)
    view = xg[:, -1]
    assert not view.is_contiguous()
    got = select_tokens(view, do_sample=False)
    assert got.dtype == torch.long and got.shape == (B,)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(got, view.float().argmax(-1))
    # a NaN compares as largest, as in torch.argmax
    xn = view.float().contiguous()
    xn[5, V // 2] = float("nan")
    assert torch.equal(select_tokens(xn, do_sample=False), xn.argmax(-1))


def test_sampled_distribution_and_determinism():
    V, B, T, K, P = 70, 128, 0.7, 20, 0.9
    neg = 11
    for seed in range(200):
        g = torch.Generator().manual_seed(424242 + seed)
        row = torch.randn(V, generator=g) * 2.0
        row[neg] = float("-inf")
        if row.unique().numel() == V and _boundary_margin(row, T, K, P) >= 1e-4:
            break
    else:
        raise AssertionError("no seed gives a clear nucleus boundary")
    keep = keep_mask_reference(row[None], T, K, P)[0]
    q = torch.where(keep, torch.exp((row.double() - row.max().double()) / T),
                    torch.zeros(V, dtype=torch.double))
    q = q / q.sum()
    assert not keep[neg] and 1 < int(keep.sum()) <= K

    logits = row.to(DEV).expand(B, V).contiguous()
    kw = dict(do_sample=True, temperature=T, top_k=K, top_p=P)
    draws = [select_tokens(logits, seed=2024, draw=d, **kw) for d in range(64)]
    toks = torch.stack(draws).cpu()  # (64, 128)
    N = toks.numel()
    counts = torch.bincount(toks.flatten(), minlength=V).double()
    assert counts[~keep].sum() == 0, "a token outside the kept set was drawn"
    assert counts[neg] == 0
    for t in keep.nonzero().flatten().tolist():
        qt = float(q[t])
        bound = 6 * math.sqrt(N * qt * (1 - qt)) + 1
        assert abs(float(counts[t]) - N * qt) <= bound, (t, float(counts[t]), N * qt, bound)

    # replays are deterministic given (seed, draw) ...
    again = select_tokens(logits, seed=2024, draw=5, **kw)
    assert torch.equal(again.cpu(), toks[5])
    # ... and fresh for another seed or another draw index
    assert not torch.equal(select_tokens(logits, seed=2025, draw=5, **kw).cpu(), toks[5])
    assert not torch.equal(toks[5], toks[6])
    # per-row mix: greedy rows of a sampling batch stay greedy
    ds = torch.zeros(B, dtype=torch.bool)
    ds[::2] = True
    mixed = select_tokens(logits, seed=2024, draw=5, do_sample=ds.to(DEV), temperature=T,
                          top_k=K, top_p=P).cpu()
    assert (mixed[1::2] == int(row.argmax())).all()
    assert torch.equal(mixed[::2], toks[5][::2])


def test_bookkeeping_in_the_same_launch():
    from perceiver_amd.ops import hip

    B, V, eos, fill = 5, 61, 5, 9
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(3))
    x[0, 7] = 50.0           # plain row
    x[1] = float("-inf")     # nothing to choose from: still a valid id
    x[2, eos] = 50.0         # emits EOS
    x[3, 7] = 50.0           # already done: emits the fill id
    x[4, 20] = float("nan")  # NaN row, sampled: still a valid id
    i32 = dict(dtype=torch.int32, device=DEV)
    prev = torch.tensor([10, 11, 12, 13, 14], device=DEV)
    tok = prev.clone()
    out_buf = torch.full((B, 8), -1, dtype=torch.long, device=DEV)
    done = torch.tensor([False, False, False, True, False], device=DEV)
    ret = hip.ext().decode_select(
        x.to(DEV), torch.tensor([0, 1, 0, 0, 1], **i32), torch.ones(B, device=DEV),
        torch.zeros(B, **i32), torch.full((B,), 0.9, device=DEV),
        torch.tensor([1], device=DEV), torch.tensor([0], device=DEV),
        tok=tok, out_buf=out_buf, step=torch.tensor([3], device=DEV), done=done,
        eos_fill=torch.tensor([eos, fill], device=DEV))
    assert ret.data_ptr() == tok.data_ptr()
    tok = tok.cpu()
    assert tok[0] == 7 and tok[2] == eos and tok[3] == fill
    assert 0 <= tok[1] < V and 0 <= tok[4] < V
    assert tok[4] == 20  # the NaN is the arg-max
    assert done.cpu().tolist() == [False, bool(tok[1] == eos), True, True, False]
    assert torch.equal(out_buf[:, 3], prev)  # previous token at the cursor column
    rest = torch.cat([out_buf[:, :3], out_buf[:, 4:]], dim=1)
    assert (rest == -1).all()


@pytest.mark.parametrize("V", [1024, 1025, 4099])
def test_sampled_tokens_stay_in_the_kept_set_at_the_tier_edge(V):
    x = _rows(V, torch.float32)
    B = x.shape[0]
    keep = keep_mask_reference(x, *_params("cpu"))
    xg = x.to(DEV)
    T, k, p = _params(DEV)
    seen = torch.zeros(B, V, dtype=torch.bool)
    for d in range(16):
        t = select_tokens(xg, do_sample=True, temperature=T, top_k=k, top_p=p, seed=9, draw=d)
        assert torch.equal(t, select_tokens(xg, do_sample=True, temperature=T, top_k=k, top_p=p,
                                            seed=9, draw=d))
        seen[torch.arange(B), t.cpu()] = True
    assert not (seen & ~keep).any()
    assert (seen.sum(-1) > 1).any()  # the draws do vary
    top1 = select_tokens(xg, do_sample=True, temperature=T, top_k=1, top_p=p, seed=9, draw=0)
    assert torch.equal(top1.cpu(), x.argmax(-1))


def test_largest_vocabulary_uses_the_big_lds_row():
    # V = 32768 is the last size the block tier takes: a 128 KiB row, past the
    # 64 KiB a kernel gets without opting in
    V = 32768
    params = [(1.0, 50, 1.0), (1.0, 0, 0.3), (0.7, 200, 0.6)]
    # 32768 fp32 normals collide now and then: ties are the reference's business too
    x = _rows(V, torch.float32, params=params, distinct=False)
    want = keep_mask_reference(x, *_params("cpu", params))
    xg = x.to(DEV)
    T, k, p = _params(DEV, params)
    got = keep_mask(xg, T, k, p)
    for row in range(len(params)):
        assert torch.equal(got[row].cpu(), want[row]), (row, params[row])
    assert int(want[0].sum()) == 50
    assert torch.equal(select_tokens(xg, do_sample=False).cpu(), x.argmax(-1))
    t = select_tokens(xg, do_sample=True, temperature=T, top_k=k, top_p=p, seed=3, draw=1)
    assert want[torch.arange(len(params)), t.cpu()].all()
