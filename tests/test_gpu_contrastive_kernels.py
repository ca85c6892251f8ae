"""The contrastive-search kernels (ops/csrc/contrastive.hip) against the fp64
oracle of the rules: contrastive_sim over channel counts, candidate counts,
capacities and history lengths around every edge of its row granule and its
slices; contrastive_commit over vocabularies and logit dtypes; contrastive_copy.

Worst measured error / bound ratios are printed by every case."""
import pytest
import torch

import _contrastive_ref as ref

from perceiver_amd.ops import beam
from perceiver_amd.ops import contrastive as cs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
G = ref.SIM_GROUPS


def _length(n):
    return torch.tensor([n], dtype=torch.long, device=DEV)


def _finish(part, h, k):
    """sim (G, k) from the partial maxima, as contrastive_commit finishes it."""
    return part[:, :, :k].amax(0) * cs.recip_norm(h).view(-1, k)


@pytest.mark.parametrize("cap", ref.SIM_CAPS)
@pytest.mark.parametrize("k", ref.SIM_K)
@pytest.mark.parametrize("C", ref.SIM_CHANNELS)
def test_sim_against_the_oracle(C, k, cap):
    nsplit, granule = cs.plan(G, cap, C)
    assert (nsplit, granule) == ref.plan_twin(G, cap, C)
    assert nsplit == (1 if cap == 16 else 16)
    assert granule == {8: 64, 32: 16, 40: 8, 520: 1, 1280: 1}[C]
    h, hist, rnorm = ref.sim_inputs(C, k, cap)
    want = ref.sim_oracle_all(h, hist, k)
    h, hist, rnorm = h.to(DEV), hist.to(DEV), rnorm.to(DEV)
    worst, n_t = 0.0, _length(0)
    for n in ref.hist_lens(G, cap, C):
        n_t.fill_(n)
        part = cs.contrastive_sim(h, hist, rnorm, n_t, k)
        assert part.shape == (nsplit, G, 8) and part.dtype == torch.float32
        # slices past the history hold -inf, the others a real maximum
        per = ref.slice_rows(n, nsplit, granule)
        live = torch.arange(nsplit) * per < n
        assert torch.equal(torch.isinf(part[:, :, :k]).all(-1).all(-1).cpu(), ~live)
        got = _finish(part, h, k).double().cpu()
        err = float((got - want[:, :n].amax(1)).abs().max())
        worst = max(worst, err / ref.sim_bound(C))
    print(f"C={C} k={k} cap={cap}: worst sim error / bound = {worst:.3f}")
    assert worst <= 1.0


def test_sim_strided_hiddens_equal_a_contiguous_copy_and_runs_repeat():
    C, k, cap = 40, 3, 1024
    h, hist, rnorm = (t.to(DEV) for t in ref.sim_inputs(C, k, cap))
    wide = torch.randn(G * k, 3, C, device=DEV).bfloat16()
    wide[:, -1] = h
    view = wide[:, -1, :]
    assert not view.is_contiguous()
    n_t = _length(777)
    a = cs.contrastive_sim(h, hist, rnorm, n_t, k)
    b = cs.contrastive_sim(view, hist, rnorm, n_t, k)
    c = cs.contrastive_sim(view, hist, rnorm, n_t, k)
    assert torch.equal(a[:, :, :k], b[:, :, :k]) and torch.equal(b[:, :, :k], c[:, :, :k])


@pytest.mark.parametrize("n,clamped", [(-1, 0), (-2 ** 40, 0), (1025, 1024), (2 ** 40, 1024)])
def test_sim_garbage_length_is_clamped(n, clamped):
    C, k, cap = 32, 2, 1024
    h, hist, rnorm = ref.sim_inputs(C, k, cap)
    h = h.to(DEV)
    # the history and its norms sit between neighbours: NaN guards that would
    # poison a maximum if the sweep read them, and that must stay as they are
    pad = 4 * C
    big = torch.full((hist.numel() + 2 * pad,), float("nan"), dtype=torch.bfloat16, device=DEV)
    hist_d = big[pad:-pad].view(hist.shape)
    hist_d.copy_(hist)
    rbig = torch.full((rnorm.numel() + 8,), float("nan"), device=DEV)
    rnorm_d = rbig[4:-4].view(rnorm.shape)
    rnorm_d.copy_(rnorm)
    got = cs.contrastive_sim(h, hist_d, rnorm_d, _length(n), k)[:, :, :k]
    want = cs.contrastive_sim(h, hist.to(DEV), rnorm.to(DEV), _length(clamped), k)[:, :, :k]
    assert torch.equal(got, want) and not bool(torch.isnan(got).any())
    assert bool(torch.isnan(big[:pad]).all()) and bool(torch.isnan(big[-pad:]).all())
    assert bool(torch.isnan(rbig[:4]).all()) and bool(torch.isnan(rbig[-4:]).all())
    assert torch.equal(hist_d.view(torch.int16), hist.to(DEV).view(torch.int16))
    assert torch.equal(rnorm_d, rnorm.to(DEV))
    if clamped == 0:
        assert bool(torch.isinf(got).all()) and bool((got < 0).all())


def test_sim_at_the_widest_rows():
    # 8 candidate slots of MAX_CHANNELS bf16 plus the waves' maxima are exactly
    # 64 KiB of LDS; a lane takes 7 or 8 of a row's 511 chunks
    C, k, cap = ref.MAX_CHANNELS, 8, 16
    assert cs.in_range(61, k, C) and not cs.in_range(61, k, C + 8)
    assert cs.plan(G, cap, C) == ref.plan_twin(G, cap, C) == (1, 1)
    h, hist, rnorm = ref.sim_inputs(C, k, cap)
    want = ref.sim_oracle_all(h, hist, k)
    h, hist, rnorm = h.to(DEV), hist.to(DEV), rnorm.to(DEV)
    worst = 0.0
    for n in (1, 15, 16):
        got = _finish(cs.contrastive_sim(h, hist, rnorm, _length(n), k), h, k).double().cpu()
        worst = max(worst, float((got - want[:, :n].amax(1)).abs().max()) / ref.sim_bound(C))
    print(f"C={C} k={k} cap={cap}: worst sim error / bound = {worst:.3f}")
    assert worst <= 1.0
    with pytest.raises(RuntimeError):
        wide = torch.zeros(G * k, C + 8, dtype=torch.bfloat16, device=DEV)
        cs.contrastive_sim(wide, torch.zeros(G, cap, C + 8, dtype=torch.bfloat16, device=DEV),
                           rnorm, _length(1), k)


def test_sim_nan_hidden_gives_nan_sim():
    C, k, cap = 520, 3, 16
    h, hist, rnorm = (t.to(DEV) for t in ref.sim_inputs(C, k, cap))
    h[k + 1, 77] = float("nan")  # group 1, candidate 1
    sim = _finish(cs.contrastive_sim(h, hist, rnorm, _length(11), k), h, k)
    nan = torch.isnan(sim).cpu()
    assert nan.tolist() == [[False] * 3, [False, True, False]]
    # a NaN in the history reaches every candidate of its group
    h, hist, rnorm = (t.to(DEV) for t in ref.sim_inputs(C, k, cap))
    hist[0, 4, 3] = float("nan")
    sim = _finish(cs.contrastive_sim(h, hist, rnorm, _length(11), k), h, k)
    assert torch.isnan(sim).cpu().tolist() == [[True] * 3, [False] * 3]
    sim = _finish(cs.contrastive_sim(h, hist, rnorm, _length(4), k), h, k)
    assert not bool(torch.isnan(sim).any())


# ------------------------------------------------------------------- commit

GROUPS, K, C, CAP, N = 3, 4, 32, 16, 9
ALPHA, FILL, STEP, SENTINEL = 0.6, 3, 5, -7


def _commit_inputs(V, dtype, seed):
    """Three groups of four candidates with a history of N rows; group 1 is
    already done. The logits and hidden states are (B, 2, .)[:, -1, :] views."""
    g = torch.Generator().manual_seed(seed)
    h3 = (torch.randn(GROUPS * K, 2, C, generator=g) * 2).bfloat16()
    hist = (torch.randn(GROUPS, CAP, C, generator=g) * 0.5).bfloat16()
    logits3 = (torch.randn(GROUPS * K, 2, V, generator=g) * 3).to(dtype)
    tok = torch.stack([torch.randperm(V, generator=g)[:K] for _ in range(GROUPS)]).reshape(-1)
    prob = torch.rand(GROUPS * K, generator=g) * 0.3
    done = torch.tensor([False, True, False])
    return h3, hist, cs.recip_norm(hist), logits3, tok, prob, done


def _oracle(h, hist, tok, prob, done, eos, n=N):
    return [ref.step64(h[g * K:(g + 1) * K], hist[g], n, tok[g * K:(g + 1) * K],
                       prob[g * K:(g + 1) * K], bool(done[g]), ALPHA, eos, FILL)
            for g in range(GROUPS)]


def _clear_gap_inputs(V, dtype):
    for seed in range(50):
        inp = _commit_inputs(V, dtype, seed)
        h3, hist, rnorm, logits3, tok, prob, done = inp
        steps = _oracle(h3[:, -1], hist, tok, prob, done, -1)
        tol = ref.score_tolerance(ALPHA, C, logits3[:, -1].float())
        gaps = [float(s[4].sort(descending=True).values[:2].diff().abs()) for s in steps]
        if min(gaps) >= 64 * tol and any(s[0] != 0 for s in steps):
            return inp, steps
    raise AssertionError("no seed gives a clear gap in every group")


def _run_commit(h, hist, rnorm, logits, tok, prob, done, eos, n=N):
    """One sim + commit on the device; returns the state the kernel wrote."""
    st = dict(
        tok=tok.to(DEV), prob=prob.to(DEV), done=done.to(DEV),
        src=torch.full((GROUPS * K,), -1, dtype=torch.int32, device=DEV),
        rec=torch.full((CAP + 1, GROUPS), SENTINEL, dtype=torch.long, device=DEV),
        sim=torch.zeros(GROUPS * K, device=DEV), score=torch.zeros(GROUPS * K, device=DEV),
        hist=hist, rnorm=rnorm)
    n_t = _length(n)
    part = cs.contrastive_sim(h, hist, rnorm, n_t, K)
    cs.commit_step(logits, st["tok"], st["prob"], K, h=h, part=part, hist=hist, rnorm=rnorm,
                   hist_len=n_t, done=st["done"], src=st["src"],
                   alpha=torch.tensor([ALPHA], device=DEV),
                   eos_fill=torch.tensor([eos, FILL], device=DEV),
                   step=_length(STEP), rec=st["rec"], sim_out=st["sim"], score_out=st["score"])
    torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", ref.COMMIT_VOCABS)
def test_commit_against_the_oracle(V, dtype):
    (h3, hist, rnorm, logits3, tok, prob, done), free = _clear_gap_inputs(V, dtype)
    eos = free[0][1]  # group 0 emits it in this very step
    want = _oracle(h3[:, -1], hist, tok, prob, done, eos)
    h, logits = h3.to(DEV)[:, -1, :], logits3.to(DEV)[:, -1, :]
    assert not logits.is_contiguous()
    hist_d, rnorm_d = hist.to(DEV), rnorm.to(DEV)
    st = _run_commit(h, hist_d, rnorm_d, logits, tok, prob, done, eos)

    sel = [w[0] for w in want]
    assert st["src"].cpu().view(GROUPS, K).tolist() == [[s] * K for s in sel]
    assert any(s != 0 for s in sel)
    sim_err = max(float((st["sim"].cpu().view(GROUPS, K)[g].double() - want[g][3]).abs().max())
                  for g in range(GROUPS))
    tol = ref.score_tolerance(ALPHA, C, logits3[:, -1].float())
    score_err = max(float((st["score"].cpu().view(GROUPS, K)[g].double() - want[g][4]).abs().max())
                    for g in range(GROUPS))
    assert sim_err <= ref.sim_bound(C) and score_err <= tol

    # done and fill: group 0 reaches EOS now, group 1 was done and emits the fill id
    emitted = [w[1] for w in want]
    assert emitted[0] == eos and emitted[1] == FILL
    assert st["done"].cpu().tolist() == [w[2] for w in want] and want[0][2] and want[1][2]
    # the record lands in row STEP and nowhere else
    rec = st["rec"].cpu()
    assert rec[STEP].tolist() == emitted
    rec[STEP] = SENTINEL
    assert bool((rec == SENTINEL).all())
    # the append lands at row N and nowhere else
    rows = torch.tensor([g * K + sel[g] for g in range(GROUPS)])
    new_hist, new_rnorm = st["hist"].cpu(), st["rnorm"].cpu()
    assert torch.equal(new_hist[:, N].view(torch.int16), h3[rows, -1].view(torch.int16))
    r64 = 1.0 / h3[rows, -1].double().norm(dim=-1)
    assert float(((new_rnorm[:, N].double() - r64) / r64).abs().max()) <= (C + 4) * 2.0 ** -24
    keep = torch.ones(CAP, dtype=torch.bool)
    keep[N] = False
    assert torch.equal(new_hist[:, keep].view(torch.int16), hist[:, keep].view(torch.int16))
    assert torch.equal(new_rnorm[:, keep], rnorm[:, keep])

    # the next candidates come from row sel's logits: valid, ordered, full-softmax p
    x = logits3[rows, -1].float()
    new_tok, new_prob = st["tok"].cpu().view(GROUPS, K), st["prob"].cpu().view(GROUPS, K)
    assert bool((new_tok >= 0).all()) and bool((new_tok < V).all())
    p_err, p_tol = 0.0, ref.prob_tolerance(x)
    for g in range(GROUPS):
        want_tok, want_p = ref.propose64(x[g], K)
        assert new_tok[g].tolist() == want_tok
        p_err = max(p_err, float((new_prob[g].double() - torch.tensor(want_p)).abs().max()))
    print(f"V={V} {dtype}: sim error / bound = {sim_err / ref.sim_bound(C):.3f}, "
          f"score error / tolerance = {score_err / tol:.3f}, p error / tolerance = {p_err / p_tol:.3f}")
    assert p_err <= p_tol

    # two runs agree bit for bit
    again = _run_commit(h, hist.to(DEV), rnorm.to(DEV), logits, tok, prob, done, eos)
    for name in ("tok", "prob", "done", "src", "rec", "sim", "score", "hist", "rnorm"):
        assert torch.equal(st[name], again[name]), name


def test_commit_ties():
    V = 262
    h3, hist, rnorm, logits3, tok, prob, done = _commit_inputs(V, torch.float32, 0)
    done[:] = False
    # group 0: candidates 1 and 2 share a hidden state and a probability, far from the history
    h3[2] = h3[1]
    hist[0, :N] -= (2 * h3[1, -1].float()).bfloat16()
    prob[:K] = torch.tensor([0.2, 0.3, 0.3, 0.1])
    # every row's logits: three equal maxima below one larger value
    logits3[:] = -3.0
    logits3[:, -1, [170, 40, 90]] = 2.0
    logits3[:, -1, 200] = 2.5
    rnorm = cs.recip_norm(hist)
    want = _oracle(h3[:, -1], hist, tok, prob, done, -1)
    assert want[0][0] == 1 and float(want[0][4][1]) == float(want[0][4][2])
    st = _run_commit(h3.to(DEV)[:, -1, :], hist.to(DEV), rnorm.to(DEV), logits3.to(DEV)[:, -1, :],
                     tok, prob, done, -1)
    score = st["score"].cpu().view(GROUPS, K)
    assert float(score[0, 1]) == float(score[0, 2]) == float(score[0].max())
    assert st["src"].cpu()[:K].tolist() == [1] * K  # equal scores: the lowest j
    assert st["tok"].cpu().view(GROUPS, K).tolist() == [[200, 40, 90, 170]] * GROUPS
    assert not bool(st["done"].any())


def test_commit_garbage_length_stays_inside_the_history():
    V = 61
    h3, hist, rnorm, logits3, tok, prob, done = _commit_inputs(V, torch.float32, 1)
    pad = 4 * C
    for n, at in ((-5, 0), (CAP, CAP - 1), (CAP + 7, CAP - 1), (2 ** 40, CAP - 1)):
        big = torch.full((GROUPS * CAP * C + 2 * pad,), 1.5, dtype=torch.bfloat16, device=DEV)
        hist_d = big[pad:-pad].view(GROUPS, CAP, C)
        hist_d.copy_(hist)
        rbig = torch.full((GROUPS * CAP + 8,), 2.5, device=DEV)
        rnorm_d = rbig[4:-4].view(GROUPS, CAP)
        rnorm_d.copy_(rnorm)
        st = _run_commit(h3.to(DEV)[:, -1, :], hist_d, rnorm_d, logits3.to(DEV)[:, -1, :],
                         tok, prob, done, -1, n=n)
        assert bool((big[:pad] == 1.5).all()) and bool((big[-pad:] == 1.5).all())
        assert bool((rbig[:4] == 2.5).all()) and bool((rbig[-4:] == 2.5).all())
        keep = torch.ones(CAP, dtype=torch.bool)
        keep[at] = False
        assert torch.equal(hist_d.cpu()[:, keep].view(torch.int16), hist[:, keep].view(torch.int16))
        sel = st["src"].cpu().view(GROUPS, K)[:, 0].long()
        rows = sel + torch.arange(GROUPS) * K
        assert torch.equal(hist_d.cpu()[:, at].view(torch.int16), h3[rows, -1].view(torch.int16))
        if n < 0:  # no rows: every similarity is 0
            assert float(st["sim"].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_proposal_alone_reads_row_0_of_every_group(dtype):
    V = 1500
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(GROUPS * K, V, generator=g) * 3).to(dtype)
    tok = torch.full((GROUPS * K,), -1, dtype=torch.long, device=DEV)
    prob = torch.zeros(GROUPS * K, device=DEV)
    cs.propose_step(logits.to(DEV), tok, prob, K)
    x = logits[::K].float()
    for gi in range(GROUPS):
        want_tok, want_p = ref.propose64(x[gi], K)
        assert tok.cpu().view(GROUPS, K)[gi].tolist() == want_tok
        err = (prob.cpu().view(GROUPS, K)[gi].double() - torch.tensor(want_p)).abs().max()
        assert float(err) <= ref.prob_tolerance(x)


# --------------------------------------------------------------------- copy

@pytest.mark.parametrize("width", [32, 13])
def test_copy_moves_one_row_of_every_buffer(width):
    k, groups, cap = 3, 2, 10
    bufs = [torch.randn(groups * k, cap, width, device=DEV).bfloat16() for _ in range(3)]
    before = [b.clone() for b in bufs]
    table = beam.reorder_table(bufs, [0, 0, 0], [0, 1, 1]).to(DEV)
    counters = torch.tensor([4, 7, 0, 0], dtype=torch.long, device=DEV)
    src = torch.tensor([2, 2, 2, 0, 0, 0], dtype=torch.int32, device=DEV)
    cs.contrastive_copy(table, counters, src, k, buffers=bufs)
    with pytest.raises(ValueError):
        cs.contrastive_copy(table, counters, src[:k], k, buffers=bufs)
    for buf, old, row in zip(bufs, before, (4, 7, 7)):
        want = old.clone().view(groups, k, cap, width)
        want[0, :, row] = want[0, 2, row]
        want[1, :, row] = want[1, 0, row]
        assert torch.equal(buf.view(torch.int16), want.view(groups * k, cap, width).view(torch.int16))
    # a garbage counter is clamped into the buffer, a garbage source into the group
    counters.fill_(2 ** 40)
    src.fill_(99)
    cs.contrastive_copy(table, counters, src, k, buffers=bufs)
    with pytest.raises(ValueError):
        cs.contrastive_copy(table, counters, src, k, buffers=bufs[:2])
    v = bufs[0].view(groups, k, cap, width)
    assert torch.equal(v[:, 0, cap - 1], v[:, 2, cap - 1])
