"""beam_reorder kernel: the in-place permutation of rows [row0, len] of every
described buffer equals index_select bit for bit, and every other row stays
bit-unchanged. A ragged channel count (C % 8 != 0) is taken, not refused: such
a buffer moves in 2-byte units."""
import pytest
import torch

from perceiver_amd.ops import beam as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BSZ = 3


def _src(nb):
    """identity, a swap / duplicates, all-zero: one pattern per group."""
    ident = list(range(nb))
    mixed = [1, 0] + [max(0, j - 2) for j in range(2, nb)]  # a swap, then duplicates
    return torch.tensor(ident + mixed + [0] * nb, dtype=torch.int32)


def _expected(buf, src, nb, row0, length):
    rows = src.long() + (torch.arange(src.numel()) // nb) * nb
    want = buf.clone()
    want[:, row0:length + 1] = buf.index_select(0, rows)[:, row0:length + 1]
    return want


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


@pytest.mark.parametrize("nb", [4, 8])
@pytest.mark.parametrize("cap,C", [(40, 32), (16, 32), (40, 13), (16, 7)])
@pytest.mark.parametrize("rows", ["from_zero", "mid", "single"])
def test_one_buffer_matches_index_select(nb, cap, C, rows):
    length = cap - 3
    row0 = {"from_zero": 0, "mid": cap // 2, "single": length}[rows]
    g = torch.Generator().manual_seed(cap * 1000 + C * 10 + nb)
    buf = torch.randn(BSZ * nb, cap, C, generator=g).to(torch.bfloat16)
    src = _src(nb)
    want = _expected(buf, src, nb, row0, length)
    assert not torch.equal(_bits(want), _bits(buf))

    dbuf = buf.to(DEV)
    table = B.reorder_table([dbuf], [row0], [1])
    assert table[0, 3] == (16 if C % 8 == 0 else 2)
    counters = torch.tensor([0, length, 0, 0], dtype=torch.long, device=DEV)
    B.beam_reorder(table.to(DEV), counters, src.to(DEV), nb, buffers=[dbuf])
    torch.cuda.synchronize()
    got = dbuf.cpu()
    assert torch.equal(_bits(got), _bits(want))
    # rows below row0 and above len are the input's, bit for bit
    assert torch.equal(_bits(got[:, :row0]), _bits(buf[:, :row0]))
    assert torch.equal(_bits(got[:, length + 1:]), _bits(buf[:, length + 1:]))


@pytest.mark.parametrize("nb", [2, 3, 5, 8])
def test_several_buffers_in_one_launch(nb):
    # different capacities, channel counts, element sizes, start rows and counters
    specs = [(40, 32, torch.bfloat16, 5, 0), (16, 64, torch.bfloat16, 0, 1),
             (24, 13, torch.bfloat16, 7, 1), (16, 8, torch.float32, 3, 1),
             (40, 20, torch.float16, 30, 0)]
    lens = [33, 12]
    g = torch.Generator().manual_seed(nb)
    src = torch.randint(0, nb, (BSZ * nb,), generator=g, dtype=torch.int32)
    src[:nb] = torch.arange(nb, dtype=torch.int32)  # one identity group
    bufs = [torch.randn(BSZ * nb, cap, C, generator=g).to(dt) for cap, C, dt, _, _ in specs]
    want = [_expected(b, src, nb, r0, lens[ci]) for b, (_, _, _, r0, ci) in zip(bufs, specs)]
    dbufs = [b.to(DEV) for b in bufs]
    table = B.reorder_table(dbufs, [s[3] for s in specs], [s[4] for s in specs]).to(DEV)
    counters = torch.tensor(lens, dtype=torch.long, device=DEV)
    B.beam_reorder(table, counters, src.to(DEV), nb, buffers=dbufs)
    torch.cuda.synchronize()
    for got, w in zip(dbufs, want):
        assert torch.equal(_bits(got.cpu()), _bits(w))


def test_a_counter_past_the_capacity_stays_inside_the_buffer():
    nb, cap, C = 4, 16, 32
    g = torch.Generator().manual_seed(5)
    pair = torch.randn(2, BSZ * nb, cap, C, generator=g).to(torch.bfloat16).to(DEV)
    before = pair.cpu()
    src = _src(nb)
    table = B.reorder_table([pair[0]], [4], [0]).to(DEV)
    # a stale counter a few rows past the end: were it not clamped, the rows would land in pair[1]
    counters = torch.tensor([cap + 5], dtype=torch.long, device=DEV)
    B.beam_reorder(table, counters, src.to(DEV), nb, buffers=[pair[0]])
    torch.cuda.synchronize()
    want = _expected(before[0], src, nb, 4, cap - 1)
    assert torch.equal(_bits(pair[0].cpu()), _bits(want))
    assert torch.equal(_bits(pair[1].cpu()), _bits(before[1]))  # the neighbour is untouched
