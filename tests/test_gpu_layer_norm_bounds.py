"""GPU tests of ln_fwd, add_ln_fwd and ln_bwd against the fp64 oracle in
tests/_norm_gemm_ref.py, over every input family (N(0, 1), offset, near-constant,
constant, eps-dominated, large) and the shapes of test_gpu_add_layer_norm.py
plus a ragged four-chunk row.

Every bound is a function of _norm_gemm_ref with its roundings counted in the
docstring; test_norm_gemm_oracle.py shows on the CPU that the kernels'
arithmetic can meet each of them and that the defects these tests exist for
cannot, the one-pass variance sumsq / C - mean^2 among them. Each test prints
its worst |got - ref| / bound before it asserts.
"""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

import _norm_gemm_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = list(R.LN_FAMILIES)


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _ratio(name, got, want, bound):
    r = R.worst_ratio(got.cpu(), want, bound)
    print(f"{name}: worst |got - ref| / bound = {r:.4f}")
    return r


def _fwd_refs(family, rows, C, with_bias):
    """fp64 references and bounds of one forward case, shared by ln_fwd and add_ln_fwd."""
    x, _ = R.ln_case(family, rows, C)
    w, b = R.ln_params(C)
    b = b if with_bias else None
    mean, _, rstd = R.ln_stats_ref(x)
    return dict(mean=mean, rstd=rstd, y=R.ln_y_ref(x, w, b)[0], mean_bound=R.ln_mean_bound(x),
                rstd_bound=R.ln_rstd_rel_bound(x) * rstd, y_bound=R.ln_y_bound(x, w, b))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,C", R.LN_SHAPES)
def test_ln_fwd_and_add_ln_fwd_statistics_and_output(rows, C, family):
    x, _ = R.ln_case(family, rows, C)
    w, b = R.ln_params(C)
    h, r = R.ln_split_sum(x)  # bf16(h + r) is the family's row, bit for bit
    xg, wg, hg, rg = x.cuda(), w.cuda(), h.cuda(), r.cuda()
    for with_bias in (True, False):
        ref = _fwd_refs(family, rows, C, with_bias)
        bg = b.cuda() if with_bias else None
        s, *added = _ext().add_ln_fwd(hg, rg, wg, bg, R.LN_EPS)
        assert torch.equal(s.cpu().view(torch.int16), x.view(torch.int16))
        for name, (y, mean, rstd) in (("ln_fwd", _ext().ln_fwd(xg, wg, bg, R.LN_EPS)),
                                      ("add_ln_fwd", added)):
            tag = f"{name} {family} {rows}x{C} bias={with_bias}"
            assert mean.dtype == torch.float32 and rstd.dtype == torch.float32
            assert _ratio(f"{tag} mean", mean, ref["mean"], ref["mean_bound"]) <= 1.0
            assert _ratio(f"{tag} rstd", rstd, ref["rstd"], ref["rstd_bound"]) <= 1.0
            assert _ratio(f"{tag} y", y, ref["y"], ref["y_bound"]) <= 1.0


@pytest.mark.parametrize("rows,C", R.LN_SHAPES)
def test_constant_rows_give_the_bias_back(rows, C):
    x, _ = R.ln_case("constant", rows, C)
    w, b = R.ln_params(C)
    want_rstd = torch.full((rows,), float(R.f32(R.LN_EPS)), dtype=torch.float64).rsqrt()
    for bias in (b, None):
        y, mean, rstd = _ext().ln_fwd(x.cuda(), w.cuda(), None if bias is None else bias.cuda(),
                                      R.LN_EPS)
        want = (b if bias is not None else torch.zeros_like(b)).expand(rows, C).contiguous()
        assert torch.equal(y.cpu().view(torch.int16), want.view(torch.int16))  # +0 without bias
        assert torch.equal(mean.cpu(), torch.full((rows,), 64.0))
        assert _ratio(f"constant {rows}x{C} rstd", rstd, want_rstd,
                      R.ln_rstd_rel_bound(x) * want_rstd) <= 1.0


def _planted(rows):
    """A mean and rstd that belong to no row: ln_bwd has to use what it is handed."""
    return (torch.linspace(-0.5, 0.5, rows, dtype=torch.float32),
            torch.linspace(0.5, 2.0, rows, dtype=torch.float32))


@pytest.mark.parametrize("planted", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("rows,C", R.LN_SHAPES)
def test_ln_bwd_against_the_statistics_it_was_given(rows, C, family, planted):
    # the Python-side copy of the launcher's block count, against the table
    nblocks = R.LN_SHAPE_BLOCKS[rows]
    assert R.reduction_blocks(rows, R.LN_WPB) == nblocks
    x, dy = R.ln_case(family, rows, C)
    w, b = R.ln_params(C)
    xg, dyg, wg = x.cuda(), dy.cuda(), w.cuda()
    if planted:
        mean, rstd = _planted(rows)
        meang, rstdg = mean.cuda(), rstd.cuda()
    else:
        _, meang, rstdg = _ext().ln_fwd(xg, wg, b.cuda(), R.LN_EPS)
        mean, rstd = meang.cpu(), rstdg.cpu()
    tag = f"ln_bwd {family} {rows}x{C} planted={planted}"
    dx_ref = R.ln_dx_ref(dy, x, w, mean, rstd)
    dx_bound = R.ln_dx_bound(dy, x, w, mean, rstd)
    dx_only, none_w, none_b = _ext().ln_bwd(dyg, xg, wg, meang, rstdg, False)
    assert none_w is None and none_b is None
    assert _ratio(f"{tag} dx (dx only)", dx_only, dx_ref, dx_bound) <= 1.0
    dx, dw, db = _ext().ln_bwd(dyg, xg, wg, meang, rstdg, True)
    assert _ratio(f"{tag} dx (fused)", dx, dx_ref, dx_bound) <= 1.0
    xh = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    dw_ref, db_ref = R.ln_dwdb_ref(dy, x, mean, rstd)
    assert dw.shape == (C,) and db.shape == (C,) and dw.dtype == torch.bfloat16
    assert _ratio(f"{tag} dw", dw, dw_ref, R.ln_dwdb_bound(dy.double() * xh, nblocks)) <= 1.0
    assert _ratio(f"{tag} db", db, db_ref, R.ln_dwdb_bound(dy.double(), nblocks)) <= 1.0


EXACT_CASES = [(rows, C) for rows in R.LN_EXACT_ROWS for C in R.LN_EXACT_C]
_OWN_EXACT = {}  # (rows, C) -> this process's result, made once


def _digest(t):
    return hashlib.sha256(t.contiguous().view(torch.int16).numpy().tobytes()).hexdigest()


def _run_exact(rows, C):
    """The exact case on this process's kernels: {has_ds: (dw == want, db == want,
    digest of dx's bits)}."""
    dy, x, ds, w, dw, db = R.ln_exact_case(rows, C)
    dyg, xg, wg = dy.cuda(), x.cuda(), w.cuda()
    mean = torch.zeros(rows, device="cuda")
    rstd = torch.ones(rows, device="cuda")
    out = {}
    for has_ds in (False, True):
        dx, got_w, got_b = _ext().ln_bwd(dyg, xg, wg, mean, rstd, True,
                                         ds.cuda() if has_ds else None)
        out[has_ds] = (torch.equal(got_w.cpu(), dw), torch.equal(got_b.cpu(), db),
                       _digest(dx.cpu()))
    return out


def _own_exact(rows, C):
    if (rows, C) not in _OWN_EXACT:
        _OWN_EXACT[(rows, C)] = _run_exact(rows, C)
    return _OWN_EXACT[(rows, C)]


@pytest.mark.parametrize("rows,C", EXACT_CASES)
def test_ln_bwd_dwdb_exact_on_small_integers(rows, C):
    """mean = 0 and rstd = 1 planted, integer dy and x: no row lost, none read
    twice, in (no ds, PIPE), (ds, no PIPE) at C <= 1024 and (ds, PIPE) above."""
    # the Python-side copy of the launcher's block count, against the table
    assert R.reduction_blocks(rows, R.LN_WPB) == R.LN_EXACT_BLOCKS[rows]
    for has_ds, (dw_ok, db_ok, _) in _own_exact(rows, C).items():
        assert dw_ok and db_ok, (has_ds, dw_ok, db_ok)


def _lever_child(path):
    """Body of a forced-lever child process: every exact case, results as JSON."""
    out = {f"{rows}x{C}": {str(k): v for k, v in _run_exact(rows, C).items()}
           for rows, C in EXACT_CASES}
    with open(path, "w") as f:
        json.dump(out, f)


def test_ln_bwd_forced_pipe_levers_agree(tmp_path):
    """PERCEIVER_LN_BWD_PIPE is read once per process: one fresh child per value,
    one after the other, each running every exact case. 0 reaches (no ds, no
    PIPE) and (ds, no PIPE) above 1024 channels, 1 reaches (ds, PIPE) below.
    dw/db are exact in each and dx is bit-equal (by digest) across the two
    children and this process's own run."""
    here = os.path.dirname(os.path.abspath(__file__))
    runs = {}
    for lever in ("0", "1"):
        out = tmp_path / f"lever{lever}.json"
        env = dict(os.environ, PERCEIVER_LN_BWD_PIPE=lever)
        env["PYTHONPATH"] = os.pathsep.join(
            [os.path.dirname(here), here] + [p for p in [env.get("PYTHONPATH")] if p])
        done = subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=env,
                              capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
        with open(out) as f:
            runs[lever] = json.load(f)
    for rows, C in EXACT_CASES:
        own = _own_exact(rows, C)
        for has_ds in (False, True):
            for lever in ("0", "1"):
                dw_ok, db_ok, dx = runs[lever][f"{rows}x{C}"][str(has_ds)]
                assert dw_ok and db_ok, (rows, C, has_ds, lever, dw_ok, db_ok)
                assert dx == own[has_ds][2], (rows, C, has_ds, lever)


def test_ln_bwd_checks_its_arguments():
    """As ln_fwd does: none of these may reach a kernel."""
    ext = _ext()

    def args(C=64, rows=4, device="cuda", dtype=torch.bfloat16):
        t = torch.zeros(rows, C, dtype=dtype, device=device)
        stat = torch.zeros(rows, dtype=torch.float32, device=device)
        return t, torch.zeros(C, dtype=torch.bfloat16, device=device), stat

    t, w, stat = args(C=2056)  # a fifth chunk: columns >= 2048 would be ignored
    for needs_dwdb in (False, True):
        with pytest.raises(RuntimeError, match="2048"):
            ext.ln_bwd(t, t, w, stat, stat, needs_dwdb)
        with pytest.raises(RuntimeError, match="2048"):
            ext.ln_fwd(t, w, None, R.LN_EPS)
    t, w, stat = args()
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t.float(), t, w, stat, stat, True)      # fp32 dy
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t.float(), w, stat, stat, True)      # fp32 x
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t, w, stat.double(), stat, True)     # fp64 mean
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t, w, stat, stat[:3], True)          # rstd of another row count
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t.cpu(), t, w, stat, stat, True)        # CPU dy
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t, w, stat.cpu(), stat, True)        # CPU mean
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t, w, stat, stat, True, t.cpu())     # CPU ds
    with pytest.raises(RuntimeError):
        ext.ln_bwd(t, t, w, stat, stat, False, t.float())  # fp32 ds
    c, cw, cstat = args(device="cpu")
    with pytest.raises(RuntimeError):
        ext.ln_bwd(c, c, cw, cstat, cstat, True)
    with pytest.raises(RuntimeError):
        ext.ln_fwd(c, cw, None, R.LN_EPS)


if __name__ == "__main__":
    _lever_child(sys.argv[1])
