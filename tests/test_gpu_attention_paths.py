"""GPU tests of the flash attention split, mask, layout and masked-row paths.

Every case first asserts the route it exists for (forward kernel, and the
gridDim.z plan of the forward, dq and dkv launches) through the extension's
own flash_split_plan / flash_fwd_pipe_applicable, then compares the kernels
with the fp64 reference in tests/_attention_ref.py under the bound derived
there. test_attention_oracle.py shows on the CPU that this bound catches a
skipped tile, a skipped split and a mis-weighted merge at these shapes.
"""
import pytest
import torch

import _attention_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
DROP_P, DROP_SEED = 0.25, 20240607


def _ext():
    from perceiver_amd.ops import hip

    return hip.ext()


def _route(shape, causal):
    ext = _ext()
    return R.route(shape, causal, plan=ext.flash_split_plan, pipe=ext.flash_fwd_pipe_applicable)


def _dev(*ts):
    return tuple(None if t is None else t.to(DEV) for t in ts)


def _fwd(q, k, v, pad, causal, p=0.0, seed=0):
    return _ext().flash_fwd(q, k, v, pad, causal, p, seed)


def _bwd(dout, q, k, v, out, lse, pad, causal, p=0.0, seed=0):
    return _ext().flash_bwd(dout, q, k, v, out, lse, pad, causal, p, seed)


def _check_out(label, out, lse, want_out, want_lse, bound, live):
    """|out - want_out| <= bound elementwise, lse within LSE_TOL on the live rows."""
    out, lse = out.cpu(), lse.cpu()
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), label
    ratio = R.worst_ratio(out, want_out.cpu(), bound)
    live = live.expand_as(lse)
    lse_err = (lse.double() - want_lse.cpu().double())[live].abs().max().item()
    print(f"{label}: error/tol {ratio:.3f}, lse error {lse_err:.2e}")
    assert ratio <= 1.0, f"{label}: error is {ratio:.3f} of the bound"
    assert lse_err <= R.LSE_TOL, f"{label}: lse error {lse_err:.3e}"


def _check_grads(label, got, want):
    """The project criterion (max abs error / max |ref| < 5e-2), applied per
    (b, h) slice so one bad head cannot hide in another head's scale."""
    for g, w, name in zip(got, want, ("dq", "dk", "dv")):
        g, w = g.cpu().double(), w.cpu().double()
        assert torch.isfinite(g).all(), f"{label} {name} not finite"
        err = (g - w).abs().amax(dim=(-2, -1))
        rel = err / (w.abs().amax(dim=(-2, -1)) + 1e-6)
        print(f"{label} {name}: worst slice rel err {rel.max().item():.4f}")
        assert rel.max().item() < R.GRAD_REL, f"{label} {name} rel err per slice {rel.tolist()}"


# ---------------------------------------------------------------- forward

@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fwd_case_matches_reference(name):
    case = R.CASES[name]
    shape, causal = case["shape"], case["causal"]
    R.check_route(case, _route(shape, causal))
    q, k, v, pad, (out_ref, lse_ref, _, abs_pv) = R.case_data(name)
    qd, kd, vd, padd = _dev(q, k, v, pad)
    if name == "v3_decode_cache":
        # K/V are prefixes of a longer cache buffer; what lies past Lk is not
        # part of the problem and must never reach the result
        cap = 1024
        kbuf = torch.full((*k.shape[:2], cap, k.shape[-1]), float("nan"),
                          dtype=torch.bfloat16, device=DEV)
        vbuf = torch.full((*v.shape[:2], cap, v.shape[-1]), float("nan"),
                          dtype=torch.bfloat16, device=DEV)
        kbuf[:, :, :shape[3]] = kd
        vbuf[:, :, :shape[3]] = vd
        kd, vd = kbuf[:, :, :shape[3]], vbuf[:, :, :shape[3]]
        assert not kd.is_contiguous() and not vd.is_contiguous()
    out, lse = _fwd(qd, kd, vd, padd, causal)
    _check_out(name, out, lse, out_ref, lse_ref, R.tol(out_ref, abs_pv), R.live_rows(pad, shape))
    if name in R.DEAD_BATCH:
        # every key padded: uniform attention, the mean of V over all Lk keys
        b = R.DEAD_BATCH[name]
        mean_v = v[b].double().mean(dim=-2, keepdim=True).expand_as(out_ref[b])
        ratio = R.worst_ratio(out[b].cpu(), mean_v, R.tol(out_ref, abs_pv)[b])
        print(f"{name}: fully masked rows vs mean(V), error/tol {ratio:.3f}")
        assert ratio <= 1.0, ratio


# ---------------------------------------------------------------- backward

BWD_CASES = ["pipe_split_causal", "v3_split_pad", "dkv_qsplit_pad", "dead_unsplit", "dead_v3_split"]


@pytest.mark.parametrize("name", BWD_CASES)
def test_bwd_case_matches_autograd(name):
    case = R.CASES[name]
    shape, causal = case["shape"], case["causal"]
    R.check_route(case, _route(shape, causal))
    q, k, v, pad, _ = R.case_data(name)
    # fully masked rows get zero weight in the backward kernels (masked entries
    # have P = 0), where the reference spreads dout / Lk over every key: the
    # kernels equal the reference with those rows' dout zeroed (docs/kernels.md)
    dout, want = R.case_grads(name, zero_dead_dout=name in R.DEAD_BATCH)
    qd, kd, vd, padd, doutd = _dev(q, k, v, pad, dout)
    out, lse = _fwd(qd, kd, vd, padd, causal)
    got = _bwd(doutd, qd, kd, vd, out, lse, padd, causal)
    _check_grads(name, got, want)
    dq, dk, dv = got
    for b, lo, hi in case["pad"]:
        assert torch.count_nonzero(dk[b, :, lo:hi]) == 0, f"dk on padded keys of batch {b}"
        assert torch.count_nonzero(dv[b, :, lo:hi]) == 0, f"dv on padded keys of batch {b}"
    if name in R.DEAD_BATCH:
        b = R.DEAD_BATCH[name]
        for g, gname in zip(got, ("dq", "dk", "dv")):
            assert torch.count_nonzero(g[b]) == 0, f"{gname} of the fully masked batch element"


# ---------------------------------------------------------------- split vs unsplit

def _replicas_for_unsplit(shape, causal):
    """Smallest head count at which no launch of the problem is split."""
    for h in (128, 256, 512, 1024):
        rep = (1, h) + tuple(shape[2:])
        got = _route(rep, causal)
        if all(got[key][0] == 1 for key in ("fwd", "dq", "dkv")):
            return h
    raise AssertionError(f"no unsplit twin for {shape}")


@pytest.mark.parametrize("p", [0.0, DROP_P], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("name", ["v3_split_pad", "pipe_split_causal", "pipe_split_pad",
                                  "dkv_qsplit_pad"])
def test_split_matches_unsplit(name, p):
    """The same problem split over gridDim.z and, with the head axis
    replicated until the grid fills the chip, unsplit. Both runs have B = 1
    and the compared head is bh = 0 in both, so the counter-hash dropout mask
    is identical: this is where dropout x split is checked."""
    case = R.CASES[name]
    shape, causal = case["shape"], case["causal"]
    assert shape[1] == 1
    q, k, v, pad, (out_ref, lse_ref, _, abs_pv) = R.case_data(name)
    dout = R.make_dout(shape, seed=7)
    one = (1,) + tuple(shape[1:])
    split_route = _route(one, causal)
    for key, want in case["route"].items():  # B = 1 keeps every split of the case
        if key != "pipe" and want[0] > 1:
            assert split_route[key] == want, (key, split_route[key])
    heads = _replicas_for_unsplit(shape, causal)
    with_bwd = any(case["route"].get(key, (1,))[0] > 1 for key in ("dq", "dkv"))
    live = R.live_rows(pad, shape)

    for b in range(shape[0]):
        qd, kd, vd, doutd = _dev(q[b:b + 1], k[b:b + 1], v[b:b + 1], dout[b:b + 1])
        padd = None if pad is None else pad[b:b + 1].to(DEV)
        qr, kr, vr, doutr = (t.expand(1, heads, -1, -1).contiguous() for t in (qd, kd, vd, doutd))

        out_s, lse_s = _fwd(qd, kd, vd, padd, causal, p, DROP_SEED)
        out_u, lse_u = _fwd(qr, kr, vr, padd, causal, p, DROP_SEED)
        label = f"{name}[b={b}, p={p}]"
        # each run is within tol / 2 of the reference by derivation (tol carries
        # a factor 2 of margin), so two runs agree within tol; under dropout
        # each is within tol(p) of the same dropped result, so within 2 * tol(p)
        bound = R.tol(out_ref[b:b + 1], abs_pv[b:b + 1], p)
        _check_out(label + " split vs unsplit", out_s, lse_s, out_u[:, :1], lse_u[:, :1],
                   bound if p == 0.0 else 2.0 * bound, live[b:b + 1])
        if p == 0.0:
            _check_out(label + " unsplit vs reference", out_u[:, :1], lse_u[:, :1],
                       out_ref[b:b + 1], lse_ref[b:b + 1], bound, live[b:b + 1])
        if with_bwd:
            got = _bwd(doutd, qd, kd, vd, out_s, lse_s, padd, causal, p, DROP_SEED)
            want = _bwd(doutr, qr, kr, vr, out_u, lse_u, padd, causal, p, DROP_SEED)
            _check_grads(label, got, [w[:, :1] for w in want])


# ---------------------------------------------------------------- layouts

def _head_transposed(x):
    """x (B, H, N, D) as a head-transposed view of a (B, N, H*D) buffer, the
    way the attention modules split heads."""
    b, h, n, d = x.shape
    buf = x.transpose(1, 2).reshape(b, n, h * d).contiguous()
    return buf.view(b, n, h, d).transpose(1, 2)


@pytest.mark.parametrize("expand_q", [False, True], ids=["head_transposed", "expanded_q"])
def test_model_layouts_are_bit_equal_to_contiguous(expand_q):
    """Forward and backward with the layouts the model passes: q/k/v as
    head-transposed views, q optionally a batch-1 tensor expanded over the
    batch (stride 0), dout in merged-heads memory, the pad mask a stride-0
    expand. The kernels are deterministic and atomic-free and only addresses
    differ, so every result equals the contiguous run bit for bit."""
    shape, causal = (2, 2, 40, 330, 32, 160), False
    got = _route(shape, causal)
    assert not got["pipe"] and got["fwd"] == (2, 192) and got["dq"] == (2, 192), got
    q, k, v = R.make_qkv(shape, seed=31)
    if expand_q:
        q = q[:1]
    dout = R.make_dout(shape, seed=31)
    pad_row = torch.zeros(1, shape[3], dtype=torch.bool)
    pad_row[0, 100:260] = True
    qd, kd, vd, doutd, pad_row = _dev(q, k, v, dout, pad_row)

    ql, kl, vl = _head_transposed(qd), _head_transposed(kd), _head_transposed(vd)
    if expand_q:
        ql = ql.expand(shape[0], -1, -1, -1)
        assert ql.stride(0) == 0
    doutl = doutd.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    padl = pad_row.expand(shape[0], -1)
    assert padl.stride(0) == 0
    for t in (ql, kl, vl, doutl):
        assert not t.is_contiguous() and t.stride(3) == 1

    out_l, lse_l = _fwd(ql, kl, vl, padl, causal)
    grads_l = _bwd(doutl, ql, kl, vl, out_l, lse_l, padl, causal)
    qc, kc, vc, doutc, padc = (t.contiguous() for t in (ql, kl, vl, doutl, padl))
    out_c, lse_c = _fwd(qc, kc, vc, padc, causal)
    grads_c = _bwd(doutc, qc, kc, vc, out_c, lse_c, padc, causal)

    assert torch.equal(out_l, out_c) and torch.equal(lse_l, lse_c)
    # dq of the expanded q is compared per batch element, before any reduction
    for g_l, g_c, name in zip(grads_l, grads_c, ("dq", "dk", "dv")):
        assert g_l.shape == g_c.shape and torch.equal(g_l, g_c), name
    # and the contiguous twin is right
    out_ref, lse_ref, _, abs_pv = R.reference(qc.cpu(), kc.cpu(), vc.cpu(), padc.cpu(), causal)
    _check_out("layouts", out_c, lse_c, out_ref, lse_ref, R.tol(out_ref, abs_pv),
               R.live_rows(padc.cpu(), shape))


def test_decode_layout_is_bit_equal_to_contiguous():
    """Single-token decode as the graphed decoder runs it: q a head-transposed
    view, K/V head-transposed views of a cache buffer longer than Lk."""
    name = "v3_decode_cache"
    case = R.CASES[name]
    shape = case["shape"]
    R.check_route(case, _route(shape, False))
    q, k, v, pad, _ = R.case_data(name)
    qd, kd, vd, padd = _dev(q, k, v, pad)
    cap = 1024

    def cache_view(x):
        b, h, n, d = x.shape
        buf = torch.zeros(b, cap, h * d, dtype=x.dtype, device=DEV)
        buf[:, :n] = x.transpose(1, 2).reshape(b, n, h * d)
        return buf.view(b, cap, h, d).transpose(1, 2)[:, :, :n]

    ql, kl, vl = _head_transposed(qd), cache_view(kd), cache_view(vd)
    assert not kl.is_contiguous() and not vl.is_contiguous()
    out_l, lse_l = _fwd(ql, kl, vl, padd, False)
    out_c, lse_c = _fwd(qd.contiguous(), kd.contiguous(), vd.contiguous(), padd, False)
    assert torch.equal(out_l, out_c) and torch.equal(lse_l, lse_c)
