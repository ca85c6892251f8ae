"""CPU-side checks of the weight-gradient GEMM's host API: the shape gate and
the tile / M-split plan. The extension cross-compiles for gfx950 and imports
without a GPU, as in test_ext_host.py.
"""
import pytest

K_STEP = 64
NUM_CU = 256

# (M, N, K) of the MLM flagship's Linear weight gradients: dw is (N, K), the
# reduction runs over M = batch * latents (16384) or batch * seq (65536)
FLAGSHIP = [
    (16384, 1280, 1280), (16384, 1792, 1280), (16384, 256, 1280), (16384, 768, 1280),
    (65536, 1280, 768), (65536, 768, 768), (65536, 256, 768),
]
FLAGSHIP_NK = sorted({(n, k) for _, n, k in FLAGSHIP})


def _ext():
    from perceiver_amd.ops import hip

    try:
        return hip.ext()
    except ImportError:
        pytest.skip("in-tree extension not built")


def test_extension_exposes_wgrad_api():
    ext = _ext()
    for name in ["gemm_wgrad", "gemm_wgrad_applicable", "wgrad_plan"]:
        assert hasattr(ext, name), name


def test_gemm_wgrad_applicable_accepts_flagship_shapes():
    ext = _ext()
    for n, k in FLAGSHIP_NK:
        for m in (16384, 65536):
            assert ext.gemm_wgrad_applicable(m, n, k), (m, n, k)
    # smallest accepted problem: one K-step, one tile
    assert ext.gemm_wgrad_applicable(64, 256, 128)


def test_gemm_wgrad_applicable_rejects_one_case_per_rule():
    ext = _ext()
    assert not ext.gemm_wgrad_applicable(16384, 320, 1280)   # N not whole 256-row tiles
    assert not ext.gemm_wgrad_applicable(16384, 1280, 320)   # K not whole 128-column tiles
    assert not ext.gemm_wgrad_applicable(16384 + 32, 1280, 1280)  # M not whole K-steps
    assert not ext.gemm_wgrad_applicable(0, 1280, 1280)      # below the minimum M
    assert not ext.gemm_wgrad_applicable(32, 1280, 1280)     # below the minimum M


def _check_plan(ext, m, n, k):
    tile_n, tile_k, nsplit, rows = ext.wgrad_plan(m, n, k)
    case = (m, n, k, tile_n, tile_k, nsplit, rows)
    assert tile_n == 256 and tile_k in (128, 256), case
    assert n % tile_n == 0 and k % tile_k == 0, case
    assert nsplit >= 1, case
    assert rows > 0 and rows % K_STEP == 0, case
    assert nsplit * rows >= m, case
    assert (nsplit - 1) * rows < m, case  # no empty split
    return (n // tile_n) * (k // tile_k), nsplit


def test_wgrad_plan_invariants():
    ext = _ext()
    for m in (64, 192, 4096, 12288, 16384, 55296, 65536):
        for n, k in FLAGSHIP_NK + [(512, 512), (512, 2048), (2048, 512), (256, 128)]:
            assert ext.gemm_wgrad_applicable(m, n, k)
            _check_plan(ext, m, n, k)


def test_wgrad_plan_fills_the_chip_on_flagship_shapes():
    ext = _ext()
    for m, n, k in [(m, n, k) for n, k in FLAGSHIP_NK for m in (16384, 65536)]:
        tiles, nsplit = _check_plan(ext, m, n, k)
        blocks = tiles * nsplit
        rounds = -(-blocks // NUM_CU)
        assert blocks >= 0.9 * rounds * NUM_CU, (m, n, k, tiles, nsplit)
