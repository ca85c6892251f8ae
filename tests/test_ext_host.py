"""CPU-side checks of the in-tree HIP extension's host API.

The .so cross-compiles for gfx950 and imports without a GPU; these run in the
CPU gate and catch a stale/broken in-tree build before any GPU tier does.
"""
import pytest


def _ext():
    from perceiver_amd.ops import hip

    try:
        return hip.ext()
    except ImportError:
        pytest.skip("in-tree extension not built")


def test_extension_loads_and_exposes_api():
    ext = _ext()
    for name in ["flash_fwd", "flash_bwd", "flash_supported", "flash_split_plan",
                 "flash_fwd_pipe_applicable", "ln_fwd", "ln_bwd",
                 "adamw_step", "rotary_apply", "dropout_add_fwd", "dropout_add_bwd",
                 "colsum_bf16", "gemm_bt", "gemm_bt_gelu", "gemm_bt_applicable",
                 "transpose_bf16", "gelu_bias_fwd", "gelu_bias_bwd"]:
        assert hasattr(ext, name), name


def test_gemm_bt_applicability_host_rules():
    ext = _ext()
    # flagship projection shapes (fwd orientation)
    assert ext.gemm_bt_applicable(16384, 1280, 1280)
    assert ext.gemm_bt_applicable(16384, 1792, 1280)
    assert ext.gemm_bt_applicable(65536, 256, 768)
    # the BN=160 exact-fill family
    assert ext.gemm_bt_applicable(16384, 1280, 2816)
    assert ext.gemm_bt_applicable(512, 160, 192)
    # rejections: M tile, N tile, K tile, ring depth
    assert not ext.gemm_bt_applicable(100, 128, 192)
    assert not ext.gemm_bt_applicable(256, 100, 192)
    assert not ext.gemm_bt_applicable(256, 128, 100)
    assert not ext.gemm_bt_applicable(256, 128, 128)


def test_flash_supported_host_gate():
    ext = _ext()
    assert ext.flash_supported(32, 160, 0)
    assert ext.flash_supported(64, 64, 0)


@pytest.mark.parametrize("blocks,length,tile,expected", [
    (1, 4096, 64, (16, 256)),
    (1, 500, 64, (2, 256)),
    (8, 50176, 64, (32, 1600)),
    (1, 200, 32, (2, 128)),
    (1, 2048, 64, (8, 256)),
    (512, 4096, 64, (1, 4096)),
])
def test_flash_split_plan_pinned(blocks, length, tile, expected):
    assert tuple(_ext().flash_split_plan(blocks, length, tile)) == expected


def test_flash_split_plan_invariants():
    ext = _ext()
    for blocks in (1, 3, 64, 511, 512):
        for length in (1, 63, 256, 257, 500, 4096, 182528):
            for tile in (32, 64):
                nsplit, chunk = ext.flash_split_plan(blocks, length, tile)
                case = (blocks, length, tile, nsplit, chunk)
                assert 1 <= nsplit <= 32, case
                if nsplit > 1:
                    assert chunk % tile == 0, case
                assert nsplit * chunk >= length, case
                assert (nsplit - 1) * chunk < length, case  # no empty split
                if blocks >= 512 or length <= 4 * tile:
                    assert nsplit == 1, case


PIPE_TEMPLATES = [(32, 32), (32, 64), (32, 96), (32, 128), (32, 160),
                  (64, 64), (64, 128), (128, 128)]


def test_flash_fwd_pipe_applicable_template_list():
    ext = _ext()
    for d, dv in PIPE_TEMPLATES:
        assert ext.flash_fwd_pipe_applicable(d, dv, 128), (d, dv)
        assert not ext.flash_fwd_pipe_applicable(d, dv, 127), (d, dv)
    # exactly those eight: no other pair on the 16-channel grid up to 352 qualifies
    for d in range(16, 353, 16):
        for dv in range(16, 353, 16):
            assert ext.flash_fwd_pipe_applicable(d, dv, 128) == ((d, dv) in PIPE_TEMPLATES), (d, dv)
    for d, dv in [(48, 80), (32, 48), (128, 64), (261, 261)]:
        assert not ext.flash_fwd_pipe_applicable(d, dv, 128), (d, dv)
