"""What the launcher of the fused decoder stage hands its kernel instead of having every wave compute it (csrc/fused_stage.hip:
stage_geometry, exported as cips3d_fused_stage_geometry; host only, no GPU): for every shape the stage takes over a grid of sizes,
the shift or the reciprocal gives bid / tiles_x and bid % tiles_x for EVERY workgroup id of the launch, the XCD-aware permutation
of the linear id included, and the per-sample byte strides are the ones the kernel used to compute itself
(b * C * HWlo elements of y_lo, b * C * HWo of out2, b * (C / 2) * HWo of y_next, b * 3 * HWo of rgb, b * 3 * HWlo | HWo of skip).
The tile shapes are those of the launch table, replayed by tests/_fused_stage_cases.py.
"""
import ctypes as C

import numpy as np
import pytest

from cips_3dplusplus_amd import _lib, hip

import _fused_stage_cases as FC

HS = (2, 4, 6, 12, 36, 130)


def geometry(lib, Cc, chained, H, W, flags):
    g = _lib.StageGeom()
    rc = lib.cips3d_fused_stage_geometry(Cc, int(chained), H, W, flags, C.byref(g))
    return rc, g


def kernel_quotient(bid, g):
    """the kernel's arithmetic on a uint32 workgroup id, in uint64 numpy"""
    if g.tx_shift >= 0:
        return bid >> np.uint64(g.tx_shift)
    q = (bid * np.uint64(g.tx_rcp)) >> np.uint64(32)
    return q - (q * np.uint64(g.tiles_x) > bid).astype(np.uint64)


@pytest.mark.parametrize("flat", [False, True], ids=["up", "flat"])
@pytest.mark.parametrize("base", FC.BASE, ids=[f"C{c}{'c' if ch else 'u'}" for c, ch in FC.BASE])
def test_the_launcher_divides_every_workgroup_id_exactly(base, flat):
    lib = _lib.load()
    Cc, chained = base
    WM, WGM, WGN, RW, BK, _ = (FC.CHAINED if chained else FC.UNCHAINED)[Cc]
    TH, TW, up = RW * WGN, 64 // RW, 1 if flat else 2
    supported = lib.cips3d_fused_flat_conv_supported if flat else lib.cips3d_fused_up_conv_supported
    n = shifts = 0
    for H in HS:
        for W in range(64 if flat else 32, 4096 + 1, 64 if flat else 32):
            rc, g = geometry(lib, Cc, chained, H, W, hip.STAGE_FLAT if flat else 0)
            if not supported(Cc, H, W):
                assert rc == -2
                continue
            assert rc == 0
            OH, OW = up * H, up * W
            assert (g.tile_h, g.tile_w, g.threads) == (TH, TW, 64 * WGM * WGN) and (g.tiles_x, g.tiles_y) == (OW // TW, OH // TH)
            assert (g.HWlo, g.HWo) == (H * W, OH * OW)
            pow2 = g.tiles_x & (g.tiles_x - 1) == 0
            assert (g.tx_shift >= 0) == pow2 and (not pow2 or 1 << g.tx_shift == g.tiles_x)
            tiles = g.tiles_x * g.tiles_y
            lin = np.arange(tiles, dtype=np.uint64)
            bid = (lin & np.uint64(7)) * np.uint64(tiles >> 3) + (lin >> np.uint64(3)) if tiles % 8 == 0 else lin
            assert np.array_equal(np.sort(bid), lin)
            q = kernel_quotient(bid, g)
            assert np.array_equal(q, bid // np.uint64(g.tiles_x)) and np.array_equal(bid - q * np.uint64(g.tiles_x), bid % np.uint64(g.tiles_x))
            n += 1
            shifts += pow2
    assert n > 100 and 0 < shifts < n


def test_the_reciprocal_is_exact_for_every_32_bit_id():
    """tx_rcp = 2^32 / d + 1: the high word of bid * tx_rcp is the quotient or one more for every bid < 2^32, so the kernel's one
    correction is enough -- at the ends of the range and around every multiple near them, for the row lengths no shift takes"""
    for d in (3, 5, 6, 7, 9, 12, 48, 127, 129, 1023, 4097, 65535, (1 << 18) - 1, (1 << 19) - 3):
        g = _lib.StageGeom()
        g.tiles_x, g.tx_shift, g.tx_rcp = d, -1, (1 << 32) // d + 1
        top = (1 << 32) - 1
        ks = np.array([0, 1, 2, top // d - 1, top // d], dtype=np.uint64)
        bid = np.unique(np.clip(np.concatenate([ks * np.uint64(d) + np.uint64(o) for o in (0, 1, d - 1)] + [np.array([top], dtype=np.uint64)]), 0, top))
        assert np.array_equal(kernel_quotient(bid, g), bid // np.uint64(d)), d


@pytest.mark.parametrize("flags,es,rgb_es", [(0, 4, 4), (hip.GEMM_BF16 | hip.Y_BF16, 2, 4), (hip.RGB_U8 | hip.GEMM_SPLIT, 4, 1)])
def test_the_strides_are_the_ones_the_kernel_computed(flags, es, rgb_es):
    lib = _lib.load()
    for Cc, chained in FC.BASE:
        for flat, skip_up, H, W in ((False, 1, 6, 96), (False, 0, 512, 512), (True, 0, 8, 128), (True, 0, 256, 1024)):
            rc, g = geometry(lib, Cc, chained, H, W, flags | skip_up | (hip.STAGE_FLAT if flat else 0))
            assert rc == 0
            HWlo, HWo = H * W, H * W * (1 if flat else 4)
            assert (g.ylo_bs, g.out2_bs, g.ynext_bs) == (Cc * HWlo * es, Cc * HWo * 4, (Cc // 2) * HWo * es)
            assert (g.rgb_bs, g.skip_bs) == (3 * HWo * rgb_es, 3 * (HWlo if skip_up else HWo) * 4)


def test_what_the_stage_does_not_take_has_no_geometry():
    lib = _lib.load()
    assert geometry(lib, 32, True, 4, 64, 0)[0] == -2             # no chained form at C = 32
    assert geometry(lib, 48, False, 4, 64, 0)[0] == -2
    assert geometry(lib, 64, False, 4, 96, hip.STAGE_FLAT)[0] == -2
    assert lib.cips3d_fused_stage_geometry(64, 0, 4, 64, 0, None) == -1
