"""The fused decoder stage (csrc/fused_stage.hip: fused_up_conv_kernel in its seven base instantiations, up-sampling and flat,
fp32 / bf16 / split arithmetic) against fp64, element by element, called through hip.fused_up_conv: interior tiles (the loads
without edge predication of up2_load_interior, float and bf16), non-square maps, both regimes of the XCD-aware tile permutation,
per-sample strides of both noise maps, every skip kind, the chained GEMM in its exchange and split-K forms, the uint8 image.
Reference: models/model_v3.py:418-482,592-637, op/upfirdn2d.py.

Cases, the reference and the per-element bounds (with their derivation) are in tests/_fused_stage_cases.py;
test_fused_stage_cases_host.py shows on the CPU that every bound admits a correct fp32 / bf16 / split implementation and rejects
every mutant.  No tolerance here is a constant.  Every call is made twice, the first call's outputs overwritten with 1e30 and freed
in between, and the second call's outputs equal the first's bit for bit.  out2, rgb and y_next are handed in through `out=` as views
into larger buffers of sentinels: the floats in front of and behind each tensor stay untouched.  rgb and y_next are checked twice:
against fp64 of the whole stage, and against fp64 ToRGB / Wn of the out2 the same launch stored (their own arithmetic alone); a
launch that does not store out2 is first shown to give the rgb and y_next bits of the same launch with the store.

Tile-order independence: for each of the seven instantiations a window of low-resolution rows of a taller case, noise and skip windows
matched, runs in the OTHER tile order (and as other tiles: interior rows of the tall case are edge rows of the window); the output
rows whose FIR taps lie inside the window are the tall case's rows bit for bit, in fp32, bf16 and the unranged split mode (with range
tracking the exponents depend on the whole map's maximum).  The flat forms have no window with a halo to match and take their tile
origins from the same lines; they are held to fp64 in both orders.

Largest |hip - fp64| / bound per output and mode, measured on an MI355X over all cases, scales (the scales agree to the digits
printed: the bounds scale with the data), ranged and unranged split runs, and the case it was seen at (ids of FC.CASES):
    out2     fp32   0.11     C32u-B1-H4-W96-nss-fir;             down to 0.019 at C256u-B1-H2-W32-ns0-none
             bf16   0.49     C32u-B1-H2-W32-n00-none;            down to 0.16 at C256c-flat-B1-H8-W128-nss-plain.  The bound charges
                             half an ulp at the bottom of a binade, 2^-8, on both operands; over a binade the average is 0.7 of that.
             split  0.029    C32u-B2-H8-W96-nps-plain-noout2;    down to 0.0036 at C256u-B1-H2-W32-ns0-none (a chain of 3 C terms
                             charged in full against a matrix instruction's own tree, as in test_gpu_gemm1x1.py)
    rgb      fp32   0.015    bf16 0.086   split 0.0072   at C32u-B2-H8-W96-nps-plain-noout2;
                             down to 0.00038 / 0.0073 / 0.000088 at C256u-B1-H2-W32-ns0-none
    y_next   fp32   0.0093   split 0.0019   at C64c-flat-B2-H8-W128-npp-plain;   bf16 0.060 at C64c-B1-H8-W96-n0s-plain;
                             down to 0.0012 / 0.014 / 0.00025 at C = 256 (C256c-B2-H2-W32-npp-plain, C256c-B2-H4-W64-nsp-norgb)
             Not a miscount: the first term of both bounds charges every channel's worst-case out2 error with one sign through a sum
             over C channels of mixed signs (out2's own errors are 0.004 to 0.5 of their bounds and average out as 1 / sqrt(C) on
             top).  Hence the second check, against the out2 the launch stored:
    rgb of the stored out2      fp32 0.26, bf16 0.26 at C32u-B2-H8-W96-nps-plain-noout2;   split 0.29 at C32u-B1-H2-W32-n00-none;
                                nothing below 0.029 (C256u-B1-H2-W32-ns0-none: eight wave rows charged, most sums far from worst)
    y_next of the stored out2   fp32 0.071 at C64c-B1-H8-W96-n0s-plain;   bf16 0.31 at C64c-flat-B2-H8-W128-npp-plain;   split 0.014 at
                                C64c-B2-H4-W96-npp-fir;   down to 0.018 / 0.16 / 0.0036 at C = 256
No ratio exceeds 1; none is below 1e-3 except, in their first check, rgb in fp32 at C = 256 and rgb and y_next in the split mode at
C = 128 and 256, settled by the second.
split bound / fp32 bound (test_fused_stage_cases_host.py, medians over the elements of out2, rgb and y_next; the same for the three
outputs to 0.03), by C:    32: 2.3 to 2.65    64: 2.55 to 2.8    128: 2.75 to 2.9    256: 2.85 to 2.95     ((3 C + 20) / (C + 8) on
the contraction's share; the epilogue's and the FIR's share is the same in both modes, which is what pulls C = 32 down)
This file: 119 tests, 7.7 s on an MI355X.
"""
import pytest
import torch

from cips_3dplusplus_amd import _lib, hip

import _fused_stage_cases as FC
from test_gpu_gemm1x1 import GUARD, Guarded, cu, per_sample_max, twice, within

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
ALL = [(c, m) for m in FC.MODES for c in FC.CASES]
all_ids = [f"{m}-{c.id}" for c, m in ALL]
ids = lambda cases: [c.id for c in cases]      # noqa: E731


class StageOperands:
    """the device operands of one case: the matrices go through cips3d_modulate_weights (no demodulation, scale 1, styles of ones:
    exact) into the fragment layouts the kernel reads"""

    def __init__(self, case, t, mode, y_bf16=False):
        self.case, self.mode = case, mode
        B, C = case.B, case.C
        lib = _lib.load()
        ones = torch.ones(B, C, device=DEV)

        def mod(W, flags):
            Wd = cu(W)
            out = torch.empty(B * W.shape[0] * C, device=DEV)
            _lib.check(lib.cips3d_modulate_weights(Wd.data_ptr(), ones.data_ptr(), C, out.data_ptr(), B, W.shape[0], C, 1, 1.0, flags,
                                                   hip.stream_ptr()), "cips3d_modulate_weights")
            torch.cuda.synchronize()
            return out

        s16 = hip.MOD_SPLIT16 if mode == "split" else 0
        self.wm2 = mod(t["W2"], hip.MOD_PACKED | s16)
        self.wmn = mod(t["Wn"], hip.MOD_PACKED | hip.MOD_CHAINED | s16) if case.chained else None
        self.wrgb = mod(t["Wrgb"], 0) if case.rgb else None
        self.y = cu(t["y"].to(torch.bfloat16)) if y_bf16 else cu(t["y"])
        self.fir = None if case.flat else cu(FC.FIR)
        self.n1, self.n2 = cu(t["n1"]), cu(t["n2"])
        self.nw1 = torch.tensor([FC.NW1], device=DEV) if self.n1 is not None else None
        self.nw2 = torch.tensor([FC.NW2], device=DEV) if self.n2 is not None else None
        self.b1, self.b2, self.brgb, self.skip = cu(t["b1"]), cu(t["b2"]), cu(t["brgb"]) if case.rgb else None, cu(t["skip"])

    def call(self, ranged=True, rgb_u8=False, want_out2=None):
        """(out2, rgb, y_next, the amax recorded for y_next), guards"""
        c = self.case
        want_out2 = c.want_out2 if want_out2 is None else want_out2
        shape = lambda ch: (c.B, ch, c.OH, c.OW)      # noqa: E731
        g2 = Guarded(*shape(c.C)) if want_out2 else None
        gr = Guarded(*shape(3)) if (c.rgb and not rgb_u8) else None
        gn = Guarded(*shape(c.C // 2), dtype=self.y.dtype) if c.chained else None
        gu = None
        if c.rgb and rgb_u8:                          # (a uint8 cannot hold Guarded's sentinel)
            n = c.B * 3 * c.OH * c.OW
            gu = torch.full((n + 2 * GUARD,), 77, device=DEV, dtype=torch.uint8)
        res = hip.fused_up_conv(self.y, self.fir, self.n1, self.nw1, self.b1, self.wm2, self.n2, self.nw2, self.b2, self.wrgb, self.brgb,
                                self.skip, skip_up=c.skip == "fir", want_out2=want_out2, bf16=self.mode == "bf16", wm_next=self.wmn,
                                split=self.mode == "split", ranged=ranged, flat=c.flat, rgb_u8=rgb_u8,
                                out=(g2.t if g2 else None, gu[GUARD:-GUARD].view(*shape(3)) if gu is not None else (gr.t if gr else None),
                                     gn.t if gn else None))
        out2, rgb, y_next = res[0], res[1], (res[2] if c.chained else None)
        assert (out2 is None) == (not want_out2) and (rgb is None) == (not c.rgb)
        if gu is not None:
            assert bool((gu[:GUARD] == 77).all()) and bool((gu[-GUARD:] == 77).all()), "a write outside the uint8 image"
        amax = None
        if self.mode == "split" and ranged and c.chained:
            amax = hip.amax_value(hip.amax_of(y_next, measure=False))
        return (out2, rgb, y_next, amax), tuple(g for g in (g2, gr, gn) if g is not None)


@pytest.mark.parametrize("case,mode", ALL, ids=all_ids)
def test_fused_stage_against_fp64(case, mode):
    for gs, ranged in FC.runs(mode):
        t = case.tensors(gs)
        exps = FC.replay_exps(case, t, ranged) if mode == "split" else None
        ref, e = FC.stage_bounds(case, t, mode, exps)
        ops = StageOperands(case, t, mode)
        what = f"fused {mode} {case.id} gs={gs} ranged={ranged}"
        out2, rgb, y_next, amax = twice(lambda: ops.call(ranged))[0]         # (the second call equals the first bit for bit)
        got = dict(out2=out2, rgb=rgb, y_next=y_next)
        for k, v in got.items():
            if v is not None:
                within(v, ref[k], e[k], f"{what} :{k}:")
        if out2 is None:
            # a launch that does not store out2: the same launch with the store gives the same rgb and y_next, bit for bit
            (out2, r2, y2, _), guards = ops.call(ranged, want_out2=True)
            torch.cuda.synchronize()
            assert all(g.intact() for g in guards)
            out2 = out2.cpu()
            within(out2, ref["out2"], e["out2"], f"{what} :out2:")
            for a, b in ((rgb, r2), (y_next, y2)):
                assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.cpu().view(torch.int32)), f"{what}: storing out2 changes the rest"
            del r2, y2, guards
        if rgb is not None or y_next is not None:
            # rgb and y_next alone: fp64 ToRGB / Wn of the out2 this launch stored, e(out2) = 0
            ref2, e2 = FC.stage_bounds(case, t, mode, exps, out2=out2)
            for k in ("rgb", "y_next"):
                if got[k] is not None:
                    within(got[k], ref2[k], e2[k], f"{what} :{k}-of-output:")
        if amax is not None:         # split, chained, measured (next_gain not set)
            assert torch.equal(amax, per_sample_max(y_next, case.B)), f"{what}: the recorded amax is not max |y_next| of the sample"


@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("pair", FC.ORDER_PAIRS, ids=[f"{p[0].id}-rows{p[1]}+{p[2]}" for p in FC.ORDER_PAIRS])
def test_the_tile_order_does_not_change_a_bit(pair, mode):
    tall, r, Hs = pair
    t = tall.tensors()
    short, s = tall.window(t, r, Hs)
    assert tall.regime()["swizzled"] != short.regime()["swizzled"]
    ot, os_ = StageOperands(tall, t, mode), StageOperands(short, s, mode)
    a, b = twice(lambda: ot.call(ranged=False))[0], twice(lambda: os_.call(ranged=False))[0]      # (guard bands checked in twice)
    n = 0
    for k, va, vb in zip(("out2", "rgb", "y_next"), a, b):
        if va is not None:
            wa, wb = va[:, :, 2 * r + 2:2 * (r + Hs) - 2].contiguous(), vb[:, :, 2:2 * Hs - 2].contiguous()
            assert bool(torch.isfinite(wa).all()) and wa.numel() > 0
            assert torch.equal(wa.view(torch.int32), wb.view(torch.int32)), f"{tall.id} {mode} {k}: the two tile orders differ"
            n += 1
    assert n >= 2


@pytest.mark.parametrize("case", FC.YB_CASES, ids=ids(FC.YB_CASES))
def test_bf16_storage_is_the_bf16_launch_on_the_same_values(case):
    """CIPS3D_Y_BF16 on non-square cases with interior tiles (up2_load_interior's bf16_t overload beside up2_load's): a
    torch.bfloat16 y_lo gives exactly the result of the bf16-operand launch on the fp32 copy of the same values, and the bf16
    y_next is the bf16 rounding of that launch's fp32 y_next, bit for bit."""
    rg = case.regime()
    assert rg["interior"] > 0 and rg["interior"] < rg["tiles"] and not rg["square"]
    t = case.tensors()
    t["y"] = t["y"].to(torch.bfloat16).float()
    out2, rgb, y32, _ = twice(StageOperands(case, t, "bf16").call)[0]
    ops16 = StageOperands(case, t, "bf16", y_bf16=True)
    assert ops16.y.dtype == torch.bfloat16
    for o2, r16, y16, _ in twice(ops16.call):
        assert torch.equal(o2, out2)
        if case.rgb:
            assert torch.equal(r16, rgb)
        if case.chained:
            assert y16.dtype == torch.bfloat16 and torch.equal(y16.view(torch.int16), y32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("mode", FC.MODES)
@pytest.mark.parametrize("case", FC.U8_CASES, ids=ids(FC.U8_CASES))
def test_uint8_image_is_rgb_to_uint8_of_the_fp32_image(case, mode):
    """CIPS3D_RGB_U8 through hip.fused_up_conv(rgb_u8=True), on interior, non-square cases whose image has values on both sides
    of +1 and of -1: the bytes of hip.rgb_to_uint8 on the fp32 image of the same launch without the flag."""
    rg = case.regime()
    assert rg["interior"] > 0 and not rg["square"]
    t = case.tensors()
    ops = StageOperands(case, t, mode)
    (out2, rgb, y_next, _), _g = ops.call()
    for lo, hi in ((-1e30, -1.0), (-1.0, 0.0), (0.0, 1.0), (1.0, 1e30)):
        assert bool(((rgb > lo) & (rgb < hi)).any())
    want = hip.rgb_to_uint8(rgb.contiguous()).cpu()
    assert int(want.min()) == 0 and int(want.max()) == 255 and want.unique().numel() > 100
    rest = [v.cpu() if v is not None else None for v in (out2, y_next)]
    for _ in range(2):                            # (twice() fills with 1e30, which a uint8 cannot hold)
        (o2, u8, yn, _), guards = ops.call(rgb_u8=True)
        torch.cuda.synchronize()
        assert all(g.intact() for g in guards), "a write outside an output tensor"
        assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), want)
        for v, w in zip((o2, yn), rest):          # the other outputs do not notice the flag
            assert (v is None and w is None) or torch.equal(v.cpu(), w)
        u8.fill_(3)
        del o2, u8, yn, guards


def test_what_the_stage_cannot_take_is_refused_before_any_launch():
    """beside test_flat_stage_refuses_what_it_does_not_tile (a flat H the tiles do not divide): the documented codes of
    include/cips3d_hip.h, CIPS3D_E_BADARG = -1, CIPS3D_E_UNSUPP = -2"""
    lib = _lib.load()
    st = hip.stream_ptr()
    SENT = -77.5
    out = torch.full((1 << 18,), SENT, device=DEV)
    a = torch.zeros(1 << 18, device=DEV)
    A, o = a.data_ptr(), out.data_ptr()
    o2, orgb, onext = o, o + 4 * (1 << 16), o + 4 * (1 << 17)

    def stage(C, H, W, flags, nxt=False, B=1):
        return lib.cips3d_fused_up_conv_next(A, A, None, 0, None, A, A, None, 0, None, A, o2, A, A, None, flags, orgb, A if nxt else None,
                                             onext if nxt else None, B, C, H, W, None, st)

    refused = {
        "W % 32": (stage(32, 2, 48, 0), -2), "H odd": (stage(32, 3, 32, 0), -2),
        "flat with skip_up": (stage(32, 4, 64, hip.STAGE_FLAT | 1), -1),
        "wm_next at C = 32": (stage(32, 2, 32, 0, nxt=True), -2),
        "Y_BF16 without GEMM_BF16": (stage(64, 2, 32, hip.Y_BF16), -1),
        "split | bf16": (stage(64, 2, 32, hip.GEMM_SPLIT | hip.GEMM_BF16), -1),
    }
    for what, (code, want) in refused.items():
        assert code == want, f"{what}: returned {code}, documented {want}"
        with pytest.raises(RuntimeError):
            hip.check(code, what)
    assert stage(32, 2, 32, 0, B=0) == 0              # B = 0 succeeds and launches nothing
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    with pytest.raises(RuntimeError, match="cips3d_fused_up_conv_next"):
        hip.fused_up_conv(z(1, 32, 2, 48), z(4, 4), None, None, z(32), z(32 * 32), None, None, z(32))
    with pytest.raises(RuntimeError, match="cips3d_fused_up_conv_next"):
        hip.fused_up_conv(z(1, 32, 3, 32), z(4, 4), None, None, z(32), z(32 * 32), None, None, z(32))
    with pytest.raises(RuntimeError, match="bf16"):
        hip.fused_up_conv(z(1, 64, 2, 32).to(torch.bfloat16), z(4, 4), None, None, z(64), z(64 * 64), None, None, z(64))
    with pytest.raises(RuntimeError, match="out2"):
        hip.fused_up_conv(z(1, 32, 2, 32), z(4, 4), None, None, z(32), z(32 * 32), None, None, z(32), out=(z(1, 32, 4, 32), None, None))
