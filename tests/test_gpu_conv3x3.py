"""The LDS-tiled MFMA 3x3 ModulatedConv2d (csrc/conv3x3.hip; reference models/model_v3.py:264-314) against the oracle
(which the reference's own `mc_k3_*` fixtures pin, tests/test_oracle_golden.py): plain and up-sampling branches, ragged
tiles, fused StyledConv epilogue, tap-major weight packing, fallback for shapes the kernel does not tile.

Below those, the same kernels -- modconv3x3_kernel and modconv3x3_split_kernel as <WM = 1 | 2, UP = false | true>, the 3x3 fragment
layouts of cips3d_modulate_weights and the direct modconv_kxk_kernel -- against fp64, element by element, with no constant
tolerance.  Cases, the model-order reference (conv2d; conv_transpose2d + blur), the per-element bounds with their derivation and the
mutants are in tests/_conv3x3_cases.py; test_conv3x3_cases_host.py shows on the CPU that every bound admits a correct fp32
evaluation, the commuted form and the split emulation, and rejects every mutant.  Every launch is made twice and compared bit for
bit; outputs are views into a sentinel-filled buffer whose guard bands stay intact (test_gpu_gemm1x1.py's `twice`, `Guarded`, `within`).
The split kernel runs at three data scales with its range and once at gs = 1 through the raw entry point with a NULL range.

Largest |hip - fp64| / bound per kernel form and mode, measured on an MI355X over all cases, scales and both calls (the scales
agree to the digits printed), and the smallest over the cases:
    modconv3x3_kernel        plain WM1  0.024   (16, 48, H4, W64);   down to 0.0079 at Cin = 32
                             plain WM2  0.024   (16, 32, H4, W8);    down to 0.0015 at the Cin = 256 case
                             up    WM1  0.028 on the convolution (Cin = 16); 0.41 where a sample is all zero and the epilogue's
                                        own two roundings are all there is to see;  down to 0.011 at Cin = 32
                             up    WM2  0.029   (16, 32, H8, W64);   down to 0.0012 at the Cin = 256 case
    modconv3x3_split_kernel  plain WM1  0.0051  plain WM2  0.0039  up WM1  0.0054 (0.41 on the zero sample)  up WM2  0.0059
                             down to 0.0019 at Cin = 32, 0.00026 (plain) / 0.00029 (up) at the Cin = 256 case
    The two figures below 1e-3 belong to the one deep case, not to a small one, and are no miscount: the bound charges a chain of
    27 Cin + 8 = 6920 roundings in the worst case of every sign, the products of the halves are exact and the matrix instruction
    adds 32 of them at a time; the 1x1 GEMM's split mode measures 0.0029 at 3 K + 8 = 392 charged roundings (test_gpu_gemm1x1.py),
    6920 / 392 times fewer is 0.00016.  The fp32 kernel's ratios fall with Cin in the same way (0.024, 0.0079, 0.0015).  What a
    bound this far above the error still catches is shown mutant by mutant on the CPU; a lost cross product wl zh is caught only
    where the contraction is short (Cin = 16, a few pixels) -- the honest reach of a worst-case bound.
    modulate_weights, ksq = 9   fp32 fragments 0.93 without demodulation (two roundings against 2 u), 0.16 with, at Cin 9 = 1152;
                             split tap pairs 0.98 / 0.87;  the same with and without FLIP;  the tenth tap is zero
    modconv_kxk              k = 1: 0.23 (Cin = 8), 0.12 (Cin = 17);   k = 3: 0.036 / 0.014;   k = 5: 0.013 / 0.0043;  transpose2
                             the same to two digits (a chain of k^2 Cin charged in full where at most a quarter of the taps meet an
                             input pixel)
No ratio exceeds 1.
split bound / fp32 bound (test_conv3x3_cases_host.py, median at gs = 1 with a measured amax), by Cin:
    plain   16: 2.98   32: 2.99   48: 3.00   256: 3.00          ((27 Cin + 20) / (9 Cin + 8))
    up      16: 2.91   32: 2.95   48: 2.97   256: 3.00          (the term sum |w| e(Z) is the same in both modes)
This file: 104 tests, 1.9 s on an MI355X."""
import pytest
import torch

import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, hip, weights
from conftest import maxdiff
from oracle import path as O

import _conv3x3_cases as CC
from test_gpu_gemm1x1 import Guarded, amax_array, twice, within

pytestmark = pytest.mark.gpu
DEV = "cuda"


def cu(t):
    return t.to(DEV).contiguous()


def _dec():
    import cips_3dplusplus_amd.decoder as dec
    return dec


def _conv(cin, cout, up, demod, seed):
    dec = _dec()
    m = dec.ModulatedConv2d(cin, cout, 3, 32, demodulate=demod, upsample=up)
    sd = {k: weights.det_normal(f"c3.{seed}.{k}", v.shape, 1.0, seed) if v.is_floating_point() and "kernel" not in k else v
          for k, v in m.state_dict().items()}
    sd["modulation.bias"] = 1.0 + weights.det_uniform(f"c3.{seed}.mb", (cin,), 0.3, seed)
    m.load_state_dict(sd)
    return m, sd


def test_tap_major_packing_matches_plain_layout():
    """cips3d_modulate_weights(ksq = 9, PACKED [| FLIP]) holds exactly the values of the plain layout, fragment-ordered per tap."""
    B, Cin, Cout = 2, 32, 48
    m, _ = _conv(Cin, Cout, False, True, 1)
    m = m.to(DEV)
    style = cu(weights.det_normal("c3.style", (B, 32), 1.0, 1))
    plain = m.modulated_weight(style, packed=False).view(B, Cout, Cin, 9).cpu()
    for flip in (False, True):
        packed = m.modulated_weight(style, packed=True, flip=flip).view(B, 9, Cout // 16, Cin // 16, 64, 4).cpu()
        # packed[b][t'][ot][kq][lane = (q << 4) | o_lo][j] = plain[b][16 ot + o_lo][16 kq + 4 j + q][t],  t' = 8 - t if flip
        p = packed.view(B, 9, Cout // 16, Cin // 16, 4, 16, 4)                # b, t', ot, kq, q, o_lo, j
        un = p.permute(0, 2, 5, 3, 6, 4, 1).reshape(B, Cout, Cin, 9)          # b, ot, o_lo, kq, j, q, t'
        if flip:
            un = un.flip(-1)
        assert torch.equal(un, plain)


@pytest.mark.parametrize("cin,cout,H,W,up,B,demod", [
    (16, 16, 8, 8, False, 1, True), (32, 48, 12, 20, False, 2, True), (64, 32, 7, 68, False, 1, False),
    (128, 128, 32, 64, False, 1, True), (16, 32, 5, 6, True, 2, True), (64, 64, 16, 16, True, 1, True),
    (128, 64, 9, 40, True, 1, False), (32, 16, 64, 64, True, 1, True)])
def test_modconv3x3_vs_oracle(cin, cout, H, W, up, B, demod):
    m, sd = _conv(cin, cout, up, demod, cin + cout + H)
    x = weights.det_normal("c3.x", (B, cin, H, W), 1.0, H)
    style = weights.det_normal("c3.s", (B, 32), 1.0, W)
    sdp = {"m." + k: v for k, v in sd.items()}
    ref = O.modulated_conv2d(sdp, "m", x, style, demodulate=demod, upsample=up)
    m = m.to(DEV)
    assert m.tiled3x3(H, W)
    y = m(cu(x), cu(style))
    assert y.shape == ref.shape and y.is_contiguous()
    assert maxdiff(y.cpu(), ref) < 3e-5 * max(1.0, float(ref.abs().max())), (cin, cout, H, W, up)


def test_split_tap_pair_packing_matches_plain_layout():
    """cips3d_modulate_weights(ksq = 9, PACKED | SPLIT [| FLIP]): the tap-pair fragments of modconv3x3_split_kernel hold hi + lo of
    2^8 w of the plain layout -- lane quarter q = channels 8 (q & 1) .. + 7 of tap 2 pair + (q >> 1), zeros in the tenth tap."""
    B, Cin, Cout = 2, 32, 48
    m, _ = _conv(Cin, Cout, False, True, 1)
    m = m.to(DEV)
    style = cu(weights.det_normal("c3.style", (B, 32), 1.0, 1))
    plain = m.modulated_weight(style, packed=False).view(B, Cout, Cin, 9).cpu()
    for flip in (False, True):
        buf = m.modulated_weight(style, packed=True, flip=flip, split=True)
        n = B * 10 * Cout * Cin * 2                                    # fp16 elements written (five tap pairs)
        h = buf.view(torch.float16)[:n].view(B, 5, Cout // 16, Cin // 16, 2, 4, 16, 8).float().cpu()   # b, pair, ot, kq, plane, q, o_lo, j
        val = (h[:, :, :, :, 0] + h[:, :, :, :, 1]) / 256.0            # hi + lo of 2^8 w
        # q = 2 h + cg: tap = 2 pair + h, channel = 16 kq + 8 cg + j
        v = val.view(B, 5, Cout // 16, Cin // 16, 2, 2, 16, 8)         # b, pair, ot, kq, h, cg, o_lo, j
        w = v.permute(0, 2, 6, 3, 5, 7, 1, 4).reshape(B, Cout, Cin, 10)    # b, (ot, o_lo), (kq, cg, j), (pair, h) = tap
        assert float(w[..., 9].abs().max()) == 0.0
        got = w[..., :9].flip(-1) if flip else w[..., :9]
        assert maxdiff(got, plain) <= 2.0 ** -21 * float(plain.abs().max())


@pytest.mark.parametrize("cin,cout,H,W,up,B,demod,scale", [
    (16, 16, 8, 8, False, 1, True, 1.0), (32, 48, 12, 20, False, 2, True, 1e-6), (64, 32, 7, 68, False, 1, False, 3e4),
    (128, 128, 32, 64, False, 1, True, 1.0), (16, 32, 5, 6, True, 2, True, 1.0), (64, 64, 16, 16, True, 1, True, 1e5),
    (128, 64, 9, 40, True, 1, False, 1e-5), (32, 16, 64, 64, True, 1, True, 1.0), (512, 512, 16, 16, False, 1, True, 1.0)])
def test_modconv3x3_split_vs_oracle(cin, cout, H, W, up, B, demod, scale):
    """modconv3x3_split_kernel (three fp16 products per fp32 product on v_mfma_f32_16x16x32_f16, two taps per MFMA step) against
    the oracle at the fp32 kernel's bar, on data of any magnitude (the input is split under its measured maximum)."""
    m, sd = _conv(cin, cout, up, demod, cin + cout + H)
    x = weights.det_normal("c3.x", (B, cin, H, W), 1.0, H) * scale
    style = weights.det_normal("c3.s", (B, 32), 1.0, W)
    ref = O.modulated_conv2d({"m." + k: v for k, v in sd.items()}, "m", x, style, demodulate=demod, upsample=up)
    m = m.to(DEV)
    wm = m.modulated_weight(cu(style), packed=True, flip=up, split=True)
    y = hip.modconv3x3(cu(x), wm, cout, up=up, fir=m.blur.kernel if up else None, split=True)
    y32 = m(cu(x), cu(style))
    assert y.shape == ref.shape
    r = max(float(ref.abs().max()), 1e-30)
    assert maxdiff(y.cpu(), ref) < 3e-5 * r, (cin, cout, H, W, up, maxdiff(y.cpu(), ref) / r)
    assert maxdiff(y, y32) < 3e-5 * r


@pytest.mark.parametrize("up,per_sample_noise", [(False, False), (False, True), (True, False), (True, True)])
def test_styled_conv_k3_fused_epilogue_vs_oracle(up, per_sample_noise):
    dec = _dec()
    B, cin, cout, H, W = 2, 32, 64, 10, 12
    sc = dec.StyledConv(cin, cout, 3, 32, upsample=up)
    sd = {k: weights.det_normal(f"sc3.{k}", v.shape, 1.0, 4) if v.is_floating_point() and "kernel" not in k else v
          for k, v in sc.state_dict().items()}
    sd["noise.weight"] = torch.full((1,), 0.3)
    sd["activate.bias"] = weights.det_uniform("sc3.ab", (cout,), 0.3, 4)
    sc.load_state_dict(sd)
    x = weights.det_normal("sc3.x", (B, cin, H, W), 1.0, 5)
    style = weights.det_normal("sc3.s", (B, 32), 1.0, 6)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    nz = weights.det_normal("sc3.n", (B if per_sample_noise else 1, 1, Ho, Wo), 1.0, 7)
    ref = O.styled_conv({"s." + k: v for k, v in sd.items()}, "s", x, style, nz, upsample=up)
    sc = sc.to(DEV)
    assert sc.conv.tiled3x3(H, W)
    for split in (True, False):                 # the default arithmetic (split-fp16 products) and the fp32 matrix instruction
        sc.split = split
        y = sc(cu(x), cu(style), noise=cu(nz))
        assert y.shape == ref.shape and maxdiff(y.cpu(), ref) < 3e-5 * max(1.0, float(ref.abs().max())), split


def test_k3_generator_uses_the_tiled_kernel_and_matches_the_reference(golden):
    """The k = 3 tiny generator of the reference fixture: every StyledConv of its decoder is tiled by the MFMA kernel (so the
    golden comparison in test_gpu_parity.py::test_tiny_generator_golden[h32_d2_k3] exercises it), and shapes the kernel does
    not tile (the reference's Cin = 8 fixtures) still run on the direct kernel."""
    fx = golden("tiny_generator")
    cfg = configs.tiny_G_cfg(32, 2, 3)
    G = pkg.build_generator(cfg, DEV, state_dict=fx.sub("h32_d2_k3.sd."))
    dec = G.decoder
    res = 8
    for conv in [dec.conv1] + list(dec.convs):
        assert conv.conv.kernel_size == 3 and conv.conv.tiled3x3(res, res), conv
        if conv.conv.upsample:
            res *= 2
    assert not _dec().ModulatedConv2d(8, 12, 3, 16).tiled3x3(6, 6)
    assert hip.modconv3x3_supported(16, 16, 4, 4, False) and not hip.modconv3x3_supported(16, 16, 4, 6, False)
    assert hip.modconv3x3_supported(16, 16, 3, 6, True) and not hip.modconv3x3_supported(16, 24, 4, 4, False)


# ------------------------------------------------------------------------------------------------------------------------------
# Against fp64, element by element, under the derived bounds of tests/_conv3x3_cases.py (the module docstring has the table)
# ------------------------------------------------------------------------------------------------------------------------------
F64 = torch.float64
GC = CC.GC
ALL_CONV = [(c, m) for m in CC.MODES for c in CC.CASES]
WORST = {}                                        # kernel form and mode -> the largest |hip - fp64| / bound seen, printed as it grows


class ConvOperands:
    """the device tensors of one launch of a case: the weights come from cips3d_modulate_weights without demodulation, with scale
    1.0 and styles of ones -- the exact values of w in the fragment layout of the mode"""

    def __init__(self, case, t, mode, ranged):
        self.case, self.split, self.ranged = case, mode == "split", ranged
        B, Cin, Cout = case.B, case.Cin, case.Cout
        self.x = cu(t["x"])
        ones = torch.ones(B, Cin, device=DEV)
        self.wmp = hip.modulate_weights(cu(t["w"]).view(1, Cout, Cin, 3, 3), ones, Cin, B, Cout, Cin, 9, 1.0, False, True, flip=case.up,
                                        split=self.split)
        self.fir = cu(CC.FIR) if case.up else None
        ep = case.epilogue == 1
        self.noise = cu(t["noise"]).view(-1, 1, case.OH, case.OW) if (ep and t["noise"] is not None) else None
        self.nw = torch.tensor([CC.NOISE_W], device=DEV) if self.noise is not None else None
        self.bias = cu(t["bias"]) if ep else None
        self.x_amax = None
        if self.split and ranged:      # measured by the library's own pass, or a producer's upper bound
            self.x_amax = hip.absmax(self.x) if case.amax == "measured" else amax_array(case.amax_given(t))
            if case.amax == "measured":
                assert torch.equal(hip.amax_value(self.x_amax).cpu(), case.amax_given(t))

    def launch(self):
        c = self.case
        g = Guarded(c.B, c.Cout, c.OH, c.OW)
        if self.split and not self.ranged:      # the raw entry point with a NULL range: hip.modconv3x3 always measures one
            ptr = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
            nb = c.OH * c.OW if c.per_sample_noise else 0
            _lib.check(_lib.load().cips3d_modconv3x3(self.x.data_ptr(), self.wmp.data_ptr(), g.t.data_ptr(), c.B, c.Cin, c.Cout, c.H, c.W,
                                                     int(c.up), ptr(self.fir), c.epilogue | hip.GEMM_SPLIT, ptr(self.noise), nb,
                                                     ptr(self.nw), ptr(self.bias), None, hip.stream_ptr()), "cips3d_modconv3x3")
            return (g.t,), (g,)
        y = hip.modconv3x3(self.x, self.wmp, c.Cout, up=c.up, fir=self.fir, epilogue=c.epilogue, noise=self.noise, noise_w=self.nw,
                           bias=self.bias, split=self.split, x_amax=self.x_amax, out=g.t)
        assert y.data_ptr() == g.t.data_ptr()
        return (y,), (g,)


@pytest.mark.parametrize("case,mode", ALL_CONV, ids=[f"{m}-{c.id}" for c, m in ALL_CONV])
def test_modconv3x3_against_fp64(case, mode):
    """|hip - fp64| <= bound at every element, finite, twice bit for bit, guard bands intact; the split kernel and the fp32 kernel
    each to their own bound"""
    assert hip.modconv3x3_supported(case.Cin, case.Cout, case.H, case.W, case.up)
    for gs, ranged in CC.runs(mode):
        t = case.tensors(gs)
        exps = CC.replay_exps(case, t, ranged) if mode == "split" else None
        ref, e = CC.conv_bound(case, t, mode, exps)
        ops = ConvOperands(case, t, mode, ranged)
        form = f"modconv3x3 {mode} {'up' if case.up else 'plain'} WM{case.WM}"
        for i, (y,) in enumerate(twice(ops.launch)):
            within(y, ref, e, f"{form} | {case.id} gs={gs} ranged={ranged} call {i}")
            WORST[form] = max(WORST.get(form, 0.0), GC.worst((y.double() - ref).abs(), e)[0])
    print(f"{form}: worst ratio so far {WORST[form]:.3g}")


@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("case", CC.MOD3_CASES, ids=[c.id for c in CC.MOD3_CASES])
def test_modulate_weights_3x3_layouts_against_fp64(case, demod):
    """PACKED, PACKED | FLIP, PACKED | SPLIT, PACKED | SPLIT | FLIP of ksq = 9 un-packed and held to GC.mod_bound (+ rep(w) of the two
    fp16 halves) against the fp64 modulation -- not against the plain layout of the same kernel; the tenth tap is exactly zero"""
    t = case.tensors()
    W, s_buf = cu(t["W"]), cu(t["s_buf"])
    B, M, K = case.B, case.Cout, case.Cin
    ref, e = GC.mod_ref(case, t, F64, demod), GC.mod_bound(case, t, demod)
    for flip in (False, True):
        for split in (False, True):
            def call():
                n = B * M * K * (10 if split else 9)
                g = Guarded(n, fill=123.0)
                hip.modulate_weights(W, s_buf, case.s_stride, B, M, K, 9, case.scale, demod, True, s_offset=case.s_offset, out=g.t,
                                     flip=flip, split=split)
                return (g.t,), (g,)

            for i, (packed,) in enumerate(twice(call)):
                what = f"modulate 3x3 {'split' if split else 'fp32'}{' flip' if flip else ''} {case.id} demod={demod} call {i}"
                if split:
                    got, tenth = CC.unpack3x3_split(packed, B, M, K, flip)
                    assert bool((tenth == 0).all()), f"{what}: the tenth tap is not zero"
                    within(got, ref, e + 2.0 ** -22 * ref.abs() + 2.0 ** -33, what)
                else:
                    within(CC.unpack3x3(packed, B, M, K, flip), ref, e, what)


@pytest.mark.parametrize("gs", CC.SCALES)
@pytest.mark.parametrize("case", CC.KXK_CASES, ids=[c.id for c in CC.KXK_CASES])
def test_modconv_kxk_against_fp64(case, gs):
    """the direct kernel at shapes the MFMA kernel refuses: one fma chain of k^2 Cin terms"""
    assert case.k != 3 or not hip.modconv3x3_supported(case.Cin, case.Cout, case.H, case.W, case.transpose2)
    t = case.tensors(gs)
    x, w = cu(t["x"]), cu(t["w"])
    ref, e = CC.kxk_ref(case, t, F64), CC.kxk_bound(case, t)
    for i, (y,) in enumerate(twice(lambda: ((hip.modconv_kxk(x, w, case.Cout, case.k, transpose2=case.transpose2),), ()))):
        assert tuple(y.shape) == tuple(ref.shape)
        within(y, ref, e, f"modconv_kxk k{case.k}{' transpose2' if case.transpose2 else ''} | {case.id} gs={gs} call {i}")
