"""The per-op decoder backward kernels (csrc/backward.hip: gemm_wgrad_kernel, act_bwd_kernel, sum_to_scalar_kernel,
noise_bwd_kernel, torgb_bwd_kernel, modulate_bwd_du / dw / ds_kernel, pack_kernel) against fp64, element by element, called
directly through hip.gemm_wgrad, hip.noise_bias_act_bwd, hip.torgb_bwd, hip.modulate_bwd and hip.pack_weights at the block and
chunk edges: more than one pixel chunk / 1024-pixel block, a last block with one live thread, ragged wave rows and columns,
channel counts that are no multiple of 32, every `need_*` combination and both memset layouts of the accumulators.
Reference: models/model_v3.py:267-278 (modulation), :327-341 and op/fused_act.py:20-84 (noise, bias, leaky ReLU), :469-482 (ToRGB).

Cases, references and the per-element bounds (with their derivation) are in tests/_decoder_bwd_cases.py;
test_decoder_bwd_cases_host.py shows on the CPU that every bound admits torch fp32 and rejects every mutant.  No tolerance of a
single-kernel test here is a constant.  Every call is made twice, the first call's outputs overwritten with 1e30 and freed in
between: the caching allocator hands the second call those blocks, so an accumulator that a memset misses is seen.

Largest |hip - fp64| / bound per kernel and output, measured on an MI355X over all cases, both gradient scales and both calls
(the two scales agree to the last digit printed almost everywhere: the bounds scale with the data), and the case it was seen at:
    gemm_wgrad          dwm     0.155   P = 4;  0.021 at P = 260, 0.018 at 512, 0.0061 at 1028, 0.0026 at 2144, 0.0011 at 4112:
                                        the worst case over all orders grows with P, the error of sixteen-pixel steps does not
    noise_bias_act_bwd  dx      0.997   one rounding against u |dx|: cannot be looser
                        dbias   0.231   HW = 4;  0.005 .. 0.032 at 1024 pixels and more
                        dnoise  0.488   (3, 5, 2052, per-sample);  0.26 at HW = 4
                        dnw     0.0187  (3, 5, 2052);  0.0076 at HW = 4, 0.0011 at (2, 33, 1028): every term of the sum over
                                        B C HW products is charged the whole tree, and the sentinel products (2^12 fp32(sqrt 2),
                                        most of the sum of absolute terms) are exact
    torgb_bwd           dx      0.889   dwm  0.211 (HW = 4), 0.15 .. 0.18 at two and three blocks    dbias  0.481 (HW = 4)
    modulate_bwd        dW      0.443   (3, 3, 40, 1, no demodulation);  0.145 .. 0.216 with demodulation
                        ds      0.115   the same case;  0.0082 .. 0.034 with demodulation (the errors of du are charged with one
                                        sign through a sum over Cout ksq terms of mixed signs)
    pack_weights        plain: bit for bit;  split: |hi + lo - 2^8 w| <= 6.8e-8 of 2^8 max|w| (bar 2^-21 = 4.8e-7)
No ratio is near 1 except the single rounding of dx, none of a small case is below 1e-3.
The module-level tests at the end run StyledConv and ToRGB at H != W with the bars of test_gpu_backward.py."""
import pytest
import torch

from cips_3dplusplus_amd import autograd as AG
from cips_3dplusplus_amd import _lib, hip
from oracle import path as O

import _decoder_bwd_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
SENTINEL = -77.25
ids = lambda cases: [c.id for c in cases]      # noqa: E731


def cu(t):
    return t.to(DEV).contiguous() if t is not None else None


def within(got, ref, bound, what):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    ratio, at = BC.worst(err, bound)
    print(f"{what}: worst |hip - fp64| / bound = {ratio:.3g}")
    assert bool((err <= bound).all()), (f"{what}: |hip - fp64| is {ratio:.3g} x its bound at flat element {at} "
                                        f"(hip {float(got.reshape(-1)[at])!r}, fp64 {float(ref.reshape(-1)[at])!r})")


def twice(call):
    """[outputs of the first call, outputs of the second] on the CPU; the first call's device outputs are overwritten with
    1e30 and freed before the second call allocates its own"""
    results = []
    for _ in range(2):
        out = call()
        torch.cuda.synchronize()
        results.append([None if o is None else o.detach().cpu().clone() for o in out])
        for o in out:
            if o is not None:
                o.fill_(1e30)
        torch.cuda.synchronize()
        del out
    return results


# ------------------------------------------------------------------------------------------------------------- gemm_wgrad
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.WGRAD_CASES, ids=ids(BC.WGRAD_CASES))
def test_gemm_wgrad_against_fp64(case, gs):
    t = case.tensors(gs)
    dy, x = cu(t["dy"]), cu(t["x"])
    ref, e = BC.wgrad_ref(t, F64), BC.wgrad_bound(t["dy"], t["x"])
    for i, (dwm,) in enumerate(twice(lambda: (hip.gemm_wgrad(dy, x),))):
        assert dwm.shape == (case.B, case.M, case.K)
        within(dwm, ref, e, f"gemm_wgrad {case.id} gs={gs} call {i}")


# ----------------------------------------------------------------------------------------------------- noise + bias + lrelu
def act_within(outs, ref, e, kw, has_noise, what):
    want = (True, has_noise and kw["need_dnoise"], has_noise and kw["need_dnw"], kw["need_db"])
    for k, name in enumerate(("dx", "dnoise", "dnw", "db")):
        assert (outs[k] is not None) == want[k], f"{what}: {name}"
        if want[k]:
            within(outs[k], ref[k], e[k], f"noise_bias_act_bwd {what} {name}")


@pytest.mark.parametrize("flags", BC.ACT_FLAGS, ids=[f[0] for f in BC.ACT_FLAGS])
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.ACT_CASES, ids=ids(BC.ACT_CASES))
def test_noise_bias_act_bwd_against_fp64(case, gs, flags):
    name, kw, has_noise = flags
    t = case.tensors(gs)
    dy, y = cu(t["dy"]), cu(t["y"])
    noise, nw = (cu(t["noise"]), torch.tensor([BC.NOISE_W], device=DEV)) if has_noise else (None, None)
    ref, e = BC.act_ref(t, F64, case.per_sample), BC.act_bounds(t, case.per_sample)
    for i, outs in enumerate(twice(lambda: hip.noise_bias_act_bwd(dy, y, noise, nw, **kw))):
        if outs[1] is not None:
            assert outs[1].shape == t["noise"].shape
        act_within(outs, ref, e, kw, has_noise, f"{case.id} gs={gs} {name} call {i}")


@pytest.mark.parametrize("gs", BC.SCALES)
def test_noise_bias_act_bwd_with_accumulators_that_are_not_adjacent(gs):
    """dbias and the per-channel scratch of dnoise_w both given, but apart: the two-memset path of cips3d_noise_bias_act_bwd
    (hip.noise_bias_act_bwd always lays them out back to back); both dirty before the call"""
    case = BC.ACT_CASES[1]
    t = case.tensors(gs)
    B, C, HW = case.B, case.C, case.HW
    dy, y, noise = cu(t["dy"]), cu(t["y"]), cu(t["noise"])
    nw = torch.tensor([BC.NOISE_W], device=DEV)
    dx = torch.empty_like(y)
    acc = torch.full((3 * C + 1,), 1e30, device=DEV)          # [dbias | C floats nobody owns | scratch | dnw]
    db, gap, scratch, dnw = acc[:C], acc[C:2 * C], acc[2 * C:3 * C], acc[3 * C:]
    gap.fill_(SENTINEL)
    assert scratch.data_ptr() != db.data_ptr() + 4 * C
    hip.check(_lib.load().cips3d_noise_bias_act_bwd(dy.data_ptr(), y.data_ptr(), noise.data_ptr(), 0, nw.data_ptr(), dx.data_ptr(),
                                                    None, dnw.data_ptr(), db.data_ptr(), scratch.data_ptr(), B, C, HW,
                                                    hip.stream_ptr()), "cips3d_noise_bias_act_bwd")
    ref, e = BC.act_ref(t, F64, False), BC.act_bounds(t, False)
    within(dx, ref[0], e[0], "dx")
    within(dnw, ref[2], e[2], "dnw")
    within(db, ref[3], e[3], "db")
    assert bool((gap == SENTINEL).all())


# --------------------------------------------------------------------------------------------------------------------- ToRGB
@pytest.mark.parametrize("need_db", [True, False])
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.RGB_CASES, ids=ids(BC.RGB_CASES))
def test_torgb_bwd_against_fp64(case, gs, need_db):
    t = case.tensors(gs)
    drgb, x, wm = cu(t["drgb"]), cu(t["x"]), cu(t["wm"])
    ref, e = BC.rgb_ref(t, F64), BC.rgb_bounds(t)
    for i, (dx, dwm, db) in enumerate(twice(lambda: hip.torgb_bwd(drgb, x, wm, need_db=need_db))):
        what = f"torgb_bwd {case.id} gs={gs} need_db={need_db} call {i}"
        within(dx, ref[0], e[0], what + " dx")
        within(dwm, ref[1], e[1], what + " dwm")
        assert (db is not None) == need_db
        if need_db:
            within(db, ref[2], e[2], what + " db")


@pytest.mark.parametrize("gs", BC.SCALES)
def test_torgb_bwd_with_a_bias_gradient_that_is_not_adjacent(gs):
    """dbias given, but not behind dwm: the two-memset path of cips3d_torgb_bwd with a bias; both dirty before the call"""
    case = BC.RGB_CASES[1]
    t = case.tensors(gs)
    B, C, HW = case.B, case.C, case.HW
    drgb, x, wm = cu(t["drgb"]), cu(t["x"]), cu(t["wm"])
    dx = torch.empty_like(x)
    acc = torch.full((B * 3 * C + 3 + 3,), 1e30, device=DEV)          # [dwm | 3 floats nobody owns | dbias]
    dwm, gap, db = acc[:B * 3 * C], acc[B * 3 * C:B * 3 * C + 3], acc[B * 3 * C + 3:]
    gap.fill_(SENTINEL)
    hip.check(_lib.load().cips3d_torgb_bwd(drgb.data_ptr(), x.data_ptr(), wm.data_ptr(), dx.data_ptr(), dwm.data_ptr(),
                                           db.data_ptr(), B, C, HW, hip.stream_ptr()), "cips3d_torgb_bwd")
    ref, e = BC.rgb_ref(t, F64), BC.rgb_bounds(t)
    within(dx, ref[0], e[0], "dx")
    within(dwm, ref[1], e[1], "dwm")
    within(db, ref[2], e[2], "db")
    assert bool((gap == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- modulation
@pytest.mark.parametrize("need_dW", [True, False])
@pytest.mark.parametrize("gs", BC.SCALES)
@pytest.mark.parametrize("case", BC.MOD_CASES, ids=ids(BC.MOD_CASES))
def test_modulate_bwd_against_fp64_autograd(case, gs, need_dW):
    t = case.tensors(gs)
    W, s, dwm = cu(t["W"]), cu(t["s"]), cu(t["dwm"])
    ref, e = BC.mod_grads(t, case, F64), BC.mod_bounds(t, case)

    def call():       # (dwm is consumed)
        return hip.modulate_bwd(dwm.clone(), W, s, case.Cout, case.Cin, case.ksq, case.scale, case.demod, need_dW=need_dW)

    for i, (dW, ds) in enumerate(twice(call)):
        what = f"modulate_bwd {case.id} gs={gs} need_dW={need_dW} call {i}"
        assert (dW is not None) == need_dW and ds.shape == (case.B, case.Cin)
        if need_dW:
            assert dW.shape == t["W"].shape
            within(dW, ref[0], e[0], what + " dW")
        within(ds, ref[1], e[1], what + " ds")
    assert torch.equal(dwm.cpu(), t["dwm"])


# ------------------------------------------------------------------------------------------------------------------- packing
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("B,M,K", BC.PACK_CASES)
def test_pack_weights_bit_for_bit(B, M, K, transpose):
    wm = BC.pack_input(B, M, K)
    packed = hip.pack_weights(cu(wm), transpose=transpose)
    assert packed.shape == (B * M * K,)
    want = wm.transpose(1, 2).contiguous() if transpose else wm
    got = BC.unpack(packed.cpu(), B, M, K, transpose).contiguous()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("B,M,K,transpose", BC.PACK_SPLIT_CASES)
def test_pack_weights_split_holds_hi_plus_lo(B, M, K, transpose):
    wm = BC.pack_input(B, M, K)
    packed = hip.pack_weights(cu(wm), transpose=transpose, split=True)
    want = wm.transpose(1, 2) if transpose else wm
    got = BC.unpack_split(packed.cpu(), B, M, K, transpose)
    err = float((got - want).abs().max())
    print(f"pack split {B}x{M}x{K} transpose={transpose}: max |hi + lo - 2^8 w| / 2^8 max|w| = {err / float(wm.abs().max()):.3g}")
    assert err <= 2.0 ** -21 * float(wm.abs().max())


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_shapes_the_kernels_cannot_take_are_refused_before_any_launch():
    """M or K no multiple of 32, a pixel count no multiple of 4, a packed contraction no multiple of 16: RuntimeError from `check`,
    and the output the library was given keeps every bit"""
    lib = _lib.load()
    z = lambda *s: torch.zeros(*s, device=DEV)                          # noqa: E731
    with pytest.raises(RuntimeError, match="cips3d_gemm_wgrad"):
        hip.gemm_wgrad(z(1, 48, 8), z(1, 32, 8))
    with pytest.raises(RuntimeError, match="cips3d_gemm_wgrad"):
        hip.gemm_wgrad(z(1, 32, 6), z(1, 32, 6))
    with pytest.raises(RuntimeError, match="cips3d_noise_bias_act_bwd"):
        hip.noise_bias_act_bwd(z(1, 2, 6), z(1, 2, 6), z(1, 1, 6), z(1))
    with pytest.raises(RuntimeError, match="cips3d_torgb_bwd"):
        hip.torgb_bwd(z(1, 3, 6), z(1, 2, 6), z(1, 3, 2))
    with pytest.raises(RuntimeError, match="cips3d_pack_weights"):
        hip.pack_weights(z(1, 32, 24))
    # the same calls on the library, over outputs filled with a sentinel
    out = torch.full((4096,), SENTINEL, device=DEV)
    o = out.data_ptr()
    st = hip.stream_ptr()
    a, b = z(4096), z(4096)
    codes = [lib.cips3d_gemm_wgrad(a.data_ptr(), b.data_ptr(), o, 1, 48, 32, 8, st),
             lib.cips3d_gemm_wgrad(a.data_ptr(), b.data_ptr(), o, 1, 32, 32, 6, st),
             lib.cips3d_noise_bias_act_bwd(a.data_ptr(), b.data_ptr(), None, 0, None, o, None, None, o + 4 * 1024, None, 1, 2, 6, st),
             lib.cips3d_torgb_bwd(a.data_ptr(), b.data_ptr(), b.data_ptr(), o, o + 4 * 1024, o + 4 * 2048, 1, 2, 6, st),
             lib.cips3d_pack_weights(a.data_ptr(), o, 1, 32, 24, 0, st)]
    for code in codes:
        assert code != 0
        with pytest.raises(RuntimeError):
            hip.check(code, "refused")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------- whole modules at H != W
def close(a, b, rel=2e-4, what=""):
    """the bar of test_gpu_backward.py"""
    a = a.detach().cpu().reshape(b.shape)
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-6, f"{what}: err {err:.3e} vs scale {scale:.3e}"


def leaf(t):
    return t.clone().requires_grad_(True)


@pytest.mark.parametrize("k,cin,cout,H,W,up,B,per_sample_noise", [
    (1, 32, 64, 4, 10, False, 2, False), (1, 64, 32, 6, 10, True, 2, True), (3, 32, 64, 4, 6, False, 2, False),
    (3, 64, 32, 6, 4, True, 2, False)])
def test_styled_conv_bwd_at_a_height_that_is_not_the_width(k, cin, cout, H, W, up, B, per_sample_noise):
    """AG.styled_conv (1 x 1 and 3 x 3, plain and up-sampling) at H != W against torch autograd through the CPU oracle: the
    nine shifted views of ConvKxKFn.backward, the pixel counts of gemm_wgrad and noise_bias_act_bwd with H and W apart"""
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(cin + cout + H + 10 * W + k)
    sc = dec.StyledConv(cin, cout, k, 64, upsample=up)
    sc.noise.weight.data.fill_(0.3)
    sc.activate.bias.data = torch.randn(cout) * 0.2
    sd = {"m." + n: leaf(v) if v.is_floating_point() and "kernel" not in n else v.clone() for n, v in sc.state_dict().items()}
    x, st = torch.randn(B, cin, H, W), torch.randn(B, 64)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    nz = torch.randn(B if per_sample_noise else 1, 1, Ho, Wo)
    dy = torch.randn(B, cout, Ho, Wo)
    xr, sr, nr = leaf(x), leaf(st), leaf(nz)
    ref = O.styled_conv(sd, "m", xr, sr, nr, upsample=up)
    assert ref.shape == dy.shape
    ref.backward(dy)
    sc = sc.to(DEV)
    xg, sg, ng = leaf(cu(x)), leaf(cu(st)), leaf(cu(nz))
    y = AG.styled_conv(sc, xg, sg, ng)
    close(y, ref.detach(), 3e-5, "y")
    y.backward(cu(dy))
    close(xg.grad, xr.grad, what="dx"); close(sg.grad, sr.grad, what="dstyle"); close(ng.grad, nr.grad, what="dnoise")
    for name, p in sc.named_parameters():
        if name == "bias":            # present in checkpoints, unused in forward (model_v3.py:440)
            assert p.grad is None
            continue
        close(p.grad, sd["m." + name].grad, what=name)


def test_to_rgb_bwd_with_an_odd_channel_count_at_a_height_that_is_not_the_width():
    import cips_3dplusplus_amd.decoder as dec
    torch.manual_seed(33)
    C, H, W, B = 33, 8, 12, 2
    tr = dec.ToRGB(C, 32, upsample=True)
    tr.bias.data = torch.randn(1, 3, 1, 1)
    sd = {"m." + k: leaf(v) if "kernel" not in k else v.clone() for k, v in tr.state_dict().items()}
    x, st = torch.randn(B, C, H, W), torch.randn(B, 32)
    skip = torch.randn(B, 3, H // 2, W // 2)
    dy = torch.randn(B, 3, H, W)
    xr, sr, kr = leaf(x), leaf(st), leaf(skip)
    ref = O.to_rgb(sd, "m", xr, sr, kr, upsample=True)
    ref.backward(dy)
    tr = tr.to(DEV)
    xg, sg, kg = leaf(cu(x)), leaf(cu(st)), leaf(cu(skip))
    y = AG.to_rgb(tr, xg, sg, kg)
    close(y, ref.detach(), 3e-5, "rgb")
    y.backward(cu(dy))
    close(xg.grad, xr.grad, what="dx"); close(sg.grad, sr.grad, what="dstyle"); close(kg.grad, kr.grad, what="dskip")
    for name, p in tr.named_parameters():
        close(p.grad, sd["m." + name].grad, what=name)
