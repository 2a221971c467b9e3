"""The forward 1x1 GEMM (csrc/gemm1x1.hip: modconv1x1_kernel in its eight tile forms and three arithmetic modes, with the noise +
bias + leaky-ReLU epilogue, the ToRGB fold and the range tracking), torgb_reduce_kernel, up2_fir_act_kernel, noise_bias_act_kernel,
the four torgb kernels and the forward of modulate_kernel against fp64, element by element, called directly through hip.modconv1x1,
cips3d_modconv1x1_torgb + cips3d_torgb_reduce, hip.up2_fir_act, hip.noise_bias_act, hip.torgb and hip.modulate_weights: ragged last
pixel tiles of both tile widths, contractions shorter than the ring, every row-block size of the fold, per-sample strides, rows
longer than the modulation's register cache.
Reference: models/model_v3.py:218-341 (modulation, convolution, noise, activation), :418-482 (ToRGB), op/upfirdn2d.py.

Cases, references and the per-element bounds (with their derivation) are in tests/_gemm1x1_cases.py; test_gemm1x1_cases_host.py
shows on the CPU that every bound admits torch fp32 (and the bf16 / split emulations) and rejects every mutant.  No tolerance here is
a constant.  Every call is made twice, the first call's outputs overwritten with 1e30 and freed in between, and the second call's
outputs equal the first's bit for bit (nothing in these kernels is atomic except the amax, a maximum).  Outputs handed in through
`out=` are views into a larger buffer filled with a sentinel: the floats in front of and behind the tensor stay untouched.  The
fold's partial sums start as NaN; the row-block count the library returns equals Cout / BM of the Python replay of gemm_tile() --
the one observable that ties the replay to the library: the tile forms of launches without a fold are labelled by the replay alone.

Largest |hip - fp64| / bound per kernel, output and mode, measured on an MI355X over all cases, scales and both calls (the scales
agree to the last digit printed: the bounds scale with the data), and the case it was seen at; (B, Cin, Cout, HW) for the GEMM:
    modconv1x1 out   fp32   0.092   (1, 32, 256, 132) {1,2,2,32,4};   down to 0.018 at (1, 160, 64, 128)
                     bf16   0.050   the same case;                    down to 0.0064 at (1, 192, 64, 132)
                     split  0.021   the same case;                    down to 0.0029 at (1, 128, 128, 4)
                     The worst case over all orders grows with K, the error of a matrix instruction's own tree does not; the split
                     bound charges a chain of 3 K terms.  out_bf16: bit for bit in every mode.
    fold, against ToRGB of the fp64 output   fp32 0.0034   bf16 0.0023   split 0.00087   at (2, 64, 64, 124), one 64-row block;
                     down to 0.0006 / 0.0003 / 0.0001 at 224 to 256 rows.  Not a miscount: the first term of the bound charges every
                     row's worst-case GEMM error with one sign through a sum over Cout rows of mixed signs (the GEMM's own errors
                     are 0.02 to 0.09 of their bounds and average out as 1 / sqrt(Cout) on top).  Hence the second check:
    fold, against ToRGB of the stored output (the fold alone)   fp32 0.115 at (2, 128, 96, 252), three 32-row blocks;
                     bf16 0.109, split 0.097 at (2, 64, 64, 124);  nothing below 0.034
    on modulate_weights' fragments   fp32 0.054   bf16 0.019   split 0.012
    torgb_reduce     0.49    3 slots, 1 bias, skip;  exact (0) for one slot alone
    up2_fir_act      0.45    (2, 33, 5, 10) per-sample noise;  0.12 at (1, 1, 1, 2);   amax exact
    noise_bias_act   0.81    (3, 33, 1025) per-sample noise;  0.042 at the single pixel
    torgb            plain 0.24   split<4> 0.12   split<16> 0.057   scalar 0.056 (a chain of 33 charged in full)
    modulate         0.93 without demodulation (two roundings against 2 u: cannot be looser), 0.22 with, at (3, 3, 40, 1)
                     packed fp32 0.84;  split 0.74;  bf16 0.99 (half an ulp of bf16 is reached: the rounding IS the bound)
No ratio exceeds 1; none of a small case is below 1e-3 except the first fold check, settled above.
split bound / fp32 bound (test_gemm1x1_cases_host.py, median = max to three digits, the same at every scale), by K:
    32: 2.90   64: 2.95   96: 2.96   128: 2.97   160: 2.98   192: 2.98          ((3 K + 20) / (K + 8))
This file: 215 tests, 2.8 s on an MI355X.
"""
import ctypes as C

import pytest
import torch

from cips_3dplusplus_amd import _lib, hip

import _gemm1x1_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SENTINEL = -77.5                                  # (a bf16 number too)
GUARD = 256                                       # elements in front of and behind a guarded tensor (16-byte aligned)
ids = lambda cases: [c.id for c in cases]      # noqa: E731
ALL_GEMM = [(c, m) for m in GC.MODES for c in GC.cases_of(m)]
gemm_ids = [f"{m}-{c.id}" for c, m in ALL_GEMM]


def cu(t):
    return t.to(DEV).contiguous() if t is not None else None


def within(got, ref, bound, what):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err = (got - ref).abs()
    ratio, at = GC.worst(err, bound)
    print(f"{what}: worst |hip - fp64| / bound = {ratio:.3g}")
    assert bool((err <= bound).all()), (f"{what}: |hip - fp64| is {ratio:.3g} x its bound at flat element {at} "
                                        f"(hip {float(got.reshape(-1)[at])!r}, fp64 {float(ref.reshape(-1)[at])!r})")


class Guarded:
    """a tensor inside a buffer of sentinels"""

    def __init__(self, *shape, dtype=F32, fill=SENTINEL):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=dtype)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if fill != SENTINEL:
            self.t.fill_(fill)
        self.n = n

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


def twice(call):
    """[outputs of the first call, outputs of the second] on the CPU; call() returns (tensors, guards); the first call's device
    outputs are overwritten with 1e30 and freed before the second call allocates its own; every guard band is checked; the second
    call's outputs equal the first's bit for bit"""
    results = []
    for _ in range(2):
        out, guards = call()
        torch.cuda.synchronize()
        for g in guards:
            assert g.intact(), "a write outside the output tensor"
        results.append([None if o is None else o.detach().cpu().clone() for o in out])
        for g in guards:
            g.buf.fill_(1e30)
        for o in out:
            if o is not None:
                o.fill_(1e30)
        torch.cuda.synchronize()
        del out, guards
    for a, b in zip(*results):
        if a is not None:
            ai, bi = (v.view(torch.int16) if v.dtype == torch.bfloat16 else v.view(torch.int32) for v in (a, b))
            assert torch.equal(ai, bi), "the second call differs from the first"
    return results


def amax_array(values):
    """an amax array [B, AMAX_FLOATS] holding the given per-sample bounds"""
    a = torch.zeros(len(values), hip.amax_floats())
    a[:] = values.reshape(-1, 1).float()
    return cu(a)


def per_sample_max(y, B):
    return y.reshape(B, -1).abs().amax(1)


# --------------------------------------------------------------------------------------------------------------------- GEMM
class GemmOperands:
    def __init__(self, case, t, mode):
        self.case, self.mode = case, mode
        B, HW = case.B, case.HW
        self.x = cu(t["x"]).view(B, case.Cin, 1, HW)
        self.wmp = hip.pack_weights(cu(t["w"]), split=(mode == "split"))
        ep = case.epilogue == 1
        self.noise = cu(t["noise"]).view(-1, 1, 1, HW) if (ep and t["noise"] is not None) else None
        self.nw = torch.tensor([GC.NOISE_W], device=DEV) if self.noise is not None else None
        self.bias = cu(t["bias"]) if ep else None
        self.x_amax = None
        if mode == "split":      # measured by the library's own pass, or a caller's looser bound
            self.x_amax = hip.absmax(self.x) if case.amax == "measured" else amax_array(case.amax_given(t))
            if case.amax == "measured":
                assert torch.equal(hip.amax_value(self.x_amax).cpu(), case.amax_given(t))
        self.w_rgb, self.rgb_bias, self.skip = cu(t["w_rgb"]), cu(t["rgb_bias"]), cu(t["skip"])

    def plain(self, out_bf16=False, track=True):
        c = self.case
        g = Guarded(c.B, c.Cout, 1, c.HW, dtype=torch.bfloat16 if out_bf16 else F32)
        y = hip.modconv1x1(self.x, self.wmp, c.Cout, epilogue=c.epilogue, noise=self.noise, noise_w=self.nw, bias=self.bias, out=g.t,
                           bf16=self.mode == "bf16", out_bf16=out_bf16, split=self.mode == "split", x_amax=self.x_amax, track=track)
        amax = hip.amax_value(hip.amax_of(y, measure=False)) if (track and not out_bf16) else None
        return (y, amax), (g,)

    def folded(self):
        """the launch with the fold and the reduce behind it, as test_modconv1x1_torgb_fold_vs_oracle calls them:
        (y, amax, rgb, part), guards"""
        c = self.case
        lib = _lib.load()
        max_blocks = c.Cout // 32                                     # the smallest row block any tile has
        gy, gp, gr = Guarded(c.B, c.Cout, c.HW), Guarded(max_blocks, c.B, 3, c.HW, fill=float("nan")), Guarded(c.B, 3, c.HW)
        out_amax = hip.new_amax(c.B, DEV)
        rg, _keep = hip._range(x_amax=self.x_amax, out_amax=out_amax)
        flags = c.epilogue | {"fp32": 0, "bf16": hip.GEMM_BF16, "split": hip.GEMM_SPLIT}[self.mode]
        nblk = C.c_int(0)
        nb = c.HW if c.per_sample_noise else 0
        ptr = lambda v: v.data_ptr() if v is not None else None      # noqa: E731
        _lib.check(lib.cips3d_modconv1x1_torgb(self.x.data_ptr(), self.wmp.data_ptr(), gy.t.data_ptr(), c.B, c.Cin, c.Cout, c.HW, flags,
                                               ptr(self.noise), nb, ptr(self.nw), ptr(self.bias), self.w_rgb.data_ptr(), gp.t.data_ptr(),
                                               C.byref(nblk), C.byref(rg), hip.stream_ptr()), "cips3d_modconv1x1_torgb")
        assert nblk.value == c.Cout // c.BM, f"{nblk.value} row blocks, the replayed tile {c.tile} has {c.Cout // c.BM}"
        biases = (C.c_void_p * 1)(self.rgb_bias.data_ptr())
        _lib.check(lib.cips3d_torgb_reduce(gp.t.data_ptr(), nblk.value, biases, 1, self.skip.data_ptr(), gr.t.data_ptr(), c.B, c.HW,
                                           hip.stream_ptr()), "cips3d_torgb_reduce")
        assert bool(torch.isfinite(gp.t[:nblk.value]).all()), "a partial sum was not written"
        assert bool(torch.isnan(gp.t[nblk.value:]).all()), "a write behind the last row block"
        return (gy.t, hip.amax_value(out_amax), gr.t, gp.t[:nblk.value]), (gy, gp, gr)


@pytest.mark.parametrize("case,mode", ALL_GEMM, ids=gemm_ids)
def test_modconv1x1_against_fp64(case, mode):
    for gs in GC.scales_of(mode):
        t = case.tensors(gs)
        ops = GemmOperands(case, t, mode)
        amax = case.amax_given(t) if mode == "split" else None
        ref, e = GC.gemm_out_ref(case, t, F64, mode)[1], GC.gemm_out_bound(case, t, mode, amax)
        what = f"modconv1x1 {mode} {case.tile} {case.id} gs={gs}"
        if not case.fold:
            for i, (y, got_amax) in enumerate(twice(ops.plain)):
                within(y, ref, e, f"{what} out call {i}")
                assert torch.equal(got_amax, per_sample_max(y, case.B)), f"{what}: the recorded amax is not max |out|"
            continue
        f_ref, f_e = GC.fold_ref(case, t, F64, mode), GC.fold_bound(case, t, mode, amax)
        for i, (y, got_amax, rgb, part) in enumerate(twice(ops.folded)):
            within(y, ref, e, f"{what} out call {i}")
            assert torch.equal(got_amax, per_sample_max(y, case.B)), f"{what}: the recorded amax is not max |out|"
            within(rgb, f_ref, f_e, f"{what} fold call {i}")
            # the fold alone: ToRGB of the output this launch stored, e(y) = 0
            within(rgb, GC.fold_ref(case, t, F64, mode, y=y), GC.fold_bound(case, t, mode, y=y), f"{what} fold-of-output call {i}")


@pytest.mark.parametrize("mode", GC.MODES)
@pytest.mark.parametrize("case", GC.OUT_BF16_CASES, ids=ids(GC.OUT_BF16_CASES))
def test_modconv1x1_bf16_output_is_the_rounded_fp32_output(case, mode):
    """CIPS3D_Y_BF16 at ragged tiles, in every mode the C entry admits: the bits of the bf16 rounding of the fp32 result, the bar of
    test_gpu_bf16_storage.py::test_gemm_bf16_output_is_the_rounded_fp32_output"""
    t = case.tensors()
    ops = GemmOperands(case, t, mode)
    (y32, _), _g = ops.plain()
    for y16, _ in twice(lambda: ops.plain(out_bf16=True)):
        assert y16.dtype == torch.bfloat16 and torch.equal(y16.view(torch.int16), y32.cpu().to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("mode", GC.MODES)
def test_modconv1x1_on_weights_from_modulate_weights(mode):
    """the same launch on the fragments hip.modulate_weights(packed=True[, split=True]) writes: the modulation's bound pushed through
    the contraction is added.  bf16 mode: where the modulation's error reaches over a bf16 rounding boundary the weight may round
    the other way, and that step is what is charged."""
    B, Cin, Cout, HW, demod = GC.MODULATED_GEMM_CASE
    mc = GC.ModCase(B, Cout, Cin, 1)
    case = GC.GemmCase(B, Cin, Cout, HW, epilogue=0)
    for gs in GC.scales_of(mode):
        mt = mc.tensors()
        wm64, e_wm = GC.mod_ref(mc, mt, F64, demod), GC.mod_bound(mc, mt, demod)
        t = case.tensors(gs)
        t["w"] = wm64.float()
        amax = case.amax_given(t) if mode == "split" else None
        x64 = t["x"].double()
        if mode == "bf16":
            lo, hi = GC.bf16_round((wm64 - e_wm).float()).double(), GC.bf16_round((wm64 + e_wm).float()).double()
            ref, e_w = torch.bmm(GC.bf16_round(t["w"]).double(), GC.bf16_round(t["x"]).double()), (hi - lo).abs()
            e_x = GC.bf16_round(t["x"]).double().abs()
        else:
            ref, e_w, e_x = torch.bmm(wm64, x64), e_wm, x64.abs()
        e = GC.gemm_bound(t, mode, amax) + torch.bmm(e_w, e_x)
        W, s_buf, x = cu(mt["W"]), cu(mt["s_buf"]), cu(t["x"]).view(B, Cin, 1, HW)

        def call():
            wmp = hip.modulate_weights(W, s_buf, mc.s_stride, B, Cout, Cin, 1, mc.scale, demod, True, s_offset=mc.s_offset,
                                       split=(mode == "split"))
            g = Guarded(B, Cout, 1, HW)
            return (hip.modconv1x1(x, wmp, Cout, out=g.t, bf16=mode == "bf16", split=mode == "split"),), (g,)

        for i, (y,) in enumerate(twice(call)):
            within(y, ref, e, f"modconv1x1 modulated {mode} gs={gs} call {i}")


# -------------------------------------------------------------------------------------------------------------------- reduce
def reduce_call(t, B, HW, n_slots=None, n_bias=None):
    part, skip = cu(t["part"]), cu(t["skip"])
    bl = [cu(b) for b in t["biases"]]
    n_bias = len(bl) if n_bias is None else n_bias
    barr = (C.c_void_p * max(n_bias, 1))(*[b.data_ptr() for b in bl][:n_bias])
    g = Guarded(B, 3, HW)
    code = _lib.load().cips3d_torgb_reduce(part.data_ptr(), part.shape[0] if n_slots is None else n_slots, barr, n_bias,
                                           skip.data_ptr() if skip is not None else None, g.t.data_ptr(), B, HW, hip.stream_ptr())
    return code, g


@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.REDUCE_CASES, ids=ids(GC.REDUCE_CASES))
def test_torgb_reduce_against_fp64(case, gs):
    t = case.tensors(gs)
    ref, e = GC.reduce_ref(t, F64), GC.reduce_bound(t)

    def call():
        code, g = reduce_call(t, case.B, case.HW)
        _lib.check(code, "cips3d_torgb_reduce")
        return (g.t,), (g,)

    for i, (rgb,) in enumerate(twice(call)):
        within(rgb, ref, e, f"torgb_reduce {case.id} gs={gs} call {i}")


# --------------------------------------------------------------------------------------------------------- the per-op kernels
@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.UP_CASES, ids=ids(GC.UP_CASES))
def test_up2_fir_act_against_fp64(case, gs):
    t = case.tensors(gs)
    B, Cc, H, W = case.B, case.C, case.H, case.W
    y_lo, fir, bias = cu(t["y"]), cu(GC.FIR), cu(t["bias"])
    noise = cu(t["noise"]).view(-1, 1, 2 * H, 2 * W) if t["noise"] is not None else None
    nw = torch.tensor([GC.NOISE_W], device=DEV) if noise is not None else None
    ref, e = GC.up_ref(case, t, F64), GC.up_bound(case, t)

    def call():
        g = Guarded(B, Cc, 2 * H, 2 * W)
        out = hip.up2_fir_act(y_lo, fir, noise, nw, bias, out=g.t, track=True)
        return (out, hip.amax_value(hip.amax_of(out, measure=False))), (g,)

    for i, (out, amax) in enumerate(twice(call)):
        within(out, ref, e, f"up2_fir_act {case.id} gs={gs} call {i}")
        assert torch.equal(amax, per_sample_max(out, B)), "the recorded amax is not max |out| of the sample"
    (plain, _), _g = call()
    untracked = hip.up2_fir_act(y_lo, fir, noise, nw, bias)
    assert torch.equal(untracked, plain)


@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.NBA_CASES, ids=ids(GC.NBA_CASES))
def test_noise_bias_act_against_fp64(case, gs):
    t = case.tensors(gs)
    x, bias = cu(t["x"]).view(case.B, case.C, 1, case.HW), cu(t["bias"])
    noise = cu(t["noise"]).view(-1, 1, 1, case.HW) if t["noise"] is not None else None
    nw = torch.tensor([GC.NOISE_W], device=DEV) if noise is not None else None
    ref, e = GC.nba_ref(case, t, F64), GC.nba_bound(case, t)
    for i, (out,) in enumerate(twice(lambda: ((hip.noise_bias_act(x, noise, nw, bias),), ()))):
        within(out, ref, e, f"noise_bias_act {case.id} gs={gs} call {i}")


@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.RGB_CASES, ids=ids(GC.RGB_CASES))
def test_torgb_against_fp64(case, gs):
    t = case.tensors(gs)
    x, wm, bias, skip = cu(t["x"]).view(case.B, case.Cin, case.H, case.W), cu(t["wm"]), cu(t["bias"]), cu(t["skip"])
    fir = cu(GC.FIR) if case.skip == "fir" else None
    ref, e = GC.rgb_ref(case, t, F64), GC.rgb_bound(case, t)

    def call():
        g = Guarded(case.B, 3, case.H, case.W)
        return (hip.torgb(x, wm, bias, skip=skip, skip_up=case.skip == "fir", fir=fir, out=g.t),), (g,)

    for i, (rgb,) in enumerate(twice(call)):
        within(rgb, ref, e, f"torgb {case.regime()['arm']} {case.id} gs={gs} call {i}")


# ---------------------------------------------------------------------------------------------------------------- modulation
@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.MOD_CASES, ids=ids(GC.MOD_CASES))
def test_modulate_weights_against_fp64(case, gs, demod):
    t = case.tensors(gs)
    W, s_buf = cu(t["W"]), cu(t["s_buf"])
    ref, e = GC.mod_ref(case, t, F64, demod), GC.mod_bound(case, t, demod)

    def call():
        g = Guarded(case.B * case.Cout * case.Cin * case.ksq)
        return (hip.modulate_weights(W, s_buf, case.s_stride, case.B, case.Cout, case.Cin, case.ksq, case.scale, demod, False,
                                     s_offset=case.s_offset, out=g.t),), (g,)

    for i, (wm,) in enumerate(twice(call)):
        within(wm, ref, e, f"modulate {case.id} gs={gs} demod={demod} call {i}")


@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("case", GC.MOD_PACKED_CASES, ids=ids(GC.MOD_PACKED_CASES))
def test_modulate_weights_packed_layouts_against_fp64(case, demod):
    """the fp32 fragments hold the plain matrix's bound; the split fragments add the representation error of two fp16 halves, the
    bf16 fragments half an ulp of bf16, 2^-8 relative (both from the formats, _gemm1x1_cases.py)"""
    t = case.tensors()
    W, s_buf = cu(t["W"]), cu(t["s_buf"])
    B, M, K = case.B, case.Cout, case.Cin
    ref, e = GC.mod_ref(case, t, F64, demod), GC.mod_bound(case, t, demod)
    kw = dict(s_offset=case.s_offset)
    mw = lambda **k: hip.modulate_weights(W, s_buf, case.s_stride, B, M, K, 1, case.scale, demod, True, **kw, **k).cpu()   # noqa: E731
    within(GC.unpack(mw(), B, M, K, False), ref, e, f"modulate packed {case.id}")
    within(GC.unpack_split(mw(split=True), B, M, K, False), ref, e + 2.0 ** -22 * ref.abs() + 2.0 ** -33, f"modulate split {case.id}")
    within(GC.unpack_bf16(mw(bf16=True), B, M, K), ref, e + 2.0 ** -8 * (ref.abs() + e), f"modulate bf16 {case.id}")


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_shapes_and_flags_the_entry_points_cannot_take_are_refused_before_any_launch():
    lib = _lib.load()
    st = hip.stream_ptr()
    out = torch.full((1 << 16,), SENTINEL, device=DEV)
    a, b, c = (torch.zeros(1 << 16, device=DEV) for _ in range(3))
    o, A, Bp, Cp = out.data_ptr(), a.data_ptr(), b.data_ptr(), c.data_ptr()
    nblk = C.c_int(0)
    gemm = lambda Cin, Cout, HW, flags, bias=None, B=1: lib.cips3d_modconv1x1(A, Bp, o, B, Cin, Cout, HW, flags, None, 0, None, bias, None, st)   # noqa: E731
    fold = lambda flags, rgb_w, part: lib.cips3d_modconv1x1_torgb(A, Bp, o, 1, 32, 32, 8, flags, None, 0, None, None, rgb_w, part,   # noqa: E731
                                                                  C.byref(nblk), None, st)
    biases9 = (C.c_void_p * 9)(*[Cp] * 9)
    refused = {
        "gemm HW % 4": gemm(32, 32, 6, 0), "gemm Cin % 32": gemm(48, 32, 8, 0), "gemm Cout % 32": gemm(32, 48, 8, 0),
        "gemm bf16 | split": gemm(32, 32, 8, hip.GEMM_BF16 | hip.GEMM_SPLIT),
        "gemm out_bf16 with an epilogue": gemm(32, 32, 8, 1 | hip.Y_BF16, bias=Cp),
        "gemm out_bf16 with a fold": fold(hip.Y_BF16, Cp, o + 4 * 32768),
        "gemm rgb_w without rgb_part": fold(0, Cp, None), "gemm rgb_part without rgb_w": fold(0, None, o + 4 * 32768),
        "gemm epilogue 1 without a bias": gemm(32, 32, 8, 1),
        "up2_fir_act odd W": lib.cips3d_up2_fir_act(A, Bp, o, 1, 2, 2, 3, None, 0, None, Cp, None, st),
        "torgb skip_up odd H": lib.cips3d_torgb(A, Bp, Cp, Cp, 1, Cp, o, 1, 4, 3, 4, st),
        "torgb skip_up without a FIR": lib.cips3d_torgb(A, Bp, Cp, Cp, 1, None, o, 1, 4, 4, 4, st),
        "torgb_reduce HW % 4": lib.cips3d_torgb_reduce(A, 2, biases9, 1, None, o, 1, 6, st),
        "torgb_reduce too many biases": lib.cips3d_torgb_reduce(A, 2, biases9, GC.FOLD_MAX + 1, None, o, 1, 8, st),
        # a packed ksq = 1 layout indexes 16-channel k-groups: Cin = 24 used to be laid out scrambled
        "modulate packed Cin % 16": lib.cips3d_modulate_weights(A, Bp, 24, o, 1, 32, 24, 1, 0.5, hip.MOD_PACKED, st),
        "modulate packed | demodulate Cin % 16": lib.cips3d_modulate_weights(A, Bp, 40, o, 1, 32, 40, 1, 0.5, 3, st),
        "modulate packed split Cin % 32": lib.cips3d_modulate_weights(A, Bp, 48, o, 1, 32, 48, 1, 0.5, hip.MOD_PACKED | hip.MOD_SPLIT, st),
    }
    for what, code in refused.items():
        assert code != 0, f"{what}: accepted"
        with pytest.raises(RuntimeError):
            hip.check(code, what)
    # B = 0 succeeds and launches nothing
    empty = {
        "gemm": gemm(32, 32, 8, 0, B=0), "up2_fir_act": lib.cips3d_up2_fir_act(A, Bp, o, 0, 2, 2, 4, None, 0, None, Cp, None, st),
        "noise_bias_act": lib.cips3d_noise_bias_act(A, None, 0, None, Cp, o, 0, 2, 8, st),
        "torgb": lib.cips3d_torgb(A, Bp, Cp, None, 0, None, o, 0, 4, 4, 4, st),
        "torgb_reduce": lib.cips3d_torgb_reduce(A, 2, biases9, 1, None, o, 0, 8, st),
        "modulate": lib.cips3d_modulate_weights(A, Bp, 32, o, 0, 32, 32, 1, 0.5, 0, st),
    }
    for what, code in empty.items():
        assert code == 0, f"{what} with B = 0: {code}"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    # the wrappers raise
    z = lambda *s: torch.zeros(*s, device=DEV)      # noqa: E731
    with pytest.raises(RuntimeError, match="cips3d_modulate_weights"):
        hip.modulate_weights(z(1, 32, 24, 1, 1), z(1, 24), 24, 1, 32, 24, 1, 0.5, False, True)
    with pytest.raises(RuntimeError, match="cips3d_modconv1x1"):
        hip.modconv1x1(z(1, 32, 1, 6), z(32 * 32), 32)
    with pytest.raises(RuntimeError, match="cips3d_up2_fir_act"):
        hip.up2_fir_act(z(1, 2, 2, 3), z(4, 4), None, None, z(2))
    with pytest.raises(RuntimeError, match="cips3d_torgb"):
        hip.torgb(z(1, 4, 3, 4), z(1, 3, 4), z(3), skip=z(1, 3, 1, 2), skip_up=True, fir=z(4, 4))
    # an unpacked row of 24 channels is still modulated
    assert hip.modulate_weights(z(1, 32, 24, 1, 1), z(1, 24), 24, 1, 32, 24, 1, 0.5, True, False).shape == (32 * 24,)
