"""The bounds and cases of tests/_gemm1x1_cases.py, checked without a GPU on every case test_gpu_gemm1x1.py runs, in every mode
and at every data scale: (a) the same expression evaluated by torch in fp32 on the CPU -- for the bf16 mode on the rounded
operands, for the split mode the emulation built from the header's definitions -- stays inside the bound against fp64: a correct
implementation passes; (b) every subtly wrong reference leaves it on at least one element: the GPU test has teeth, without
sentinels; (c) every case is in the regime it is listed for, and the list covers every (tile form, mode) with an epilogue and a
ragged last tile, every tile form with the fold, and every form with per-sample noise.  Prints the ratio of the split bound to the
fp32 bound per case (recorded in the docstring of test_gpu_gemm1x1.py, not asserted)."""
import pytest
import torch

import _gemm1x1_cases as GC

F32, F64 = torch.float32, torch.float64
ids = lambda cases: [c.id for c in cases]      # noqa: E731
ALL_GEMM = [(c, m) for m in GC.MODES for c in GC.cases_of(m)]
gemm_ids = [f"{m}-{c.id}" for c, m in ALL_GEMM]


def admits_and_rejects(what, ref, bound, fp32, mutants):
    """mutants: {name: tensor}"""
    assert ref.shape == bound.shape == fp32.shape, what
    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all()), what
    ratio, at = GC.worst((fp32.double() - ref).abs(), bound)
    assert GC.inside(fp32, ref, bound), f"{what}: the fp32 implementation is {ratio:.2f} x the bound at element {at}"
    for name, m in mutants.items():
        assert m.shape == ref.shape, (what, name)
        assert not GC.inside(m, ref, bound), f"{what}: the mutant `{name}` stays inside the bound"
    return ratio


def in_its_regime(case):
    got = case.regime()
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.id}: {k} is {got[k]}, the case is listed for {v}"


def correct_fp32(case, t, mode, amax):
    """(accumulator, stored output) of a correct implementation of `mode` in fp32 on the CPU"""
    if mode != "split":
        return GC.gemm_out_ref(case, t, F32, mode)
    v = GC.split_emulated(t, amax)
    return v, (GC.epilogue_ref(v, t, F32, case.per_sample_noise) if case.epilogue == 1 else v)


# ------------------------------------------------------------------------------------------------------------------- the GEMM
@pytest.mark.parametrize("case,mode", ALL_GEMM, ids=gemm_ids)
def test_gemm_bounds(case, mode):
    for gs in GC.scales_of(mode):
        t = case.tensors(gs)
        amax = case.amax_given(t) if mode == "split" else None
        what = f"{mode} {case.id} gs={gs}"
        v64, y64 = GC.gemm_out_ref(case, t, F64, mode)
        v32, y32 = correct_fp32(case, t, mode, amax)
        e_v, e_y = GC.gemm_bound(t, mode, amax), GC.gemm_out_bound(case, t, mode, amax)
        # the accumulator: the contraction's mutants without the epilogue in front of them
        admits_and_rejects(what + " acc", v64, e_v, v32, {m: GC.gemm_ref(t, F64, mode, m, case) for m in case.gemm_mutants()})
        muts = {m: GC.gemm_out_ref(case, t, F64, mode, m)[1] for m in case.gemm_mutants() + case.epilogue_mutants()}
        admits_and_rejects(what + " out", y64, e_y, y32, muts)
        if mode == "split":
            r = e_v / GC.gemm_bound(t, "fp32")
            print(f"split / fp32 bound {case.id} gs={gs}: median {float(r.median()):.3f} max {float(r.max()):.3f} "
                  f"((3 K + 20) / (K + 8) = {(3 * case.Cin + 20) / (case.Cin + 8):.3f})")
        if case.fold:
            f64 = GC.fold_ref(case, t, F64, mode)
            w32 = t["w_rgb"]
            f32_ = torch.bmm(w32, y32) + t["rgb_bias"][None, :, None] + t["skip"]
            admits_and_rejects(what + " fold", f64, GC.fold_bound(case, t, mode, amax), f32_,
                               {m: GC.fold_ref(case, t, F64, mode, m) for m in case.fold_mutants()})
            # the fold alone, given the output it folds
            admits_and_rejects(what + " fold of the output", GC.fold_ref(case, t, F64, mode, y=y32), GC.fold_bound(case, t, mode, y=y32),
                               f32_, {m: GC.fold_ref(case, t, F64, mode, m, y=y32) for m in case.fold_mutants()})


@pytest.mark.parametrize("case", GC.GEMM_CASES + GC.SPLIT_ONLY_CASES + GC.OUT_BF16_CASES,
                         ids=ids(GC.GEMM_CASES + GC.SPLIT_ONLY_CASES + GC.OUT_BF16_CASES))
def test_gemm_case_is_in_its_regime(case):
    in_its_regime(case)
    assert case.Cin % 32 == 0 and case.Cout % 32 == 0 and case.HW % 4 == 0 and case.tile in GC.TILE_FORMS
    assert case.Cout % case.BM == 0 and case.Cin % case.tile[3] == 0
    assert case.Cout * case.HW * case.B * 4 <= 8.5e6                       # the largest output: about 8.4 MB


def test_gemm_cases_cover_the_tile_forms():
    cases = GC.GEMM_CASES
    forms = set(GC.TILE_FORMS)
    assert {c.tile for c in cases if c.epilogue == 1} == forms              # (every case runs in every mode)
    assert {c.tile for c in cases if c.epilogue == 1 and c.ragged} == forms
    assert {c.tile for c in cases if c.fold} == forms
    assert {c.tile for c in cases if c.B > 1 and c.per_sample_noise} == forms
    # the ring against the contraction: fewer stages than the prologue wants in flight, exactly as many, a wrap; one stage of
    # the 64-deep forms
    ring4 = {c.regime()["stages"] for c in cases if c.tile == (1, 2, 2, 32, 4)}
    assert {1, 2, 3, 5} <= ring4
    assert any(c.regime()["stages"] == 1 for c in cases if c.tile == (1, 4, 2, 64, 2))
    assert any(c.regime()["stages"] == 1 for c in cases if c.tile == (2, 4, 2, 64, 2))
    # pixel tails of both tile widths: 4, BN - 4, BN, BN + 4 pixels in all (a tail of 4 behind a full tile), and HW = 4
    for bn in (64, 128):
        tails = {c.regime()["tail"] for c in cases if c.BN == bn}
        assert {4, bn - 4, bn} <= tails, (bn, tails)
        assert any(c.HW == bn + 4 for c in cases if c.BN == bn)
        assert any(c.HW == 4 for c in cases if c.BN == bn)
    # row blocks of the fold's partials: 32-, 64- and 128-row blocks, more than one of each of the first two
    blocks = {(c.BM, c.regime()["row_blocks"]) for c in cases if c.fold}
    assert {32, 64, 128} == {b for b, _ in blocks} and (32, 3) in blocks and (64, 4) in blocks and (128, 2) in blocks
    assert {c.tile[1] for c in cases if c.fold} == {2, 4, 8}                # WGM of the LDS reduction
    # the switches
    assert any(c.epilogue == 0 and not c.fold for c in cases) and any(c.epilogue == 0 and c.fold for c in cases)
    assert any(c.epilogue == 1 and c.noise is None for c in cases) and any(c.noise == "shared" and c.B == 1 for c in cases)
    assert any(c.amax == "loose" for c in GC.SPLIT_ONLY_CASES)
    spread = [c for c in GC.SPLIT_ONLY_CASES if c.sample_scale]
    assert spread and spread[0].sample_scale[1] / spread[0].sample_scale[0] == 2.0 ** 37
    t = spread[0].tensors()
    a = spread[0].amax_given(t)
    assert GC.split_exp(float(a[1])) - GC.split_exp(float(a[0])) in (36, 37, 38)
    # sample 1 split with sample 0's exponent overflows fp16
    assert float(t["x"][1].abs().max()) * 2.0 ** -GC.split_exp(float(a[0])) > 65520.0
    # every mutant is applied somewhere
    assert {m for c in cases for m in c.gemm_mutants()} == {"drop_stage_last_channel", "kgroup_twice", "swap_pixels", "tail_shift4"}
    assert {m for c in cases for m in c.epilogue_mutants()} == {"bias_row16", "slope_sign", "gain_before_bias", "noise_sample0"}
    assert {m for c in cases for m in c.fold_mutants()} == {"fold_drop_block", "fold_wrong_row", "fold_preact"}


def test_tile_replay_on_the_listed_regimes():
    """the table of the issue, (B, Cin, Cout, HW, fold) -> tile"""
    A, B_, C, D, E, F, G, H = GC.TILE_FORMS
    for args, tile in [((1, 32, 256, 132, False), A), ((1, 96, 256, 132, False), A), ((1, 160, 256, 260, False), A),
                       ((1, 64, 288, 132, False), A), ((2, 160, 224, 132, False), A), ((1, 64, 256, 4100, False), B_),
                       ((1, 192, 256, 132, True), B_), ((3, 64, 256, 2692, False), C), ((3, 64, 256, 2692, True), C),
                       ((1, 96, 256, 4228, False), D), ((1, 96, 256, 132, True), D), ((1, 64, 320, 6532, False), D),
                       ((2, 32, 128, 68, False), E), ((1, 128, 128, 4, False), E), ((2, 64, 128, 196, True), E),
                       ((1, 160, 128, 196, False), G), ((1, 160, 128, 196, True), G), ((2, 64, 64, 124, False), D),
                       ((2, 64, 64, 124, True), D), ((1, 160, 64, 128, False), H), ((1, 160, 64, 256, False), H),
                       ((1, 32, 32, 4, False), F), ((2, 128, 96, 252, True), F)]:
        assert GC.gemm_tile(*args) == tile, args
        listed = [c for c in GC.GEMM_CASES if (c.B, c.Cin, c.Cout, c.HW, c.fold) == args]
        assert listed, f"{args} is not in GEMM_CASES"


def test_split_exponent_and_halves():
    """cips3d_split_exp: bound 2^-e in [2^14, 2^15); the halves of cips3d_split16 hold 22 bits, fp16 subnormals kept"""
    for a in (1.0, 1.5, 2.0, 3.999, 2.0 ** -20, 7.3e9, 6.0e-20):
        e = GC.split_exp(a)
        assert 2.0 ** 14 <= GC.f32(a) * 2.0 ** -e < 2.0 ** 15
    assert GC.split_exp(0.0) == -100 and GC.split_exp(2.0 ** 120) == 100
    v = torch.randn(20000, generator=torch.Generator().manual_seed(1)) * torch.tensor([1e-9, 1e-6, 1e-3, 1.0, 3e3]).repeat(4000)
    hi, lo = GC.split16(v)
    err = (v.double() - hi.double() - lo.double()).abs()
    assert bool((err <= 2.0 ** -22 * v.double().abs() + 2.0 ** -25).all())
    assert bool((lo.double().abs() <= (2.0 ** -11 + 2.0 ** -22) * v.double().abs() + 2.0 ** -24).all())


# --------------------------------------------------------------------------------------------------------------------- reduce
@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.REDUCE_CASES, ids=ids(GC.REDUCE_CASES))
def test_torgb_reduce_bounds(case, gs):
    t = case.tensors(gs)
    admits_and_rejects(case.id, GC.reduce_ref(t, F64), GC.reduce_bound(t), GC.reduce_ref(t, F32),
                       {m: GC.reduce_ref(t, F64, m) for m in case.mutants()})


def test_reduce_cases_are_the_regimes_the_kernel_has():
    assert {c.n_slots for c in GC.REDUCE_CASES} == {1, 3, 4, 5, 16, 17, 48}
    assert {c.n_bias for c in GC.REDUCE_CASES} == {0, 1, GC.FOLD_MAX}
    assert {c.skip for c in GC.REDUCE_CASES} == {True, False} and {c.B for c in GC.REDUCE_CASES} == {1, 2}
    assert {c.HW for c in GC.REDUCE_CASES} == {4, 260}
    assert {m for c in GC.REDUCE_CASES for m in c.mutants()} == {"last_slot_lost", "bias_twice"}
    assert GC.reduce_counts(1, 0, False) == (3, 1) and GC.reduce_counts(17, 8, True) == (9, 9) and GC.reduce_counts(48, 1, True) == (16, 2)


# --------------------------------------------------------------------------------------------------------- the per-op kernels
@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.UP_CASES, ids=ids(GC.UP_CASES))
def test_up2_fir_act_bounds(case, gs):
    t = case.tensors(gs)
    admits_and_rejects(case.id, GC.up_ref(case, t, F64), GC.up_bound(case, t), GC.up_ref(case, t, F32),
                       {m: GC.up_ref(case, t, F64, m) for m in case.mutants()})


def test_upfir_is_the_tap_formula():
    """the reference's convolution against up2_tap's formula, pixel by pixel, in fp64"""
    g = torch.Generator().manual_seed(2)
    H, W = 3, 4
    y = torch.randn(1, H, W, generator=g, dtype=F64)
    fir = GC.FIR.double()
    got = GC.upfir(y, fir)[0]
    for oy in range(2 * H):
        for ox in range(2 * W):
            acc = 0.0
            for ky in range(oy & 1, 4, 2):
                for kx in range(ox & 1, 4, 2):
                    iy, ix = (oy + ky - 2) >> 1, (ox + kx - 2) >> 1
                    if 0 <= iy < H and 0 <= ix < W:
                        acc += float(y[0, iy, ix]) * float(fir[3 - ky, 3 - kx])
            assert abs(acc - float(got[oy, ox])) <= 1e-14


def test_up_cases_are_the_regimes_the_kernel_has():
    shapes = {(c.B, c.C, c.H, c.W) for c in GC.UP_CASES}
    assert shapes == {(1, 1, 1, 2), (2, 3, 1, 6), (3, 5, 3, 6), (1, 2, 7, 2), (2, 33, 5, 10)}
    assert {c.noise for c in GC.UP_CASES} == {"shared", "per_sample", "none"}
    assert any(c.B > 1 and (c.C * c.H * c.W // 2) % 256 != 0 for c in GC.UP_CASES)          # a workgroup across samples
    assert {m for c in GC.UP_CASES for m in c.mutants()} == {"tap_mirrored", "right_border_inside", "slope_sign", "gain_before_bias",
                                                            "noise_sample0"}


@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.NBA_CASES, ids=ids(GC.NBA_CASES))
def test_noise_bias_act_bounds(case, gs):
    t = case.tensors(gs)
    admits_and_rejects(case.id, GC.nba_ref(case, t, F64), GC.nba_bound(case, t), GC.nba_ref(case, t, F32),
                       {m: GC.nba_ref(case, t, F64, m) for m in case.mutants()})


def test_noise_bias_act_cases():
    assert {c.HW for c in GC.NBA_CASES} == {1, 3, 4, 1025} and {c.C for c in GC.NBA_CASES} == {1, 33}
    assert {c.B for c in GC.NBA_CASES} == {1, 3} and {c.noise for c in GC.NBA_CASES} == {"shared", "per_sample", "none"}


@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.RGB_CASES, ids=ids(GC.RGB_CASES))
def test_torgb_bounds(case, gs):
    in_its_regime(case)
    t = case.tensors(gs)
    admits_and_rejects(case.id, GC.rgb_ref(case, t, F64), GC.rgb_bound(case, t), GC.rgb_ref(case, t, F32),
                       {m: GC.rgb_ref(case, t, F64, m) for m in case.mutants()})


def test_torgb_cases_reach_every_launch_arm_with_every_skip():
    assert {(c.regime()["arm"], c.skip) for c in GC.RGB_CASES} == {(a, s) for a in ("scalar", "split16", "split4", "plain")
                                                                   for s in ("none", "plain", "fir")}
    assert all(c.H != c.W and c.H % 2 == 0 and c.W % 2 == 0 for c in GC.RGB_CASES)
    assert any(c.regime()["arm"] == "split16" and c.regime()["quads"] > 16 and c.regime()["last_block_quads"] < 16 for c in GC.RGB_CASES)
    assert any(c.regime()["arm"] == "split4" and c.regime()["uneven_slices"] for c in GC.RGB_CASES)


# ---------------------------------------------------------------------------------------------------------------- modulation
@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("gs", GC.SCALES)
@pytest.mark.parametrize("case", GC.MOD_CASES + GC.MOD_PACKED_CASES, ids=ids(GC.MOD_CASES + GC.MOD_PACKED_CASES))
def test_modulate_bounds(case, gs, demod):
    t = case.tensors(gs)
    admits_and_rejects(case.id, GC.mod_ref(case, t, F64, demod), GC.mod_bound(case, t, demod), GC.mod_ref(case, t, F32, demod),
                       {m: GC.mod_ref(case, t, F64, demod, m) for m in case.mutants(demod, gs)})


def test_modulate_cases_are_the_regimes_the_kernel_has():
    for c in GC.MOD_CASES:
        in_its_regime(c)
    shapes = {(c.B, c.Cout, c.Cin, c.ksq) for c in GC.MOD_CASES}
    assert shapes >= {(1, 1, 1, 1), (3, 5, 63, 1), (2, 6, 64, 1), (1, 3, 1024, 1), (1, 3, 1028, 1), (2, 2, 120, 9), (3, 3, 40, 1)}
    assert all(c.s_offset > 0 and c.s_stride > c.Cin for c in GC.MOD_CASES + GC.MOD_PACKED_CASES)
    assert all(c.Cout % 32 == 0 and c.Cin % 32 == 0 and c.ksq == 1 for c in GC.MOD_PACKED_CASES)
    muts = {m for c in GC.MOD_CASES for gs in GC.SCALES for m in c.mutants(True, gs)}
    assert muts == {"style_shifted", "norm_short", "eps_after_rsqrt"}
    # the un-packers invert the kernel's index maps (modulate_row: plain packed, split, bf16 fragments)
    B, M, K = 2, 32, 64
    wm = torch.randn(B, M, K, generator=torch.Generator().manual_seed(4))
    e = torch.arange(B * M * K)
    b, o, i = e // (M * K), (e // K) % M, e % K
    at = ((b * (M // 16) + o // 16) * (K // 16) + i // 16) * 256 + ((i % 4) * 16 + o % 16) * 4 + (i // 4) % 4
    packed = torch.empty(B * M * K)
    packed[at] = wm.reshape(-1)
    assert torch.equal(GC.unpack(packed, B, M, K, False), wm)
    at16 = ((b * (M // 16) + o // 16) * (K // 32) + i // 32) * 512 + (((i // 8) % 4) * 16 + o % 16) * 8 + i % 8
    halves = torch.zeros(2 * B * M * K, dtype=torch.bfloat16)
    halves[at16] = wm.reshape(-1).to(torch.bfloat16)
    assert torch.equal(GC.unpack_bf16(halves.view(F32), B, M, K), wm.to(torch.bfloat16).float())
