"""The bounds and cases of tests/_conv3x3_cases.py, checked without a GPU on every case test_gpu_conv3x3.py runs, in both modes and
at every data scale: (a) the reference evaluated by torch in fp32 on the CPU in the model's order, the fp32 evaluation of the
commuted form the kernel uses (FIR first, flipped valid correlation) and -- for the split mode -- the emulation built from
mfma_frag.h's definitions under the replayed exponents stay inside the bound against the model-order fp64 reference: a correct
implementation passes; (b) every mutant leaves the bound, on the case named here for it and on every other case it applies to;
(c) every case sits in the regime it is listed for and the list covers the edges the kernel has; (d) the un-packers invert the
index maps of the 3x3 fragment layouts, and the direct kernel's bound admits fp32 and rejects its mutants.
Prints split bound / fp32 bound per case (not asserted).  Median by Cin at gs = 1 with a measured amax (median = max to three
digits in the plain form, within 0.02 in the up form):
    plain   16: 2.98   32: 2.99   48: 3.00   256: 3.00          ((27 Cin + 20) / (9 Cin + 8) to first order)
    up      16: 2.90 to 2.92   32: 2.95   48: 2.97   256: 3.00   (the term sum |w| e(Z) is the same in both modes)"""
import pytest
import torch

import _conv3x3_cases as CC

F32, F64 = torch.float32, torch.float64
GC = CC.GC
ALL = [(c, m) for m in CC.MODES for c in CC.CASES]
all_ids = [f"{m}-{c.id}" for c, m in ALL]
NAMED = {"halo_left_zero": "up-B1-i32-o16-H16-W66", "halo_right_zero": "pl-B1-i48-o48-H12-W132", "halo_top_zero": "pl-B1-i32-o16-H7-W12",
         "taps_unflipped": "up-B1-i16-o16-H1-W2", "fir_mirrored": "up-B1-i16-o16-H2-W34", "row_parity": "up-B1-i16-o32-H5-W6-ep0n",
         "hw_exchanged": "pl-B1-i32-o32-H32-W132", "tile_slot_copied": "up-B1-i32-o16-H16-W66",
         "drop_stage_last_channel": "pl-B1-i16-o16-H1-W4", "last_stage_skipped": "up-B2-i48-o64-H6-W66-big_first",
         "block2_first_weights": "pl-B1-i256-o32-H4-W8", "tap9_twice": "up-B1-i256-o32-H2-W4", "cross_lost": "pl-B1-i16-o16-H1-W4",
         "noise_sample0": "up-B2-i32-o64-H4-W64-epB-big_second", "bias_next_channel": "pl-B1-i16-o32-H5-W8-ep",
         "slope_sign": "up-B1-i16-o48-H3-W10-ep-loose", "gain_before_bias": "pl-B2-i32-o16-H4-W8-ep0n-big_first"}


def check(case, mode, only=None):
    for gs, ranged in CC.runs(mode):
        t = case.tensors(gs)
        exps = CC.replay_exps(case, t, ranged) if mode == "split" else None
        what = f"{mode} {case.id} gs={gs} ranged={ranged}"
        ref, e = CC.conv_bound(case, t, mode, exps)
        assert bool(torch.isfinite(e).all()) and bool((e >= 0).all()), what
        if only is None:
            impls = {"model order": CC.correct_fp32(case, t, mode, exps),
                     "commuted": CC.finish(case, CC.commuted(case, t, F32), t, F32) if mode == "fp32" else None}
            for name, got in impls.items():
                if got is not None:
                    ratio, at = GC.worst((got.double() - ref).abs(), e)
                    assert GC.inside(got, ref, e), f"{what}: the {name} implementation is {ratio:.2f} x the bound at element {at}"
        for m in (case.mutants(mode) if only is None else [only]):
            assert not GC.inside(CC.mutated(case, t, m, exps), ref, e), f"{what}: the mutant `{m}` stays inside the bound"
        if mode == "split" and gs == 1.0 and ranged and only is None and case.epilogue == 0:
            r = e / CC.conv_bound(case, t, "fp32")[1]
            r = r[torch.isfinite(r)]
            print(f"split / fp32 bound Cin={case.Cin} {case.id}: median {float(r.median()):.3f} max {float(r.max()):.3f} "
                  f"((27 K + 20) / (9 K + 8) = {(27 * case.Cin + 20) / (9 * case.Cin + 8):.3f})")


@pytest.mark.parametrize("case,mode", ALL, ids=all_ids)
def test_conv_bounds(case, mode):
    check(case, mode)


@pytest.mark.parametrize("mutant", CC.MUTANTS)
def test_every_mutant_is_rejected_on_its_named_case(mutant):
    case = next(c for c in CC.CASES if c.id == NAMED[mutant])
    for mode in CC.MODES:
        if mutant in case.mutants(mode):
            check(case, mode, only=mutant)
    assert any(mutant in case.mutants(mode) for mode in CC.MODES)


def test_named_cases_exist_and_cover_the_mutants():
    ids = {c.id for c in CC.CASES}
    assert len(ids) == len(CC.CASES)
    assert set(NAMED) == set(CC.MUTANTS) == {m for c in CC.CASES for mode in CC.MODES for m in c.mutants(mode)}
    assert set(NAMED.values()) <= ids


@pytest.mark.parametrize("case", CC.CASES, ids=[c.id for c in CC.CASES])
def test_case_is_in_its_regime(case):
    got = case.regime()
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.id}: {k} is {got[k]}, the case is listed for {v}"
    # what cips3d_modconv3x3_supported asks for
    assert case.Cin % 16 == 0 and case.Cout % 16 == 0 and case.OW % 4 == 0 and (case.up or case.W % 4 == 0)
    assert case.Cin <= 64 or (case.Cin == 256 and case.tiles == 1)
    assert 4 * case.B * max(case.Cout * case.OH * case.OW, case.Cin * case.H * case.W) <= 2.1e6


def test_cases_cover_the_edges():
    for up in (False, True):
        rg = [(c, c.regime()) for c in CC.CASES if c.up == up]
        assert any(c.OH == (2 if up else 1) and c.OW == 4 for c, _ in rg)
        assert {c.OH for c, r in rg if r["ragged_rows"]} >= ({10} if up else {5, 7})
        assert any(c.OW == 68 for c, _ in rg) and any(c.OW == 64 for c, _ in rg) and any(c.OW == 128 for c, _ in rg)
        assert any(r["tiles_x"] >= 2 and r["tiles_y"] >= 2 for _, r in rg)
        assert {8, 24} <= {r["tiles"] for _, r in rg if r["swizzled"]}
        assert any(r["tiles"] == 24 and r["tiles_x"] == 3 for _, r in rg)
        assert any(not r["swizzled"] and r["tiles"] > 1 and r["tiles_x"] == 3 and not r["square"] for _, r in rg)
        assert {1, 2, 3, 16} <= {r["nstage"] for _, r in rg}
        assert {16, 48, 32, 64} <= {c.Cout for c, _ in rg}
        assert {c.spread for c, _ in rg if c.B == 2} >= {"big_first", "big_second"}
        assert {(c.epilogue, c.noise) for c, _ in rg} >= {(0, None), (1, "shared"), (1, None)}
        assert any(c.per_sample_noise for c, _ in rg)
        assert any(c.amax == "loose" for c, _ in rg) and any(c.zero is not None for c, _ in rg)
    assert {c.zero for c in CC.CASES} >= {0, 1}
    assert (1.0, False) in CC.runs("split") and (1.0, False) not in CC.runs("fp32")
    # biases differ per channel
    t = CC.CASES[2].tensors()
    assert len(set(t["bias"].tolist())) == CC.CASES[2].Cout


def test_sample_spread_and_exponents():
    """samples 2^9 apart: the exponents follow; the small sample's exponent overflows the large one's fp16 halves; a loose amax
    moves the exponent by three; a zero sample has the lowest exponent; the unranged run fits fp16"""
    for c in CC.CASES:
        for gs in CC.SPLIT_SCALES:
            t = c.tensors(gs)
            ex = CC.replay_exps(c, t)
            z = CC.z_of(c, t["x"].double())
            for b in range(c.B):
                zmax = float(z[b].abs().max())
                assert zmax * 2.0 ** -ex[b] < 2.0 ** 15, (c.id, gs, b)
                if zmax == 0.0:
                    assert ex[b] == -100
            if c.spread:
                big, small = (0, 1) if c.spread == "big_first" else (1, 0)
                assert ex[big] - ex[small] in (8, 9, 10), (c.id, ex)
                assert float(z[big].abs().max()) * 2.0 ** -ex[small] > 65520.0, (c.id, gs)
            if c.amax == "loose":
                tight = CC.ConvCase(c.Cin, c.Cout, c.H, c.W, c.up, c.B, spread=c.spread)
                assert [a - b for a, b in zip(ex, CC.replay_exps(tight, t))] == [3] * c.B
        assert float(CC.z_of(c, c.tensors()["x"].double()).abs().max()) < 2.0 ** 15, c.id
        assert CC.replay_exps(c, c.tensors(), ranged=False) == [0] * c.B
    assert abs(CC.fir_gain() - float(CC.FIR.double().abs().sum())) < 1e-5


def test_commuted_form_is_the_model_in_fp64():
    """Z by the kernel's polyphase rule equals upfirdn2d(up = 2, pad = (3, 2)), and the valid correlation of Z with the flipped taps
    equals conv_transpose2d + blur, to fp64 rounding"""
    for c in CC.CASES:
        t = c.tensors()
        x = t["x"].double()
        if c.up:
            za, zb = CC.z_of(c, x, CC.FIR.double()), CC.z_upfir(x, CC.FIR.double())
            assert za.shape == zb.shape and float((za - zb).abs().max()) <= 1e-12 * float(zb.abs().max())
        a, b = CC.commuted(c, t, F64), CC.conv_ref(c, t, F64)
        assert a.shape == b.shape == (c.B, c.Cout, c.OH, c.OW)
        assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300), c.id


def test_unpackers_invert_the_3x3_index_maps():
    """modulate_row, ksq = 9: the tap-major fp32 fragments and the split tap pairs with their zero tenth tap"""
    B, M, K = 2, 32, 32
    wm = torch.randn(B, M, K, 9, generator=torch.Generator().manual_seed(5))
    e = torch.arange(B * M * K * 9)
    b, o, i, tp = e // (M * K * 9), (e // (K * 9)) % M, (e // 9) % K, e % 9
    for flip in (False, True):
        tap = 8 - tp if flip else tp
        at = (((b * 9 + tap) * (M // 16) + o // 16) * (K // 16) + i // 16) * 256 + ((i % 4) * 16 + o % 16) * 4 + (i // 4) % 4
        packed = torch.empty(B * M * K * 9)
        packed[at] = wm.reshape(-1)
        assert torch.equal(CC.unpack3x3(packed, B, M, K, flip), wm.reshape(B, M, K * 9))
        pr, hh = tap // 2, tap % 2
        blk = (((b * 5 + pr) * (M // 16) + o // 16) * (K // 16) + i // 16) * 1024
        ln = ((hh * 2 + (i // 8) % 2) * 16 + o % 16) * 8 + i % 8
        halves = torch.full((B * 10 * M * K * 2,), 7.0, dtype=torch.float16)
        hi, lo = GC.split16(wm.reshape(-1) * 256.0)
        halves[blk + ln], halves[blk + 512 + ln] = hi.half(), lo.half()
        got, tenth = CC.unpack3x3_split(halves.view(F32), B, M, K, flip)
        assert torch.equal(got, ((hi.double() + lo.double()) / 256.0).reshape(B, M, K * 9))
        assert bool((tenth == 7.0).all())                                   # the positions the map above never writes
    for c in CC.MOD3_CASES:
        got = c.regime()
        for k, v in c.expect.items():
            assert got[k] == v, (c.id, k)
        assert c.ksq == 9 and c.Cout % 16 == 0 and c.Cin % 16 == 0
    assert [c.regime()["cached"] for c in CC.MOD3_CASES] == [True, False]


@pytest.mark.parametrize("demod", [True, False])
@pytest.mark.parametrize("case", CC.MOD3_CASES, ids=[c.id for c in CC.MOD3_CASES])
def test_modulate_bound_admits_fp32_at_3x3(case, demod):
    t = case.tensors()
    ref, e = GC.mod_ref(case, t, F64, demod), GC.mod_bound(case, t, demod)
    assert GC.inside(GC.mod_ref(case, t, F32, demod), ref, e)
    for m in case.mutants(demod, 1.0):
        assert not GC.inside(GC.mod_ref(case, t, F64, demod, m), ref, e), m


@pytest.mark.parametrize("gs", CC.SCALES)
@pytest.mark.parametrize("case", CC.KXK_CASES, ids=[c.id for c in CC.KXK_CASES])
def test_kxk_bounds(case, gs):
    t = case.tensors(gs)
    ref, e = CC.kxk_ref(case, t, F64), CC.kxk_bound(case, t)
    assert ref.shape == (case.B, case.Cout, *case.out_hw)
    got = CC.kxk_ref(case, t, F32)
    ratio, at = GC.worst((got.double() - ref).abs(), e)
    assert GC.inside(got, ref, e), f"{case.id}: fp32 is {ratio:.2f} x the bound at {at}"
    for m in case.mutants():
        assert not GC.inside(CC.kxk_ref(case, t, F64, m), ref, e), f"{case.id}: `{m}` stays inside"


def test_kxk_cases_are_shapes_the_mfma_kernel_refuses():
    assert {(c.Cin, c.W) for c in CC.KXK_CASES} == {(8, 6), (17, 5)} and {c.k for c in CC.KXK_CASES} == {1, 3, 5}
    assert {c.transpose2 for c in CC.KXK_CASES} == {True, False} and all(c.B == 2 and c.Cout == 12 for c in CC.KXK_CASES)
    assert all(c.Cin % 16 != 0 and c.Cout % 16 != 0 for c in CC.KXK_CASES)
