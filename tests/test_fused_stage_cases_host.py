"""The bounds and cases of tests/_fused_stage_cases.py, checked without a GPU on every case test_gpu_fused_stage.py runs, in every
mode and at every data scale: (a) the reference evaluated by torch in fp32 on the CPU -- for the bf16 mode with both operands of
every contraction rounded, for the split mode with the fp16 halves of GC.split16 under the replayed exponents -- stays inside the
bound against fp64 on out2, rgb and y_next, and again on rgb and y_next against their own arithmetic on the out2 that implementation
produced: a correct implementation passes; (b) every mutant leaves a bound that the GPU test holds the case to, on a case named
here for it and on every other case it applies to: the mutants of conv1 and conv2 the bound of out2, rgb or y_next (out2 counts for
every case: where a case does not store it, the GPU test checks the out2 of the same launch with the store, after showing that the
store changes no other bit), the mutants of ToRGB's and the chained GEMM's own arithmetic (FC.OWN_MUTANTS) the second bound, given the
out2 they fold -- in bf16, whose first bound carries 2^-8 of every channel's magnitude through a sum over C channels, only that one;
(c) every case sits in the regime it is listed for, and interior tiles, non-square maps and both tile orders appear for every one
of the seven base instantiations.  Prints split bound / fp32 bound per C (recorded in test_gpu_fused_stage.py, not asserted)."""
import pytest
import torch

import _fused_stage_cases as FC

F32, F64 = torch.float32, torch.float64
OUTS = ("out2", "rgb", "y_next")
ALL = [(c, m) for m in FC.MODES for c in FC.CASES]
all_ids = [f"{m}-{c.id}" for c, m in ALL]
# the case each mutant is shown on by name (every applicable mutant of every case is checked as well)
NAMED = {"halo_left_zero": "C32u-B1-H4-W96-nss-fir", "tile_slot_copied": "C256u-B2-H4-W64-nps-plain-noout2",
         "hw_exchanged": "C128u-B2-H6-W96-npp-fir", "n1_row_down": "C64c-B2-H4-W96-npp-fir",
         "drop_stage_last_channel": "C256c-B1-H6-W96-nss-fir", "kgroups_swapped": "C128c-B1-H4-W96-nss-fir",
         "rgb_row_lost": "C256u-B1-H6-W96-nss-fir", "skip_parity": "C64u-B2-H4-W96-nsp-fir-noout2",
         "n1_sample0": "C32u-B2-H8-W96-nps-plain-noout2", "n2_sample0": "C256c-B2-H4-W64-nsp-norgb",
         "slope_sign": "C128c-flat-B1-H4-W64-n0s-plain", "gain_before_bias": "C64c-flat-B2-H8-W128-npp-plain"}


def observed(case):
    """the outputs the GPU test holds to fp64 (out2 of the launch with the store where the case itself does not store it)"""
    return [k for k in OUTS if (k != "rgb" or case.rgb) and (k != "y_next" or case.chained)]


def admitted(what, got, ref, bound, keys):
    worst = 0.0
    for k in keys:
        assert bool(torch.isfinite(bound[k]).all()) and bool((bound[k] >= 0).all()), (what, k)
        ratio, at = FC.GC.worst((got[k].double() - ref[k]).abs(), bound[k])
        assert FC.GC.inside(got[k], ref[k], bound[k]), f"{what} {k}: a correct implementation is {ratio:.2f} x the bound at element {at}"
        worst = max(worst, ratio)
    return worst


def rejected(case, t, mode, ref, bound, mutant, keys):
    m = FC.stage_ref(case, t, F64, mutant)
    return any(not FC.GC.inside(m[k], ref[k], bound[k]) for k in keys)


def rejected_given_out2(case, t, mode, exps, mutant, out2):
    """against rgb's and y_next's own arithmetic on `out2`"""
    ref2, e2 = FC.stage_bounds(case, t, mode, exps, out2=out2)
    m = FC.stage_ref(case, t, F64, mutant, out2=out2)
    return any(ref2[k] is not None and not FC.GC.inside(m[k], ref2[k], e2[k]) for k in OUTS[1:])


runs = FC.runs


@pytest.mark.parametrize("case,mode", ALL, ids=all_ids)
def test_stage_bounds(case, mode):
    for gs, ranged in runs(mode):
        t = case.tensors(gs)
        exps = FC.replay_exps(case, t, ranged) if mode == "split" else None
        what = f"{mode} {case.id} gs={gs} ranged={ranged}"
        ref, e = FC.stage_bounds(case, t, mode, exps)
        got = FC.emulate(case, t, mode, exps)
        admitted(what, got, ref, e, ("act1",) if mode == "fp32" else ())
        admitted(what, got, ref, e, OUTS[:1] + tuple(k for k in OUTS[1:] if ref[k] is not None))
        # rgb and y_next alone, given the out2 this implementation produced
        ref2, e2 = FC.stage_bounds(case, t, mode, exps, out2=got["out2"])
        admitted(what + " of the output", got, ref2, e2, tuple(k for k in OUTS[1:] if ref2[k] is not None))
        for m in case.mutants():
            if m in FC.OWN_MUTANTS:
                assert rejected_given_out2(case, t, mode, exps, m, got["out2"]), f"{what}: `{m}` stays inside the bound of the output's own arithmetic"
            if m not in FC.OWN_MUTANTS or mode != "bf16":
                assert rejected(case, t, mode, ref, e, m, observed(case)), f"{what}: the mutant `{m}` stays inside the bounds"
        if mode == "split" and gs == 1.0 and ranged:
            _, e32 = FC.stage_bounds(case, t, "fp32")
            for k in observed(case):
                r = e[k] / e32[k]
                print(f"split / fp32 bound C={case.C} {k} {case.id}: median {float(r.median()):.3f} max {float(r.max()):.3f}")


@pytest.mark.parametrize("mutant", FC.MUTANTS)
def test_every_mutant_is_rejected_on_its_named_case(mutant):
    case = next(c for c in FC.CASES if c.id == NAMED[mutant])
    assert mutant in case.mutants()
    for mode in FC.MODES:
        for gs, ranged in runs(mode):
            t = case.tensors(gs)
            exps = FC.replay_exps(case, t, ranged) if mode == "split" else None
            ref, e = FC.stage_bounds(case, t, mode, exps)
            if mutant in FC.OWN_MUTANTS:
                assert rejected_given_out2(case, t, mode, exps, mutant, FC.emulate(case, t, mode, exps)["out2"]), (mutant, mode, gs)
            if mutant not in FC.OWN_MUTANTS or mode != "bf16":
                assert rejected(case, t, mode, ref, e, mutant, observed(case)), (mutant, mode, gs)


def test_named_cases_exist_and_cover_the_mutants():
    ids = {c.id for c in FC.CASES}
    assert len(ids) == len(FC.CASES)
    assert set(NAMED) == set(FC.MUTANTS) == {m for c in FC.CASES for m in c.mutants()}
    assert set(NAMED.values()) <= ids


@pytest.mark.parametrize("case", FC.CASES, ids=[c.id for c in FC.CASES])
def test_case_is_in_its_regime(case):
    got = case.regime()
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.id}: {k} is {got[k]}, the case is listed for {v}"
    assert case.OW % case.TW == 0 and case.OH % case.TH == 0 and case.C == 16 * case.WM * case.WGM
    if case.flat:
        assert case.W % 64 == 0 and case.H % 4 == 0
    else:
        assert case.W % 32 == 0 and case.H % 2 == 0
    assert case.B * case.C * case.OH * case.OW * 4 <= 3.2e6


def test_launch_table_replay():
    """the table of the issue: tile, tile count and interior tiles of the smallest shape of each regime"""
    rows = [((32, False, 4, 96), (2, 64), 12, 2), ((64, False, 8, 96), (2, 64), 24, 6), ((64, True, 4, 96), (2, 64), 12, 2),
            ((128, True, 8, 96), (2, 64), 24, 6), ((128, False, 6, 96), (4, 64), 9, 1), ((128, False, 16, 96), (4, 64), 24, 6),
            ((256, False, 6, 96), (2, 32), 36, 16), ((256, True, 4, 64), (2, 32), 16, 4), ((256, True, 2, 32), (2, 32), 4, 0),
            ((32, False, 2, 32), (2, 64), 2, 0), ((128, False, 2, 32), (4, 64), 1, 0)]
    for (C, ch, H, W), tile, tiles, interior in rows:
        rg = FC.StageCase(C, ch, False, 1, H, W).regime()
        assert (rg["tile"], rg["tiles"], rg["interior"], rg["swizzled"]) == (tile, tiles, interior, tiles % 8 == 0), (C, ch, H, W, rg)
    assert FC.StageCase(32, False, True, 1, 8, 128, skip="plain").regime()["tiles"] == 8
    assert [FC.StageCase(C, True, False, 1, 2, 32).regime()["xchg"] for C in (64, 128, 256)] == [True, False, True]
    assert FC.next_counts(FC.StageCase(128, True, False, 1, 2, 32)) == (64 + 8 + 1, 192 + 8 + 1)
    assert FC.next_counts(FC.StageCase(256, True, False, 1, 2, 32)) == (264, 776)


def test_cases_cover_the_three_regimes_for_every_instantiation():
    up = [c for c in FC.CASES if not c.flat]
    for base in FC.BASE:
        mine = [c.regime() for c in up if c.base == base]
        assert any(r["interior"] > 0 and not r["swizzled"] for r in mine), f"{base}: no interior tile in plain order"
        assert any(r["interior"] > 0 and r["swizzled"] for r in mine), f"{base}: no interior tile in the permuted order"
        assert any(r["interior"] == 0 for r in mine), f"{base}: no case without interior tiles"
        assert any(not r["square"] and r["interior"] > 0 for r in mine), f"{base}: no non-square map"
        assert {r["swizzled"] for r in mine} == {True, False}
        flat = [c.regime() for c in FC.CASES if c.flat and c.base == base]
        assert flat, f"{base}: no flat form"
    # both tile orders of every tile shape among the flat forms
    assert {(c.regime()["tile"], c.regime()["swizzled"]) for c in FC.CASES if c.flat} >= {(t, s) for t in ((2, 64), (4, 64), (2, 32))
                                                                                         for s in (True, False)} - {((4, 64), False)}
    # the switches
    assert {c.B for c in FC.CASES} == {1, 2}
    arr = {(c.n1, c.n2) for c in FC.CASES if c.B > 1}
    assert {("per_sample", "shared"), ("shared", "per_sample"), ("per_sample", "per_sample")} <= arr
    assert any(c.n1 is None and c.n2 is None for c in FC.CASES) and any((c.n1 is None) != (c.n2 is None) for c in FC.CASES)
    assert {c.skip for c in FC.CASES if c.rgb} == {"none", "plain", "fir"}
    assert {c.want_out2 for c in FC.CASES} == {True, False}
    assert {c.C for c in FC.CASES if c.chained and not c.rgb} == {64, 128, 256}
    # sample 0's y_lo is 2^9 times sample 1's: both exponents sit 8 or more above, at every scale
    for c in (c for c in FC.CASES if c.B == 2):
        for gs in FC.SPLIT_SCALES:
            ex = FC.replay_exps(c, c.tensors(gs))
            assert ex[0][0] - ex[1][0] >= 8 and ex[0][1] - ex[1][1] >= 8, (c.id, gs, ex)


def test_order_pairs_have_one_order_each():
    assert {p[0].base for p in FC.ORDER_PAIRS} == set(FC.BASE)
    for tall, r, Hs in FC.ORDER_PAIRS:
        t = tall.tensors()
        short, s = tall.window(t, r, Hs)
        a, b = tall.regime(), short.regime()
        assert a["swizzled"] != b["swizzled"] and a["interior"] > 0 and b["interior"] > 0, (tall.id, a, b)
        # the window's output rows whose FIR taps all lie inside it are the tall case's rows, in fp64 exactly
        ra, rb = FC.stage_ref(tall, t, F64), FC.stage_ref(short, s, F64)
        for k in OUTS:
            if ra[k] is not None:
                va = ra[k].reshape(tall.B, -1, tall.OH, tall.OW)[:, :, 2 * r + 2:2 * (r + Hs) - 2]
                vb = rb[k].reshape(tall.B, -1, short.OH, short.OW)[:, :, 2:2 * Hs - 2]
                assert torch.equal(va, vb), (tall.id, k)


def test_replayed_exponents():
    """U1, U2 of a hand-made case: the constants of layer_consts"""
    c = FC.StageCase(64, True, False, 1, 2, 32)
    t = c.tensors()
    (e1, e2), = FC.replay_exps(c, t)
    fir = FC.FIR.double().abs()
    gain = max(float(fir[0::2, 0::2].sum()), float(fir[0::2, 1::2].sum()), float(fir[1::2, 0::2].sum()), float(fir[1::2, 1::2].sum()))
    u1 = FC.GAIN * gain * float(t["y"].abs().max()) + FC.GAIN * (0.3 * float(t["n1"].abs().max()) + float(t["b1"].abs().max()))
    assert 2.0 ** 14 <= u1 * 2.0 ** -e1 < 2.0 ** 15
    u2 = FC.GAIN * 8.0 * u1 + FC.GAIN * (abs(FC.NW2) * float(t["n2"].abs().max()) + float(t["b2"].abs().max()))
    assert 2.0 ** 14 <= u2 * 2.0 ** -e2 < 2.0 ** 15
    assert FC.replay_exps(c, t, ranged=False) == [(0, 0)]
    # the bounds U1, U2 hold for the reference's act1 and out2: no half overflows fp16
    for case in FC.CASES:
        for gs in FC.SPLIT_SCALES:
            tt = case.tensors(gs)
            r = FC.stage_ref(case, tt, F64)
            for b, (x1, x2) in enumerate(FC.replay_exps(case, tt)):
                assert float(r["act1"][b].abs().max()) * 2.0 ** -x1 < 2.0 ** 15
                assert float(r["out2"][b].abs().max()) * 2.0 ** -x2 < 2.0 ** 15
        # the unranged run (gs = 1, exponents 0): fp16's largest number is 65504
        r = FC.stage_ref(case, case.tensors(), F64)
        assert float(r["act1"].abs().max()) < 2.0 ** 15 and float(r["out2"].abs().max()) < 2.0 ** 15
