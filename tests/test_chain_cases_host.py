"""The checks and cases of tests/_chain_cases.py, run without a GPU on every case test_gpu_chain.py runs and at every data scale:
(a) an fp32 emulation of the kernel built from the header's definitions (torch fp16 / bf16 casts, one fp32 matmul over the 3 K
products, the exponent replay) passes every check of check_outputs: a correct implementation passes; (b) every subtly wrong
emulation fails them at the cases REJECTED_BY names: the GPU test has teeth; (c) every case sits in the regime it is listed for
and the list covers what the issue sets; (d) no replayed bound lies within 2^-20 of a power of two; (e) the hand-built planes hold
their block maxima in [2^5, 2^15); (f) planes_of / planes_value round-trip to 2^-22 |x| + 2^-25 2^e.

Which cases reject which mutant (REJECTED_BY: a predicate on the case; every case that lists the mutant and satisfies the predicate
must reject it at every scale, and test_every_mutant_is_rejected_somewhere asserts that there is at least one such case):
    drop_wl_xh, drop_wh_xl, swap_planes   split cases of at most 3 stages (Cin <= 192).  The dropped product is 2^-11 of the result
                     term by term with mixed signs, sqrt(K) of them; the bound charges gamma_(3 K + 8) on K terms of one sign,
                     K^2 against sqrt(K): from 8 stages on the worst-case bound is above a lost lo product.  This is the
                     price of a bound that holds for any order of the additions, as in _gemm1x1_cases.py.
    lo_twice         every planes exit                        exp_kept       every ranged split case
    exp_neighbour    every ranged case of two or more blocks  exp_sample0    every ranged case of two or more samples whose
                     later samples are not all zero (rng "e");  drop_wh_xl and lo_twice not on raw halves at 2^-20, whose
                     lo planes are all zero;  noise_past_hw not under the spike of rng "e", which is the sample's maximum
    noise_other      every case with per-sample noise         bias_row16, slope_sign, gain_before_bias   every case with an epilogue
    noise_past_hw    every ranged fp32 exit with per-sample noise and HW % 128 != 0 (the amax check)
    fold_tiles       every fold of two or more slots (the per-slot check: the slots' sum does not see it)
"""
import pytest
import torch

import _chain_cases as CC

F32, F64 = torch.float32, torch.float64
CASES = CC.CHAIN_CASES
ids = [c.id for c in CASES]

always = lambda c, gs: True      # noqa: E731
short = lambda c, gs: c.Cin <= 192      # noqa: E731
REJECTED_BY = {
    "drop_wl_xh": short, "drop_wh_xl": lambda c, gs: short(c, gs) and not (c.rng == "d" and gs < 1.0), "swap_planes": short,
    "lo_twice": lambda c, gs: not (c.rng == "d" and gs < 1.0), "exp_kept": always, "exp_neighbour": always,
    "exp_sample0": lambda c, gs: c.rng != "e", "noise_other": always, "noise_past_hw": lambda c, gs: c.rng != "e", "bias_row16": always, "slope_sign": always,
    "gain_before_bias": always, "fold_tiles": always,
}


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_checks_admit_the_emulation_and_reject_the_mutants(case):
    for gs in case.scales:
        t = case.tensors(gs)
        ops = case.operands(t)
        ref = CC.reference(case, t, ops)
        for k in ("e_v", "e_out"):
            assert bool(torch.isfinite(ref[k]).all()) and bool((ref[k] >= 0).all()), (case.id, k)
        ratios = CC.check_outputs(case, t, ops, ref, CC.planes_emulated(case, t, ops))
        print(f"{case.id} gs={gs}: " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        for m in case.mutants():
            rejected = not CC.passes(case, t, ops, ref, CC.planes_emulated(case, t, ops, m))
            if REJECTED_BY[m](case, gs):
                assert rejected, f"{case.id} gs={gs}: the mutant `{m}` passes every check"


def test_every_mutant_is_rejected_somewhere():
    assert set(REJECTED_BY) == set(CC.MUTANTS)
    for m in CC.MUTANTS:
        assert any(m in c.mutants() and all(REJECTED_BY[m](c, gs) for gs in c.scales) for c in CASES), m


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_case_is_in_its_regime(case):
    got = case.regime()
    for k, v in case.expect.items():
        assert got[k] == v, f"{case.id}: {k} is {got[k]}, the case is listed for {v}"
    assert case.Cin % 64 == 0 and case.Cout % 64 == 0 and 16 <= case.HW <= 6400 and case.Cin <= 576
    assert case.rng != "e" or case.B >= 2
    assert not (case.split and case.rng not in ("b", "d") and case.exit == "planes" and case.Cin > 512)   # refused with patch maxima


def test_the_cases_cover_what_the_issue_sets():
    sp, p16 = [c for c in CASES if c.split], [c for c in CASES if not c.split]
    assert {1, 2, 3, 8, 9} <= {c.regime()["nstage"] for c in sp} and {1, 2, 3, 4, 8} <= {c.regime()["nstage"] for c in p16}
    for cs in (sp, p16):
        assert {64, 128, 192, 256} <= {c.Cout for c in cs}
        assert {16, 60, 64, 65, 128, 129, 200, 250} <= {c.HW for c in cs}
        assert {1, 2, 3} <= {c.B for c in cs}
        assert {None, "shared", "per_sample"} <= {c.noise for c in cs if c.epilogue == 1} and any(c.epilogue == 0 for c in cs)
        assert any(c.fold and c.epilogue == 0 for c in cs) and any(c.fold and c.epilogue == 1 for c in cs)
        kinds = {"one_ragged_half", "one_half", "two_halves_second_ragged", "full"}
        exits = {"planes", "fp32", "bf16"} if cs is sp else {"planes16", "fp32", "bf16"}
        assert {(c.regime()["kind"], c.exit) for c in cs} >= {(k, e) for k in kinds for e in exits}
        # a ragged half behind a full block, and alone
        assert any(c.regime()["kind"] == "one_ragged_half" and c.nblk == 2 for c in cs) and any(c.HW < 64 for c in cs)
    assert {"a", "b", "c", "d", "e"} == {c.rng for c in sp}
    for r in "abcde":
        assert any(c.rng == r and c.exit == "planes" for c in sp) and any(c.rng == r and c.exit == "fp32" for c in sp)
    assert any(c.Cin == 576 and c.rng == "b" and c.exit == "planes" for c in sp)
    assert any(c.lc == 2 for c in sp)
    half = [c for c in sp if c.regime()["form"] == "128x128"]
    assert {(c.B, c.Cin, c.Cout, c.HW) for c in half} == {(3, 64, 128, 33 * 128 + 37), (1, 128, 256, 49 * 128 + 65)}
    assert any(c.fold for c in half) and any(c.ride for c in half) and all(192 < c.regime()["tiles64"] <= 256 for c in half)
    near = {c.regime()["tiles64"] for c in sp if c.hint and c.regime()["form"] == "64x128"}
    assert near == {192, 258}
    assert set(CC.SPLIT_SCALES) == {1.0, 2.0 ** -20, 2.0 ** 17}


@pytest.mark.parametrize("case", [c for c in CASES if c.ranged], ids=[c.id for c in CASES if c.ranged])
def test_hand_built_planes_and_the_exponent_replay(case):
    for gs in case.scales:
        t = case.tensors(gs)
        ops = case.operands(t)
        e = t["exps"]
        # exponents: 2^12 and more between neighbouring blocks, 2^9 and more between samples
        if case.nblk > 1 and case.rng != "e":
            assert int((e[:, 1:] - e[:, :-1]).abs().min()) >= 12
        if case.B > 1 and case.rng != "e":
            assert int((e[1:] - e[:-1]).abs().min()) >= 9
        stored = (ops["xh"].double() + ops["xl"].double()).abs()
        assert bool((stored < 2.0 ** 15).all())
        for j in range(case.nblk):
            m = stored[:, :, j * CC.BLOCK:(j + 1) * CC.BLOCK].amax((1, 2))
            live = m > 0 if case.rng == "e" else torch.ones_like(m, dtype=torch.bool)
            assert bool(((m >= 2.0 ** 5) & (m < 2.0 ** 15))[live].all()), (case.id, j, m.tolist())
        if case.rng == "e":
            assert float(t["x"][1].abs().max()) == 0.0
            a = t["x"][0, :, :CC.BLOCK].abs().reshape(-1)
            assert float(a.max()) >= 2.0 ** 30 * float(a.sort().values[-2])
        # the round trip of the format
        back = CC.planes_value(ops["p"], e)
        pe = CC.per_pixel(e, case.HW)
        assert bool(((back - t["x"].double()).abs() <= 2.0 ** -22 * t["x"].double().abs() + 2.0 ** -25 * pe).all())
        if ops["pmax"] is not None:
            exact = CC.patch_maxima(back)
            assert torch.equal(ops["pmax"].double(), exact * (4.0 if case.rng == "c" else 1.0))
        if not case.tracked:
            continue
        # the bound the exponent is taken from is not within 2^-20 of a power of two: the replay is unambiguous
        _, bound, layer = CC.replayed_exponents(case, ops)
        nz = bound[bound > 0]
        mant = nz / torch.pow(2.0, torch.floor(torch.log2(nz)))
        assert bool(((mant - 1.0 > 2.0 ** -20) & (2.0 - mant > 2.0 ** -19)).all()), (case.id, gs)
        assert bool((layer <= bound * (1 + 2.0 ** -20)).all())


def test_planes16_format_round_trip():
    x = torch.randn(2, 32, 70, generator=torch.Generator().manual_seed(3))
    p = CC.planes16_of(x)
    assert p.shape == (2, 4, 70, 8) and p.dtype == torch.bfloat16
    assert torch.equal(CC.planes16_value(p), CC.bf16_round(x).double())
    assert p[1, 2, 69, 5] == x[1, 21, 69].to(torch.bfloat16)
    q = CC.planes_of(x, None)
    assert q.shape == (2, 4, 2, 70, 8) and q[1, 2, 0, 69, 5] == x[1, 21, 69].to(torch.float16)
    pm = CC.patch_maxima(x)
    assert pm.shape == (2, 2, 2) and float(pm[1, 1, 1]) == float(x[1, 16:, 64:].abs().max())


def test_split_fragment_unpacking_matches_unpack_split():
    g = torch.Generator().manual_seed(5)
    h = torch.randn(2 * 32 * 64 * 2, generator=g).to(torch.float16)
    packed = h.view(torch.float32)
    wh, wl = CC.unpack_split_halves(packed, 2, 32, 64)
    assert torch.equal((wh + wl) / 256.0, CC.unpack_split(packed, 2, 32, 64, False))
