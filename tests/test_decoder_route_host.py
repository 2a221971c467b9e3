"""The decoder's route (csrc/decoder_route.hip) on the CPU: flags, ToRGB slots and the step list against
tests/golden/decoder_routes.json, and the refusals of flags that promise a launch the layers cannot take.

The fixture's "recorded" cases are `tools/plan_dump.py --json` on an MI355X at the commit BEFORE the resolver existed (flags from
plan.py's own decision, marks from a real forward); its "synthetic" cases are that commit's decision block run on hand-made
layer lists (flags and slots only).  Every layer of the synthetic lists is demodulated."""
import ctypes as C
import json
import os

import pytest

from cips_3dplusplus_amd import _lib, plan

E_BADARG, E_UNSUPP = -1, -2
FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_routes.json")))
RECORDED, SYNTHETIC = FIXTURE["recorded"], FIXTURE["synthetic"]
BY_NAME = {c["name"]: c for c in RECORDED + SYNTHETIC}


def layer_array(rows, flags):
    layers = (plan.DecLayer * plan.MAX_DEC)()
    for L, (kind, Cin, Cout, H, W), f in zip(layers, rows, flags):
        L.kind, L.Cin, L.Cout, L.H, L.W, L.flags = kind, Cin, Cout, H, W, f
    return layers


def resolve_flags(case):
    """(flags, slots) of the resolver for a fixture case: the layer list, the options and each layer's DEMOD bit go in."""
    layers = layer_array(case["layers"], [f & _lib.DEC_DEMOD for f in case["flags"]])
    slots = C.c_int64(-1)
    rc = _lib.load().cips3d_decoder_route_flags(C.byref(layers), len(case["layers"]), C.byref(_lib.DecRouteOpts(**case["options"])),
                                                C.byref(slots))
    assert rc == 0
    return [layers[i].flags for i in range(len(case["layers"]))], slots.value


def steps_rc(case, flags, max_steps=_lib.MAX_DEC_STEPS):
    """(return code, steps) of cips3d_decoder_steps for a fixture case's layers with these flags."""
    steps = (_lib.DecStep * _lib.MAX_DEC_STEPS)()
    rc = _lib.load().cips3d_decoder_steps(C.byref(layer_array(case["layers"], flags)), len(case["layers"]), case["options"]["B"],
                                          int(case["options"]["mode"] == 1), case["rgb_part_slots"], steps, max_steps)
    return rc, list(steps[:max(rc, 0)])


def test_fixture_covers_the_cases():
    names = set(BY_NAME)
    for res in (64, 128, 256, 512, 1024):
        for b in (1, 4):
            for prec in ("fp32", "fp32_exact", "bf16", "bf16_storage"):
                assert f"ffhq{res}_d2_b{b}_{prec}_s64" in names
    for res in (256, 1024):
        for knob in ("chain_stages", "flat_stages", "planes_run", "planes16_run"):
            assert f"ffhq{res}_d2_b1_fp32_s64_no_{knob}" in names and f"ffhq{res}_d2_b1_bf16_s64_no_{knob}" in names
    assert any(c["options"]["nerf_res"] != 64 for c in RECORDED)
    assert all("marks" in c and len(c["marks"]) >= 10 for c in RECORDED)
    for stem in ("up_stage_width_refused", "unequal_widths_in_block", "torgb_cin_mismatch", "more_than_fold_max",
                 "ends_in_standalone_torgb", "flat_stage_chained"):
        assert f"{stem}_b1_mode1" in names


@pytest.mark.parametrize("case", RECORDED + SYNTHETIC, ids=lambda c: c["name"])
def test_flags_and_slots_equal_the_fixture(case):
    flags, slots = resolve_flags(case)
    assert flags == case["flags"]
    assert slots == case["rgb_part_slots"]


@pytest.mark.parametrize("case", RECORDED, ids=lambda c: c["name"])
def test_step_marks_equal_the_recorded_timeline(case):
    rc, steps = steps_rc(case, case["flags"])
    assert rc == len(steps) > 0
    assert [list(s.mark) for s in steps if s.mark[0] >= 0] == case["marks"]
    flush = _lib.STEP_KINDS.index("flush")
    for k, s in enumerate(steps):
        # a riding flush has no mark of its own: the low-resolution planes GEMM behind it carries the sum
        if s.kind == flush and s.form & 64:
            assert s.mark[0] < 0 and steps[k + 1].kind == _lib.STEP_KINDS.index("lowres_gemm") and steps[k + 1].form & 1
        else:
            assert s.mark[0] > 0
    assert (steps[-1].kind == _lib.STEP_FUSED_STAGE) == case["u8_capable"]


def test_the_recorded_cases_take_every_route():
    seen = set()
    for case in RECORDED:
        for s in steps_rc(case, case["flags"])[1]:
            seen.add((_lib.STEP_KINDS[s.kind], s.form))
    kinds = {k for k, _ in seen}
    assert kinds == set(_lib.STEP_KINDS)                 # (gemm_fir: the 48^2 feature map, whose 48-pixel rows no fused stage takes)
    assert ("flush", 64) in seen and ("flush", 0) in seen                                        # riding and stand-alone
    assert any(k == "fused_stage" and f & 4 for k, f in seen) and any(k == "fused_stage" and f & 8 for k, f in seen)
    assert any(k == "planes_gemm" and f & 2 for k, f in seen) and any(k == "gemm" and f & 32 for k, f in seen)


@pytest.mark.parametrize("case", SYNTHETIC, ids=lambda c: c["name"])
def test_synthetic_steps(case):
    rc, steps = steps_rc(case, case["flags"])
    assert rc == len(steps) > 0
    assert (steps[-1].kind == _lib.STEP_FUSED_STAGE) == case["u8_capable"]
    name = {k: i for i, k in enumerate(_lib.STEP_KINDS)}
    by_layer = {}                                        # the first launch of every layer that heads one
    for s in steps:
        if s.kind != name["flush"]:
            by_layer.setdefault(s.layer, s)
    if case["name"].startswith("up_stage_width_refused"):
        assert by_layer[2].kind == name["gemm_fir"] and list(by_layer[2].mark) == [6, 512, 512, 64]
        assert by_layer[3].kind == name["gemm"] and by_layer[4].kind == name["torgb"] and by_layer[5].kind == name["lowres_gemm"]
    if case["name"].startswith("unequal_widths_in_block"):
        assert [by_layer[i].kind for i in (2, 3, 4)] == [name["gemm_fir"], name["gemm"], name["torgb"]]
    if case["name"].startswith("torgb_cin_mismatch"):
        assert by_layer[1].kind == name["torgb"] and not by_layer[0].form & 32 and by_layer[2].form & 32
    if case["name"].startswith("more_than_fold_max"):
        # eight ToRGBs join one sum; the ninth conv finds the bias list full: its ToRGB runs alone, behind a flush of the eight
        folds = [s for s in steps if s.form & 32 and s.kind != name["flush"]]
        flushes = [s for s in steps if s.kind == name["flush"]]
        assert len(folds) == 9 and flushes[0].n_bias == _lib.TORGB_FOLD_MAX and flushes[0].layer == 17
        assert by_layer[17].kind == name["torgb"] and flushes[1].n_bias == 1
        per = _lib.load().cips3d_planes_torgb_blocks(128) if case["options"]["mode"] else \
            _lib.load().cips3d_modconv1x1_torgb_blocks(case["options"]["B"], 128, 128, 32 * 32)
        assert [s.slot for s in folds[:8]] == [k * per for k in range(8)] and flushes[0].slot == 8 * per
    if case["name"].startswith("ends_in_standalone_torgb"):
        assert steps[-1].kind == name["torgb"] and steps[-1].form & 16


def _broken(name, layer, bit, layers=None):
    case = dict(BY_NAME[name])
    if layers is not None:
        case["layers"] = layers
    flags = list(case["flags"])
    assert not flags[layer] & bit
    flags[layer] |= bit
    return case, flags


def test_broken_flags_are_refused():
    """Flags that promise a launch the layers cannot take: CIPS3D_E_BADARG, what the forward's loop returned for them."""
    # chained weights on a stage head whose predecessor is no stage that chains: the first up-sampling conv of the 1024 recipe
    case = BY_NAME["ffhq1024_d2_b1_fp32_s64"]
    head = next(i for i, row in enumerate(case["layers"]) if row[0] == 1)
    assert steps_rc(*_broken("ffhq1024_d2_b1_fp32_s64", head, _lib.DEC_CHAINED))[0] == E_BADARG
    # planes into an up-conv that takes GEMM + FIR (C = 512 is no width of the fused stage)
    assert steps_rc(*_broken("up_stage_width_refused_b1_mode1", 2, _lib.DEC_PLANES_IN))[0] == E_BADARG
    # a flat head whose block has unequal widths
    rows = [list(r) for r in BY_NAME["flat_stage_chained_b1_mode1"]["layers"]]
    rows[6][2], rows[7][1] = 32, 32
    case, flags = _broken("flat_stage_chained_b1_mode1", 0, 0, layers=rows)
    assert flags[5] & _lib.DEC_FLAT_HEAD and steps_rc(case, flags)[0] == E_BADARG
    # planes out of a conv whose ToRGB cannot be folded (its Cin is not the conv's Cout)
    assert steps_rc(*_broken("torgb_cin_mismatch_b1_mode1", 0, _lib.DEC_PLANES_OUT))[0] == E_BADARG
    # ... and each of those lists is accepted with the flags the resolver wrote
    for name in ("ffhq1024_d2_b1_fp32_s64", "up_stage_width_refused_b1_mode1", "flat_stage_chained_b1_mode1", "torgb_cin_mismatch_b1_mode1"):
        assert steps_rc(BY_NAME[name], BY_NAME[name]["flags"])[0] > 0


def test_argument_errors():
    lib = _lib.load()
    case = BY_NAME["ffhq256_d2_b1_fp32_s64"]
    n = len(case["layers"])
    assert steps_rc(case, case["flags"], max_steps=3)[0] == E_BADARG
    layers, steps, slots = layer_array(case["layers"], case["flags"]), (_lib.DecStep * _lib.MAX_DEC_STEPS)(), C.c_int64(0)
    opts = _lib.DecRouteOpts(**case["options"])
    assert lib.cips3d_decoder_steps(None, n, 1, 1, 80, steps, len(steps)) == E_BADARG
    assert lib.cips3d_decoder_steps(C.byref(layers), 0, 1, 1, 80, steps, len(steps)) == E_BADARG
    assert lib.cips3d_decoder_steps(C.byref(layers), plan.MAX_DEC + 1, 1, 1, 80, steps, len(steps)) == E_BADARG
    assert lib.cips3d_decoder_steps(C.byref(layers), n, 1, 1, 80, None, 0) == E_BADARG
    assert lib.cips3d_decoder_route_flags(None, n, C.byref(opts), C.byref(slots)) == E_BADARG
    assert lib.cips3d_decoder_route_flags(C.byref(layers), n, None, C.byref(slots)) == E_BADARG
    assert lib.cips3d_decoder_route_flags(C.byref(layers), n, C.byref(opts), None) == E_BADARG
    opts.mode = 3
    assert lib.cips3d_decoder_route_flags(C.byref(layers), n, C.byref(opts), C.byref(slots)) == E_BADARG
    layers[4].kind = 7
    assert lib.cips3d_decoder_steps(C.byref(layers), n, 1, 1, 80, steps, len(steps)) == E_BADARG


def test_forward_refuses_before_it_enqueues():
    """cips3d_generator_forward resolves the route first: a uint8 image from a decoder that ends in a stand-alone ToRGB is
    CIPS3D_E_UNSUPP with nothing enqueued -- the io pointers below point nowhere, and no GPU is needed.  (range_ws is set with
    range_ws_words = 0: the check behind the route's refuses this plan as well, with CIPS3D_E_BADARG.)"""
    lib = _lib.load()
    case = BY_NAME["ends_in_standalone_torgb_b1_mode1"]
    p, io = plan.GeneratorPlan(), plan.ForwardIO()
    p.B, p.n_dec_layers, p.range_ws, p.range_ws_words = 1, len(case["layers"]), 64, 0
    p.rgb_part, p.rgb_part_slots = 64, case["rgb_part_slots"]
    for L, src in zip(p.layers, layer_array(case["layers"], case["flags"])):
        L.kind, L.Cin, L.Cout, L.H, L.W, L.flags = src.kind, src.Cin, src.Cout, src.H, src.W, src.flags
    io.cam_poses = io.focals = io.near_ = io.far_ = io.rgb = io.thumb = io.xyz = io.mask = 64
    io.rgb_is_u8 = 1
    assert lib.cips3d_generator_forward(C.byref(p), C.byref(io), None) == E_UNSUPP
