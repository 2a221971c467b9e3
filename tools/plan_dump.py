"""Which route every decoder layer of a plan takes, and the launches the one-call forward makes of it.

    python tools/plan_dump.py [--res 1024] [--depth 2] [--batch 1] [--precision fp32] [--nerf-size 64] [--off KNOB ...] [--json]

The table lists every layer with its tags, then the step list the forward enqueues (cips3d_decoder_steps).  --json prints one
object instead: the layer list, the options the route was decided under, the flags, the ToRGB slot count and the decoder mark
timeline (hip.DecoderMarks: kind, Cin, Cout, H per launch) of ONE forward.  That form reads nothing but the plan struct, the
knobs of plan.py and the marks, so it records a commit that has no step list as well: tests/golden/decoder_routes.json is made
of it.  --off names knobs of plan.py to switch off (CHAIN_STAGES, FLAT_STAGES, PLANES_RUN, PLANES16_RUN)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import cips_3dplusplus_amd as pkg
from cips_3dplusplus_amd import _lib, configs, hip, plan as plan_mod
from cips_3dplusplus_amd.camera import Camera

KNOBS = ("CHAIN_STAGES", "FLAT_STAGES", "PLANES_RUN", "PLANES16_RUN")
N_SAMPLES = 8


def build(res, depth, batch, precision, nerf_size, off=()):
    """(generator, plan, marks) of one forward of this configuration, with the knobs in `off` switched off while the plan is built."""
    saved = {k: getattr(plan_mod, k) for k in KNOBS}
    for k in off:
        setattr(plan_mod, k, False)
    try:
        dev = "cuda"
        G = pkg.build_generator(configs.ffhq_G_cfg(res, depth), dev, seed=0)
        G.set_precision(precision)
        e, f, n, fa, _ = Camera.generate_camera_params(nerf_size, dev, locations=torch.zeros(batch, 2, device=dev))
        zs = [torch.randn(batch, 256, device=dev), torch.randn(batch, 256, device=dev)]
        marks = hip.DecoderMarks(96)
        hip.DECODER_MARKS = marks
        G(zs=zs, cam_poses=e, focals=f, img_size=nerf_size, near=n, far=fa,
          nerf_cfg=dict(N_samples=N_SAMPLES, perturb=False, static_viewdirs=False))
        torch.cuda.synchronize()
        pl = G._forward_plan(batch, nerf_size, N_SAMPLES, False)
    finally:
        for k, v in saved.items():
            setattr(plan_mod, k, v)
    return G, pl, marks


def record(res, depth, batch, precision, nerf_size, off=()):
    """The --json object of one configuration."""
    _, pl, marks = build(res, depth, batch, precision, nerf_size, off)
    p = pl.plan
    layers = [p.layers[i] for i in range(p.n_dec_layers)]
    return {"name": f"ffhq{res}_d{depth}_b{batch}_{precision}_s{nerf_size}" + "".join(f"_no_{k.lower()}" for k in off),
            "layers": [[L.kind, L.Cin, L.Cout, L.H, L.W] for L in layers],
            # mode: which arithmetic the decoder runs: 0 = plain fp32, 1 = split-fp16, 2 = bf16
            "options": dict(B=p.B, nerf_res=nerf_size, mode=2 if p.decoder_bf16 else (1 if p.range_ws else 0),
                            **{k.lower(): int(k not in off) for k in KNOBS}),
            "flags": [L.flags for L in layers], "rgb_part_slots": int(p.rgb_part_slots), "u8_capable": bool(pl.u8_capable),
            # (the two START marks in front are the timeline's own; launches follow)
            "marks": [[marks.info[4 * k + j] for j in range(4)] for k in range(marks.count.value) if marks.info[4 * k] != 0]}


def describe_step(s):
    forms = " ".join(name for bit, name in _lib.STEP_FORMS.items() if s.form & bit)
    what = f"{_lib.STEP_KINDS[s.kind]:12s} layer {s.layer:2d}  {forms}"
    if _lib.STEP_KINDS[s.kind] == "flush":
        return what + f"  {s.slot} slots of ToRGBs {list(s.bias_layer[:s.n_bias])} @ {s.H}"
    return what + (f"  slot {s.slot}" if s.form & 32 else "") + f"  mark {tuple(s.mark)}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--nerf-size", type=int, default=64)
    ap.add_argument("--off", nargs="*", default=[], choices=KNOBS)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    if a.json:
        print(json.dumps(record(a.res, a.depth, a.batch, a.precision, a.nerf_size, a.off)))
        return
    _, pl, _ = build(a.res, a.depth, a.batch, a.precision, a.nerf_size, a.off)
    kinds = {0: "conv", 1: "conv(up)", 2: "torgb", 3: "torgb(up)"}
    for i, li in enumerate(pl._layer_info):
        tags = [k for k in ("planes_in", "planes_out", "p16", "split", "split16", "chained", "flat_head") if li.get(k)]
        print(f"{i:2d} {kinds[li['kind']]:10s} {li['Cin']:4d} -> {li['Cout']:4d} @ {li['H']:4d}  {' '.join(tags)}")
    print("u8_capable", pl.u8_capable, " out_res", pl.out_res)
    print("steps:")
    for s in pl.steps():
        print("  " + describe_step(s))


if __name__ == "__main__":
    main()
