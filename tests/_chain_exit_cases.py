"""Cases of tests/test_gpu_chain_exits.py and of the generator of its fixtures (tests/golden/chain_exits/make_chain_exits.py): every
compiled form of chain_gemm_kernel (csrc/chain.hip: the chain_forms table -- exit x epilogue x fold x range workspace x riding
fold, for both tiles of the split-fp16 kernel and for the planes16 kernel) at the smallest shapes that reach its branches, the
seeded inputs of a case, the launch, and what of its results is kept.

A fixture holds, per result array, the sha256 of its bytes and -- up to FULL_BYTES -- the bytes themselves (larger arrays: every
SAMPLE_STEP-th 32-bit word), so that a mismatch can be located; the comparison is bit for bit either way.
"""
import hashlib

import numpy as np
import torch

FULL_BYTES = 160 * 1024
SAMPLE_STEP = 61


class ExitCase:
    def __init__(self, kernel, B, Cin, Cout, HW, exit, epi=True, noise="shared", fold=False, ranged=True, pmax_in=True, hint=False,
                 ride=False, form=""):
        """kernel "split" | "p16"; exit "planes" | "planes16" | "fp32" | "bf16"; noise "shared" | "per_sample" | None (epi only);
        ranged: the input planes carry exponents (the range workspace is handed over); pmax_in: ... and patch maxima; hint:
        cips3d_range.half_chip; form: the row of chain_forms the launch takes (documentation)"""
        self.kernel, self.B, self.Cin, self.Cout, self.HW, self.exit = kernel, B, Cin, Cout, HW, exit
        self.epi, self.noise, self.fold = epi, (noise if epi else None), fold
        self.ranged, self.pmax_in, self.hint, self.ride, self.form = ranged and kernel == "split", pmax_in, hint, ride, form

    @property
    def id(self):
        sw = ("" if self.epi else "-ep0") + {"shared": "", "per_sample": "-nzB", None: "-nonoise"}[self.noise if self.epi else "shared"] + \
            ("-fold" if self.fold else "") + ("-ride" if self.ride else "") + ("-hint" if self.hint else "")
        rg = "" if self.kernel == "p16" else ("-rg" + ("" if self.pmax_in else "nopm") if self.ranged else "-raw")
        return f"{self.kernel}{rg}-B{self.B}-i{self.Cin}-o{self.Cout}-HW{self.HW}-{self.exit}{sw}"

    @property
    def wide(self):
        """the 128-row tile: the hint inside the launcher's window (192 < 64-row tiles <= 256)"""
        t = self.B * (self.Cout // 64) * ((self.HW + 127) // 128)
        return self.ranged and self.hint and self.Cout % 128 == 0 and 192 < t <= 256


S, P = "split", "p16"
CASES = [
    # ---- split-fp16 planes, 64 x 128 tiles: a row of the table each, then what the generic form takes
    ExitCase(S, 1, 64, 64, 128, "planes", form="planes epi noise ranged"),
    ExitCase(S, 2, 64, 128, 192, "planes", noise="per_sample", fold=True, pmax_in=False, form="planes epi noise fold ranged"),
    ExitCase(S, 1, 256, 512, 128, "planes", fold=True, hint=True, form="planes epi noise fold ranged (hint outside its window)"),
    ExitCase(S, 1, 128, 64, 192, "planes", fold=True, ranged=False, form="generic: planes without the workspace"),
    ExitCase(S, 2, 128, 128, 128, "planes", ranged=False, form="generic"),
    ExitCase(S, 1, 64, 64, 128, "planes", noise=None, form="generic: no noise map"),
    ExitCase(S, 1, 64, 128, 192, "planes", epi=False, form="generic: planes without the epilogue"),
    ExitCase(S, 1, 64, 64, 192, "fp32", form="fp32 epi noise ranged"),
    ExitCase(S, 2, 128, 64, 128, "fp32", fold=True, form="fp32 epi noise fold ranged"),
    ExitCase(S, 1, 64, 128, 192, "fp32", fold=True, ranged=False, form="fp32 epi noise fold, no workspace"),
    ExitCase(S, 2, 64, 64, 128, "fp32", noise="per_sample", ranged=False, form="fp32 epi noise, no workspace"),
    ExitCase(S, 1, 128, 128, 192, "fp32", epi=False, hint=True, form="fp32 ranged (the low-resolution GEMM)"),
    ExitCase(S, 1, 64, 64, 128, "fp32", epi=False, ranged=False, form="fp32, no workspace"),
    ExitCase(S, 1, 64, 64, 192, "fp32", epi=False, ride=True, form="fp32 ranged ride"),
    ExitCase(S, 2, 64, 64, 192, "bf16", epi=False, form="generic: bf16 NCHW"),
    ExitCase(S, 1, 64, 128, 128, "bf16", epi=False, ranged=False, form="generic: bf16 NCHW"),
    ExitCase(S, 1, 128, 64, 192, "bf16", fold=True, form="generic: bf16 NCHW with the epilogue and the fold"),
    ExitCase(S, 1, 64, 64, 128, "bf16", fold=True, ranged=False, form="generic"),
    # ---- 64^2, 256 -> 512: the one shape here inside the half-chip window (256 64-row tiles); eight ToRGB slots of four 16-row tiles
    ExitCase(S, 1, 256, 512, 4096, "planes", fold=True, hint=True, form="128 x 128: planes epi noise fold ranged"),
    ExitCase(S, 1, 256, 512, 4096, "planes", fold=True, hint=False, form="64 x 128: planes epi noise fold ranged"),
    # ---- planes16 (bf16 mode)
    ExitCase(P, 1, 64, 64, 128, "planes16", form="planes16 epi noise"),
    ExitCase(P, 2, 128, 64, 192, "planes16", noise="per_sample", fold=True, form="planes16 epi noise fold"),
    ExitCase(P, 1, 64, 128, 192, "fp32", form="fp32 epi noise"),
    ExitCase(P, 1, 64, 128, 128, "fp32", fold=True, form="fp32 epi noise fold"),
    ExitCase(P, 2, 64, 64, 128, "fp32", epi=False, form="fp32"),
    ExitCase(P, 1, 128, 128, 192, "bf16", epi=False, form="bf16"),
    ExitCase(P, 1, 64, 64, 128, "planes16", epi=False, form="generic: planes16 without the epilogue"),
    ExitCase(P, 1, 64, 64, 192, "bf16", fold=True, form="generic: bf16 NCHW with the epilogue and the fold"),
]
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS)


def inputs(case):
    """the seeded CPU tensors of a case (never modified)"""
    B, Cin, Cout, HW = case.B, case.Cin, case.Cout, case.HW
    g = torch.Generator().manual_seed(7919 + 31 * B + 17 * Cin + 13 * Cout + HW)
    # pixel blocks and samples of different sizes: the exponents of the blocks differ
    x = torch.randn(B, Cin, HW, generator=g) * (1.0 + 3.0 * torch.rand(B, Cin, 1, generator=g))
    x = x * (2.0 ** (3 * (torch.arange(HW) // 128 % 3)).float()).reshape(1, 1, HW) * (4.0 ** torch.arange(B).float()).reshape(B, 1, 1)
    t = dict(x=x, W=torch.randn(1, Cout, Cin, 1, 1, generator=g), s=1.0 + 0.4 * (2.0 * torch.rand(B, Cin, generator=g) - 1.0),
             bias=0.5 * torch.randn(Cout, generator=g), w_rgb=torch.randn(B, 3, Cout, generator=g) / Cout ** 0.5,
             noise=torch.randn(B if (case.noise == "per_sample" and B > 1) else 1, 1, HW, generator=g),
             noise_w=torch.tensor([0.37]))
    if case.ride:
        t.update(ride_part=torch.randn(5, 1, 3, 260, generator=g), ride_bias=torch.randn(2, 3, generator=g),
                 ride_skip=torch.randn(1, 3, 260, generator=g))
    return t


def inputs_digest(t):
    h = hashlib.sha256()
    for k in sorted(t):
        h.update(k.encode())
        h.update(t[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def run(case, t, hip, dev="cuda"):
    """one launch of the case through the loaded library; dict name -> device tensor of everything the launch wrote"""
    cu = lambda v: v.to(dev)      # noqa: E731
    B, Cin, Cout, HW = case.B, case.Cin, case.Cout, case.HW
    split = case.kernel == "split"
    wm = hip.modulate_weights(cu(t["W"]), cu(t["s"]), Cin, B, Cout, Cin, 1, 1.0 / Cin ** 0.5, True, True, split=split, bf16=not split)
    x4 = cu(t["x"]).reshape(B, Cin, 1, HW)
    kw = dict(epilogue=1 if case.epi else 0)
    if case.epi:
        kw.update(bias=cu(t["bias"]))
        if case.noise:
            kw.update(noise=cu(t["noise"]), noise_w=cu(t["noise_w"]))
    out = {}
    if case.fold:
        part = torch.full((Cout // 64, B, 3, HW), float("nan"), device=dev)
        kw.update(rgb_w=cu(t["w_rgb"]), rgb_part=part)
        out["rgb_part"] = part
    if not split:
        y, _ = hip.modconv1x1_planes16(hip.to_planes16(x4), wm, Cout, HW, case.exit, **kw)
        out["out"] = y
        return out
    xp = hip.to_planes(x4, ranged=case.ranged)
    if case.ranged and not case.pmax_in:
        xp.cips3d_pmax = None
    if case.ranged and case.exit != "planes":
        out["amax"] = torch.zeros(B, hip.amax_floats(), device=dev)
        kw.update(out_amax=out["amax"])
    if case.ride:
        out["ride"] = torch.full((1, 3, 260), float("nan"), device=dev)
        rb = cu(t["ride_bias"])
        kw.update(ride=dict(part=cu(t["ride_part"]), biases=[rb[0].contiguous(), rb[1].contiguous()], skip=cu(t["ride_skip"]), out=out["ride"]))
    y = hip.modconv1x1_planes(xp, wm, Cout, HW, case.exit, half_chip=case.hint, **kw)
    out["out"] = y
    if case.ranged and case.exit == "planes":
        out["out_exp"], out["out_pmax"] = y.cips3d_exp, y.cips3d_pmax
    return out


def raw_bytes(tensor):
    return tensor.detach().contiguous().cpu().view(torch.uint8).reshape(-1).numpy()


def record(results):
    """the fixture entries of a launch's results: <name>.sha256 (uint8[32]), <name>.bytes (all of them, or <name>.sample)"""
    fx = {}
    for k, v in results.items():
        b = raw_bytes(v)
        fx[f"{k}.sha256"] = np.frombuffer(hashlib.sha256(b.tobytes()).digest(), dtype=np.uint8)
        fx[f"{k}.nbytes"] = np.int64(b.size)
        if b.size <= FULL_BYTES:
            fx[f"{k}.bytes"] = b
        else:
            fx[f"{k}.sample"] = b.view(np.uint32)[::SAMPLE_STEP].copy()
    return fx
