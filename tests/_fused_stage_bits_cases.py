"""Cases of tests/test_gpu_fused_stage_bits.py and of the generator of its fixtures (tests/golden/fused_stage_bits/
make_fused_stage_bits.py): every compiled form of fused_up_conv_kernel (csrc/fused_stage.hip: the stage_forms table -- per base
shape, precision and kind the forms the shipped generators launch, plus one generic form that reads its features at run time) at
the smallest shapes that reach its branches, the launch through the C entry point, and what of its results is kept.

Shapes, data and operands are those of tests/_fused_stage_cases.py (FC): its CASES in the five runs fp32 / bf16 / bf16 storage /
split with and without range tracking, its YB_CASES and U8_CASES, and -- what those lists do not hold -- the exact feature set of
the launches the shipped generators make (ROWS below: nine shapes x four precisions; 28 of the 36 have a row of stage_forms, the flat
ones in plain bf16 and exact fp32 run on the generic forms): both noise maps per sample, ToRGB, the skip image (FIR-up-sampled;
output-sized for a flat stage), no out2, B = 2 with sample 0 at 2^9 times sample 1, the chained stages measuring max |y_next| except C = 64, which
publishes its bound (next_gain = sqrt C), the last stage (C = 32) with an fp32 and with a uint8 image; each row once where the
tile row length tiles_x is a power of two (the kernel shifts) and once where it is not (it multiplies by a reciprocal).

A fixture holds, per result array, the sha256 of its bytes, their count and -- up to FULL_BYTES -- the bytes themselves (larger
arrays: every k-th 32-bit word, k = ceil(words / SAMPLE_WORDS)), so that a mismatch can be located; the comparison is bit for bit
either way.  Outputs are preset (-77.5; uint8: 77): what a launch does not write is part of the bytes.
"""
import ctypes as C
import hashlib
import math

import numpy as np
import torch

import _fused_stage_cases as FC

FULL_BYTES = 2048
SAMPLE_WORDS = 384
RUNS = ("fp32", "bf16", "bf16s", "split", "split-raw")      # bf16s: bf16 storage of y_lo / y_next; split-raw: no range workspace


class BitsCase:
    def __init__(self, stage, run, u8=False, bound=False, form="generic"):
        assert run in RUNS and not (bound and not (run == "split" and stage.chained)) and not (u8 and not stage.rgb)
        self.stage, self.run, self.u8, self.bound, self.form = stage, run, u8, bound, form

    @property
    def id(self):
        return f"{self.run}-{self.stage.id}" + ("-u8" if self.u8 else "") + ("-bound" if self.bound else "")


def _row_cases():
    """the launches the rows of stage_forms are compiled for: (C, chained, flat, u8) x the four precisions x two tiles_x"""
    P = "per_sample"
    out = []
    for C_, chained, flat, u8 in ((256, True, False, False), (128, True, False, False), (64, True, False, False), (32, False, False, False),
                                  (32, False, False, True), (128, True, True, False), (64, True, True, False), (32, False, True, False),
                                  (32, False, True, True)):
        if flat:
            shapes = ((8, 128), (8, 192))                                                # 2 x 64 tiles: tiles_x = 2 | 3
        elif C_ == 256:
            shapes = ((4, 64), (6, 96))                                                  # 2 x 32 tiles: tiles_x = 4 | 6
        else:
            shapes = ((4, 128), (4, 96))                                                 # 2 x 64 tiles: tiles_x = 4 | 3
        for H, W in shapes:
            st = FC.StageCase(C_, chained, flat, 2, H, W, n1=P, n2=P, skip="plain" if flat else "fir", want_out2=False)
            for run in ("fp32", "bf16", "bf16s", "split"):
                out.append(BitsCase(st, run, u8=u8, bound=(run == "split" and chained and C_ == 64),
                                    form=f"row: C{C_}{'c' if chained else 'u'}{' flat' if flat else ''}{' u8' if u8 else ''}"))
    return out


ROWS = _row_cases()
CASES = ([BitsCase(c, r) for r in RUNS for c in FC.CASES] + [BitsCase(c, "bf16s") for c in FC.YB_CASES if c.id not in {k.id for k in FC.CASES}] +
         [BitsCase(c, r, u8=True) for r in ("fp32", "bf16", "bf16s", "split") for c in FC.U8_CASES] + ROWS)
IDS = [c.id for c in CASES]
assert len(set(IDS)) == len(IDS), [i for i in IDS if IDS.count(i) > 1]


def tiles_x(case):
    return case.stage.OW // case.stage.TW


def inputs(case):
    """the seeded CPU tensors of a case (never modified); bf16 storage: y_lo rounded to bf16 once, here"""
    t = case.stage.tensors()
    if case.run == "bf16s":
        t = dict(t)
        t["y"] = t["y"].to(torch.bfloat16)
    return t


def inputs_digest(t):
    h = hashlib.sha256()
    for k in sorted(t):
        if t[k] is not None:
            h.update(k.encode())
            h.update(raw_bytes(t[k]).tobytes())
    return h.hexdigest()


def run(case, t, hip, _lib, dev="cuda"):
    """one launch of the case through cips3d_fused_up_conv_next of the loaded library; dict name -> device tensor of everything the
    launch can write (out2, rgb, y_next, the next_amax array)"""
    st = case.stage
    B, Cc, H, W, OH, OW = st.B, st.C, st.H, st.W, st.OH, st.OW
    lib = _lib.load()
    cu = lambda v: None if v is None else v.to(dev).contiguous()      # noqa: E731
    split, bf16 = case.run.startswith("split"), case.run in ("bf16", "bf16s")
    ones = torch.ones(B, Cc, device=dev)

    def mod(Wm, flags):
        out = torch.empty(B * Wm.shape[0] * Cc, device=dev)
        _lib.check(lib.cips3d_modulate_weights(cu(Wm).data_ptr(), ones.data_ptr(), Cc, out.data_ptr(), B, Wm.shape[0], Cc, 1, 1.0, flags,
                                               hip.stream_ptr()), "cips3d_modulate_weights")
        return out

    s16 = hip.MOD_SPLIT16 if split else 0
    wm2 = mod(t["W2"], hip.MOD_PACKED | s16)
    wmn = mod(t["Wn"], hip.MOD_PACKED | hip.MOD_CHAINED | s16) if st.chained else None
    wrgb = mod(t["Wrgb"], 0) if st.rgb else None
    y, fir = cu(t["y"]), None if st.flat else cu(FC.FIR)
    n1, n2, b1, b2, skip = cu(t["n1"]), cu(t["n2"]), cu(t["b1"]), cu(t["b2"]), cu(t["skip"])
    brgb = cu(t["brgb"]) if st.rgb else None
    nw1 = torch.tensor([FC.NW1], device=dev) if n1 is not None else None
    nw2 = torch.tensor([FC.NW2], device=dev) if n2 is not None else None
    res = {}
    if st.want_out2:
        res["out2"] = torch.full((B, Cc, OH, OW), -77.5, device=dev)
    if st.rgb:
        res["rgb"] = torch.full((B, 3, OH, OW), 77, device=dev, dtype=torch.uint8) if case.u8 else torch.full((B, 3, OH, OW), -77.5, device=dev)
    if st.chained:
        res["y_next"] = torch.full((B, Cc // 2, OH, OW), -77.5, device=dev, dtype=y.dtype)
    rg = keep = None
    if case.run == "split":
        lc1 = hip.range_consts(B, b1, nw1, 0.0, fir=fir, noise=n1)
        lc2 = hip.range_consts(B, b2, nw2, Cc ** 0.5, noise=n2)
        if st.chained:
            res["next_amax"] = hip.new_amax(B, dev)
        rg, keep = hip._range(x_amax=hip.absmax(y), lconst=lc1, lconst2=lc2, next_amax=res.get("next_amax"))
        rg.next_gain = math.sqrt(Cc) if case.bound else 0.0
    flags = ((1 if st.skip == "fir" else 0) | (hip.GEMM_BF16 if bf16 else 0) | (hip.Y_BF16 if case.run == "bf16s" else 0) |
             (hip.GEMM_SPLIT if split else 0) | (hip.STAGE_FLAT if st.flat else 0) | (hip.RGB_U8 if case.u8 else 0))
    p = lambda v: None if v is None else v.data_ptr()      # noqa: E731
    bs = lambda nz: OH * OW if (nz is not None and nz.shape[0] == B and B > 1) else 0      # noqa: E731
    _lib.check(lib.cips3d_fused_up_conv_next(p(y), p(fir), p(n1), bs(n1), p(nw1), p(b1), p(wm2), p(n2), bs(n2), p(nw2), p(b2), p(res.get("out2")),
                                             p(wrgb), p(brgb), p(skip), flags, p(res.get("rgb")), p(wmn), p(res.get("y_next")), B, Cc, H, W,
                                             C.byref(rg) if rg is not None else None, hip.stream_ptr()), "cips3d_fused_up_conv_next")
    torch.cuda.synchronize()
    del keep
    return res


def raw_bytes(tensor):
    return tensor.detach().contiguous().cpu().view(torch.uint8).reshape(-1).numpy()


def sample_step(nbytes):
    return -(-(nbytes // 4) // SAMPLE_WORDS)


def record(results):
    """the fixture entries of a launch's results: <name>.sha256 (uint8[32]), <name>.nbytes, <name>.bytes (all of them) or <name>.sample"""
    fx = {}
    for k, v in results.items():
        b = raw_bytes(v)
        fx[f"{k}.sha256"] = np.frombuffer(hashlib.sha256(b.tobytes()).digest(), dtype=np.uint8)
        fx[f"{k}.nbytes"] = np.int64(b.size)
        if b.size <= FULL_BYTES:
            fx[f"{k}.bytes"] = b
        else:
            fx[f"{k}.sample"] = b.view(np.uint32)[::sample_step(b.size)].copy()
    return fx
