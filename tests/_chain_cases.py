"""Cases, fp64 references and rounding-error bounds of the chain GEMM on planes (csrc/chain.hip): chain_gemm_kernel in its three
instantiations -- <1,4,2,64,2> (split-fp16 planes, 64 x 128 tiles), <2,4,2,64,2> (the half-chip 128 x 128 form) and <1,4,2,64,3,1>
(one bf16 plane, "planes16") -- and the four converters to_planes / from_planes / to_planes16 / from_planes16.  Shared by
test_chain_cases_host.py (CPU: every check admits an fp32 emulation built from the header's definitions and rejects every mutant;
every case sits in its regime) and test_gpu_chain.py (the kernels).  Imports no GPU code.

Formats (the layout comment at the top of chain.hip), written here in plain torch:
    planes    P[b][C/8][hi|lo][HW][8] fp16 holding x 2^-e, one exponent e per (sample, block of 128 pixels): planes_of / planes_value
    planes16  P16[b][C/8][HW][8] bf16, round to nearest even:                                                 planes16_of / planes16_value
    patch maxima [b][ceil(HW/64)][C/16]: the largest |x| of a (16 channels x 64 pixels) patch:                patch_maxima
The inputs of a case are HAND-BUILT in these formats, so every sample and every pixel block carries an exponent of its own
(13 between neighbouring blocks, 10 between samples: 2^13 and 2^10 apart), whatever a producer kernel would have written.

Reference.  The fp64 GEMM of the STORED operands: x = (xh + xl) 2^e_in from the planes, w = (wh + wl) 2^-8 from the fragments
cips3d_modulate_weights(MOD_PACKED | MOD_SPLIT) wrote (the host test splits a torch modulation instead).  The kernel adds the three
exact fp16 products wl xh + wh xl + wh xh in fp32 and scales by 2^-8 2^e_in (exact), e_in the exponent of the element's OWN
pixel block; it never forms wl xl.  Eight roundings are set aside for the inside of a matrix instruction (_gemm1x1_cases.py):
    e(v) = 2^-8 2^e_in [ sum |wl xl| + gamma_(3 K + 8) sum (|wh xh| + |wh xl| + |wl xh|) ]
planes16: one exact product of the stored bf16 operands per term, e(v) = gamma_(K + 8) sum |w x|.
Epilogue: epilogue_bound of _gemm1x1_cases.py unchanged (the 2^-e' of a planes output rides on the sqrt 2: exact).
Planes exit: the pair hi = fp16(s), lo = fp16(s - hi) of the stored value s = out 2^-e' loses 2^-22 |s| + 2^-25, so the bound grows
by 2^-22 (|out| + e) + 2^-25 2^e', e' the exponent the launch wrote for the block.  bf16 / planes16 exits: no bound -- the RNE
rounding of the fp32 exit of the same launch inputs, bit for bit.
Exponent of a planes output: e' = cips3d_split_exp(fma(c1, m_in 1.000001f, c0)), c1 = max(lc[1], sqrt2 lc[2]), c0 = lc[0], m_in the
largest of the block's 2 x Cin/16 patch maxima (Cin/16 where the block has one 64-pixel half), or 2^(e_in + 15) without patch maxima:
out_exp_replay, the fma in fp64 rounded once.  test_chain_cases_host.py shows that no case's bound lies within 2^-20 of a power
of two, so the replay is unambiguous.
Fold (rgb_part).  A lane folds the 4 rows it holds of a 16-row tile with one fma each, two shuffle additions join the lane quarters,
the four tiles of a 64-row slot are added in tile order onto zero (the scaling back by 2^e' is exact):  k_fold = 4 + 2 + 4 = 10,
the same for the 128-row form, whose two slots hold the bits two 64-row workgroups would have written.  Every SLOT is held to
    gamma_10 sum_(rows of the slot) |w_rgb y|     (+ sum |w_rgb| e(y) against the fp64 output)
and the slots' sum, through reduce_ref / reduce_bound, as ToRGB of the whole output -- once against the fp64 output and once
against the output the launch stored (the fold alone; the registers folded are the fp32 values BEFORE the exit's rounding, so a
planes exit adds sum |w_rgb| (2^-22 |y| + 2^-25 2^e') and the bf16 / planes16 exits are folded from the fp32 exit's output).
Riding fold (ride): reduce_ref / reduce_bound of _gemm1x1_cases.py.
Patch maxima of a planes output: at least the largest stored |hi + lo| 2^e' (1 - 2^-21) of the patch's valid pixels (the maximum is
taken before the split; minus the pair's absolute floor 2^-25 2^e', which the issue's form of this check left out), at most the layer bound c1 m_in + c0.  Amax of an fp32 exit: max |out|, bit for bit, where no column past
HW exists (HW % 128 == 0) or such a column equals the last pixel (no noise); otherwise at least that and at most the larger of it
and |the last pixel without its noise| + its bound -- the columns past HW repeat that pixel (the comment at the `mx` update).

The lconst of a case is built here from the stored weights: c1 = [sqrt 2] max_o sum_i |w| and c0 = sqrt 2 (|nw| max |noise| +
max |bias|), both times 1 + 2^-10 for the roundings of the kernel's own arithmetic -- a rigorous, tight bound, so the stored
values of an output reach up to just below 2^15.  Cases with lc = 2 hand c1 over through lc[2] (the row-L1 slot) instead.

`regime()` replays the host's choice (tiles64, the half-chip form, nstage, the kind of the last pixel block) to LABEL the cases,
never to compute a reference.  The observable that ties it to the library: in the 128-row form the patch maxima 2 j and 2 j + 1
are equal (one wave holds both 16-row tiles), in the 64-row form they are the patches' own.

Notes on the case list.  HW = 200 = 128 + 72 has a last block of TWO halves, the second of 8 pixels (it is listed as the issue
lists it and labelled as what it is); HW = 180 is the one-half, itself ragged, last block behind a full one.  tiles64 = 257 is a
prime: no launch with Cout % 128 == 0 and HW <= 6400 has it, so the upper neighbour of the half-chip window is tiles64 = 258.
"""
import math

import torch

from _gemm1x1_cases import (F32, F64, GAIN, NOISE_W, SPLIT_SCALES, U, bf16_round, ceil_div, epilogue_bound,  # noqa: F401
                            epilogue_ref, f32, gamma, inside, reduce_bound, reduce_ref, split16, split_exp, unpack_bf16,
                            unpack_split, worst, _gen)

BLOCK, HALF = 128, 64                       # CIPS3D_PLANES_EXP_BLOCK; the pixels of a patch
K_FOLD = 4 + 2 + 4
SLACK = 1.0 + 2.0 ** -10                    # of the hand-built lconst over the exact row norms
MARGIN = f32(1.000001)
MUTANTS = ("drop_wl_xh", "drop_wh_xl", "swap_planes", "lo_twice", "exp_neighbour", "exp_sample0", "exp_kept", "noise_other",
           "noise_past_hw", "bias_row16", "fold_tiles", "slope_sign", "gain_before_bias")


def pow2(e, dtype=F64):
    return torch.pow(torch.tensor(2.0, dtype=F64), torch.as_tensor(e).double()).to(dtype)


def px_block(HW):
    return torch.arange(HW) // BLOCK


# ------------------------------------------------------------------------------------------------------------------ formats
def _to_layout(v):
    B, C, HW = v.shape
    return v.reshape(B, C // 8, 8, HW).permute(0, 1, 3, 2).contiguous()


def _from_layout(p):
    B, C8, HW, _ = p.shape
    return p.permute(0, 1, 3, 2).reshape(B, C8 * 8, HW)


def per_pixel(exps, HW, dtype=F64, sign=1):
    """2^(sign e) of every pixel's block, [B,1,HW]"""
    return pow2(sign * exps[:, px_block(HW)], dtype).reshape(exps.shape[0], 1, HW)


def planes_of(x, exps):
    """[B,C/8,2,HW,8] fp16 from fp32 x [B,C,HW]; exps int32 [B, ceil(HW/128)] or None (raw halves)"""
    v = x.float() if exps is None else x.float() * per_pixel(exps, x.shape[2], F32, -1)
    hi, lo = split16(v)
    return torch.stack([_to_layout(hi), _to_layout(lo)], 2).to(torch.float16)


def planes_halves(p):
    """(hi, lo) as fp32 [B,C,HW]"""
    return _from_layout(p[:, :, 0].float()), _from_layout(p[:, :, 1].float())


def planes_value(p, exps):
    hi, lo = planes_halves(p)
    v = hi.double() + lo.double()
    return v if exps is None else v * per_pixel(exps, v.shape[2])


def planes16_of(x):
    return _to_layout(x.float().to(torch.bfloat16))


def planes16_value(p):
    return _from_layout(p.float()).double()


def patch_maxima(x):
    """[B, ceil(HW/64), C/16] of x [B,C,HW]"""
    B, C, HW = x.shape
    nh = ceil_div(HW, HALF)
    pad = torch.zeros(B, C, nh * HALF, dtype=x.dtype)
    pad[:, :, :HW] = x.abs()
    return pad.reshape(B, C // 16, 16, nh, HALF).amax((2, 4)).permute(0, 2, 1).contiguous()


def unpack_split_halves(packed, B, M, K):
    """(wh, wl) fp32 [B,M,K], the fp16 values (2^8-scaled) of the split fragments: unpack_split's layout, the planes apart"""
    h = packed.reshape(-1).view(torch.float16)[:B * M * K * 2].reshape(B, M // 16, K // 32, 2, 4, 16, 8).float()
    un = lambda v: v.permute(0, 1, 4, 2, 3, 5).reshape(B, M, K)      # noqa: E731
    return un(h[:, :, :, 0]), un(h[:, :, :, 1])


# -------------------------------------------------------------------------------------------------------------------- cases
class ChainCase:
    def __init__(self, kernel, B, Cin, Cout, HW, exit, epilogue=1, noise="shared", fold=False, rng="a", hint=False, ride=False,
                 lc=1, **expect):
        """kernel: "split" | "p16"; exit: "planes" | "fp32" | "bf16" ("planes16" for p16); noise: "shared" | "per_sample" | None;
        rng (split): "a" exact patch maxima, "b" none, "c" 4 x the true ones, "d" unranged, "e" an all-zero sample and a spike;
        hint: cips3d_range.half_chip; lc: the lconst slot that carries c1"""
        self.kernel, self.B, self.Cin, self.Cout, self.HW, self.exit, self.epilogue = kernel, B, Cin, Cout, HW, exit, epilogue
        self.noise = noise if epilogue == 1 else None
        self.fold, self.rng, self.hint, self.ride, self.lc, self.expect = fold, (rng if kernel == "split" else None), hint, ride, lc, expect

    @property
    def id(self):
        sw = ("" if self.epilogue else "-ep0") + ("" if self.epilogue == 0 else {"shared": "", "per_sample": "-nzB", None: "-nonoise"}[self.noise]) + \
            ("-fold" if self.fold else "") + ("-ride" if self.ride else "") + ("-hint" if self.hint else "") + ("-lc2" if self.lc == 2 else "")
        return f"{self.kernel}{'-' + self.rng if self.rng else ''}-B{self.B}-i{self.Cin}-o{self.Cout}-HW{self.HW}-{self.exit}{sw}"

    @property
    def split(self):
        return self.kernel == "split"

    @property
    def ranged(self):
        return self.split and self.rng != "d"

    @property
    def tracked(self):
        """a planes output under range tracking: exponents and patch maxima are written"""
        return self.ranged and self.exit == "planes"

    @property
    def scales(self):
        if self.HW > 1024:       # the half-chip window: what it adds is the form, not the range; one scale keeps the test quick
            return (2.0 ** -20,) if self.exit == "fp32" else (1.0,)
        return (1.0, 2.0 ** -20) if (self.split and not self.ranged) else SPLIT_SCALES       # raw halves: fp16's own range

    @property
    def nblk(self):
        return ceil_div(self.HW, BLOCK)

    @property
    def nhalf(self):
        return ceil_div(self.HW, HALF)

    @property
    def per_sample_noise(self):
        return self.noise == "per_sample" and self.B > 1

    def regime(self):
        tiles64 = self.B * (self.Cout // 64) * self.nblk
        half_chip = self.split and self.ranged and self.hint and self.Cout % 128 == 0 and 192 < tiles64 <= 256
        tail = self.HW - (self.nblk - 1) * BLOCK
        kind = "full" if tail == BLOCK else "one_half" if tail == HALF else "one_ragged_half" if tail < HALF else "two_halves_second_ragged"
        return dict(tiles64=tiles64, form="128x128" if half_chip else "64x128", nstage=self.Cin // 64, ring=2 if self.split else 3,
                    tail=tail, kind=kind, blocks=self.nblk, slots=self.Cout // 64)

    # ---- data
    def tensors(self, gs=1.0):
        """x [B,Cin,HW], exps [B,nblk] | None, W [Cout,Cin], s [B,Cin], w [B,Cout,Cin] (torch's modulation of them), noise
        [1 | B,1,HW] | None, bias [Cout], w_rgb [B,3,Cout]; a ride's part / biases / skip"""
        B, Cin, Cout, HW = self.B, self.Cin, self.Cout, self.HW
        g = _gen(21, B, Cin, Cout, HW)
        blk = px_block(HW)
        spread = not (self.split and not self.ranged)
        step = (13 * (blk % 3)) if spread else torch.zeros(HW, dtype=torch.int64)
        samp = (10 * torch.arange(B)) if spread else torch.zeros(B, dtype=torch.int64)
        x = torch.randn(B, Cin, HW, generator=g) * (1.0 + 3.0 * torch.rand(B, Cin, 1, generator=g))
        x = x * pow2(step[None, :] + samp[:, None], F32).reshape(B, 1, HW) * gs
        exps = None
        if self.ranged:     # the stored values are randn (1 .. 4) 2^9: block maxima of 2^10 .. 2^13.3
            first = torch.arange(self.nblk) * BLOCK
            exps = (round(math.log2(gs)) - 9 + step[first][None, :] + samp[:, None]).to(torch.int32).contiguous()
        if self.rng == "e":
            x[1] = 0.0
            x[0, 5, 3] = 2.0 ** 30 * float(x[0, :, :BLOCK].abs().max())       # (stored where the block's maximum was)
            exps[0, 0] += 30
        scale = f32(1.0 / math.sqrt(Cin))
        W = torch.randn(Cout, Cin, generator=g)
        s = 1.0 + 0.4 * (2.0 * torch.rand(B, Cin, generator=g) - 1.0)
        v = (scale * W)[None] * s[:, None, :]
        w = v * torch.rsqrt((v * v).sum(-1, keepdim=True) + 1e-8)
        noise = None
        if self.noise:
            nb = B if self.per_sample_noise else 1
            noise = torch.randn(nb, 1, HW, generator=g) * gs       # (of the size of the lowest block's data: c0 is per sample)
            if self.per_sample_noise:       # (the later samples' first pixels are loud: what a read past a sample's row would find)
                noise = noise * pow2(samp, F32).reshape(B, 1, 1)
                noise[1:, :, :HALF] *= 1024.0
        bias = torch.randn(Cout, generator=g) * 0.5 * gs
        w_rgb = torch.randn(B, 3, Cout, generator=g) / math.sqrt(Cout)
        t = dict(x=x, exps=exps, W=W, s=s, scale=scale, w=w, noise=noise, bias=bias, w_rgb=w_rgb)
        if self.ride:
            t["ride"] = dict(part=torch.randn(5, 1, 3, 260, generator=g) * gs, biases=torch.randn(2, 3, generator=g) * gs,
                             skip=torch.randn(1, 3, 260, generator=g) * gs)
        return t

    def operands(self, t, wh=None, wl=None, w16=None):
        """what the launch reads, as stored: split -- p (planes), xh / xl / wh / wl (fp32 holding fp16 values, the weights 2^8-
        scaled), exps, pmax (as handed over) | None, lconst [B,4] | None;  p16 -- p (planes16), x / w (fp32 holding bf16 values)"""
        if not self.split:
            p = planes16_of(t["x"])
            return dict(p=p, x=_from_layout(p.float()), w=bf16_round(t["w"]) if w16 is None else w16)
        if wh is None:
            wh, wl = split16(t["w"] * 256.0)
        p = planes_of(t["x"], t["exps"])
        xh, xl = planes_halves(p)
        o = dict(p=p, xh=xh, xl=xl, wh=wh, wl=wl, exps=t["exps"], pmax=None, lconst=None)
        if not self.ranged:
            return o
        if self.rng != "b":
            o["pmax"] = patch_maxima(planes_value(p, t["exps"])).float() * (4.0 if self.rng == "c" else 1.0)
        if self.exit == "planes":
            L1 = ((wh.double() + wl.double()).abs() / 256.0).sum(2).amax(1)                 # [B]
            g_ = float(GAIN) if self.epilogue == 1 else 1.0
            c1 = (g_ * L1 * SLACK).float()
            c0 = torch.zeros(self.B)
            if self.epilogue == 1:
                nz = t["noise"].abs().amax((1, 2)).expand(self.B).double() if t["noise"] is not None else torch.zeros(self.B, dtype=F64)
                c0 = (float(GAIN) * (NOISE_W * nz + float(t["bias"].abs().max())) * SLACK).float()
            lconst = torch.zeros(self.B, 4)
            lconst[:, 0] = c0
            if self.lc == 1:
                lconst[:, 1] = c1
            else:           # through the row-L1 slot: the kernel multiplies it by sqrt 2
                lconst[:, 1], lconst[:, 2] = c1 / 2.0, (c1.double() / float(GAIN) * (1.0 + 2.0 ** -20)).float()
            o["lconst"] = lconst
        return o

    def mutants(self):
        m = []
        if self.split:
            m += ["drop_wl_xh", "drop_wh_xl", "swap_planes"]
            if self.exit == "planes":
                m += ["lo_twice"]
            if self.ranged:
                m += ["exp_kept"] + (["exp_neighbour"] if self.nblk > 1 else []) + (["exp_sample0"] if self.B > 1 else [])
        if self.epilogue == 1:
            m += ["bias_row16", "slope_sign", "gain_before_bias"]
            if self.per_sample_noise:
                m += ["noise_other"]
                if self.ranged and self.exit == "fp32" and self.HW % BLOCK:
                    m += ["noise_past_hw"]
        if self.fold and self.Cout > 64:
            m += ["fold_tiles"]
        return m


# ------------------------------------------------------------------------------------------------- the output's exponent
def out_exp_replay(lconst, m_in):
    """(e', the fp32 bound it is the exponent of, c1) for one (sample, block): lconst [4] and m_in as Python floats (fp32 values)"""
    c0, c1 = float(lconst[0]), max(float(lconst[1]), f32(float(GAIN) * float(lconst[2])))
    bound = f32(c1 * f32(float(m_in) * MARGIN) + c0)
    return split_exp(bound), bound, c1


def block_m_in(case, ops):
    """[B,nblk] fp32: max |in| as the kernel takes it for each pixel block"""
    if ops["pmax"] is None:
        return pow2(ops["exps"] + 15, F32)
    pm = ops["pmax"]
    out = torch.zeros(case.B, case.nblk)
    for j in range(case.nblk):
        out[:, j] = pm[:, 2 * j:min(2 * j + 2, case.nhalf)].amax((1, 2))
    return out


def replayed_exponents(case, ops):
    """(e' int32 [B,nblk], the fp32 bounds [B,nblk], the layer bound c1 m_in + c0 in fp64 [B,nblk])"""
    m = block_m_in(case, ops)
    e, bound, layer = torch.zeros(case.B, case.nblk, dtype=torch.int32), torch.zeros(case.B, case.nblk, dtype=F64), \
        torch.zeros(case.B, case.nblk, dtype=F64)
    for b in range(case.B):
        for j in range(case.nblk):
            ee, bb, c1 = out_exp_replay(ops["lconst"][b], float(m[b, j]))
            e[b, j], bound[b, j], layer[b, j] = ee, bb, c1 * float(m[b, j]) + float(ops["lconst"][b, 0])
    return e, bound, layer


# --------------------------------------------------------------------------------------------------- reference and bounds
def _kin(case, exps, HW, dtype):
    if not case.split:
        return torch.ones(1, 1, 1, dtype=dtype)
    k = torch.full((1, 1, 1), 2.0 ** -8, dtype=dtype)
    return k if exps is None else k * per_pixel(exps, HW, dtype)


def _ep_t(t, noise=None):
    return dict(noise=t["noise"] if noise is None else noise, bias=t["bias"])


def reference(case, t, ops):
    """fp64: v (accumulator), out, e_v, e_out (the fp32 exit's bound), and for a tracked planes exit exp / exp_bound / layer,
    e_planes (the planes exit's bound)"""
    HW = case.HW
    if case.split:
        wh, wl, xh, xl = (ops[k].double() for k in ("wh", "wl", "xh", "xl"))
        kin = _kin(case, ops["exps"] if case.ranged else None, HW, F64)
        v = torch.bmm(wh + wl, xh + xl) * kin
        three = torch.bmm(torch.cat([wh, wh, wl], 2).abs(), torch.cat([xh, xl, xh], 1).abs())
        e_v = kin * (torch.bmm(wl.abs(), xl.abs()) + gamma(3 * case.Cin + 8) * three)
    else:
        w, x = ops["w"].double(), ops["x"].double()
        v, e_v = torch.bmm(w, x), gamma(case.Cin + 8) * torch.bmm(w.abs(), x.abs())
    r = dict(v=v, e_v=e_v)
    if case.epilogue == 1:
        r["out"], r["e_out"] = epilogue_ref(v, _ep_t(t), F64, case.per_sample_noise), epilogue_bound(v, e_v, _ep_t(t))
    else:
        r["out"], r["e_out"] = v, e_v
    if case.exit == "planes":
        if case.tracked:
            r["exp"], r["exp_bound"], r["layer"] = replayed_exponents(case, ops)
            floor = 2.0 ** -25 * per_pixel(r["exp"], HW)
        else:
            floor = torch.full((1, 1, 1), 2.0 ** -25, dtype=F64)
        r["floor"] = floor
        r["e_planes"] = r["e_out"] + 2.0 ** -22 * (r["out"].abs() + r["e_out"]) + floor
    return r


def last_pixel_without_noise(case, t, ref):
    """[B] |the last pixel's output without its noise| + its bound, the largest over the rows: what a column past HW may hold"""
    v, e_v = ref["v"][:, :, -1:], ref["e_v"][:, :, -1:]
    if case.epilogue != 1:
        return (v.abs() + e_v).amax((1, 2))
    tt = dict(noise=None, bias=t["bias"])
    return (epilogue_ref(v, tt, F64, False).abs() + epilogue_bound(v, e_v, tt)).amax((1, 2))


def slot_refs(case, t, y, bound_y=None):
    """([slots,B,3,HW] ToRGB of the 64-row blocks of y in fp64, its bound)"""
    w, y = t["w_rgb"].double(), y.double()
    refs, bounds = [], []
    for s in range(case.Cout // 64):
        rows = slice(64 * s, 64 * s + 64)
        refs.append(torch.bmm(w[:, :, rows], y[:, rows]))
        e = gamma(K_FOLD) * torch.bmm(w[:, :, rows].abs(), y[:, rows].abs())
        if bound_y is not None:
            e = e + torch.bmm(w[:, :, rows].abs(), bound_y[:, rows].expand_as(y[:, rows]))
        bounds.append(e)
    return torch.stack(refs), torch.stack(bounds)


def reference_ride(tr):
    """(fp64 reference, bound) of a riding fold: part [n_slots,Br,3,HWr], biases [n,3], skip"""
    return reduce_ref(tr, F64), reduce_bound(tr)


# --------------------------------------------------------------------------------------------------------- fp32 emulation
def planes_emulated(case, t, ops, mutant=None):
    """what a correct fp32 implementation built from the header's definitions leaves (a subtly wrong one with `mutant`), in the
    form check_outputs takes: out32 (the fp32 value every exit rounds), and hi / lo / exp / pmax (tracked planes exit), amax
    (ranged fp32 exit), slots (fold)"""
    B, HW = case.B, case.HW
    if case.split:
        wh, wl, xh, xl = ops["wh"], ops["wl"], ops["xh"], ops["xl"]
        exps = ops["exps"] if case.ranged else None
        if mutant == "exp_neighbour":
            exps = torch.roll(exps, 1, 1)
        if mutant == "exp_sample0":
            exps = exps[0:1].expand(B, -1)
        if mutant == "exp_kept":
            exps = None
        if mutant == "swap_planes":
            xh, xl = xl, xh
        a, b_ = [wl, wh, wh], [xh, xl, xh]
        if mutant == "drop_wl_xh":
            a, b_ = a[1:], b_[1:]
        if mutant == "drop_wh_xl":
            a, b_ = [wl, wh], [xh, xh]
        v = torch.bmm(torch.cat(a, 2), torch.cat(b_, 1)) * _kin(case, exps, HW, F32)
    else:
        v = torch.bmm(ops["w"], ops["x"])
    noise = t["noise"]
    if mutant == "noise_other":
        noise = torch.roll(noise, 1, 0)
    em = mutant if mutant in ("bias_row16", "slope_sign", "gain_before_bias") else None
    out = epilogue_ref(v, _ep_t(t, noise), F32, case.per_sample_noise, em) if case.epilogue == 1 else v
    got = dict(out32=out)
    if case.exit == "planes":
        if case.tracked:
            e_out = replayed_exponents(case, ops)[0]
            s = out * per_pixel(e_out, HW, F32, -1)
            got["exp"], got["pmax"] = e_out, patch_maxima(out)
        else:
            s = out
        hi, lo = split16(s)
        got["hi"], got["lo"] = hi, (lo * 2.0 if mutant == "lo_twice" else lo)
    if case.ranged and case.exit == "fp32":
        am = out.abs().amax((1, 2))
        if HW % BLOCK and case.epilogue == 1 and noise is not None:
            # the columns past HW: the last pixel's accumulator without noise -- or, wrongly, with what lies behind the sample's row
            pad = case.nblk * BLOCK - HW
            tail = torch.zeros(B, 1, pad)
            if mutant == "noise_past_hw":
                flat = torch.cat([noise.reshape(-1), torch.zeros(pad)])
                stride = HW if case.per_sample_noise else 0
                for b in range(B):
                    tail[b, 0] = flat[b * stride + HW:b * stride + HW + pad]
            rep = epilogue_ref(v[:, :, -1:].expand(-1, -1, pad), dict(noise=tail, bias=t["bias"]), F32, True)
            am = torch.maximum(am, rep.abs().amax((1, 2)))
        got["amax"] = am
    if case.fold:
        w = t["w_rgb"]
        tiles = [torch.bmm(w[:, :, 16 * i:16 * i + 16], out[:, 16 * i:16 * i + 16]) for i in range(case.Cout // 16)]
        n = len(tiles)
        pick = (lambda s_, m_: (4 * s_ + m_) if m_ < 2 else (4 * s_ + 4 + m_) % n) if mutant == "fold_tiles" else (lambda s_, m_: 4 * s_ + m_)
        got["slots"] = torch.stack([sum(tiles[pick(s_, m_)] for m_ in range(4)) for s_ in range(case.Cout // 64)])
    return got


# ----------------------------------------------------------------------------------------------------------------- checks
def _hold(err, bound, what, ratios):
    r, at = worst(err, bound.expand_as(err))
    ratios[what] = max(ratios.get(what, 0.0), r)
    assert bool((err <= bound).all()), f"{what}: error is {r:.3g} x its bound at flat element {at}"


def check_outputs(case, t, ops, ref, got):
    """every assertion on the outputs of one launch that needs the fp64 reference; `got` holds CPU tensors: out32 (fp32 exit:
    the stored output) and / or hi, lo, exp, pmax (planes exit), amax, slots.  Returns {check: worst error / bound}."""
    ratios = {}
    HW = case.HW
    y_stored, e_stored_extra = None, None
    if case.exit == "planes":
        hi, lo = got["hi"].double(), got["lo"].double()
        assert bool(torch.isfinite(hi).all()) and bool(torch.isfinite(lo).all()), "planes exit: a stored half is not finite"
        assert bool(((hi + lo).abs() < 2.0 ** 15).all()), "planes exit: a stored |hi + lo| reaches 2^15"
        assert canonical(got["hi"].float(), got["lo"].float()), "planes exit: a pair is not canonical (fp16(hi + lo) != hi off a tie)"
        val = hi + lo
        if case.tracked:
            assert torch.equal(got["exp"].to(torch.int32), ref["exp"]), \
                f"planes exit: out_exp {got['exp'].tolist()} is not the replay {ref['exp'].tolist()}"
            val = val * per_pixel(ref["exp"], HW)
            pm = got["pmax"].double()
            assert bool(torch.isfinite(pm).all()), "out_pmax: an entry was not written"
            # (a stored pair exceeds the value it was split from by 2^-22 of it and, where lo is subnormal, 2^-25 in its own units)
            low = patch_maxima((val.abs() - ref["floor"]).clamp_min(0.0)) * (1.0 - 2.0 ** -21)
            assert bool((pm >= low).all()), "out_pmax: below the largest stored value of its patch"
            layer = ref["layer"][:, torch.arange(case.nhalf) // 2].unsqueeze(-1)
            assert bool((pm <= layer).all()), "out_pmax: above the layer bound c1 m_in + c0"
        _hold((val - ref["out"]).abs(), ref["e_planes"], "planes exit", ratios)
        y_stored = val
        e_stored_extra = 2.0 ** -22 * val.abs() * (1.0 + 2.0 ** -20) + ref["floor"]
    elif "out32" in got and got["out32"] is not None:
        out = got["out32"].double()
        assert bool(torch.isfinite(out).all()), "fp32 exit: not finite"
        _hold((out - ref["out"]).abs(), ref["e_out"], "fp32 exit", ratios)
        y_stored = out
    if got.get("amax") is not None:
        true = got["out32"].abs().amax((1, 2))
        am = got["amax"]
        if HW % BLOCK == 0 or case.epilogue == 0 or case.noise is None:
            assert torch.equal(am, true), f"out_amax {am.tolist()} is not max |out| {true.tolist()}"
        else:
            assert bool((am >= true).all()), "out_amax is below max |out|"
            cap = torch.maximum(true.double(), last_pixel_without_noise(case, t, ref))
            assert bool((am.double() <= cap).all()), f"out_amax {am.tolist()} exceeds max |out| and the last pixel without noise {cap.tolist()}"
    if case.fold and got.get("slots") is not None:
        slots = got["slots"].double()
        assert slots.shape[0] == case.Cout // 64 and bool(torch.isfinite(slots).all()), "fold: a slot was not written"
        e_y = ref["e_planes"] if case.exit == "planes" else ref["e_out"]
        r64, b64 = slot_refs(case, t, ref["out"], e_y)
        _hold((slots - r64).abs(), b64, "fold slots vs fp64 output", ratios)
        if y_stored is not None:
            rs, bs = slot_refs(case, t, y_stored, e_stored_extra)
            _hold((slots - rs).abs(), bs, "fold slots vs stored output", ratios)
            tt = dict(part=slots, biases=torch.zeros(0, 3, dtype=F64), skip=None)
            total = torch.bmm(t["w_rgb"].double(), y_stored)
            e_tot = gamma(K_FOLD + case.Cout // 64 - 1) * torch.bmm(t["w_rgb"].double().abs(), y_stored.abs())
            if e_stored_extra is not None:
                e_tot = e_tot + torch.bmm(t["w_rgb"].double().abs(), e_stored_extra.expand_as(y_stored))
            _hold((reduce_ref(tt, F64) - total).abs(), e_tot + reduce_bound(tt), "fold sum vs stored output", ratios)
    return ratios


def canonical(hi, lo):
    """fp16(hi + lo) == hi, evaluated in fp32 -- or hi + lo is an exact tie between hi and its neighbour: with s just inside half
    a spacing of hi, lo = fp16(s - hi) may round ONTO the half spacing, and nearest-even then leaves the odd hi (the header's own
    split does this; the emulation meets it in about one value of 10^4).  So: fp16(hi + lo) == hi or |lo| is half hi's spacing."""
    same = (hi + lo).to(torch.float16).float() == hi
    spacing = torch.pow(2.0, torch.floor(torch.log2(hi.abs().clamp_min(2.0 ** -14))) - 10.0)
    return bool((same | (lo.abs() == 0.5 * spacing)).all())


def passes(case, t, ops, ref, got):
    try:
        check_outputs(case, t, ops, ref, got)
        return True
    except AssertionError:
        return False


# ----------------------------------------------------------------------------------------------------------------- the cases
S, P = "split", "p16"
CHAIN_CASES = [
    # ---- split kernel, 64 x 128 tiles.  Ragged kinds x exits
    ChainCase(S, 2, 64, 64, 16, "planes", noise="per_sample", nstage=1, kind="one_ragged_half", tail=16),
    ChainCase(S, 1, 64, 64, 16, "fp32", nstage=1, kind="one_ragged_half"),
    ChainCase(S, 1, 128, 64, 16, "bf16", epilogue=0, nstage=2, kind="one_ragged_half"),
    ChainCase(S, 2, 128, 128, 60, "planes", noise="per_sample", fold=True, nstage=2, kind="one_ragged_half", tail=60),
    ChainCase(S, 2, 192, 64, 60, "fp32", noise="per_sample", nstage=3, kind="one_ragged_half"),
    ChainCase(S, 1, 64, 128, 60, "bf16", nstage=1, kind="one_ragged_half"),
    ChainCase(S, 1, 192, 192, 64, "planes", rng="b", nstage=3, kind="one_half", slots=3),
    ChainCase(S, 2, 64, 64, 64, "fp32", rng="b", noise="per_sample", kind="one_half"),
    ChainCase(S, 1, 64, 64, 64, "bf16", rng="c", epilogue=0, kind="one_half"),
    ChainCase(S, 3, 128, 64, 65, "planes", rng="c", noise="per_sample", kind="two_halves_second_ragged", tail=65),
    ChainCase(S, 2, 64, 128, 65, "fp32", noise="per_sample", fold=True, kind="two_halves_second_ragged"),
    ChainCase(S, 2, 64, 64, 65, "bf16", noise="per_sample", kind="two_halves_second_ragged"),
    ChainCase(S, 2, 512, 256, 128, "planes", noise="per_sample", fold=True, nstage=8, kind="full", slots=4),
    ChainCase(S, 1, 512, 64, 128, "fp32", noise=None, nstage=8, kind="full"),
    ChainCase(S, 1, 64, 64, 128, "bf16", kind="full"),
    ChainCase(S, 2, 192, 128, 129, "planes", noise="per_sample", lc=2, nstage=3, kind="one_ragged_half", blocks=2, tail=1),
    ChainCase(S, 2, 128, 64, 129, "fp32", noise="per_sample", kind="one_ragged_half", blocks=2),
    ChainCase(S, 2, 64, 64, 129, "bf16", noise="per_sample", kind="one_ragged_half", blocks=2),
    ChainCase(S, 2, 128, 128, 180, "planes", rng="b", noise="per_sample", kind="one_ragged_half", blocks=2, tail=52),
    ChainCase(S, 1, 64, 192, 180, "fp32", fold=True, kind="one_ragged_half", blocks=2, slots=3),
    ChainCase(S, 3, 64, 64, 200, "planes", epilogue=0, kind="two_halves_second_ragged", blocks=2, tail=72),
    ChainCase(S, 2, 128, 64, 200, "fp32", noise="per_sample", rng="c", kind="two_halves_second_ragged", blocks=2),
    ChainCase(S, 2, 128, 128, 250, "planes", noise="per_sample", fold=True, lc=2, kind="two_halves_second_ragged", blocks=2, tail=122),
    ChainCase(S, 3, 64, 64, 250, "fp32", noise="per_sample", kind="two_halves_second_ragged", blocks=2),
    ChainCase(S, 1, 192, 256, 250, "bf16", epilogue=0, fold=True, nstage=3, kind="two_halves_second_ragged", slots=4),
    # nine stages: only without patch maxima
    ChainCase(S, 1, 576, 64, 129, "planes", rng="b", nstage=9, blocks=2),
    ChainCase(S, 2, 576, 128, 60, "fp32", rng="b", noise="per_sample", nstage=9),
    # unranged: raw halves, kout = 1
    ChainCase(S, 2, 64, 128, 129, "planes", rng="d", noise="per_sample", fold=True, blocks=2),
    ChainCase(S, 1, 128, 64, 250, "fp32", rng="d", nstage=2),
    ChainCase(S, 2, 64, 64, 60, "bf16", rng="d", epilogue=0),
    ChainCase(S, 1, 192, 64, 65, "planes", rng="d", epilogue=0, nstage=3),
    # an all-zero sample and a spike 2^30 above the rest
    ChainCase(S, 2, 128, 128, 250, "planes", rng="e", blocks=2),
    ChainCase(S, 2, 64, 64, 129, "planes", rng="e", epilogue=0, blocks=2),
    ChainCase(S, 2, 64, 64, 200, "fp32", rng="e", noise="per_sample"),
    # ---- the half-chip window 192 < tiles64 <= 256 and its neighbours, with and without the hint
    ChainCase(S, 3, 64, 128, 33 * 128 + 37, "planes", noise="per_sample", hint=True, tiles64=204, form="128x128", kind="one_ragged_half"),
    ChainCase(S, 1, 128, 256, 49 * 128 + 65, "planes", fold=True, hint=True, tiles64=200, form="128x128", kind="two_halves_second_ragged"),
    ChainCase(S, 1, 128, 256, 49 * 128 + 65, "planes", ride=True, hint=True, tiles64=200, form="128x128"),
    ChainCase(S, 1, 128, 256, 49 * 128 + 65, "fp32", fold=True, hint=True, tiles64=200, form="128x128"),
    ChainCase(S, 3, 64, 128, 32 * 128, "planes", noise="per_sample", hint=True, tiles64=192, form="64x128", kind="full"),
    ChainCase(S, 3, 64, 128, 43 * 128, "planes", noise="per_sample", hint=True, tiles64=258, form="64x128", kind="full"),
    # ---- planes16 kernel: a 3-slot ring against 1, 2, 3, 4 and 8 stages
    ChainCase(P, 2, 64, 64, 16, "planes16", noise="per_sample", nstage=1, ring=3, kind="one_ragged_half"),
    ChainCase(P, 1, 128, 128, 60, "fp32", fold=True, nstage=2, kind="one_ragged_half"),
    ChainCase(P, 2, 192, 64, 64, "bf16", noise="per_sample", nstage=3, kind="one_half"),
    ChainCase(P, 2, 256, 128, 65, "planes16", noise="per_sample", fold=True, nstage=4, kind="two_halves_second_ragged"),
    ChainCase(P, 1, 512, 192, 128, "fp32", epilogue=0, nstage=8, kind="full", slots=3),
    ChainCase(P, 3, 64, 64, 129, "bf16", epilogue=0, kind="one_ragged_half", blocks=2),
    ChainCase(P, 2, 256, 64, 180, "planes16", noise=None, nstage=4, kind="one_ragged_half", blocks=2),
    ChainCase(P, 2, 128, 256, 200, "fp32", noise="per_sample", fold=True, kind="two_halves_second_ragged", slots=4),
    ChainCase(P, 1, 192, 64, 250, "planes16", nstage=3, kind="two_halves_second_ragged"),
    ChainCase(P, 2, 64, 128, 250, "bf16", noise="per_sample", fold=True, kind="two_halves_second_ragged"),
    ChainCase(P, 1, 64, 64, 64, "planes16", epilogue=0, kind="one_half"),
    ChainCase(P, 1, 64, 64, 128, "planes16", kind="full"),
    ChainCase(P, 2, 128, 64, 60, "planes16", epilogue=0, fold=True, kind="one_ragged_half"),
    ChainCase(P, 1, 64, 64, 200, "bf16", kind="two_halves_second_ragged"),
    ChainCase(P, 1, 64, 64, 16, "fp32", kind="one_ragged_half"),
    ChainCase(P, 1, 64, 64, 65, "fp32", noise=None, kind="two_halves_second_ragged"),
    ChainCase(P, 3, 128, 64, 128, "bf16", noise="per_sample", kind="full"),
    ChainCase(P, 2, 192, 128, 64, "fp32", noise="per_sample", fold=True, nstage=3, kind="one_half"),
]
# the converters: (B, C, HW); C = 8 and 24 have no patch maxima (C % 16)
CONVERTER_CASES = [(B, C, HW) for C in (8, 24, 64) for B, HW in ((1, 16), (2, 60), (1, 64), (3, 65), (1, 128), (2, 129), (1, 200), (2, 250))]
# the producer-to-consumer run: three layers from to_planes, the input multiplied by 2^(3 blk) per pixel block
RUN_CASE = (2, 128, 128, 250)
