"""Cases, fp64 reference and rounding-error bounds of the fused decoder stage (csrc/fused_stage.hip: fused_up_conv_kernel behind
cips3d_fused_up_conv and cips3d_fused_up_conv_next) in its seven base instantiations -- C = 32, 64, 128, 256 unchained, C = 64, 128,
256 chained -- up-sampling and flat, in the three arithmetic modes.  Shared by test_fused_stage_cases_host.py (CPU: every bound
admits the fp32 evaluation and the bf16 / split emulations and rejects every mutant; every case sits in its regime) and
test_gpu_fused_stage.py (the kernel).  Imports no GPU code.  Built on tests/_gemm1x1_cases.py (GC below), whose conventions hold:
u = 2^-24, gamma_k = k u / (1 - k u), bounds per element in fp64, a term charged one rounding for every addition that can come
after it, eight roundings set aside for the inside of a matrix instruction's chain, data multiplied by a power of two `gs` so that
no bound has an absolute floor.

Reference (`stage_ref`): one torch expression, generic in its dtype and THE SAME in every arithmetic mode (the bf16 and split modes
are charged for their representation, below):
    act1   = lrelu(upfir(y_lo) + nw1 n1 + b1) sqrt 2          (flat: y_lo as it is)              [B,C,P]   P = OH OW
    out2   = lrelu(W2 act1 + nw2 n2 + b2) sqrt 2
    rgb    = Wrgb out2 + brgb + (upfir(skip) | skip | nothing)
    y_next = Wn out2
`epi` / `epi_bound` are GC.epilogue_ref / GC.epilogue_bound with the noise weight as an argument: nw1 = 0.3 and nw2 = -0.2 differ, so
an exchanged pointer shows.  W2 [C,C], Wn [C/2,C] and Wrgb [3,C] are explicit matrices with rows of about unit norm, shared by the
samples; the GPU test sends them through cips3d_modulate_weights without demodulation, with scale 1.0 and styles of ones -- an exact
product, so kernel and reference see the same numbers in whatever fragment layout the kernel wants.

Bounds (`stage_bounds`), composed from GC's.  ak = |a| + e(a) is what the kernel's own operand can be.
act1: GC's up2_fir_act: e(v) = gamma_4 upfir(|y_lo|, |fir|), then the epilogue; the flat form the epilogue alone (e(v) = 0).
A contraction W a with an operand that carries e(a) (`contract_bound`; k = the roundings a product can meet):
    fp32   e = sum |w| e(a) + gamma_k sum |w| ak
    bf16   pack_bf16 rounds BOTH fragments, and the rounded act1 is not observable: unlike GC's stand-alone GEMM, whose reference
           is the GEMM of the rounded operands, this bound charges the representation of both operands against the unrounded
           reference -- d(w) = 2^-8 |w|, d(a) = 2^-8 ak + e(a): bf16 has 8 significant bits, half an ulp is 2^-8 of the value at
           the bottom of a binade, as in GC's bf16 fragments -- and their product term, on top of the fp32 accumulation of the
           (exact) products of the rounded operands:
           e = sum (|w| d(a) + d(w) |a| + d(w) d(a)) + gamma_k sum (|w| + d(w)) (|a| + d(a))
    split  GC's rep / low of the two fp16 halves, the activation's absolute terms in units of 2^E:
           e = sum (|w| (e(a) + rep(a)) + rep(w) ak + rep(w) rep(a) + low(w) low(a)) + gamma_k3 sum (|wh ah| + |wh al| + |wl ah|)
           with the last sum bounded from |wh| <= |w| + low(w), |wl| <= low(w) and the same for a.
out2: k = C + 8 (k3 = 3 C + 8): one accumulator chain over the K stages; then the epilogue.
y_next, exchange form (XCHG: C = 64, 256): every wave owns output tiles over the full K: k = C + 8, k3 = 3 C + 8.
y_next, split-K form (C = 128): a wave row's chain has 16 WM terms, WGM - 1 additions join the rows:
    k = 16 WM + 8 + WGM - 1, k3 = 48 WM + 8 + WGM - 1.
rgb counts the kernel's own additions: 4 WM fmas per lane, two joins of the lane quarters, WGM additions over the wave rows of which
the first meets a zero (WGM - 1 roundings), the bias, the skip:
    k_rgb = 4 WM + 2 + WGM - 1 + 1 + [skip]
    e = sum |wrgb| e(out2) + gamma_(k_rgb) sum |wrgb| ak + gamma_(1 + [skip]) |brgb| + (gamma_5 upfir(|skip|, |fir|)  or  u |skip|)
The ToRGB sums are fp32 fmas on the unrounded out2 in every mode.
Split mode with range tracking: the kernel splits act1 2^-e1 and (chained) out2 2^-e2, e = cips3d_split_exp of
    U1 = c1 max |y_lo| + c0             c0 = sqrt 2 (|nw1| max |n1| + max |b1|), c1 = sqrt 2 x the FIR's largest polyphase L1 norm
    U2 = max(c1', sqrt 2 l1') U1 + c0'  c0' = sqrt 2 (|nw2| max |n2| + max |b2|), c1' = sqrt 2 sqrt C, l1' = 0    (flat: c1 = sqrt 2)
(the comment above layer_consts in csrc/modulate.hip; max |y_lo| per sample, the noise maxima over the whole map).  `replay_exps`
evaluates them in fp64 and takes GC.split_exp.  The kernel evaluates them in fp32: at a power-of-two boundary its exponent can differ
by one, so every absolute term of a bound is charged at ONE BINADE ABOVE the replayed exponent, 2^(e + 1), and a disagreement
cannot matter; the emulation uses the replayed exponent itself.  With ranged=False (run at gs = 1 only) both exponents are 0 by
construction and are charged the same way.  Powers of two that ride on the activations' sqrt 2 and come back in the epilogues are exact.
"Through" terms: sum |w| e(out2) charges every channel's worst case with one sign through a sum of mixed signs and dominates rgb
and y_next.  Both are therefore held a second time to the bound of their own arithmetic alone: against the fp64 ToRGB, resp. Wn x,
of the out2 THE SAME LAUNCH stored, with e(out2) = 0 (`stage_bounds(..., out2=stored)`; bf16 and split keep their representation terms).

Cases: (C, chained, flat, B, H, W) with H, W at LOW resolution, the arrangement of both noise maps (shared | per_sample | None,
independently: the nbs1 / nbs2 strides), the skip (fir | plain | none), want_out2, rgb (absent in some chained cases), and the regime
each is listed for.  `regime()` replays the launch table at the bottom of fused_stage.hip -- tile (TH, TW), tile count per sample,
swizzled = tiles % 8 == 0 (the XCD-aware permutation), interior tiles, K stages -- to CHOOSE and label cases, never for a reference.
With B = 2 sample 0's y_lo is 2^9 times sample 1's (noise and bias are shared; the small sample is the second, where noise read
from sample 0 shows): its exponents sit 8 or 9 above, sample 1's would overflow its fp16 halves and its own would cost sample 1 eight
bits; the unranged split run at gs = 1 still fits fp16 (the host test checks both).
The largest stored tensor is out2 of C = 128 at H16 x W96, 3.1 MB (C = 256 at H6 x W96: 2.4 MB).

Mutants (subtly wrong references; each leaves its bound on the CPU, test_fused_stage_cases_host.py):
    halo_left_zero            the left halo column of the first interior tile read as zero
    tile_slot_copied          the workgroup of permuted index 1 computes at the position of plain index 1: tile tiles / 8 holds tile
                              1's values (a bijective exchange of the two orders is invisible: every tile is still computed once)
    hw_exchanged              H and W exchanged in an index into y_lo.  (H W itself is symmetric: the exchange is made where it is
                              not, in the row stride, iy H + ix for iy W + ix inside the plane.)  Visible only when H != W.
    n1_row_down               the n1 tile fetched one image row down
    drop_stage_last_channel   the last channel of K stage 0 dropped from conv2
    kgroups_swapped           k-groups 0 and 1 of the chained pack exchanged
    rgb_row_lost              wave row WGM - 1's ToRGB partial lost
    skip_parity               the FIR'd skip's row parity (oy & 1) inverted
    n1_sample0, n2_sample0    per-sample noise read from sample 0
    slope_sign (conv1), gain_before_bias (conv2)   as in GC
"""
import math

import torch

import _gemm1x1_cases as GC
from _gemm1x1_cases import F32, F64, FIR, GAIN, MODES, SCALES, SPLIT_SCALES, U, bf16_round, gamma, split16, split_exp, upfir  # noqa: F401

NW1, NW2 = GC.NOISE_W, GC.f32(-0.2)
SPREAD = (2.0 ** 9, 1.0)
# C -> (WM, WGM, WGN, RW, BK, XCHG): the launch table of cips3d_fused_up_conv_next
UNCHAINED = {32: (1, 2, 2, 1, 32, False), 64: (2, 2, 2, 1, 16, False), 128: (4, 2, 4, 1, 32, False), 256: (2, 8, 1, 2, 64, False)}
CHAINED = {64: (2, 2, 2, 1, 16, True), 128: (4, 2, 2, 1, 32, False), 256: (2, 8, 1, 2, 64, True)}
BASE = [(32, False), (64, False), (128, False), (256, False), (64, True), (128, True), (256, True)]


def runs(mode):
    """[(gs, ranged)]: every data scale of the mode; the split mode without range tracking at gs = 1 as well"""
    return [(gs, True) for gs in GC.scales_of(mode)] + ([(1.0, False)] if mode == "split" else [])


class StageCase:
    def __init__(self, C, chained, flat, B, H, W, n1="shared", n2="shared", skip="fir", want_out2=True, rgb=True, **expect):
        assert not (flat and skip == "fir") and (chained or rgb or want_out2) and B in (1, 2)
        self.C, self.chained, self.flat, self.B, self.H, self.W = C, chained, flat, B, H, W
        self.n1, self.n2, self.skip, self.want_out2, self.rgb, self.expect = n1, n2, skip if rgb else "none", want_out2, rgb, expect
        self.WM, self.WGM, self.WGN, self.RW, self.BK, self.XCHG = (CHAINED if chained else UNCHAINED)[C]
        self.TH, self.TW = self.RW * self.WGN, 64 // self.RW
        self.up = 1 if flat else 2
        self.OH, self.OW = self.up * H, self.up * W

    @property
    def id(self):
        nz = {"shared": "s", "per_sample": "p", None: "0"}
        return (f"C{self.C}" + ("c" if self.chained else "u") + ("-flat" if self.flat else "") +
                f"-B{self.B}-H{self.H}-W{self.W}-n{nz[self.n1]}{nz[self.n2]}" +
                (f"-{self.skip}" if self.rgb else "-norgb") + ("" if self.want_out2 else "-noout2"))

    @property
    def base(self):
        return (self.C, self.chained)

    def per_sample(self, which):
        return getattr(self, which) == "per_sample" and self.B > 1

    def tile_origin(self, i):
        tx = self.OW // self.TW
        return (i // tx) * self.TH, (i % tx) * self.TW

    def is_interior(self, i):
        oy0, ox0 = self.tile_origin(i)
        return (not self.flat) and oy0 // 2 >= 1 and oy0 // 2 + self.TH // 2 < self.H and ox0 // 2 >= 1 and ox0 // 2 + self.TW // 2 < self.W

    @property
    def tiles(self):
        return (self.OW // self.TW) * (self.OH // self.TH)

    def regime(self):
        return dict(tile=(self.TH, self.TW), tiles=self.tiles, swizzled=self.tiles % 8 == 0,
                    interior=sum(self.is_interior(i) for i in range(self.tiles)), stages=self.C // self.BK, square=self.H == self.W,
                    xchg=self.XCHG)

    def tensors(self, gs=1.0):
        """y [B,C,H,W]; n1, n2 [1 | B,1,OH,OW] | None; b1, b2 [C]; W2 [C,C], Wn [C/2,C], Wrgb [3,C]; brgb [3];
        skip [B,3,H,W] (fir) | [B,3,OH,OW] (plain) | None"""
        B, C, H, W, OH, OW = self.B, self.C, self.H, self.W, self.OH, self.OW
        g = GC._gen(21, C, self.chained, self.flat, B, H, W)
        y = torch.randn(B, C, H, W, generator=g) * (1.0 + 3.0 * torch.rand(1, C, 1, 1, generator=g))
        if B > 1:
            y = y * torch.tensor(SPREAD).reshape(B, 1, 1, 1)
        n1 = torch.randn(B if self.per_sample("n1") else 1, 1, OH, OW, generator=g)
        n2 = torch.randn(B if self.per_sample("n2") else 1, 1, OH, OW, generator=g)
        b1, b2 = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
        W2, Wn = torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C // 2, C, generator=g) / math.sqrt(C)
        Wrgb, brgb = torch.randn(3, C, generator=g) / math.sqrt(C), torch.randn(3, generator=g)
        skip = torch.randn(B, 3, *((H, W) if self.skip == "fir" else (OH, OW)), generator=g)
        return dict(y=y * gs, n1=n1 * gs if self.n1 else None, n2=n2 * gs if self.n2 else None, b1=b1 * gs, b2=b2 * gs, W2=W2, Wn=Wn,
                    Wrgb=Wrgb, brgb=brgb * gs, skip=skip * gs if self.skip != "none" else None)

    def window(self, t, r, Hs):
        """(case, tensors) of the low-resolution rows r .. r + Hs - 1 of this up-sampling case, noise and skip windows matched: its
        output rows 2 .. 2 Hs - 3 (every FIR tap inside the window) are rows 2 r + 2 .. of this case's"""
        assert not self.flat and 0 <= r and r + Hs <= self.H
        c = StageCase(self.C, self.chained, False, self.B, Hs, self.W, self.n1, self.n2, self.skip, self.want_out2, self.rgb)
        s = dict(t)
        s["y"] = t["y"][:, :, r:r + Hs].contiguous()
        for k in ("n1", "n2"):
            s[k] = t[k][:, :, 2 * r:2 * (r + Hs)].contiguous() if t[k] is not None else None
        if t["skip"] is not None:
            s["skip"] = (t["skip"][:, :, r:r + Hs] if self.skip == "fir" else t["skip"][:, :, 2 * r:2 * (r + Hs)]).contiguous()
        return c, s

    def mutants(self):
        rg = self.regime()
        m = ["drop_stage_last_channel", "slope_sign", "gain_before_bias"]
        m += ["halo_left_zero"] if rg["interior"] else []
        m += ["tile_slot_copied"] if (rg["swizzled"] and rg["tiles"] >= 16) else []
        m += ["hw_exchanged"] if self.H != self.W else []
        m += ["n1_row_down"] if self.n1 else []
        m += ["kgroups_swapped"] if self.chained else []
        m += ["rgb_row_lost"] if self.rgb else []
        m += ["skip_parity"] if self.skip == "fir" else []
        m += ["n1_sample0"] if self.per_sample("n1") else []
        m += ["n2_sample0"] if self.per_sample("n2") else []
        return m


# the mutants of rgb's and y_next's own arithmetic: held to the second bound, given the out2 they fold
OWN_MUTANTS = ("kgroups_swapped", "rgb_row_lost", "skip_parity")
MUTANTS = ["halo_left_zero", "tile_slot_copied", "hw_exchanged", "n1_row_down", "drop_stage_last_channel", "kgroups_swapped",
           "rgb_row_lost", "skip_parity", "n1_sample0", "n2_sample0", "slope_sign", "gain_before_bias"]


# ------------------------------------------------------------------------------------------------------------------ reference
def epi(v, nz, nw, bias, dtype, mutant=None):
    """GC.epilogue_ref with the noise weight as an argument; v [B,C,P], nz [1 | B,1,P] | None"""
    t1 = v if nz is None else v + nw * nz.to(dtype)
    b = bias.to(dtype)[None, :, None]
    if mutant == "gain_before_bias":
        return GC.lrelu(t1 * GAIN + b)
    return GC.lrelu(t1 + b, mutant) * GAIN


def epi_bound(v64, e_v, nz, nw, bias):
    """GC.epilogue_bound with the noise weight as an argument"""
    nzw = nw * nz.double() if nz is not None else torch.zeros(1, 1, 1, dtype=F64)
    t1 = v64 + nzw
    t2 = t1 + bias.double()[None, :, None]
    out = GC.lrelu(t2) * GAIN
    return GAIN * (e_v + U * (nzw.abs() + t1.abs() + t2.abs())) + 2 * U * out.abs()


def _flat_noise(nz):
    return None if nz is None else nz.reshape(nz.shape[0], 1, -1)


def _skip_term(case, skip, dtype, absolute=False, mutant=None):
    if skip is None:
        return None
    skip = skip.to(dtype)
    if case.skip == "fir":
        fir = FIR.to(dtype)
        s = upfir((skip.abs() if absolute else skip).reshape(-1, case.H, case.W), fir.abs() if absolute else fir)
        s = s.reshape(case.B, 3, case.OH, case.OW)
        if mutant == "skip_parity":
            s = s.reshape(case.B, 3, case.OH // 2, 2, case.OW).flip(3)
        return s.reshape(case.B, 3, -1)
    return (skip.abs() if absolute else skip).reshape(case.B, 3, -1)


def stage_ref(case, t, dtype, mutant=None, gemm=None, out2=None):
    """dict(act1, out2, rgb, y_next), each [B,ch,P] (rgb / y_next None where the case has none).  gemm(which, w, a): the
    contraction of conv2 (which = 0) and of the chained GEMM (which = 1), torch.matmul unless an emulation of the bf16 or split
    mode replaces it; out2: the activation to take rgb and y_next of instead of the reference's own."""
    gemm = gemm if gemm is not None else (lambda which, w, a: torch.matmul(w, a))
    B, C, H, W, OH, OW = case.B, case.C, case.H, case.W, case.OH, case.OW
    y = t["y"].to(dtype)
    if mutant == "hw_exchanged":
        iy, ix = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        y = y.reshape(B, C, -1)[:, :, ((iy * H + ix) % (H * W)).reshape(-1)].reshape(B, C, H, W)
    if case.flat:
        v1 = y
    else:
        v1 = upfir(y.reshape(-1, H, W), FIR).reshape(B, C, OH, OW)
        if mutant == "halo_left_zero":
            oy0, ox0 = case.tile_origin(next(i for i in range(case.tiles) if case.is_interior(i)))
            y0 = y.clone()
            y0[..., ox0 // 2 - 1] = 0
            v0 = upfir(y0.reshape(-1, H, W), FIR).reshape(B, C, OH, OW)
            v1 = v1.clone()
            v1[:, :, oy0:oy0 + case.TH, ox0:ox0 + case.TW] = v0[:, :, oy0:oy0 + case.TH, ox0:ox0 + case.TW]
    v1 = v1.reshape(B, C, -1)
    n1, n2 = t["n1"], t["n2"]
    if mutant == "n1_row_down":
        n1 = torch.roll(n1, -1, 2)
    if mutant == "n1_sample0":
        n1 = n1[0:1]
    if mutant == "n2_sample0":
        n2 = n2[0:1]
    act1 = epi(v1, _flat_noise(n1), NW1, t["b1"], dtype, mutant if mutant == "slope_sign" else None)
    W2, Wn, Wrgb = (t[k].to(dtype).clone() for k in ("W2", "Wn", "Wrgb"))
    if mutant == "drop_stage_last_channel":
        W2[:, case.BK - 1] = 0
    if mutant == "kgroups_swapped":
        Wn[:, 0:16], Wn[:, 16:32] = Wn[:, 16:32].clone(), Wn[:, 0:16].clone()
    if mutant == "rgb_row_lost":
        Wrgb[:, C - 16 * case.WM:] = 0
    if out2 is None:
        out2 = epi(gemm(0, W2, act1), _flat_noise(n2), NW2, t["b2"], dtype, mutant if mutant == "gain_before_bias" else None)
    else:
        out2 = out2.to(dtype).reshape(B, C, -1)
    rgb = y_next = None
    if case.rgb:
        rgb = torch.matmul(Wrgb, out2) + t["brgb"].to(dtype)[None, :, None]
        s = _skip_term(case, t["skip"], dtype, mutant=mutant)
        rgb = rgb + s if s is not None else rgb
    if case.chained:
        y_next = gemm(1, Wn, out2)
    res = dict(act1=act1, out2=out2, rgb=rgb, y_next=y_next)
    if mutant == "tile_slot_copied":
        (sy, sx), (dy, dx) = case.tile_origin(1), case.tile_origin(case.tiles // 8)
        for k in ("out2", "rgb", "y_next"):
            if res[k] is not None:
                v = res[k].reshape(B, -1, OH, OW).clone()
                v[:, :, dy:dy + case.TH, dx:dx + case.TW] = v[:, :, sy:sy + case.TH, sx:sx + case.TW].clone()
                res[k] = v.reshape(B, -1, OH * OW)
    return res


# ------------------------------------------------------------------------------------------------------- exponents, emulations
def replay_exps(case, t, ranged=True):
    """[(e1, e2)] per sample as the kernel's wave 0 makes them, in fp64; ranged=False: zeros"""
    if not ranged:
        return [(0, 0)] * case.B
    fir = FIR.double().abs()
    gain = 1.0 if case.flat else max(float(fir[py::2, px::2].sum()) for py in (0, 1) for px in (0, 1))
    amax = lambda v: float(v.double().abs().max()) if v is not None else 0.0      # noqa: E731
    c0, c1 = GAIN * (abs(NW1) * amax(t["n1"]) + amax(t["b1"])), GAIN * gain
    c0n, c1n = GAIN * (abs(NW2) * amax(t["n2"]) + amax(t["b2"])), GAIN * math.sqrt(case.C)
    out = []
    for b in range(case.B):
        u1 = c1 * amax(t["y"][b]) + c0
        out.append((split_exp(u1), split_exp(c1n * u1 + c0n)))
    return out


def _pow2(exps, which, sign=1.0, extra=0):
    return torch.tensor([2.0 ** (sign * (e[which] + extra)) for e in exps], dtype=F64).reshape(-1, 1, 1)


def emulate(case, t, mode, exps=None):
    """a correct implementation of `mode` in fp32 on the CPU: stage_ref with the mode's contraction"""
    if mode == "fp32":
        return stage_ref(case, t, F32)
    if mode == "bf16":
        return stage_ref(case, t, F32, gemm=lambda which, w, a: torch.matmul(bf16_round(w), bf16_round(a)))

    def gemm(which, w, a):
        k, kin = _pow2(exps, which, -1.0).to(F32), (_pow2(exps, which) / 256.0).to(F32)
        wh, wl = split16(w * 256.0)
        ah, al = split16(a * k)
        return torch.matmul(torch.cat([wl, wh, wh], 1), torch.cat([ah, al, ah], 1)) * kin

    return stage_ref(case, t, F32, gemm=gemm)


# --------------------------------------------------------------------------------------------------------------------- bounds
def contract_bound(w, a, e_a, mode, k, k3, pe=None):
    """bound of W a where the kernel's operand is within e_a of a; w [M,K], a [B,K,P] fp64; pe [B,1,1]: 2^(E + 1)"""
    aw, aa = w.double().abs(), a.double().abs()
    ak = aa + e_a
    mm = torch.matmul
    if mode == "fp32":
        return mm(aw, e_a + torch.zeros_like(aa)) + gamma(k) * mm(aw, ak)
    if mode == "bf16":
        d_w, d_a = 2.0 ** -8 * aw, 2.0 ** -8 * ak + e_a          # (half an ulp of 8 significant bits, bottom of the binade)
        return mm(aw, d_a) + mm(d_w, aa) + mm(d_w, d_a) + gamma(k) * mm(aw + d_w, aa + d_a)
    rep_w, low_w = 2.0 ** -22 * aw + 2.0 ** -33, (2.0 ** -11 + 2.0 ** -22) * aw + 2.0 ** -32
    rep_a, low_a = 2.0 ** -22 * ak + 2.0 ** -25 * pe, (2.0 ** -11 + 2.0 ** -22) * ak + 2.0 ** -24 * pe
    three = mm(aw + low_w, ak + low_a) + mm(aw + low_w, low_a) + mm(low_w, ak + low_a)
    return mm(aw, e_a + rep_a) + mm(rep_w, ak) + mm(rep_w, rep_a) + mm(low_w, low_a) + gamma(k3) * three


def next_counts(case):
    if case.XCHG:
        return case.C + 8, 3 * case.C + 8
    return 16 * case.WM + 8 + case.WGM - 1, 48 * case.WM + 8 + case.WGM - 1


def stage_bounds(case, t, mode, exps=None, out2=None):
    """(ref, bound): dicts over act1, out2, rgb, y_next in fp64.  out2 (the tensor a launch stored): rgb and y_next against
    their own arithmetic alone, e(out2) = 0."""
    B, C = case.B, case.C
    ref = stage_ref(case, t, F64, out2=out2)
    e = dict(act1=None, out2=None, rgb=None, y_next=None)
    pe1 = pe2 = None
    if mode == "split":
        pe1, pe2 = _pow2(exps, 0, extra=1), _pow2(exps, 1, extra=1)
    if out2 is None:
        y = t["y"].double()
        if case.flat:
            v1, e_v1 = y.reshape(B, C, -1), 0.0
        else:
            v1 = upfir(y.reshape(-1, case.H, case.W), FIR.double()).reshape(B, C, -1)
            e_v1 = gamma(4) * upfir(y.abs().reshape(-1, case.H, case.W), FIR.double().abs()).reshape(B, C, -1)
        e["act1"] = epi_bound(v1, e_v1, _flat_noise(t["n1"]), NW1, t["b1"])
        W2 = t["W2"].double()
        e_v2 = contract_bound(W2, ref["act1"], e["act1"], mode, C + 8, 3 * C + 8, pe1)
        e["out2"] = epi_bound(torch.matmul(W2, ref["act1"]), e_v2, _flat_noise(t["n2"]), NW2, t["b2"])
        e_o = e["out2"]
    else:
        e_o = torch.zeros_like(ref["out2"])
    if case.rgb:
        awr, has_skip = t["Wrgb"].double().abs(), t["skip"] is not None
        k_rgb = 4 * case.WM + 2 + case.WGM - 1 + 1 + (1 if has_skip else 0)
        e_rgb = torch.matmul(awr, e_o) + gamma(k_rgb) * torch.matmul(awr, ref["out2"].abs() + e_o) + \
            gamma(2 if has_skip else 1) * t["brgb"].double().abs()[None, :, None]
        if has_skip:
            e_rgb = e_rgb + (gamma(5) if case.skip == "fir" else U) * _skip_term(case, t["skip"], F64, absolute=True)
        e["rgb"] = e_rgb
    if case.chained:
        k, k3 = next_counts(case)
        e["y_next"] = contract_bound(t["Wn"], ref["out2"], e_o, mode, k, k3, pe2)
    return ref, e


# ---------------------------------------------------------------------------------------------------------------- the cases
def _c(C, chained, B, H, W, **kw):
    return StageCase(C, chained, False, B, H, W, **kw)


def _f(C, chained, B, H, W, **kw):
    kw.setdefault("skip", "plain")
    return StageCase(C, chained, True, B, H, W, **kw)


P, S, N = "per_sample", "shared", None
CASES = [
    # 2 x 64 tiles: C = 32, C = 64 unchained, C = 64 and 128 chained.  plain order + interior | swizzled + interior | no interior
    _c(32, False, 1, 4, 96, tile=(2, 64), tiles=12, interior=2, swizzled=False, stages=1),
    _c(32, False, 2, 8, 96, n1=P, n2=S, skip="plain", want_out2=False, tiles=24, interior=6, swizzled=True),
    _c(32, False, 1, 2, 32, n1=N, n2=N, skip="none", tiles=2, interior=0),
    _c(64, False, 2, 4, 96, n1=S, n2=P, want_out2=False, tile=(2, 64), tiles=12, interior=2, swizzled=False, stages=4),
    _c(64, False, 1, 8, 96, skip="none", tiles=24, interior=6, swizzled=True),
    _c(64, False, 2, 2, 32, n1=P, n2=P, skip="plain", tiles=2, interior=0),
    _c(64, True, 2, 4, 96, n1=P, n2=P, tile=(2, 64), tiles=12, interior=2, swizzled=False, stages=4, xchg=True),
    _c(64, True, 1, 8, 96, n1=N, n2=S, skip="plain", tiles=24, interior=6, swizzled=True),
    _c(64, True, 1, 2, 32, rgb=False, tiles=2, interior=0),
    _c(128, True, 1, 4, 96, tile=(2, 64), tiles=12, interior=2, swizzled=False, stages=4, xchg=False),
    _c(128, True, 2, 8, 96, n1=P, n2=S, rgb=False, tiles=24, interior=6, swizzled=True),
    _c(128, True, 2, 2, 32, n1=S, n2=P, skip="plain", want_out2=False, tiles=2, interior=0),
    # 4 x 64 tiles: C = 128 unchained
    _c(128, False, 2, 6, 96, n1=P, n2=P, tile=(4, 64), tiles=9, interior=1, swizzled=False, stages=4),
    _c(128, False, 1, 16, 96, skip="plain", tiles=24, interior=6, swizzled=True),
    _c(128, False, 1, 2, 32, n1=N, n2=N, skip="none", tiles=1, interior=0),
    # 2 x 32 tiles: C = 256, both forms
    _c(256, False, 1, 6, 96, tile=(2, 32), tiles=36, interior=16, swizzled=False, stages=4),
    _c(256, False, 2, 4, 64, n1=P, n2=S, skip="plain", want_out2=False, tiles=16, interior=4, swizzled=True),
    _c(256, False, 1, 2, 32, n1=S, n2=N, skip="none", tiles=4, interior=0),
    _c(256, True, 1, 6, 96, tile=(2, 32), tiles=36, interior=16, swizzled=False, stages=4, xchg=True),
    _c(256, True, 2, 4, 64, n1=S, n2=P, rgb=False, tiles=16, interior=4, swizzled=True),
    _c(256, True, 2, 2, 32, n1=P, n2=P, skip="plain", tiles=4, interior=0),
    # flat forms (W % 64 == 0, H % 4 == 0): both tile orders of every tile shape
    _f(32, False, 1, 4, 64, tiles=2, swizzled=False),
    _f(64, False, 1, 8, 128, skip="none", tiles=8, swizzled=True),
    _f(64, True, 2, 8, 128, n1=P, n2=P, tiles=8, swizzled=True),
    _f(128, True, 1, 4, 64, n1=N, n2=S, tiles=2, swizzled=False),
    _f(128, False, 1, 16, 128, tile=(4, 64), tiles=8, swizzled=True),
    _f(256, False, 2, 4, 64, n1=S, n2=P, want_out2=False, tiles=4, swizzled=False),
    _f(256, True, 1, 8, 128, tile=(2, 32), tiles=16, swizzled=True),
]
# tile-order independence: (the taller case, first low-resolution row and height of the window) -- one order each, same data
ORDER_PAIRS = [(_c(32, False, 1, 8, 96), 2, 4), (_c(64, False, 2, 8, 96, n1=P, n2=P), 2, 4), (_c(64, True, 2, 8, 96, n1=P, n2=P, skip="plain"), 2, 4),
               (_c(128, True, 1, 8, 96), 2, 4), (_c(128, False, 1, 16, 96), 4, 6), (_c(256, False, 1, 6, 96), 1, 4),
               (_c(256, True, 2, 6, 96, n1=P, n2=P), 1, 4)]
# bf16 storage and the uint8 image: non-square, interior tiles
YB_CASES = [_c(64, True, 1, 4, 96), _c(256, True, 2, 6, 96, n1=P, n2=P, skip="plain"), _c(128, True, 1, 4, 96, rgb=False), _c(32, False, 1, 4, 96)]
U8_CASES = [_c(32, False, 2, 4, 96, n1=P, n2=P), _c(256, False, 1, 6, 96, skip="plain"), _c(64, True, 1, 4, 96, skip="none")]
