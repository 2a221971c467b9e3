"""Cases, fp64 references and rounding-error bounds of the 3x3 modulated convolution (csrc/conv3x3.hip: modconv3x3_kernel and
modconv3x3_split_kernel, each as <WM = 1 | 2, UP = false | true>), of the 3x3 fragment layouts of cips3d_modulate_weights
(csrc/modulate.hip) and of the direct modconv_kxk_kernel (csrc/decoder_ops.hip).  Shared by test_conv3x3_cases_host.py (CPU: every
bound admits the fp32 evaluation and the split emulation, rejects every mutant; every case sits in its regime) and
test_gpu_conv3x3.py (the kernels).  Imports no GPU code.  Built on tests/_gemm1x1_cases.py (GC) and tests/_fused_stage_cases.py (FC),
whose conventions hold: u = 2^-24, gamma_k = k u / (1 - k u), bounds per element in fp64 with no absolute floor, a term charged one
rounding for every addition that can come after it, eight roundings set aside for the inside of a matrix instruction's chain, all
data multiplied by a power of two `gs`.

Reference (`conv_ref`): one torch expression, generic in its dtype, in the order of the reference model (models/model_v3.py:264-314):
    plain   conv2d(x, w, padding = 1)
    up      conv_transpose2d(x, w, stride = 2)  ->  (2H + 1) x (2W + 1),  then the 4 x 4 blur, a true convolution behind a pad of (1, 1)
then, with epilogue 1, GC.epilogue_ref (noise weight 0.3, a bias that differs per channel).  w [Cout,Cin,3,3] is one explicit
matrix shared by the samples; the GPU test sends it through cips3d_modulate_weights without demodulation, with scale 1.0 and styles
of ones -- an exact product, so kernel and reference see the same numbers in whatever fragment layout the kernel wants.  The FIR is
GC.FIR, asymmetric in both directions, handed to the kernel as it is (the kernel takes the taps "as the Blur holds them").

The kernel computes the up-sampling form COMMUTED: Z = the FIR of the zero-stuffed input (pad (3, 2): (2H + 2) x (2W + 2)), then a
valid 3 x 3 correlation of Z with the flipped taps.  `z_of` / `commuted` state that form -- Z by the kernel's polyphase rule, a0 =
(ny + 1) & 1, iy0 = (ny - 3 + a0) >> 1 and the same for columns -- for the split emulation and for the mutants, never for the
reference: the commutation, the flip and the parities are tested, the host test shows both forms agree in fp64 and that the fp32
evaluation of the commuted form stays inside the bound against the model-order fp64 reference.  In the plain form Z is x behind a
ring of stored zeros.  In Z's coordinates the tile at (oy0, ox0) reads rows oy0 .. oy0 + 5 and columns ox0 .. ox0 + 65: column ox0 is
its left halo, ox0 + 65 its right halo, row oy0 its top halo.

Bounds (`conv_bound`), as FC.contract_bound of the contraction over the 9 Cin products of an output element (the unfolded Z):
fp32, plain   one accumulator chain of v_mfma_f32_16x16x4_f32 over nstage x 3 x 4 x 3 instructions of four products = 9 Cin terms;
              taps outside the image multiply stored zeros: exact.           e = gamma_(9 Cin + 8) sum |w x|
fp32, up      fill_store: acc = 0, then four fmas per halo element:          e(Z) = gamma_4 upfir(|x|, |fir|)
                                                                            e = sum |w| e(Z) + gamma_(9 Cin + 8) sum |w| (|Z| + e(Z))
split         GC's rep / low for both operands, the activation side Z 2^-E:  per K stage five tap pairs x three instructions of 32
              products; the tenth tap's weights are stored zeros and add exact zeros, 27 Cin terms remain.
              e = sum (|w| (e(Z) + rep(Z)) + rep(w) Zk + rep(w) rep(Z) + low(w) low(Z)) + gamma_(27 Cin + 8) sum (|wh zh| + |wh zl| + |wl zh|)
              with Zk = |Z| + e(Z) and the last sum bounded from |wh| <= |w| + low(w), |wl| <= low(w) and the same for Z (FC's form:
              the kernel's Z differs from any emulated Z by e(Z), so emulated halves are not the kernel's).
              E = cips3d_split_exp(amax handed to the kernel x sum |fir| in the up form), 0 without a range (`replay_exps`).  The
              kernel forms the product in fp32: every absolute term is charged one binade above the replayed exponent, 2^(E + 1).
              Stored zeros of the plain form's ring are charged rep's absolute term 2^-24 2^E as well: 2^-38 of the amax, no teeth lost.
The epilogue is GC.epilogue_bound on top.  split / fp32 bound is (27 Cin + 20) / (9 Cin + 8) to first order in the plain form.
On the CPU the "correct implementation" of the split mode is `split_emulated`: Z in fp32, times 2^-E, GC.split16 on both operands,
one fp32 convolution over the 27 Cin products, times 2^E 2^-8 -- built from mfma_frag.h's definitions.

`regime()` replays the launch at the bottom of conv3x3.hip -- tile 4 x 64, tile columns and rows, tiles per sample, swizzled =
tiles % 8 == 0 (the XCD-aware permutation), nstage = Cin / 16, WM = 2 iff Cout % 32 == 0 -- to CHOOSE and label cases, never for a
reference.  Tile origins are multiples of 64 columns and 4 rows, so in the up form a tile boundary always falls on an even
low-resolution column (32 tx); the two polyphase column parities are met at the two halo columns instead: the left halo is an even
Z column (b0 = 1), the right halo an odd one (b0 = 0), and cases with two and three tile columns put both inside a neighbour.
With B = 2 the samples' magnitudes are 2^9 apart, in both orders: an exponent taken from the other sample either overflows the
large sample's fp16 halves or costs the small one nine bits (the host test checks the overflow).

Mutants (subtly wrong evaluations in fp64; each leaves its bound on the CPU, test_conv3x3_cases_host.py):
    halo_left_zero, halo_right_zero   the halo column of a tile with a neighbour on that side read as zero
    halo_top_zero             the top halo row of the first tile of the second tile row read as zero
    taps_unflipped            up form with the taps of the plain form
    fir_mirrored              the FIR mirrored left to right
    row_parity                a0 of the polyphase inverted
    hw_exchanged              H and W exchanged in the row stride of x (iy H + ix for iy W + ix): visible when H != W
    tile_slot_copied          as in FC: tile tiles / 8 holds tile 1's values
    drop_stage_last_channel   channel 15 lost
    last_stage_skipped        the last 16 channels lost (odd nstage)
    block2_first_weights      output channels 16 .. 31 computed from the weights of channels 0 .. 15 (WM = 2)
    tap9_twice                split: the tenth tap holds the ninth tap's weights
    cross_lost                split: the products wl zh lost.  2^-11 per term with mixed signs against a worst-case chain bound: it
                              leaves the bound where the contraction is short (Cin = 16), not at every case -- which is what the
                              constant bar of the earlier tests could not show at any size
    noise_sample0, bias_next_channel, slope_sign, gain_before_bias   the epilogue's

Weight layouts: `unpack3x3` / `unpack3x3_split` invert the index maps of modulate_row for ksq = 9 (stated in test_gpu_conv3x3.py's
packing tests); the values are held to GC.mod_bound (+ rep(w) for the split halves) against GC.mod_ref.
Direct kernel: one sequential fma chain over k^2 Cin products per output: e = gamma_(k^2 Cin) sum |w x|; transpose2 against
conv_transpose2d(stride 2) alone.
"""
import math

import torch
import torch.nn.functional as TF

import _gemm1x1_cases as GC
import _fused_stage_cases as FC
from _gemm1x1_cases import F32, F64, FIR, NOISE_W, SCALES, SPLIT_SCALES, U, gamma, split16, split_exp, upfir, worst  # noqa: F401
from _gemm1x1_cases import epilogue_bound, epilogue_ref, unpack, unpack_split  # noqa: F401

MODES = ("fp32", "split")
TH, TW, BK = 4, 64, 16
SPREADS = {"big_first": (2.0 ** 9, 1.0), "big_second": (1.0, 2.0 ** 9)}


def runs(mode):
    """[(gs, ranged)]: every data scale of the mode; the split mode without a range at gs = 1 as well"""
    return [(gs, True) for gs in GC.scales_of(mode)] + ([(1.0, False)] if mode == "split" else [])


class ConvCase:
    def __init__(self, Cin, Cout, H, W, up=False, B=1, epilogue=0, noise="shared", amax="measured", spread=None, zero=None, **expect):
        """H, W: the input's size.  noise: "shared" | "per_sample" | None (epilogue 1 only); amax (split mode): "measured" | "loose"
        (2^3 above the true maximum); spread: a key of SPREADS; zero: the index of an all-zero sample; expect: the regime."""
        self.Cin, self.Cout, self.H, self.W, self.up, self.B, self.epilogue = Cin, Cout, H, W, up, B, epilogue
        self.noise = noise if epilogue == 1 else None
        self.amax, self.spread, self.zero, self.expect = amax, spread, zero, expect
        self.OH, self.OW = (2 * H, 2 * W) if up else (H, W)

    @property
    def id(self):
        sw = ("" if self.epilogue == 0 else {"shared": "-ep", "per_sample": "-epB", None: "-ep0n"}[self.noise]) + \
            ("-loose" if self.amax == "loose" else "") + (f"-{self.spread}" if self.spread else "") + \
            (f"-zero{self.zero}" if self.zero is not None else "")
        return ("up" if self.up else "pl") + f"-B{self.B}-i{self.Cin}-o{self.Cout}-H{self.H}-W{self.W}{sw}"

    @property
    def tiles_x(self):
        return GC.ceil_div(self.OW, TW)

    @property
    def tiles_y(self):
        return GC.ceil_div(self.OH, TH)

    @property
    def tiles(self):
        return self.tiles_x * self.tiles_y

    @property
    def WM(self):
        return 2 if self.Cout % 32 == 0 else 1

    @property
    def nstage(self):
        return self.Cin // BK

    @property
    def per_sample_noise(self):
        return self.noise == "per_sample" and self.B > 1

    def tile_origin(self, i):
        return (i // self.tiles_x) * TH, (i % self.tiles_x) * TW

    def regime(self):
        return dict(tile=(TH, TW), tiles_x=self.tiles_x, tiles_y=self.tiles_y, tiles=self.tiles, swizzled=self.tiles % 8 == 0,
                    nstage=self.nstage, WM=self.WM, row_blocks=self.Cout // (16 * self.WM), ragged_rows=self.OH % TH != 0,
                    tail=self.OW - (self.tiles_x - 1) * TW, square=self.H == self.W)

    def tensors(self, gs=1.0):
        """x [B,Cin,H,W], w [Cout,Cin,3,3] (rows of about unit norm), noise [1 | B,1,OH OW] | None, bias [Cout]"""
        g = GC._gen(31, self.Cin, self.Cout, self.H, self.W, self.up, self.B)
        x = torch.randn(self.B, self.Cin, self.H, self.W, generator=g) * (1.0 + 3.0 * torch.rand(1, self.Cin, 1, 1, generator=g))
        if self.spread:
            x = x * torch.tensor(SPREADS[self.spread]).reshape(self.B, 1, 1, 1)
        if self.zero is not None:
            x[self.zero] = 0.0
        w = torch.randn(self.Cout, self.Cin, 3, 3, generator=g) / math.sqrt(9 * self.Cin)
        noise = torch.randn(self.B if self.per_sample_noise else 1, 1, self.OH * self.OW, generator=g)
        bias = torch.randn(self.Cout, generator=g) * 0.5
        return dict(x=x * gs, w=w, noise=noise * gs if self.noise else None, bias=bias * gs)

    def amax_given(self, t):
        """[B] the amax handed to the split kernel: the measured maximum of x per sample, or 2^3 times that"""
        m = t["x"].abs().amax((1, 2, 3))
        return m * 8.0 if self.amax == "loose" else m

    def mutants(self, mode):
        m = ["drop_stage_last_channel"]
        m += ["halo_left_zero", "halo_right_zero"] if self.tiles_x >= 2 else []
        m += ["halo_top_zero"] if self.tiles_y >= 2 else []
        m += ["taps_unflipped", "fir_mirrored", "row_parity"] if self.up else []
        m += ["hw_exchanged"] if self.H != self.W and min(self.H, self.W) > 1 else []
        m += ["tile_slot_copied"] if (self.tiles % 8 == 0 and self.tiles >= 16) else []
        m += ["last_stage_skipped"] if (self.nstage % 2 == 1 and self.nstage >= 3) else []
        m += ["block2_first_weights"] if self.WM == 2 else []
        m += ["tap9_twice"] if (mode == "split" and self.OH > 1) else []      # (one row: the ninth tap reads the ring of zeros)
        m += ["cross_lost"] if (mode == "split" and self.Cin == 16 and self.OH * self.OW <= 64) else []
        if self.epilogue == 1:
            m += ["bias_next_channel", "slope_sign", "gain_before_bias"] + (["noise_sample0"] if self.per_sample_noise else [])
        return m


EPILOGUE_MUTANTS = ("bias_next_channel", "slope_sign", "gain_before_bias", "noise_sample0")
MUTANTS = ["halo_left_zero", "halo_right_zero", "halo_top_zero", "taps_unflipped", "fir_mirrored", "row_parity", "hw_exchanged",
           "tile_slot_copied", "drop_stage_last_channel", "last_stage_skipped", "block2_first_weights", "tap9_twice", "cross_lost",
           "noise_sample0", "bias_next_channel", "slope_sign", "gain_before_bias"]


# ------------------------------------------------------------------------------------------------------------------ reference
def conv_ref(case, t, dtype):
    """the accumulator [B,Cout,OH,OW] in the reference model's order"""
    x, w = t["x"].to(dtype), t["w"].to(dtype)
    if not case.up:
        return TF.conv2d(x, w, padding=1)
    y = TF.conv_transpose2d(x, w.transpose(0, 1), stride=2)                      # [B,Cout,2H + 1,2W + 1]
    y = TF.pad(y, (1, 1, 1, 1)).reshape(-1, 1, case.OH + 3, case.OW + 3)
    return TF.conv2d(y, FIR.to(dtype).flip(0, 1)[None, None]).reshape(case.B, case.Cout, case.OH, case.OW)


def finish(case, v, t, dtype, mutant=None):
    """the tensor the launch stores, given the accumulator"""
    if case.epilogue != 1:
        return v
    tt = dict(t)
    if mutant == "bias_next_channel":
        tt["bias"] = torch.roll(t["bias"], -1)
    return epilogue_ref(v.reshape(case.B, case.Cout, -1), tt, dtype, case.per_sample_noise, mutant).reshape(v.shape)


def out_ref(case, t, dtype):
    return finish(case, conv_ref(case, t, dtype), t, dtype)


# ------------------------------------------------------------------------------------------------- the kernel's commuted form
def z_upfir(x, fir):
    """Z [B,C,2H + 2,2W + 2] = upfirdn2d(x, fir, up = 2, pad = (3, 2)) from GC.upfir (pad (2, 1)) of x behind one ring of zeros"""
    B, C, H, W = x.shape
    return upfir(TF.pad(x, (1, 1, 1, 1)).reshape(-1, H + 2, W + 2), fir.to(x.dtype))[:, 1:2 * H + 3, 1:2 * W + 3].reshape(B, C, 2 * H + 2, 2 * W + 2)


def z_of(case, x, fir=FIR, mutant=None):
    """what the halo tiles hold, over the whole map: [B,Cin,OH + 2,OW + 2].  Up form by the kernel's polyphase rule."""
    if mutant == "hw_exchanged":
        B, C, H, W = x.shape
        iy, ix = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
        x = x.reshape(B, C, -1)[:, :, ((iy * H + ix) % (H * W)).reshape(-1)].reshape(B, C, H, W)
    if not case.up:
        return TF.pad(x, (1, 1, 1, 1))
    fir = fir.to(x.dtype)
    if mutant == "fir_mirrored":
        fir = fir.flip(1)
    kf = fir.flip(0, 1)                                         # kf[a][b] = fir[3 - a][3 - b]
    ny, nx = torch.arange(case.OH + 2), torch.arange(case.OW + 2)
    a0, b0 = (ny + 1) & 1, (nx + 1) & 1
    if mutant == "row_parity":
        a0 = 1 - a0
    iy0 = torch.div(ny - 3 + a0, 2, rounding_mode="floor")
    ix0 = torch.div(nx - 3 + b0, 2, rounding_mode="floor")
    xp = TF.pad(x, (2, 2, 2, 2))
    z = 0
    for da in (0, 1):
        for db in (0, 1):
            tap = kf[(a0 + 2 * da)[:, None], (b0 + 2 * db)[None, :]]
            z = z + xp[:, :, (iy0 + da + 2)[:, None], (ix0 + db + 2)[None, :]] * tap
    return z


def wk_of(case, w):
    """the taps in the kernel's order: flipped in the up form (MOD_FLIP)"""
    return w.flip(2, 3) if case.up else w


def _paste(case, v, alt, tile):
    oy0, ox0 = case.tile_origin(tile)
    v = v.clone()
    v[:, :, oy0:oy0 + TH, ox0:ox0 + TW] = alt[:, :, oy0:oy0 + TH, ox0:ox0 + TW]
    return v


def commuted(case, t, dtype, mutant=None, exps=None):
    """the accumulator [B,Cout,OH,OW] as the kernel forms it: Z, then a valid correlation with the kernel-order taps; with a mutant
    (fp64) a subtly wrong one.  exps: the split exponents, for the split mode's mutants."""
    x, w = t["x"].to(dtype), wk_of(case, t["w"].to(dtype)).clone()
    z = z_of(case, x, FIR, mutant if mutant in ("hw_exchanged", "fir_mirrored", "row_parity") else None)
    if mutant == "taps_unflipped":
        w = t["w"].to(dtype)
    if mutant == "drop_stage_last_channel":
        w[:, BK - 1] = 0
    if mutant == "last_stage_skipped":
        w[:, case.Cin - BK:] = 0
    if mutant == "block2_first_weights":
        w[16:32] = w[0:16].clone()
    if mutant == "tap9_twice":
        w[:, :, 2, 2] *= 2
    v = TF.conv2d(z, w)
    if mutant == "cross_lost":
        k, kin = _pow2(exps, -1.0), _pow2(exps) / 256.0
        wl = split16(wk_of(case, t["w"]) * 256.0)[1].double()
        zh = split16(z_of(case, t["x"]) * k.to(F32))[0].double()
        v = v - TF.conv2d(zh, wl) * kin
    if mutant in ("halo_left_zero", "halo_right_zero", "halo_top_zero"):
        if mutant == "halo_top_zero":
            tile = case.tiles_x
        else:
            tile = 1 if mutant == "halo_left_zero" else max(case.tiles_x - 2, 0)
        oy0, ox0 = case.tile_origin(tile)
        z0 = z.clone()
        if mutant == "halo_top_zero":
            z0[:, :, oy0] = 0
        else:
            z0[:, :, :, ox0 if mutant == "halo_left_zero" else ox0 + TW + 1] = 0
        v = _paste(case, v, TF.conv2d(z0, w), tile)
    if mutant == "tile_slot_copied":
        (sy, sx), (dy, dx) = case.tile_origin(1), case.tile_origin(case.tiles // 8)
        v = v.clone()
        v[:, :, dy:dy + TH, dx:dx + TW] = v[:, :, sy:sy + TH, sx:sx + TW].clone()
    return v


def mutated(case, t, mutant, exps=None):
    """the stored tensor of a subtly wrong implementation, in fp64"""
    if mutant in EPILOGUE_MUTANTS:
        return finish(case, conv_ref(case, t, F64), t, F64, mutant)
    return finish(case, commuted(case, t, F64, mutant, exps), t, F64)


# ----------------------------------------------------------------------------------------------------- exponents, emulation
def fir_gain():
    """sum |taps| as the kernel adds it, an fp32 number"""
    s = torch.zeros((), dtype=F32)
    for v in FIR.flip(0, 1).reshape(-1):
        s = s + v.abs()
    return float(s)


def replay_exps(case, t, ranged=True):
    """[E] per sample: cips3d_split_exp(amax handed in x the FIR's gain); zeros without a range"""
    if not ranged:
        return [0] * case.B
    g = fir_gain() if case.up else 1.0
    return [split_exp(GC.f32(GC.f32(float(a)) * g)) for a in case.amax_given(t)]


def _pow2(exps, sign=1.0, extra=0):
    return torch.tensor([2.0 ** (sign * (e + extra)) for e in exps], dtype=F64).reshape(-1, 1, 1, 1)


def split_emulated(case, t, exps):
    """the split kernel's accumulator as mfma_frag.h defines it, in torch: Z in fp32, fp16 halves, the three products, fp32 sums"""
    k, kin = _pow2(exps, -1.0).to(F32), (_pow2(exps) / 256.0).to(F32)
    wh, wl = split16(wk_of(case, t["w"]) * 256.0)
    zh, zl = split16(z_of(case, t["x"]) * k)
    return TF.conv2d(torch.cat([zh, zl, zh], 1), torch.cat([wl, wh, wh], 1)) * kin


def correct_fp32(case, t, mode, exps=None):
    """the stored tensor of a correct implementation of `mode` in fp32 on the CPU"""
    v = conv_ref(case, t, F32) if mode == "fp32" else split_emulated(case, t, exps)
    return finish(case, v, t, F32)


# --------------------------------------------------------------------------------------------------------------------- bounds
def conv_bound(case, t, mode, exps=None):
    """(fp64 reference, bound) of the stored tensor [B,Cout,OH,OW]"""
    x, w = t["x"].double(), wk_of(case, t["w"].double())
    if case.up:
        z, e_z = z_upfir(x, FIR.double()), gamma(4) * z_upfir(x.abs(), FIR.double().abs())
    else:
        z = TF.pad(x, (1, 1, 1, 1))
        e_z = torch.zeros_like(z)
    pe = _pow2(exps, extra=1).reshape(-1, 1, 1) if mode == "split" else None
    e_v = FC.contract_bound(w.reshape(case.Cout, -1), TF.unfold(z, 3), TF.unfold(e_z, 3), mode, 9 * case.Cin + 8, 27 * case.Cin + 8, pe)
    v = conv_ref(case, t, F64)
    if case.epilogue != 1:
        return v, e_v.reshape(v.shape)
    return finish(case, v, t, F64), epilogue_bound(v.reshape(case.B, case.Cout, -1), e_v, t).reshape(v.shape)


# ------------------------------------------------------------------------------------------------------------------ the cases
def _p(Cin, Cout, H, W, **kw):
    return ConvCase(Cin, Cout, H, W, False, **kw)


def _u(Cin, Cout, H, W, **kw):
    return ConvCase(Cin, Cout, H, W, True, **kw)


P, S, N = "per_sample", "shared", None
CASES = [
    # single-tile minima
    _p(16, 16, 1, 4, tiles=1, nstage=1, WM=1, tail=4),
    _u(16, 16, 1, 2, tiles=1, nstage=1, WM=1, tail=4),
    # rows ragged against the 4-row tile
    _p(16, 32, 5, 8, epilogue=1, noise=S, tiles_y=2, ragged_rows=True, WM=2),
    _p(32, 16, 7, 12, tiles_y=2, ragged_rows=True, nstage=2),
    _u(16, 32, 5, 6, epilogue=1, noise=N, tiles_y=3, ragged_rows=True),
    # columns ragged by one 16-byte piece
    _p(16, 16, 3, 68, tiles_x=2, tail=4),
    _u(16, 16, 2, 34, tiles_x=2, tail=4),
    # width exactly 64 (the right halo outside the image) and exactly 128 (inside the neighbour); two tile columns and rows
    _p(16, 48, 4, 64, tiles_x=1, tail=64, row_blocks=3, WM=1),
    _p(32, 32, 8, 128, B=2, spread="big_first", epilogue=1, noise=P, tiles_x=2, tiles_y=2, tail=64, tiles=4, swizzled=False),
    _u(16, 16, 2, 32, tiles_x=1, tail=64),
    _u(32, 64, 4, 64, B=2, spread="big_second", epilogue=1, noise=P, tiles_x=2, tiles_y=2, tail=64, tiles=4, WM=2, row_blocks=2),
    # permuted tile orders: 8 tiles (two columns), 24 tiles (three columns), and 9 tiles in plain order; H != W
    _p(16, 16, 16, 128, tiles=8, swizzled=True, tiles_x=2),
    _u(16, 32, 8, 64, epilogue=1, noise=S, tiles=8, swizzled=True, tiles_x=2),
    _p(32, 32, 32, 132, tiles=24, swizzled=True, tiles_x=3, tail=4, nstage=2),
    _u(32, 16, 16, 66, tiles=24, swizzled=True, tiles_x=3, tail=4),
    _p(48, 48, 12, 132, tiles=9, swizzled=False, tiles_x=3, nstage=3, row_blocks=3, square=False),
    _u(48, 64, 6, 66, B=2, spread="big_first", tiles=9, swizzled=False, tiles_x=3, nstage=3, WM=2),
    # samples 2^9 apart in the other order, per-sample noise; noise arrangements
    _p(48, 64, 5, 8, B=2, spread="big_second", epilogue=1, noise=P, nstage=3, WM=2, row_blocks=2),
    _u(32, 48, 3, 6, B=2, spread="big_second", epilogue=1, noise=S, nstage=2, row_blocks=3),
    _p(32, 16, 4, 8, B=2, spread="big_first", epilogue=1, noise=N),
    # an amax that is only an upper bound; an all-zero sample beside a live one
    _p(32, 32, 6, 12, B=2, amax="loose", spread="big_second"),
    _u(16, 48, 3, 10, amax="loose", epilogue=1, noise=S),
    _p(16, 32, 4, 8, B=2, zero=0),
    _u(32, 16, 2, 6, B=2, zero=1, epilogue=1, noise=P),
    # a deeper contraction at a single small tile
    _p(256, 32, 4, 8, tiles=1, nstage=16),
    _u(256, 32, 2, 4, tiles=1, nstage=16),
]


# ------------------------------------------------------------------------------------------------------ 3x3 weight layouts
# Cin 9 <= 1024: the modulation's register cache; Cin 9 > 1024: the row path that recomputes every value
MOD3_CASES = [GC.ModCase(2, 16, 32, 9, cached=True, row_len=288), GC.ModCase(2, 16, 128, 9, cached=False, row_len=1152)]


def unpack3x3(packed, B, Cout, Cin, flip):
    """[B,Cout,Cin 9] from the tap-major fp32 fragments:
    packed[b][t'][ot][kq][lane = (q << 4) | o_lo][j] = w[b][16 ot + o_lo][16 kq + 4 j + q][t],  t' = 8 - t if flip"""
    p = packed.reshape(-1)[:B * 9 * Cout * Cin].reshape(B, 9, Cout // 16, Cin // 16, 4, 16, 4)      # b, t', ot, kq, q, o_lo, j
    un = p.permute(0, 2, 5, 3, 6, 4, 1).reshape(B, Cout, Cin, 9)                                    # b, ot, o_lo, kq, j, q, t'
    return (un.flip(-1) if flip else un).reshape(B, Cout, Cin * 9)


def unpack3x3_split(packed, B, Cout, Cin, flip):
    """([B,Cout,Cin 9] = (hi + lo) / 2^8 as fp64, the tenth tap's halves [B,Cout,Cin,2]) from the tap-pair fragments:
    [b][pair][ot][kq][hi | lo][q = 2 h + cg][o_lo][j]: tap = 2 pair + h (t' as above), channel = 16 kq + 8 cg + j"""
    n = B * 10 * Cout * Cin * 2
    h = packed.reshape(-1).view(torch.float16)[:n].reshape(B, 5, Cout // 16, Cin // 16, 2, 2, 2, 16, 8).double()  # b,pair,ot,kq,plane,h,cg,o_lo,j
    v = h.permute(0, 2, 7, 3, 6, 8, 1, 5, 4).reshape(B, Cout, Cin, 10, 2)             # b, (ot, o_lo), (kq, cg, j), (pair, h), plane
    w = (v[..., 0] + v[..., 1]) / 256.0
    w9 = w[..., :9].flip(-1) if flip else w[..., :9]
    return w9.reshape(B, Cout, Cin * 9), v[:, :, :, 9]


# ------------------------------------------------------------------------------------------------------------ direct kernel
class KxkCase:
    def __init__(self, B, Cin, Cout, H, W, k, transpose2):
        self.B, self.Cin, self.Cout, self.H, self.W, self.k, self.transpose2 = B, Cin, Cout, H, W, k, transpose2

    @property
    def id(self):
        return f"B{self.B}-i{self.Cin}-o{self.Cout}-H{self.H}-W{self.W}-k{self.k}" + ("-T" if self.transpose2 else "")

    @property
    def out_hw(self):
        return (2 * self.H - 1 + self.k - 1, 2 * self.W - 1 + self.k - 1) if self.transpose2 else (self.H, self.W)

    def tensors(self, gs=1.0):
        """x [B,Cin,H,W], w [B,Cout,Cin,k,k] (per sample, as the plain layout of the modulation)"""
        g = GC._gen(32, self.B, self.Cin, self.Cout, self.H, self.W, self.k)
        x = torch.randn(self.B, self.Cin, self.H, self.W, generator=g)
        w = torch.randn(self.B, self.Cout, self.Cin, self.k, self.k, generator=g) / math.sqrt(self.Cin * self.k * self.k)
        return dict(x=x * gs, w=w)

    def mutants(self):
        return ["last_channel_lost", "sample0_weights"] + (["taps_transposed"] if self.k > 1 else [])


def kxk_ref(case, t, dtype, mutant=None, absolute=False):
    x, w = t["x"].to(dtype), t["w"].to(dtype).clone()
    if absolute:
        x, w = x.abs(), w.abs()
    if mutant == "last_channel_lost":
        w[:, :, -1] = 0
    if mutant == "sample0_weights":
        w = w[0:1].expand_as(w)
    if mutant == "taps_transposed":
        w = w.transpose(-1, -2)
    if case.transpose2:
        out = [TF.conv_transpose2d(x[b:b + 1], w[b].transpose(0, 1), stride=2) for b in range(case.B)]
    else:
        out = [TF.conv2d(x[b:b + 1], w[b], padding=case.k // 2) for b in range(case.B)]
    return torch.cat(out, 0)


def kxk_bound(case, t):
    return gamma(case.k * case.k * case.Cin) * kxk_ref(case, t, F64, absolute=True)


KXK_CASES = [KxkCase(2, cin, 12, h, w, k, tr) for (cin, h, w) in ((8, 5, 6), (17, 6, 5)) for k in (1, 3, 5) for tr in (False, True)]
