"""Cases, fp64 references and rounding-error bounds of the forward 1x1 GEMM and the per-op kernels around it: modconv1x1_kernel
(forward instantiations, csrc/gemm1x1.hip) with its noise + bias + leaky-ReLU epilogue, its ToRGB fold and torgb_reduce_kernel,
up2_fir_act_kernel, noise_bias_act_kernel, torgb_kernel / torgb_split_kernel<16> / <4> / torgb_scalar_kernel (csrc/decoder_ops.hip)
and the forward of modulate_kernel (csrc/modulate.hip).  Shared by test_gemm1x1_cases_host.py (CPU: every bound admits torch fp32
and the bf16 / split emulations, rejects every mutant; every case sits in its regime) and test_gpu_gemm1x1.py (the kernels).
Imports no GPU code.

Every reference is a plain torch expression, generic in its dtype: evaluated in float64 it is the oracle, in float32 (on the
CPU) it is "a correct fp32 implementation", with a `mutant` it is a subtly wrong one.  Scalars (the noise weight, 0.2f, sqrt 2,
the FIR taps, the modulation's scale) are fp32 numbers, so the kernel and the reference see the same values.  All DATA of a case
(activations, noise, bias, skip, partial sums; for the modulation the weight tensor) is multiplied by `gs`, a power of two: no
bound has an absolute floor, all of them scale with the data.

`gemm_tile` replays the host's tile choice -- to CHOOSE and label cases, never to compute a reference.  The one observable that
ties it to the library is the row-block count the fold returns (Cout / BM).

Bounds.  u = 2^-24, gamma_k = k u / (1 - k u), times the sum of the absolute terms, evaluated in fp64 per element; first order
in u behind a contraction.  A term is charged one rounding for every addition that can come after it, so a count holds for any
order of the additions it covers.

GEMM, fp32 mode (v_mfma_f32_16x16x4_f32).  out[o][n] = sum_i wm[o][i] x[i][n] is one accumulator chain over K = Cin terms, four
per instruction; eight roundings are set aside for the undocumented inside of a matrix instruction (_decoder_bwd_cases.py):
    e = gamma_(K + 8) sum_i |wm x|
GEMM, bf16 mode (v_mfma_f32_16x16x16_bf16).  pack_bf16 (mfma_frag.h) rounds both fragments to bf16, nearest even; the products
of two bf16 are exact in fp32.  The reference is the fp64 GEMM of the rounded operands, the bound the fp32 accumulation of them:
    e = gamma_(K + 8) sum_i |bf16(wm) bf16(x)|
GEMM, split mode (v_mfma_f32_16x16x32_f16).  W' = 2^8 wm (kSplitScale) and x' = x 2^-E, E = cips3d_split_exp(amax) = the
exponent of the amax HANDED to the kernel minus 14 (clamped to +-100), are powers of two away from the data: exact.
cips3d_split16 / cips3d_split_pair: hi = fp16(v), r = v - hi is exact in fp32, lo = fp16(r).  fp16 has 11 significant bits, so
|r| <= 2^-11 |v| and |r - lo| <= 2^-11 |r| while lo is normal; below 2^-14 fp16 is spaced 2^-24, half of that at the most is lost:
    |v - (hi + lo)| <= 2^-22 |v| + 2^-25        |lo| <= (2^-11 + 2^-22) |v| + 2^-24
The accumulator receives the three exact products wl xh + wh xl + wh xh = (wh + wl)(xh + xl) - wl xl, 3 K terms in all, 96 per
triple of instructions; back in the units of the data (divide by 2^8 2^-E, which the epilogue does exactly):
    rep(w) = 2^-22 |w| + 2^-33                 rep(x) = 2^-22 |x| + 2^-25 2^E       (2^E <= amax 2^-14: the absolute term scales
    low(w) = (2^-11 + 2^-22) |w| + 2^-32       low(x) = (2^-11 + 2^-22) |x| + 2^-24 2^E    with the amax, not with the element)
    e = sum_i (|w| rep(x) + |x| rep(w) + rep(w) rep(x) + low(w) low(x))  +  gamma_(3 K + 8) sum_i (|wh xh| + |wh xl| + |wl xh|)
(representation of both operands, the dropped lo lo product, the accumulation of 3 K terms in any order).  The sum of the three
absolute products is evaluated from the emulated halves.  split_bound / fp32_bound is (3 K + 20) / (K + 8) to first order: the
accumulation is charged three times the terms, the representation 3 x 2^-22 = 12 u per product.
On the CPU the "correct implementation" is `split_emulated`: torch fp16 casts, the exponent rule above, one fp32 matmul over the
3 K products -- built from the header's definitions.

Epilogue (modconv1x1_kernel, noise_bias_act_kernel, up2_fir_act_kernel): t1 = fma(nw, nz, v), t2 = t1 + bias, t3 = max(t2, 0.2f t2),
out = t3 * fp32(sqrt 2).  torch fp32 rounds nw nz before it adds, and the bound charges that: with e(v) the error of v
    e = G (e(v) + u (|nw nz| + |t1| + |t2|)) + 2 u |out|          G = fp32(sqrt 2)
(leaky ReLU is 1-Lipschitz, so e(v) passes times the gain whatever side of zero; the slope's and the gain's products are the 2 u).
Without an epilogue e = e(v).  out_bf16 is compared bit for bit with the bf16 rounding of the fp32 result of the same mode.

Fold (modconv1x1_kernel, rgb_part).  A lane folds its 4 WM rows with one fma each (NOT BM of them: a wave's 16 WM rows are spread
over its four lane quarters), two shuffle additions join the quarters, WGM - 1 LDS additions the wave rows (the first addition
meets a zero):  k_fold = 4 WM + 2 + WGM - 1.
Reduce (torgb_reduce_kernel).  Group g adds slots g, g + 4, ... in a chain, the first onto zero: ceil(n_slots / 4) - 1 additions
for the longest; three LDS additions join the groups; the biases are added to each other (n_bias - 1), their sum to the value (1),
then the skip (1):
    k_part = ceil(n_slots / 4) - 1 + 3 + [n_bias > 0] + [skip]      k_bias = max(n_bias - 1, 0) + 1 + [skip]
    e = gamma_(k_part) sum_s |part_s| + gamma_(k_bias) sum_k |bias_k| + u |skip|
The fold's reference is ToRGB of the fp64 activation output y; with e(y) the bound of the GEMM's own output
    e = sum_o |w_rgb| e(y) + gamma_(k_fold + k_part) sum_o |w_rgb y| + gamma_(k_bias) sum |bias| + u |skip|
The first term charges the worst case of every row's GEMM with one sign through a sum over Cout rows of mixed signs, so the fold's
own arithmetic hides far below it.  The fold is therefore held a second time to the bound of the fold ALONE: the kernel folds the
very values it stores, so against ToRGB (in fp64) of the output the launch wrote, e(y) = 0 and only the last three terms remain.

up2_fir_act_kernel: up2_fir, four fmas per output (taps outside the image multiply zeros: exact): e(v) = gamma_4 sum |y k|, then
the epilogue.
torgb_*: Cin fmas per thread in torgb_kernel and torgb_scalar_kernel; ceil(Cin / S) fmas per slice and S - 1 additions of the
slices in torgb_split_kernel<S>; the bias (1), the skip (1).  A FIR skip is up2_tap: at most four fmas before it is added.
    e = gamma_(kc + 2) sum_i |wm x| + 2 u |bias| + (u |skip|  or  gamma_5 sum |skip k|)      kc = Cin or ceil(Cin / S) + S - 1
modulate_kernel (forward half of the derivation of modulate_bwd in _decoder_bwd_cases.py): len = Cin ksq, n = ceil(len / 64)
terms per lane.  v = (scale W) s: two roundings.  ss = sum v^2 by fma: 4 u from v, n + 6 of the chain and the butterfly; + 1e-8f
(the constant rounded to fp32, the addition): rel(ss + eps) <= (n + 12) u.  d = rsqrtf(.): half of that and the instruction at
the 2 ulp = 4 u the project allows:  rel(d) = ((n + 12) / 2 + 4) u.  wm = v d, one product more:
    e = |wm| (rel(d) + 3 u)           without demodulation  e = 2 u |wm|
The packed fp32 layout is held to the same bound after un-packing; the split layout adds rep(w) of its fp16 halves, the bf16
layout the 2^-8 |wm| of a round-to-nearest bf16 (8 significant bits).

Sentinels: none.  Every contraction here runs over at most 512 terms; test_gemm1x1_cases_host.py shows with the mutants that one
lost term of ordinary data leaves gamma_K sum |.| -- it is not assumed.
"""
import math

import torch
import torch.nn.functional as TF

from _dense_cases import U, f32, gamma, inside, worst  # noqa: F401  (re-exported)
from _decoder_bwd_cases import unpack, unpack_split  # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64
SCALES = (1.0, 2.0 ** -20)
SPLIT_SCALES = (1.0, 2.0 ** -20, 2.0 ** 17)
MODES = ("fp32", "bf16", "split")
GAIN = f32(1.41421356237309515)
SLOPE = f32(0.2)
NOISE_W = f32(0.3)
FOLD_MAX = 8                  # CIPS3D_TORGB_FOLD_MAX
# an asymmetric FIR (the production taps [1,3,3,1] x [1,3,3,1] / 16 cannot tell a mirrored tap), as fp32 numbers
FIR = (torch.tensor([1.0, 3.0, 5.0, 2.0]).outer(torch.tensor([2.0, 1.0, 4.0, 3.0])) / 27.5).float()


def ceil_div(a, b):
    return -(-a // b)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def scales_of(mode):
    return SPLIT_SCALES if mode == "split" else SCALES


# ---------------------------------------------------------------------------------------------------------------- tile choice
def gemm_tile(B, Cin, Cout, HW, fold):
    """(WM, WGM, WGN, BK, NS) as gemm_tile() of csrc/gemm1x1.hip picks it for a forward launch"""
    if Cout >= 256 and Cout % 64 == 0:
        tiles = B * (Cout // 64) * ceil_div(HW, 128)
        if not fold and tiles <= 128:
            return (1, 2, 2, 32, 4)
        if tiles <= 256 and Cin % 64 == 0:
            return (1, 4, 2, 64, 2)
        if tiles > 256 and Cout % 128 == 0 and Cin % 64 == 0:
            return (2, 4, 2, 64, 2)
        return (1, 4, 2, 32, 2)
    ns = 2 if (Cin <= 128 and Cout < 256) else 4
    if Cout == 128:
        return (1, 8, 1, 32, ns)
    if Cout == 64:
        return (1, 4, 2, 32, ns)
    return (1, 2, 2, 32, ns)


TILE_FORMS = [(1, 2, 2, 32, 4), (1, 4, 2, 64, 2), (2, 4, 2, 64, 2), (1, 4, 2, 32, 2), (1, 8, 1, 32, 2), (1, 2, 2, 32, 2),
              (1, 8, 1, 32, 4), (1, 4, 2, 32, 4)]


class GemmCase:
    def __init__(self, B, Cin, Cout, HW, fold=False, epilogue=1, noise="shared", amax="measured", sample_scale=None, **expect):
        """noise: "shared" | "per_sample" | None (epilogue 1 only); amax (split mode): "measured" | "loose" (4 x the true
        maximum); sample_scale: per-sample multipliers of x.  expect: the regime the case is listed for (tile, stages, tail =
        pixels of the last tile, row_blocks), checked against the replay by the host test."""
        self.B, self.Cin, self.Cout, self.HW, self.fold, self.epilogue = B, Cin, Cout, HW, fold, epilogue
        self.noise = noise if epilogue == 1 else None
        self.amax, self.sample_scale, self.expect = amax, sample_scale, expect

    @property
    def id(self):
        sw = ("-fold" if self.fold else "") + ("" if self.epilogue else "-ep0") + \
            ("" if self.epilogue == 0 else {"shared": "", "per_sample": "-nzB", None: "-nonoise"}[self.noise]) + \
            ("-loose" if self.amax == "loose" else "") + ("-spread" if self.sample_scale else "")
        return f"B{self.B}-i{self.Cin}-o{self.Cout}-HW{self.HW}{sw}"

    @property
    def tile(self):
        return gemm_tile(self.B, self.Cin, self.Cout, self.HW, self.fold)

    @property
    def BM(self):
        return 16 * self.tile[0] * self.tile[1]

    @property
    def BN(self):
        return 64 * self.tile[2]

    @property
    def last_tile(self):
        """first pixel of the last pixel tile"""
        return (ceil_div(self.HW, self.BN) - 1) * self.BN

    @property
    def ragged(self):
        return self.HW % self.BN != 0

    @property
    def per_sample_noise(self):
        return self.noise == "per_sample" and self.B > 1

    def regime(self):
        t = self.tile
        return dict(tile=t, stages=self.Cin // t[3], tail=self.HW - self.last_tile, row_blocks=self.Cout // self.BM,
                    pixel_tiles=ceil_div(self.HW, self.BN))

    def tensors(self, gs=1.0):
        """x [B,Cin,HW], w [B,Cout,Cin] (an explicit matrix, rows of about unit norm), noise [1 | B,1,HW] | None, bias [Cout],
        w_rgb [B,3,Cout], rgb_bias [3], skip [B,3,HW]"""
        g = _gen(11, self.B, self.Cin, self.Cout, self.HW)
        x = torch.randn(self.B, self.Cin, self.HW, generator=g) * (1.0 + 3.0 * torch.rand(self.B, self.Cin, 1, generator=g))
        if self.sample_scale:
            x = x * torch.tensor(self.sample_scale).reshape(self.B, 1, 1)
        w = torch.randn(self.B, self.Cout, self.Cin, generator=g) / math.sqrt(self.Cin)
        nb = self.B if self.per_sample_noise else 1
        noise = torch.randn(nb, 1, self.HW, generator=g)
        bias = torch.randn(self.Cout, generator=g) * 0.5
        w_rgb = torch.randn(self.B, 3, self.Cout, generator=g) / math.sqrt(self.Cout)
        rgb_bias, skip = torch.randn(3, generator=g), torch.randn(self.B, 3, self.HW, generator=g)
        return dict(x=x * gs, w=w, noise=noise * gs if self.noise else None, bias=bias * gs, w_rgb=w_rgb, rgb_bias=rgb_bias * gs,
                    skip=skip * gs)

    def amax_given(self, t):
        """[B] the amax handed to the split kernel: the measured maximum of x per sample, or 4 x that"""
        m = t["x"].abs().amax((1, 2))
        return m * 4.0 if self.amax == "loose" else m

    def gemm_mutants(self):
        m = ["drop_stage_last_channel", "kgroup_twice", "swap_pixels"]
        return m + (["tail_shift4"] if self.ragged and self.HW > 4 else [])

    def epilogue_mutants(self):
        if self.epilogue != 1:
            return []
        return ["bias_row16", "slope_sign", "gain_before_bias"] + (["noise_sample0"] if self.per_sample_noise else [])

    def fold_mutants(self):
        return (["fold_drop_block", "fold_wrong_row"] + (["fold_preact"] if self.epilogue == 1 else [])) if self.fold else []


def split_exp(amax):
    """cips3d_split_exp on a Python float (an fp32 value): the exponent field minus 127 minus 14, clamped"""
    a = f32(amax)
    if a == 0.0 or math.isinf(a) or math.isnan(a):
        return -100 if a == 0.0 else 100
    e = math.frexp(a)[1] - 1
    e = max(e, -127) - 14                      # (fp32 subnormals have exponent field 0)
    return max(-100, min(100, e))


def split16(v):
    """cips3d_split16 on an fp32 tensor: (hi, lo) as fp32 tensors holding fp16 values"""
    hi = v.to(torch.float16).to(F32)
    return hi, (v - hi).to(torch.float16).to(F32)


def bf16_round(v):
    return v.to(torch.bfloat16).to(F32)


def split_operands(t, amax):
    """(wh, wl [B,Cout,Cin], xh, xl [B,Cin,HW], kin [B,1,1]) of the split mode, fp32 tensors; amax [B]"""
    E = torch.tensor([split_exp(float(a)) for a in amax], dtype=F64)
    kx, kin = torch.pow(2.0, -E).to(F32).reshape(-1, 1, 1), (torch.pow(2.0, E) / 256.0).to(F32).reshape(-1, 1, 1)
    wh, wl = split16(t["w"] * 256.0)
    xh, xl = split16(t["x"] * kx)
    return wh, wl, xh, xl, kin


def split_emulated(t, amax):
    """the split GEMM as the header defines it, in torch: fp16 halves, the three products, fp32 accumulation"""
    wh, wl, xh, xl, kin = split_operands(t, amax)
    return torch.bmm(torch.cat([wl, wh, wh], 2), torch.cat([xh, xl, xh], 1)) * kin


def gemm_operands(t, dtype, mode, mutant=None, case=None):
    w, x = t["w"], t["x"]
    if mode == "bf16":
        w, x = bf16_round(w), bf16_round(x)
    w, x = w.to(dtype).clone(), x.to(dtype).clone()
    if mutant == "drop_stage_last_channel":           # the last channel of the first K stage
        w[:, :, case.tile[3] - 1] = 0
    if mutant == "kgroup_twice":                      # channels 0..15 counted twice, 16..31 lost
        w[:, :, 16:32], x[:, 16:32] = w[:, :, 0:16].clone(), x[:, 0:16].clone()
    return w, x


def gemm_ref(t, dtype, mode, mutant=None, case=None):
    """the GEMM's accumulator [B,Cout,HW]: in fp64 the oracle of `mode` (bf16: of the rounded operands), in fp32 torch's bmm"""
    w, x = gemm_operands(t, dtype, mode, mutant, case)
    v = torch.bmm(w, x)
    if mutant == "swap_pixels":                       # pixels c and c + 1 of the first quad of the last tile
        n = case.last_tile
        v[..., [n, n + 1]] = v[..., [n + 1, n]]
    if mutant == "tail_shift4":                       # the ragged tile's columns read 4 pixels to the left
        n = case.last_tile
        lo = max(n, 4)
        v[..., lo:] = v[..., lo - 4:case.HW - 4].clone()
    return v


def gemm_bound(t, mode, amax=None):
    w, x = gemm_operands(t, F64, mode)
    K = w.shape[2]
    aw, ax = w.abs(), x.abs()
    if mode != "split":
        return gamma(K + 8) * torch.bmm(aw, ax)
    E = torch.tensor([split_exp(float(a)) for a in amax], dtype=F64).reshape(-1, 1, 1)
    pe = torch.pow(2.0, E)
    rep_w, rep_x = 2.0 ** -22 * aw + 2.0 ** -33, 2.0 ** -22 * ax + 2.0 ** -25 * pe
    low_w, low_x = (2.0 ** -11 + 2.0 ** -22) * aw + 2.0 ** -32, (2.0 ** -11 + 2.0 ** -22) * ax + 2.0 ** -24 * pe
    rep = torch.bmm(aw, rep_x) + torch.bmm(rep_w, ax) + torch.bmm(rep_w, rep_x) + torch.bmm(low_w, low_x)
    wh, wl, xh, xl, kin = (v.double().abs() for v in split_operands(t, amax))
    three = torch.bmm(torch.cat([wl, wh, wh], 2), torch.cat([xh, xl, xh], 1)) * kin
    return rep + gamma(3 * K + 8) * three


def lrelu(t, mutant=None):
    return torch.minimum(t, t * SLOPE) if mutant == "slope_sign" else torch.maximum(t, t * SLOPE)


def epilogue_ref(v, t, dtype, per_sample, mutant=None):
    """noise + bias + leaky ReLU on v [B,C,P]; t: noise [1 | B,1,P] | None, bias [C]"""
    bias = t["bias"].to(dtype)
    if mutant == "bias_row16":
        bias = torch.roll(bias, -16)
    t1 = v
    if t["noise"] is not None:
        nz = t["noise"].to(dtype)
        if per_sample and mutant == "noise_sample0":
            nz = nz[0:1]
        t1 = v + NOISE_W * nz
    if mutant == "gain_before_bias":
        return lrelu(t1 * GAIN + bias[None, :, None])
    return lrelu(t1 + bias[None, :, None], mutant) * GAIN


def epilogue_bound(v64, e_v, t):
    """bound of epilogue_ref's output given the fp64 accumulator and its bound"""
    nzw = NOISE_W * t["noise"].double() if t["noise"] is not None else torch.zeros(1, 1, 1, dtype=F64)
    t1 = v64 + nzw
    t2 = t1 + t["bias"].double()[None, :, None]
    out = lrelu(t2) * GAIN
    return GAIN * (e_v + U * (nzw.abs() + t1.abs() + t2.abs())) + 2 * U * out.abs()


def gemm_out_ref(case, t, dtype, mode, mutant=None):
    """the tensor the launch stores: (pre-activation accumulator, output)"""
    gm = mutant if mutant in ("drop_stage_last_channel", "kgroup_twice", "swap_pixels", "tail_shift4") else None
    v = gemm_ref(t, dtype, mode, gm, case)
    if case.epilogue != 1:
        return v, v
    return v, epilogue_ref(v, t, dtype, case.per_sample_noise, mutant)


def gemm_out_bound(case, t, mode, amax=None):
    v = gemm_ref(t, F64, mode)
    e_v = gemm_bound(t, mode, amax)
    return e_v if case.epilogue != 1 else epilogue_bound(v, e_v, t)


# --------------------------------------------------------------------------------------------------------------- fold, reduce
def reduce_counts(n_slots, n_bias, skip):
    return ceil_div(n_slots, 4) - 1 + 3 + (1 if n_bias else 0) + (1 if skip else 0), max(n_bias - 1, 0) + 1 + (1 if skip else 0)


def fold_ref(case, t, dtype, mode, mutant=None, y=None):
    """rgb [B,3,HW] = ToRGB of the launch's output + bias + skip; y: the output to fold instead of the reference's own"""
    v, y_ref = gemm_out_ref(case, t, dtype, mode) if (y is None or mutant == "fold_preact") else (None, None)
    y = y_ref if y is None else y.to(dtype)
    w_rgb = t["w_rgb"].to(dtype)
    if mutant == "fold_preact":
        y = v
    if mutant == "fold_wrong_row":
        w_rgb = torch.roll(w_rgb, -1, 2)
    if mutant == "fold_drop_block":
        y, w_rgb = y[:, :case.Cout - case.BM], w_rgb[:, :, :case.Cout - case.BM]
    return torch.bmm(w_rgb, y) + t["rgb_bias"].to(dtype)[None, :, None] + t["skip"].to(dtype)


def fold_bound(case, t, mode, amax=None, y=None):
    """y: the bound of the fold alone, given the output it folds (e(y) = 0)"""
    aw = t["w_rgb"].double().abs()
    WM, WGM = case.tile[0], case.tile[1]
    k_part, k_bias = reduce_counts(case.Cout // case.BM, 1, True)
    if y is None:
        y = gemm_out_ref(case, t, F64, mode)[1]
        through = torch.bmm(aw, gemm_out_bound(case, t, mode, amax))
    else:
        y, through = y.double(), 0.0
    return (through + gamma(4 * WM + 2 + WGM - 1 + k_part) * torch.bmm(aw, y.abs()) +
            gamma(k_bias) * t["rgb_bias"].double().abs()[None, :, None] + U * t["skip"].double().abs())


class ReduceCase:
    def __init__(self, n_slots, n_bias, skip, B, HW):
        self.n_slots, self.n_bias, self.skip, self.B, self.HW = n_slots, n_bias, skip, B, HW

    @property
    def id(self):
        return f"s{self.n_slots}-b{self.n_bias}-" + ("skip" if self.skip else "noskip") + f"-B{self.B}-HW{self.HW}"

    def tensors(self, gs=1.0):
        g = _gen(12, self.n_slots, self.n_bias, self.B, self.HW)
        part = torch.randn(self.n_slots, self.B, 3, self.HW, generator=g)
        biases = torch.randn(self.n_bias, 3, generator=g)
        skip = torch.randn(self.B, 3, self.HW, generator=g)
        return dict(part=part * gs, biases=biases * gs, skip=skip * gs if self.skip else None)

    def mutants(self):
        return (["last_slot_lost"] if self.n_slots % 4 == 1 and self.n_slots > 1 else []) + (["bias_twice"] if self.n_bias else [])


def reduce_ref(t, dtype, mutant=None):
    part, biases = t["part"].to(dtype), t["biases"].to(dtype)
    if mutant == "last_slot_lost":
        part = part[:-1]
    out = part.sum(0)
    if biases.shape[0]:
        out = out + (biases.sum(0) + (biases[-1] if mutant == "bias_twice" else 0))[None, :, None]
    return out + t["skip"].to(dtype) if t["skip"] is not None else out


def reduce_bound(t):
    part, biases = t["part"].double().abs(), t["biases"].double().abs()
    k_part, k_bias = reduce_counts(part.shape[0], biases.shape[0], t["skip"] is not None)
    e = gamma(k_part) * part.sum(0)
    if biases.shape[0]:
        e = e + gamma(k_bias) * biases.sum(0)[None, :, None]
    return e + U * t["skip"].double().abs() if t["skip"] is not None else e


REDUCE_CASES = [ReduceCase(1, 0, False, 1, 4), ReduceCase(3, 1, True, 2, 260), ReduceCase(4, FOLD_MAX, True, 1, 260),
                ReduceCase(5, 1, False, 2, 4), ReduceCase(16, 0, True, 1, 260), ReduceCase(17, FOLD_MAX, False, 2, 260),
                ReduceCase(48, 1, True, 2, 260), ReduceCase(5, 0, True, 1, 260), ReduceCase(1, FOLD_MAX, True, 2, 4)]


# ----------------------------------------------------------------------------------------------------------------- the cases
def _both(*a, **kw):
    return [GemmCase(*a, **kw), GemmCase(*a, fold=True, **kw)]


T = dict(zip("ABCDEFGH", TILE_FORMS))
GEMM_CASES = [
    # {1,2,2,32,4}: the small grid, 1 / 3 / 5 stages against a ring that wants three in flight
    GemmCase(1, 32, 256, 132, tile=T["A"], stages=1, tail=4),
    GemmCase(1, 96, 256, 132, noise=None, tile=T["A"], stages=3, tail=4),
    GemmCase(1, 160, 256, 260, epilogue=0, tile=T["A"], stages=5, tail=4),
    GemmCase(1, 64, 288, 132, tile=T["A"], stages=2),                                   # via Cout % 64 != 0
    GemmCase(2, 160, 224, 132, noise="per_sample", tile=T["A"], stages=5, tail=4),      # via Cout < 256
    GemmCase(2, 160, 224, 132, fold=True, noise="per_sample", tile=T["A"], row_blocks=7),
    # {1,4,2,64,2}
    GemmCase(1, 64, 256, 4100, tile=T["B"], stages=1, tail=4, pixel_tiles=33),
    GemmCase(1, 192, 256, 132, fold=True, tile=T["B"], stages=3, row_blocks=4, tail=4),
    GemmCase(2, 128, 256, 2052, noise="per_sample", tile=T["B"], stages=2, tail=4),
    # {2,4,2,64,2}: more than 256 tiles, 128-row blocks
    *_both(3, 64, 256, 2692, noise="per_sample", tile=T["C"], stages=1, tail=4, row_blocks=2),
    # {1,4,2,32,2}
    GemmCase(1, 96, 256, 4228, tile=T["D"], stages=3, tail=4),
    GemmCase(1, 96, 256, 132, fold=True, epilogue=0, tile=T["D"], stages=3, row_blocks=4),
    GemmCase(1, 64, 320, 6532, noise=None, tile=T["D"], stages=2, tail=4),              # the largest case: 8.4 MB out
    *_both(2, 64, 64, 124, noise="per_sample", tile=T["D"], stages=2, tail=124, row_blocks=1),
    # {1,8,1,32,2}: 64-pixel tiles, eight wave rows
    GemmCase(2, 32, 128, 68, noise="per_sample", tile=T["E"], stages=1, tail=4),
    GemmCase(1, 128, 128, 4, tile=T["E"], stages=4, tail=4, pixel_tiles=1),
    GemmCase(2, 64, 128, 196, fold=True, noise="per_sample", tile=T["E"], tail=4, row_blocks=1),
    GemmCase(1, 32, 128, 124, epilogue=0, tile=T["E"], tail=60),
    GemmCase(1, 32, 128, 64, tile=T["E"], tail=64),
    # {1,8,1,32,4}
    *_both(1, 160, 128, 196, tile=T["G"], stages=5, tail=4, row_blocks=1),
    GemmCase(2, 160, 128, 60, noise="per_sample", tile=T["G"], tail=60),
    # {1,4,2,32,4}
    GemmCase(1, 160, 64, 128, tile=T["H"], stages=5, tail=128),
    GemmCase(1, 160, 64, 256, epilogue=0, tile=T["H"], tail=128, pixel_tiles=2),
    GemmCase(2, 160, 64, 132, noise="per_sample", tile=T["H"], tail=4),
    GemmCase(1, 192, 64, 132, fold=True, tile=T["H"], stages=6, row_blocks=1),
    # {1,2,2,32,2}
    GemmCase(1, 32, 32, 4, tile=T["F"], stages=1, tail=4),
    GemmCase(2, 128, 96, 252, fold=True, noise="per_sample", tile=T["F"], stages=4, tail=124, row_blocks=3),
]
# split mode only: a caller's looser bound, and two samples 2^37 apart (sample 0's exponent overflows fp16 on sample 1)
SPLIT_ONLY_CASES = [
    GemmCase(1, 64, 64, 124, amax="loose", tile=T["D"]),
    GemmCase(2, 64, 128, 68, epilogue=0, sample_scale=(1.0, 2.0 ** 37), tile=T["E"], tail=4),
]
OUT_BF16_CASES = [GemmCase(2, 64, 64, 124, epilogue=0), GemmCase(1, 64, 256, 132, epilogue=0), GemmCase(1, 32, 128, 68, epilogue=0)]
# (B, Cin, Cout, HW, demodulate): the weights come from hip.modulate_weights(packed) instead of pack_weights
MODULATED_GEMM_CASE = (2, 64, 128, 68, True)


def cases_of(mode):
    return GEMM_CASES + (SPLIT_ONLY_CASES if mode == "split" else [])


# ------------------------------------------------------------------------------------------------------- up2 + FIR + epilogue
def upfir(y, fir, mutant=None):
    """upfirdn2d(up = 2, pad = (2, 1)) of y [N,H,W] with 4 x 4 taps: out[oy][ox] = sum u[oy + ky][ox + kx] fir[3 - ky][3 - kx],
    u the zero-stuffed image behind a border of two zeros"""
    N, H, W = y.shape
    fir = fir.to(y.dtype).clone()
    if mutant == "tap_mirrored":
        fir[1, 0], fir[1, 3] = fir[1, 3].clone(), fir[1, 0].clone()      # (a row that H = 1 uses too)
    u = torch.zeros(N, 2 * H + 3, 2 * W + 3, dtype=y.dtype)
    u[:, 2:2 + 2 * H:2, 2:2 + 2 * W:2] = y
    if mutant == "right_border_inside":               # the column right of the image reads on: the next row's first pixel
        nxt = torch.cat([y.reshape(N, -1)[:, W::W], torch.zeros(N, 1, dtype=y.dtype)], 1)      # [N,H]
        u[:, 2:2 + 2 * H:2, 2 + 2 * W] = nxt
    return TF.conv2d(u[:, None], fir.flip(0, 1)[None, None])[:, 0]


class UpCase:
    def __init__(self, B, C, H, W, noise):
        self.B, self.C, self.H, self.W, self.noise = B, C, H, W, noise

    @property
    def id(self):
        return f"B{self.B}-C{self.C}-H{self.H}-W{self.W}-{self.noise}"

    @property
    def per_sample_noise(self):
        return self.noise == "per_sample" and self.B > 1

    def tensors(self, gs=1.0):
        g = _gen(13, self.B, self.C, self.H, self.W)
        y = torch.randn(self.B, self.C, self.H, self.W, generator=g)
        noise = torch.randn(self.B if self.per_sample_noise else 1, 1, 4 * self.H * self.W, generator=g)
        bias = torch.randn(self.C, generator=g) * 0.5
        return dict(y=y * gs, noise=noise * gs if self.noise != "none" else None, bias=bias * gs)

    def mutants(self):
        return ["tap_mirrored"] + (["right_border_inside"] if self.H > 1 else []) + ["slope_sign", "gain_before_bias"] + \
            (["noise_sample0"] if self.per_sample_noise else [])


def up_ref(case, t, dtype, mutant=None):
    """[B,C,4 H W]"""
    y = t["y"].to(dtype).reshape(-1, case.H, case.W)
    fm = mutant if mutant in ("tap_mirrored", "right_border_inside") else None
    v = upfir(y, FIR, fm).reshape(case.B, case.C, -1)
    return epilogue_ref(v, t, dtype, case.per_sample_noise, mutant)


def up_bound(case, t):
    y = t["y"].double().reshape(-1, case.H, case.W)
    v = upfir(y, FIR.double()).reshape(case.B, case.C, -1)
    e_v = gamma(4) * upfir(y.abs(), FIR.double().abs()).reshape(case.B, case.C, -1)
    return epilogue_bound(v, e_v, t)


UP_CASES = [UpCase(1, 1, 1, 2, "shared"), UpCase(2, 3, 1, 6, "per_sample"), UpCase(3, 5, 3, 6, "per_sample"),
            UpCase(3, 5, 3, 6, "shared"), UpCase(1, 2, 7, 2, "none"), UpCase(2, 33, 5, 10, "per_sample"), UpCase(2, 33, 5, 10, "none")]


# ----------------------------------------------------------------------------------------------------------- noise_bias_act
class NbaCase:
    def __init__(self, B, C, HW, noise):
        self.B, self.C, self.HW, self.noise = B, C, HW, noise

    @property
    def id(self):
        return f"B{self.B}-C{self.C}-HW{self.HW}-{self.noise}"

    @property
    def per_sample_noise(self):
        return self.noise == "per_sample" and self.B > 1

    def tensors(self, gs=1.0):
        g = _gen(14, self.B, self.C, self.HW)
        x = torch.randn(self.B, self.C, self.HW, generator=g)
        noise = torch.randn(self.B if self.per_sample_noise else 1, 1, self.HW, generator=g)
        bias = torch.randn(self.C, generator=g) * 0.5
        return dict(x=x * gs, noise=noise * gs if self.noise != "none" else None, bias=bias * gs)

    def mutants(self):
        return ["slope_sign", "gain_before_bias"] + (["noise_sample0"] if self.per_sample_noise else []) + \
            (["bias_next_channel"] if self.C > 1 else [])


def nba_ref(case, t, dtype, mutant=None):
    tt = dict(t)
    if mutant == "bias_next_channel":
        tt["bias"] = torch.roll(t["bias"], -1)
    return epilogue_ref(t["x"].to(dtype), tt, dtype, case.per_sample_noise, mutant)


def nba_bound(case, t):
    x = t["x"].double()
    return epilogue_bound(x, torch.zeros_like(x), t)


NBA_CASES = [NbaCase(1, 1, 1, "shared"), NbaCase(3, 33, 3, "per_sample"), NbaCase(3, 1, 4, "shared"), NbaCase(1, 33, 1025, "none"),
             NbaCase(3, 33, 1025, "per_sample"), NbaCase(3, 1, 1025, "none")]


# -------------------------------------------------------------------------------------------------------------------- ToRGB
def torgb_arm(Cin, H, W):
    """(kernel, S) as cips3d_torgb picks them"""
    if W % 4 != 0:
        return "scalar", 1
    if H * W // 4 <= 32768 and Cin >= 64:
        return "split16", 16
    if Cin >= 16:
        return "split4", 4
    return "plain", 1


class RgbCase:
    def __init__(self, B, Cin, H, W, skip, **expect):
        """skip: "none" | "plain" | "fir" (a half-resolution skip through the FIR up-sampler; H and W even)"""
        self.B, self.Cin, self.H, self.W, self.skip, self.expect = B, Cin, H, W, skip, expect

    @property
    def id(self):
        return f"B{self.B}-C{self.Cin}-H{self.H}-W{self.W}-{self.skip}"

    def regime(self):
        arm, S = torgb_arm(self.Cin, self.H, self.W)
        quads = self.H * self.W // 4
        return dict(arm=arm, quads=quads, last_block_quads=(quads - 1) % (256 // S) + 1, uneven_slices=self.Cin % S != 0)

    def tensors(self, gs=1.0):
        g = _gen(15, self.B, self.Cin, self.H, self.W)
        x = torch.randn(self.B, self.Cin, self.H * self.W, generator=g)
        wm = torch.randn(self.B, 3, self.Cin, generator=g) / math.sqrt(self.Cin)
        bias = torch.randn(3, generator=g)
        shape = (self.B, 3, self.H // 2, self.W // 2) if self.skip == "fir" else (self.B, 3, self.H, self.W)
        skip = torch.randn(*shape, generator=g)
        return dict(x=x * gs, wm=wm, bias=bias * gs, skip=skip * gs if self.skip != "none" else None)

    def mutants(self):
        return ["last_slice_lost"] + (["skip_next_channel"] if self.skip != "none" else [])


def _rgb_skip(case, skip, absolute=False):
    if case.skip == "fir":
        fir = FIR.to(skip.dtype)
        return upfir(skip.reshape(-1, case.H // 2, case.W // 2), fir.abs() if absolute else fir).reshape(case.B, 3, -1)
    return skip.reshape(case.B, 3, -1)


def rgb_ref(case, t, dtype, mutant=None):
    """[B,3,HW]"""
    x, wm = t["x"].to(dtype), t["wm"].to(dtype)
    if mutant == "last_slice_lost":                   # the channels of the last thread slice (the last channel where S = 1)
        S = torgb_arm(case.Cin, case.H, case.W)[1]
        keep = torch.arange(case.Cin) % S != S - 1 if S > 1 else torch.arange(case.Cin) < case.Cin - 1
        x, wm = x[:, keep], wm[:, :, keep]
    out = torch.bmm(wm, x) + t["bias"].to(dtype)[None, :, None]
    if t["skip"] is None:
        return out
    skip = t["skip"].to(dtype)
    if mutant == "skip_next_channel":
        skip = torch.roll(skip, -1, 1)
    return out + _rgb_skip(case, skip)


def rgb_bound(case, t):
    S = torgb_arm(case.Cin, case.H, case.W)[1]
    kc = case.Cin if S == 1 else ceil_div(case.Cin, S) + S - 1
    e = gamma(kc + 2) * torch.bmm(t["wm"].double().abs(), t["x"].double().abs()) + 2 * U * t["bias"].double().abs()[None, :, None]
    if t["skip"] is None:
        return e
    return e + (gamma(5) if case.skip == "fir" else U) * _rgb_skip(case, t["skip"].double().abs(), absolute=True)


RGB_CASES = [RgbCase(2, 33, 6, 10, s, arm="scalar") for s in ("none", "plain", "fir")] + \
            [RgbCase(2, 64, 2, 4, s, arm="split16", quads=2) for s in ("none", "plain", "fir")] + \
            [RgbCase(1, 96, 6, 12, s, arm="split16", quads=18, last_block_quads=2) for s in ("none", "plain", "fir")] + \
            [RgbCase(2, 33, 6, 12, s, arm="split4", uneven_slices=True) for s in ("none", "plain", "fir")] + \
            [RgbCase(3, 12, 4, 8, s, arm="plain") for s in ("none", "plain", "fir")]


# --------------------------------------------------------------------------------------------------------------- modulation
class ModCase:
    def __init__(self, B, Cout, Cin, ksq, s_scale=1.0, **expect):
        self.B, self.Cout, self.Cin, self.ksq, self.s_scale, self.expect = B, Cout, Cin, ksq, s_scale, expect
        self.scale = f32(1.0 / math.sqrt(Cin * ksq))
        self.s_stride, self.s_offset = Cin + 5, 3

    @property
    def id(self):
        return f"B{self.B}-o{self.Cout}-i{self.Cin}-k{self.ksq}" + ("-small" if self.s_scale != 1.0 else "")

    def regime(self):
        L = self.Cin * self.ksq
        return dict(row_len=L, cached=L <= 1024, idle_lanes=(64 - L % 64) % 64, rows=self.B * self.Cout,
                    idle_waves=(4 - self.B * self.Cout % 4) % 4)

    def tensors(self, gs=1.0):
        """W [1,Cout,Cin,k,k], s_buf [s_offset + B s_stride] (the styles at s_buf[s_offset + b s_stride + i], junk between)"""
        k = int(math.isqrt(self.ksq))
        g = _gen(16, self.B, self.Cout, self.Cin, self.ksq)
        W = torch.randn(1, self.Cout, self.Cin, k, k, generator=g)
        s_buf = 100.0 * torch.randn(self.s_offset + self.B * self.s_stride, generator=g)
        s = (1.0 + 0.5 * torch.randn(self.B, self.Cin, generator=g)) * self.s_scale
        s_buf[self.s_offset:].reshape(self.B, self.s_stride)[:, :self.Cin] = s
        return dict(W=W * gs, s_buf=s_buf, s=s)

    def mutants(self, demod, gs):
        if not demod:
            return ["style_shifted"]
        return ["style_shifted"] + (["norm_short"] if (self.Cin * self.ksq > 1024 and gs == 1.0) else []) + \
            (["eps_after_rsqrt"] if (self.s_scale != 1.0 or gs != 1.0) else [])


def mod_ref(case, t, dtype, demod, mutant=None):
    """wm [B,Cout,Cin ksq]"""
    L = case.Cin * case.ksq
    s = t["s"].to(dtype)
    if mutant == "style_shifted":                     # the style row read without its offset
        s = t["s_buf"][:case.B * case.s_stride].reshape(case.B, case.s_stride)[:, :case.Cin].to(dtype)
    sb = s[:, torch.arange(L) // case.ksq]
    v = (case.scale * t["W"].to(dtype).reshape(1, case.Cout, L)) * sb[:, None, :]
    if not demod:
        return v
    ss = ((v[..., :-1] if mutant == "norm_short" else v) ** 2).sum(-1, keepdim=True)
    d = torch.rsqrt(ss) + 1e-8 if mutant == "eps_after_rsqrt" else torch.rsqrt(ss + 1e-8)
    return v * d


def mod_bound(case, t, demod):
    wm = mod_ref(case, t, F64, demod).abs()
    n = ceil_div(case.Cin * case.ksq, 64)
    return wm * (((n + 12) / 2 + 4 + 3) * U if demod else 2 * U)


MOD_CASES = [ModCase(1, 1, 1, 1, row_len=1, rows=1), ModCase(3, 5, 63, 1, idle_lanes=1, idle_waves=1), ModCase(2, 6, 64, 1, idle_lanes=0),
             ModCase(1, 3, 1024, 1, cached=True), ModCase(1, 3, 1028, 1, cached=False, idle_lanes=60),
             ModCase(2, 2, 120, 9, cached=False, row_len=1080), ModCase(3, 3, 40, 1, idle_waves=3),
             ModCase(2, 4, 64, 1, s_scale=1e-3)]
# aligned cases whose packed fp32 / split / bf16 layouts are un-packed and held to the same bound
MOD_PACKED_CASES = [ModCase(2, 32, 64, 1), ModCase(1, 64, 96, 1)]


def unpack_bf16(packed, B, M, K):
    """the bf16 fragments (the split layout's positions, one plane) back as fp32 [B,M,K]"""
    h = packed.reshape(-1).view(torch.bfloat16)[:B * M * K].reshape(B, M // 16, K // 32, 4, 16, 8).float()
    return h.permute(0, 1, 4, 2, 3, 5).reshape(B, M, K)
