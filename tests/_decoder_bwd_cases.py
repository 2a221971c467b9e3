"""Cases, fp64 references and rounding-error bounds of the convolution half of csrc/backward.hip: gemm_wgrad_kernel,
act_bwd_kernel + sum_to_scalar_kernel + noise_bwd_kernel (cips3d_noise_bias_act_bwd), torgb_bwd_kernel, modulate_bwd_du / dw /
ds_kernel and pack_kernel.  Shared by test_decoder_bwd_cases_host.py (CPU: every bound admits torch fp32 and rejects every
mutant, the sentinels sit on the replayed chunk and block edges) and test_gpu_decoder_bwd.py (the kernels).  Imports no GPU code.

Every reference is a plain torch expression, generic in its dtype: evaluated in float64 it is the oracle, in float32 (on the
CPU) it is "a correct fp32 implementation", with a `mutant` it is a subtly wrong one.  Scalars are fp32 numbers, so the kernel
and the reference see the same values.  The gradient operand of every case is multiplied by `gs` (1 or 2^-20, exact): no bound
has an absolute floor, all of them scale with the data.

Sentinels.  On both operands of every pixel contraction the first and the last pixel of every pixel chunk (gemm_wgrad) or
1024-pixel block (act_bwd, torgb_bwd) and the first and last pixel of the tensor's last float4 hold +-2^6 on every row (one
random sign per row): a kernel that loses, or counts twice, an edge pixel is off by 2^12 in every element, far above any bound
below.  The positions come from `wgrad_launch` / `pixel_blocks`, which replay the host's launch arithmetic -- to CHOOSE cases,
never to compute a reference.

Bounds.  u = 2^-24, gamma_k = k u / (1 - k u), times the sum of the absolute terms, evaluated in fp64 per element.  The float
atomics leave the order of the partial sums free, so every count below is the worst case over all orders: a term is charged
one rounding for every addition that can come after it.  (Adding to the zero a memset left is exact.)

gemm_wgrad_kernel: dwm[b][m][k] = sum_p dy[b][m][p] x[b][k][p].  A pixel chunk of L_c pixels is one chain of fused
multiply-adds in the accumulator of v_mfma_f32_16x16x4_f32: a term passes at most L_c roundings (the zero pixels behind a ragged
last step add exactly).  The n chunks then meet through n atomics, the first on zero: n - 1 more.  Every chunk holds at least
four pixels, so L_c <= P - 4 (n - 1) and L_c + n - 1 <= P whatever the split.  What the matrix instruction does inside its four
k-slices (products rounded before they are added, a tree of its own) is not documented; eight roundings are set aside for it:
    e = gamma_(P + 8) sum_p |dy x|
(the worst-case bound grows with P: from a few thousand pixels on, one lost float4 of ORDINARY data no longer leaves it in
every element -- there the sentinels, not the margin, are what catches an edge; no case has more than 4112 pixels).

block_sum_256 (act_bwd_kernel, sum_to_scalar_kernel, torgb_bwd_kernel): six butterfly additions in a wave, then sh[0] + sh[1] +
sh[2] + sh[3].  Threads past the data hold zeros, and adding a zero is exact: with the first `live` threads of the block
holding data a value passes T(live) = ceil(log2(min(live, 64))) + (ceil(live / 64) - 1) inexact additions, 9 in a full block.
A case's `live` is that of its fullest block, min(256, HW / 4).

act_bwd_kernel: g = dy slope, slope = y > 0 ? S : (0.2f S) with S = fp32(sqrt 2), both fp32 constants: one product,
    dx:      e = u |dx|
    dbias_c = sum_{b,p} dx: the rounding of dx (1), two additions inside the float4, T(live), then nblk B atomics
             (nblk = ceil(HW / 1024)), the first on zero:
             e = gamma_(3 + T(live) + nblk B - 1) sum |dx|
    dnw = sum_{b,c,p} dx noise: dx (1), the product and three fmas inside the float4 (4), T(live), nblk B - 1 atomics into the
             channel's slot; sum_to_scalar_kernel: ceil(C / 256) - 1 additions per thread, T(min(C, 256)):
             e = gamma_(5 + T(live) + nblk B - 1 + ceil(C / 256) - 1 + T(min(C, 256))) sum |dx noise|
noise_bwd_kernel: dnoise[bn][p] = nw sum_c dx: dx (1), a chain of min(C, 32) - 1 additions over the channels of the chunk, the
    product with nw (1), then m = ceil(C / 32) (x B for a shared map) atomics, the first on zero:
             e = gamma_(min(C, 32) + m) |nw| sum |dx|

torgb_bwd_kernel:
    dx[c][p] = sum_r wm[r][c] drgb[r][p]: a product and two fmas:                    e = gamma_3 sum_r |wm drgb|
    dwm[b][r][c] = sum_p drgb x: product + three fmas (4), T(live), nblk - 1 atomics:
                                                                                     e = gamma_(4 + T(live) + nblk - 1) sum_p |drgb x|
    dbias_r = sum_{b,p} drgb: float4 (2), T(live), nblk B - 1 atomics:                 e = gamma_(2 + T(live) + nblk B - 1) sum |drgb|

modulate_bwd_*: len = Cin ksq, n = ceil(len / 64) terms per lane.  u = (scale W) s: two roundings, rel(u) = 2 u.
    du kernel (demodulate).  ss = sum u^2 by fma (the square itself is not rounded): rel 4 u from u, n + 6 of the chain and
    the butterfly; + 1e-8f (the constant rounded to fp32, the addition): rel(ss + eps) <= (n + 12) u.  d = rsqrtf(.): half of
    that, and the instruction itself (v_rsq_f32: 1 ulp; 2 ulp = 4 u allowed, as _dense_cases.py allows PixelNorm):
        rel(d) = ((n + 12) / 2 + 4) u
    dot = <dwm, u>: rel(u), the chain, the butterfly:                 e(dot) = gamma_(n + 8) sum |dwm u|
    c = d d d dot: three products, three times rel(d):                e(c) = |d|^3 e(dot) + |c| (3 rel(d) + 3 u)
    du = fma(dwm, d, -(c u)): the product c u rounded, rel(u), the fma:
        e(du) = |dwm d| rel(d) + |u| e(c) + 3 u |c u| + u |du|
    (without demodulation du = dwm, e(du) = 0).
    dW[o][e] = scale sum_b du s: B fmas, the scale:
        e = |scale| (sum_b |s| e(du) + gamma_(B + 1) sum_b |du s|)
    ds[b][i] = scale sum_o sum_t du W: ceil(Cout / 16) ksq fmas per row group, 16 additions of the partial sums, the scale:
        e = |scale| (sum |W| e(du) + gamma_(ceil(Cout / 16) ksq + 17) sum |du W|)
The reference of modulate_bwd is autograd through the FORWARD formula wm = u rsqrt(sum u^2 + 1e-8); the closed form above is used
for the bound's intermediates and the mutants only (test_decoder_bwd_cases_host.py checks that it is the same function).

pack_kernel moves bits: compared bit for bit after un-packing (`unpack`); its split form stores fp16 hi + lo of 2^8 w, held to
2^-21 of the largest |w| (the bar of test_gpu_conv3x3.py for the same split).
"""
import math

import torch

from _dense_cases import U, f32, gamma, inside, worst  # noqa: F401  (re-exported)

F32, F64 = torch.float32, torch.float64
SCALES = (1.0, 2.0 ** -20)
SENT = 64.0


def ceil_div(a, b):
    return -(-a // b)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1000003 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _plant(t, positions, g):
    """+-SENT on every row of t [..., P] at the pixel positions; one random sign per row, so that the sentinel products of an
    output element all have one sign and no two lost pixels cancel"""
    pos = torch.tensor(sorted(positions))
    sign = torch.randint(0, 2, t.shape[:-1] + (1,), generator=g).to(t.dtype) * 2 - 1
    t[..., pos] = SENT * sign


# ------------------------------------------------------------------------------------------------------------- gemm_wgrad
def wgrad_launch(B, M, K, P):
    """(row blocks, column blocks, n_chunks, chunk) as cips3d_gemm_wgrad computes them"""
    blocks = ceil_div(M, 64) * ceil_div(K, 64)
    n = min(ceil_div(1024, blocks * B), ceil_div(P, 256))
    n = max(n, 1)
    chunk = ceil_div(ceil_div(P, n), 16) * 16
    return ceil_div(M, 64), ceil_div(K, 64), ceil_div(P, chunk), chunk


def chunk_edges(P, chunk):
    """[(first pixel, one past the last pixel)] of every chunk / block"""
    return [(p, min(p + chunk, P)) for p in range(0, P, chunk)]


def edge_pixels(P, chunk):
    pos = {P - 4, P - 1}
    for a, b in chunk_edges(P, chunk):
        pos |= {a, b - 1}
    return sorted(pos)


class WgradCase:
    def __init__(self, B, M, K, P, **expect):
        """expect: the regime the case is in the list for (n_chunks, chunk, last = pixels of the last chunk, last_step =
        pixels of its last 16-pixel step, mb / kb = row / column blocks), checked against wgrad_launch by the host test"""
        self.B, self.M, self.K, self.P, self.expect = B, M, K, P, expect

    @property
    def id(self):
        return f"B{self.B}-M{self.M}-K{self.K}-P{self.P}"

    def launch(self):
        return wgrad_launch(self.B, self.M, self.K, self.P)

    def regime(self):
        mb, kb, n, chunk = self.launch()
        last = self.P - (n - 1) * chunk
        return dict(n_chunks=n, chunk=chunk, last=last, last_step=(last - 1) % 16 + 1, mb=mb, kb=kb,
                    idle_wave_row=self.M % 64 == 32, idle_wave_col=self.K % 64 == 32)

    def sentinels(self):
        return edge_pixels(self.P, self.launch()[3])

    def tensors(self, gs=1.0):
        g = _gen(1, self.B, self.M, self.K, self.P)
        dy, x = torch.randn(self.B, self.M, self.P, generator=g), torch.randn(self.B, self.K, self.P, generator=g)
        _plant(dy, self.sentinels(), g)
        _plant(x, self.sentinels(), g)
        return dict(dy=dy * gs, x=x)

    def mutants(self):
        return ["drop_tail4", "dup_tail4", "swap_mk"] + (["chunk_overlap"] if self.launch()[2] > 1 else [])


def wgrad_ref(t, dtype, mutant=None, chunk=None):
    """dwm [B,M,K]; chunk: the pixel chunk of the launch (the mutant `chunk_overlap` only)"""
    dy, x = t["dy"].to(dtype), t["x"].to(dtype)
    B, M, P = dy.shape
    K = x.shape[1]
    mm = lambda a, b: torch.einsum("bmp,bkp->bmk", a, b)      # noqa: E731
    if mutant == "swap_mk":
        return torch.einsum("bmp,bkp->bkm", dy, x).reshape(B, M, K)
    if mutant == "drop_tail4":
        return mm(dy[..., :P - 4], x[..., :P - 4])
    out = mm(dy, x)
    if mutant == "dup_tail4":
        out = out + mm(dy[..., P - 4:], x[..., P - 4:])
    if mutant == "chunk_overlap":          # the last step of a chunk counted in the next chunk too
        for _, end in chunk_edges(P, chunk)[:-1]:
            out = out + mm(dy[..., end - 16:end], x[..., end - 16:end])
    return out


def wgrad_bound(dy, x):
    dy, x = dy.double().abs(), x.double().abs()
    return gamma(dy.shape[-1] + 8) * torch.einsum("bmp,bkp->bmk", dy, x)


WGRAD_CASES = [
    WgradCase(1, 32, 32, 4, n_chunks=1, last=4, last_step=4),                    # one step, only the lane quarter q = 0 loads
    WgradCase(2, 32, 96, 260, n_chunks=2, chunk=144, last=116, last_step=4, kb=2, idle_wave_col=True),
    WgradCase(3, 96, 32, 1028, n_chunks=5, chunk=208, last=196, last_step=4, mb=2, idle_wave_row=True),
    WgradCase(1, 64, 64, 2144, n_chunks=9, last_step=16, idle_wave_row=False, idle_wave_col=False),
    WgradCase(1, 160, 96, 512, n_chunks=2, chunk=256, mb=3, kb=2, idle_wave_row=True, idle_wave_col=True),
    WgradCase(1, 32, 64, 4112, n_chunks=17, chunk=256, last=16),                 # the largest case
]


# ----------------------------------------------------------------------------------------------------- noise + bias + lrelu
S_HI = f32(1.41421356237309515)
S_LO = float(torch.tensor(0.2, dtype=F32) * torch.tensor(S_HI, dtype=F32))
NOISE_W = f32(0.3)
BLOCK_PIXELS = 1024


def pixel_blocks(HW):
    """(blocks per channel of act_bwd_kernel / torgb_bwd_kernel, live threads of the last one)"""
    n = ceil_div(HW, BLOCK_PIXELS)
    return n, ceil_div(HW - (n - 1) * BLOCK_PIXELS, 4)


def tree_adds(live):
    """T(live) of the module docstring: inexact additions a value passes in block_sum_256"""
    lanes = min(live, 64)
    return (lanes - 1).bit_length() + ceil_div(live, 64) - 1


def live_threads(HW):
    return min(256, ceil_div(HW, 4))


def noise_stride(B, noise_batch, HW):
    """the sample stride the wrappers hand to the library: per-sample noise only if B > 1"""
    return HW if (noise_batch == B and B > 1) else 0


# (name, keyword arguments of hip.noise_bias_act_bwd, noise given)
ACT_FLAGS = [("all", dict(need_dnoise=True, need_dnw=True, need_db=True), True),
             ("db_only", dict(need_dnoise=False, need_dnw=False, need_db=True), False),
             ("dnw_no_db", dict(need_dnoise=False, need_dnw=True, need_db=False), True),
             ("dnoise_no_dnw", dict(need_dnoise=True, need_dnw=False, need_db=True), True)]


class ActCase:
    def __init__(self, B, C, HW, noise_batch, **expect):
        self.B, self.C, self.HW, self.noise_batch, self.expect = B, C, HW, noise_batch, expect

    @property
    def id(self):
        return f"B{self.B}-C{self.C}-HW{self.HW}-" + ("per_sample" if self.per_sample else f"shared{self.noise_batch}")

    @property
    def per_sample(self):
        return noise_stride(self.B, self.noise_batch, self.HW) != 0

    def regime(self):
        nblk, live = pixel_blocks(self.HW)
        return dict(blocks=nblk, live_last=live, channel_chunks=ceil_div(self.C, 32), last_chunk=(self.C - 1) % 32 + 1,
                    stride=noise_stride(self.B, self.noise_batch, self.HW))

    def sentinels(self):
        return edge_pixels(self.HW, BLOCK_PIXELS)

    def tensors(self, gs=1.0):
        """dy, y [B,C,HW], noise [noise_batch,1,HW]; y holds exact 0.0 in its first two and -0.0 in its last two pixels (one
        with a sentinel gradient, one with an ordinary one: the sentinels of a pixel may cancel over the channels)"""
        g = _gen(2, self.B, self.C, self.HW, self.noise_batch)
        dy, y = torch.randn(self.B, self.C, self.HW, generator=g), torch.randn(self.B, self.C, self.HW, generator=g)
        noise = torch.randn(self.noise_batch, 1, self.HW, generator=g)
        _plant(dy, self.sentinels(), g)
        _plant(noise, self.sentinels(), g)
        y[..., :2] = 0.0
        y[..., self.HW - 2:] = -0.0
        return dict(dy=dy * gs, y=y, noise=noise)

    def mutants(self):
        return ["slope_at_zero", "drop_last_block", "dnw_skip_channel"] + (["noise_one_sample"] if self.per_sample else [])


# which outputs (dx, dnoise, dnw, db) a mutant changes
ACT_HITS = {"slope_at_zero": (0, 1, 2, 3), "drop_last_block": (0, 1, 2, 3), "dnw_skip_channel": (2,), "noise_one_sample": (1, 2)}


def act_ref(t, dtype, per_sample, mutant=None):
    """(dx [B,C,HW], dnoise like noise, dnw [1], db [C])"""
    dy, y, noise = t["dy"].to(dtype), t["y"], t["noise"].to(dtype)
    B, C, HW = dy.shape
    positive = (y >= 0) if mutant == "slope_at_zero" else (y > 0)
    dx = dy * torch.where(positive, torch.tensor(S_HI, dtype=dtype), torch.tensor(S_LO, dtype=dtype))
    if mutant == "drop_last_block":
        dx = dx.clone()
        dx[..., (pixel_blocks(HW)[0] - 1) * BLOCK_PIXELS:] = 0
    nz = noise[:, 0] if (per_sample and mutant != "noise_one_sample") else noise[0:1, 0].expand(B, HW)
    per_c = (dx * nz[:, None, :]).sum((0, 2))
    dnw = (per_c[:-1] if mutant == "dnw_skip_channel" else per_c).sum().reshape(1)
    dn = NOISE_W * dx.sum(1)                                               # [B,HW]
    if per_sample and mutant == "noise_one_sample":
        dnoise = torch.zeros_like(noise)
        dnoise[0, 0] = dn.sum(0)
    else:
        dnoise = dn[:, None, :] if per_sample else dn.sum(0)[None, None, :]
    return dx, dnoise, dnw, dx.sum((0, 2))


def act_bounds(t, per_sample):
    dx, _, _, _ = act_ref(t, F64, per_sample)
    noise = t["noise"].double()
    B, C, HW = dx.shape
    nblk = pixel_blocks(HW)[0]
    a = dx.abs()
    nz = noise[:, 0] if per_sample else noise[0:1, 0].expand(B, HW)
    T = tree_adds(live_threads(HW))
    e_db = gamma(3 + T + nblk * B - 1) * a.sum((0, 2))
    k_dnw = 5 + T + nblk * B - 1 + ceil_div(C, 256) - 1 + tree_adds(min(C, 256))
    e_dnw = gamma(k_dnw) * (a * nz.abs()[:, None, :]).sum().reshape(1)
    m = ceil_div(C, 32) * (1 if per_sample else B)
    e_dn = gamma(min(C, 32) + m) * abs(NOISE_W) * a.sum(1)
    e_dnoise = e_dn[:, None, :] if per_sample else e_dn.sum(0)[None, None, :]
    return U * a, e_dnoise, e_dnw, e_db


ACT_CASES = [
    ActCase(1, 1, 4, 1, blocks=1, live_last=1),
    ActCase(2, 33, 1028, 1, blocks=2, live_last=1, channel_chunks=2, last_chunk=1, stride=0),
    ActCase(3, 5, 2052, 3, blocks=3, live_last=1, stride=2052),
    ActCase(1, 64, 1024, 1, blocks=1, live_last=256, stride=0),                 # noise of batch 1 = B: the nb = 0 rule
]


# --------------------------------------------------------------------------------------------------------------------- ToRGB
class RgbCase:
    def __init__(self, B, C, HW, **expect):
        self.B, self.C, self.HW, self.expect = B, C, HW, expect

    @property
    def id(self):
        return f"B{self.B}-C{self.C}-HW{self.HW}"

    def regime(self):
        nblk, live = pixel_blocks(self.HW)
        return dict(blocks=nblk, live_last=live)

    def sentinels(self):
        return edge_pixels(self.HW, BLOCK_PIXELS)

    def tensors(self, gs=1.0):
        g = _gen(3, self.B, self.C, self.HW)
        drgb, x = torch.randn(self.B, 3, self.HW, generator=g), torch.randn(self.B, self.C, self.HW, generator=g)
        wm = torch.randn(self.B, 3, self.C, generator=g) / math.sqrt(self.C)
        _plant(drgb, self.sentinels(), g)
        _plant(x, self.sentinels(), g)
        return dict(drgb=drgb * gs, x=x, wm=wm)

    def mutants(self):
        return ["drop_last_block"] + (["bias_every_channel", "wm_transposed"] if self.C > 1 else [])


# which outputs (dx, dwm, db) a mutant changes
RGB_HITS = {"drop_last_block": (0, 1, 2), "bias_every_channel": (2,), "wm_transposed": (0, 1)}


def rgb_ref(t, dtype, mutant=None):
    """(dx [B,C,HW], dwm [B,3,C], db [3])"""
    g, x, wm = t["drgb"].to(dtype), t["x"].to(dtype), t["wm"].to(dtype)
    B, C, HW = x.shape
    if mutant == "wm_transposed":
        wm = wm.reshape(B, C, 3).transpose(1, 2)
    if mutant == "drop_last_block":
        g = g.clone()
        g[..., (pixel_blocks(HW)[0] - 1) * BLOCK_PIXELS:] = 0
    dx = torch.einsum("brc,brp->bcp", wm, g)
    dwm = torch.einsum("brp,bcp->brc", g, x)
    if mutant == "wm_transposed":
        dwm = dwm.transpose(1, 2).reshape(B, 3, C)
    db = g.sum((0, 2)) * (C if mutant == "bias_every_channel" else 1)
    return dx, dwm, db


def rgb_bounds(t):
    g, x, wm = t["drgb"].double().abs(), t["x"].double().abs(), t["wm"].double().abs()
    B, C, HW = x.shape
    nblk, T = pixel_blocks(HW)[0], tree_adds(live_threads(HW))
    return (gamma(3) * torch.einsum("brc,brp->bcp", wm, g), gamma(4 + T + nblk - 1) * torch.einsum("brp,bcp->brc", g, x),
            gamma(2 + T + nblk * B - 1) * g.sum((0, 2)))


RGB_CASES = [RgbCase(1, 1, 4, blocks=1, live_last=1), RgbCase(2, 33, 1028, blocks=2, live_last=1),
             RgbCase(3, 64, 2052, blocks=3, live_last=1)]


# ---------------------------------------------------------------------------------------------------------------- modulation
class ModCase:
    def __init__(self, B, Cout, Cin, ksq, demod, s_scale=1.0, **expect):
        self.B, self.Cout, self.Cin, self.ksq, self.demod, self.s_scale, self.expect = B, Cout, Cin, ksq, demod, s_scale, expect
        self.scale = f32(1.0 / math.sqrt(Cin * ksq))

    @property
    def id(self):
        return f"B{self.B}-o{self.Cout}-i{self.Cin}-k{self.ksq}" + ("-demod" if self.demod else "") + \
            ("-small" if self.s_scale != 1.0 else "")

    def regime(self):
        L = self.Cin * self.ksq
        return dict(row_len=L, idle_lanes=(64 - L % 64) % 64, rows=self.B * self.Cout, du_blocks=ceil_div(self.B * self.Cout, 4),
                    ds_col_blocks=ceil_div(self.Cin, 64), ds_last_cols=(self.Cin - 1) % 64 + 1)

    def tensors(self, gs=1.0):
        """W [1,Cout,Cin,k,k], s [B,Cin], dwm [B,Cout,Cin ksq]"""
        k = int(math.isqrt(self.ksq))
        g = _gen(4, self.B, self.Cout, self.Cin, self.ksq)
        W = torch.randn(1, self.Cout, self.Cin, k, k, generator=g)
        s = (1.0 + 0.5 * torch.randn(self.B, self.Cin, generator=g)) * self.s_scale
        dwm = torch.randn(self.B, self.Cout, self.Cin * self.ksq, generator=g)
        return dict(W=W, s=s, dwm=dwm * gs)

    def mutants(self):
        return ["tap_index"] + (["no_projection"] if self.demod else []) + (["eps_missing"] if self.s_scale != 1.0 else [])


# which outputs (dW, ds) a mutant changes, given `demod`
def mod_hits(mutant, demod):
    return (0, 1) if (demod or mutant != "tap_index") else (0,)


def mod_grads(t, c, dtype):
    """(dW like W, ds [B,Cin]) by autograd in `dtype` through the forward formula"""
    W, s = t["W"].to(dtype).clone().requires_grad_(True), t["s"].to(dtype).clone().requires_grad_(True)
    u = c.scale * W.reshape(1, c.Cout, c.Cin, c.ksq) * s[:, None, :, None]
    wm = u * torch.rsqrt((u * u).sum((2, 3), keepdim=True) + 1e-8) if c.demod else u
    (wm.reshape(c.B, c.Cout, -1) * t["dwm"].to(dtype)).sum().backward()
    return W.grad, s.grad


def _mod_parts(t, c, dtype, mutant=None):
    L = c.Cin * c.ksq
    e = torch.arange(L)
    idx = (e % c.ksq) % c.Cin if mutant == "tap_index" else e // c.ksq
    W2, g = t["W"].to(dtype).reshape(c.Cout, L), t["dwm"].to(dtype)
    sb = t["s"].to(dtype)[:, idx]                                          # [B,L]
    u = c.scale * W2[None] * sb[:, None, :]
    return W2, g, sb, u


def mod_closed(t, c, dtype, mutant=None):
    """the kernels' closed form (mutants; never the reference)"""
    W2, g, sb, u = _mod_parts(t, c, dtype, mutant)
    du = g
    if c.demod:
        d = torch.rsqrt((u * u).sum(-1, keepdim=True) + (0.0 if mutant == "eps_missing" else 1e-8))
        du = g * d
        if mutant != "no_projection":
            du = du - d ** 3 * (g * u).sum(-1, keepdim=True) * u
    dW = c.scale * (du * sb[:, None, :]).sum(0)
    ds = c.scale * (du * W2[None]).reshape(c.B, c.Cout, c.Cin, c.ksq).sum((1, 3))
    return dW.reshape(t["W"].shape), ds


def mod_bounds(t, c):
    """(e_dW, e_ds), module docstring"""
    W2, g, sb, u = _mod_parts(t, c, F64)
    L = c.Cin * c.ksq
    n = ceil_div(L, 64)
    du, e_du = g, torch.zeros_like(g)
    if c.demod:
        d = torch.rsqrt((u * u).sum(-1, keepdim=True) + 1e-8)
        rel_d = ((n + 12) / 2 + 4) * U
        dot = (g * u).sum(-1, keepdim=True)
        e_dot = gamma(n + 8) * (g * u).abs().sum(-1, keepdim=True)
        cc = d ** 3 * dot
        e_c = d ** 3 * e_dot + cc.abs() * (3 * rel_d + 3 * U)
        du = g * d - cc * u
        e_du = (g * d).abs() * rel_d + u.abs() * e_c + 3 * U * (cc * u).abs() + U * du.abs()
    sc = abs(c.scale)
    e_dW = sc * ((e_du * sb.abs()[:, None, :]).sum(0) + gamma(c.B + 1) * (du * sb[:, None, :]).abs().sum(0))
    kds = ceil_div(c.Cout, 16) * c.ksq + 17
    shape = (c.B, c.Cout, c.Cin, c.ksq)
    e_ds = sc * ((e_du * W2.abs()[None]).reshape(shape).sum((1, 3)) + gamma(kds) * (du * W2[None]).abs().reshape(shape).sum((1, 3)))
    return e_dW.reshape(t["W"].shape), e_ds


MOD_CASES = [
    ModCase(3, 3, 40, 1, False, row_len=40),                                    # a ToRGB: the du kernel is skipped
    ModCase(1, 5, 7, 9, True, row_len=63, idle_lanes=1),
    ModCase(2, 33, 72, 1, True, rows=66, du_blocks=17, ds_col_blocks=2, ds_last_cols=8),
    ModCase(2, 16, 32, 9, True, row_len=288),
    ModCase(1, 64, 64, 1, True, s_scale=1e-3),                                  # sum u^2 meets the 1e-8
]


# ------------------------------------------------------------------------------------------------------------------- packing
PACK_CASES = [(2, 48, 32), (2, 32, 80)]                       # (B, M, K), each plain and transposed
PACK_SPLIT_CASES = [(2, 48, 64, False), (2, 64, 48, True)]    # (B, M, K, transpose): the packed contraction length % 32 == 0


def pack_input(B, M, K):
    return torch.randn(B, M, K, generator=_gen(5, B, M, K))


def pack_index(B, M, K, transpose):
    """flat destination of wm[b][r][c] in the plain packed form, element by element as pack_kernel computes it"""
    e = torch.arange(B * M * K)
    b, r, c = e // (M * K), (e // K) % M, e % K
    o, i = (c, r) if transpose else (r, c)
    OM, OK = (K, M) if transpose else (M, K)
    return ((b * (OM // 16) + o // 16) * (OK // 16) + i // 16) * 256 + ((i % 4) * 16 + o % 16) * 4 + (i // 4) % 4


def unpack(packed, B, M, K, transpose):
    """the packed matrix [B,OM,OK] (wm or its transpose) back from the A-fragment order: blocks of 16 rows x 16 columns,
    inside a block [q = column % 4][row][j = column / 4]"""
    OM, OK = (K, M) if transpose else (M, K)
    return packed.reshape(B, OM // 16, OK // 16, 4, 16, 4).permute(0, 1, 4, 2, 5, 3).reshape(B, OM, OK)


def unpack_split(packed, B, M, K, transpose):
    """(hi + lo) / 2^8 as fp32 [B,OM,OK] from the split form: blocks of 16 rows x 32 columns, a plane of hi and one of lo,
    inside a plane [q = (column / 8) % 4][row][j = column % 8]"""
    OM, OK = (K, M) if transpose else (M, K)
    h = packed.reshape(-1).view(torch.float16).reshape(B, OM // 16, OK // 32, 2, 4, 16, 8).float()
    v = (h[:, :, :, 0] + h[:, :, :, 1]) / 256.0                       # b, ot, kb, q, row, j
    return v.permute(0, 1, 4, 2, 3, 5).reshape(B, OM, OK)
