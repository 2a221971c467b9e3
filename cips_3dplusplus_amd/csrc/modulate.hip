// Weight modulation and range constants of the StyleGAN2-style decoder of CIPS-3D++ on gfx950 (reference
// models/model_v3.py:218-341,418-482,592-637).
//
//   cips3d_modulate_weights  per-sample weight modulation + demodulation (model_v3.py:267-278); optionally
//                            emits the matrix in MFMA A-fragment order for the GEMMs (gemm1x1.hip, fused_stage.hip, chain.hip,
//                            conv3x3.hip)
//   cips3d_range_consts, cips3d_absmax, cips3d_split_words   the range tracking's constants, maxima and word formats

#include "mfma_frag.h"

namespace {

// ------------------------------------------------------------------------------------------------
// weight modulation.  One wave per (b, o).
//   plain : wm[b][o][i*ksq + t]
//   packed (ksq == 1, Cout % 16 == 0, Cin % 16 == 0): A-fragment order of v_mfma_f32_16x16x4_f32
//           wmp[b][ot][kq][lane][j] = wm[b][ot*16 + (lane&15)][16*kq + 4*j + (lane>>4)]
//   packed + split (ksq == 1, Cin % 32 == 0; CIPS3D_MOD_SPLIT): A fragments of v_mfma_f32_16x16x32_f16, hi and lo fp16 halves of
//           2^8 wm:  wms[b][ot][kb][plane][lane][j] (fp16) = plane(2^8 wm[b][ot*16 + (lane&15)][32 kb + 8 (lane>>4) + j]) -- one
//           o-tile x 32-channel block = 2 x 1 KiB = the bytes of the two fp32 k-groups it replaces (same LDS-DMA pieces)
//   packed + bf16 (ksq == 1, Cin % 32 == 0; CIPS3D_MOD_BF16): A fragments of v_mfma_f32_16x16x32_bf16 in the same positions,
//           one plane of bf16(wm) (round to nearest even), unscaled: wmb[b][ot][kb][lane][j] -- for cips3d_modconv1x1_planes16
//   packed, ksq == 9 (the 3x3 implicit GEMM, conv3x3.hip): the same fragment order per tap, tap-major:
//           wmp[b][t'][ot][kq][lane][j], t' = t, or 8 - t with CIPS3D_MOD_FLIP (the transposed conv of the up-sampling branch)
// ------------------------------------------------------------------------------------------------
// Range constants of a StyledConv (cips3d_range): lconst = {c0, c1, l1, 0} with |out| <= max(c1, sqrt(2) l1) max|in| + c0.
//   c0 = sqrt(2) (|noise_w| noise_bound + max |bias|)       (leaky ReLU * sqrt(2) is 1-Lipschitz * sqrt(2) through 0)
//   c1 = sqrt(2) w_gain; a demodulated row has unit L2 norm, so its L1 norm is <= sqrt(Cin ksq) = w_gain; with a FIR
//        (the conv's GEMM result is up-sampled before the activation; the result's own maximum is measured) the gain is
//        the FIR's largest polyphase L1 norm (1 for [1,3,3,1])
//   l1 : raised by the rows of a non-demodulated conv to their L1 norm (modulate_row); left 0 otherwise
// One wave.
__device__ __forceinline__ void layer_consts(const float* __restrict__ bias, int n_bias, const float* __restrict__ noise_w,
                                             float noise_bound, float w_gain, const float* __restrict__ fir,
                                             float* __restrict__ lconst, int lane) {
  float bm = 0.f;
  if (bias)
    for (int i = lane; i < n_bias; i += 64) bm = fmaxf(bm, fabsf(bias[i]));
  bm = wave_max(bm);
  float gain = w_gain;
  if (fir) {
    gain = 0.f;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      const int py = ph >> 1, px = ph & 1;
      float g = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) g += fabsf(fir[(py + 2 * (t >> 1)) * 4 + px + 2 * (t & 1)]);
      gain = fmaxf(gain, g);
    }
  }
  if (lane == 0) {
    const float nwa = noise_w ? fabsf(noise_w[0]) : 0.f;
    lconst[0] = 1.41421356237309515f * (nwa * noise_bound + bm);
    lconst[1] = 1.41421356237309515f * gain;
  }
}

__device__ __forceinline__ void modulate_row(const float* __restrict__ W, const float* __restrict__ sb_,
                                             float* __restrict__ wm_, int b, int o, int Cout, int Cin, int ksq,
                                             float scale, int demod, int packed, int lane, float* __restrict__ l1_out = nullptr) {
  const int len = Cin * ksq;
  const auto* w = cips3d_g(W + (int64_t)o * len);       // (global, whatever the pointers' provenance: see cips3d_g)
  const auto* sb = cips3d_g(sb_);
  auto* wm = cips3d_g(wm_);
  // (A 16-byte-store form of the split / bf16 layouts -- 8 consecutive channels per lane, bit-identical output -- was built
  // and measured: modulate_table_kernel 10.9 us against 10.3 us.  The launch is a chain of dependent latencies (descriptor,
  // row, reduction, store), not store-bound; not kept.)
  constexpr int MAXV = 16;                 // rows up to 1024 values stay in registers between the two passes
  const bool cached = len <= 64 * MAXV;
  float vreg[MAXV];
  float ss = 0.f;
  if (cached) {
#pragma unroll
    for (int m = 0; m < MAXV; ++m) {
      const int e = lane + 64 * m;
      vreg[m] = e < len ? (scale * w[e]) * sb[e / ksq] : 0.f;
      ss = fmaf(vreg[m], vreg[m], ss);
    }
  } else if (demod) {
    for (int e = lane; e < len; e += 64) {
      const float v = (scale * w[e]) * sb[e / ksq];
      ss = fmaf(v, v, ss);
    }
  }
  if (demod) ss = wave_sum(ss);
  const float d = demod ? rsqrtf(ss + 1e-8f) : 1.f;
  if (!demod && l1_out) {     // no unit norm to lean on: the row's L1 norm bounds |sum_i wm_oi x_i| / max|x| (cips3d_range)
    float l1 = 0.f;
    if (cached) {
#pragma unroll
      for (int m = 0; m < MAXV; ++m) l1 += fabsf(vreg[m]);
    } else {
      for (int e = lane; e < len; e += 64) l1 += fabsf((scale * w[e]) * sb[e / ksq]);
    }
    l1 = wave_sum(l1);
    if (lane == 0) atomicMax(reinterpret_cast<unsigned*>(l1_out), __float_as_uint(l1));
  }
  auto put = [&](int e, float v) {
    if (demod) v *= d;
    if (packed & 32) {            // split-fp16 fragments of the fused stages: 16-channel k-groups, [lane][hi x4 | lo x4]
      const int i = e;
      const int ot = o >> 4, kq = i >> 4;
      const bool chained = (packed & 7) == 2;      // element <-> channel as in the fp32 layouts below
      const int el = chained ? (i & 3) : ((i >> 2) & 3), q = chained ? ((i >> 2) & 3) : (i & 3);
      const float sv = v * kSplitScale;
      _Float16 hi, lo;
      cips3d_split16(sv, hi, lo);
      auto* blk = cips3d_g(reinterpret_cast<_Float16*>(wm_)) + ((((int64_t)b * (Cout >> 4) + ot) * (Cin >> 4) + kq) * 512) +
                      ((q << 4) | (o & 15)) * 8;
      blk[el] = hi;
      blk[4 + el] = lo;
    } else if ((packed & 16) && (packed & 64)) {     // split-fp16 fragments of wm^T (ksq == 1): row = input channel, k = output unit
      const int i = e;
      const int j = o & 7, q = (o >> 3) & 3;
      const float sv = v * kSplitScale;
      _Float16 hi, lo;
      cips3d_split16(sv, hi, lo);
      auto* blk = cips3d_g(reinterpret_cast<_Float16*>(wm_)) + ((((int64_t)b * (Cin >> 4) + (i >> 4)) * (Cout >> 5) + (o >> 5)) * 1024);
      blk[((q << 4) | (i & 15)) * 8 + j] = hi;
      blk[512 + ((q << 4) | (i & 15)) * 8 + j] = lo;
    } else if ((packed & 16) && ksq > 1) {     // split-fp16 tap-PAIR fragments of the 3x3 kernel (conv3x3.hip: modconv3x3_split_kernel)
      // [b][pair 5][o-tile][16-channel stage][hi | lo][lane][8]: lane quarter q holds channels 8 (q & 1) .. + 7 of tap 2 pair + (q >> 1)
      const int i = e / ksq;
      const int tap = (packed & 8) ? ksq - 1 - e % ksq : e % ksq;
      const int pr = tap >> 1, hh = tap & 1;
      const int ot = o >> 4, kq = i >> 4, cg = (i >> 3) & 1, j = i & 7;
      const float sv = v * kSplitScale;
      _Float16 hi, lo;
      cips3d_split16(sv, hi, lo);
      auto* blk = cips3d_g(reinterpret_cast<_Float16*>(wm_)) + ((((int64_t)b * 5 + pr) * (Cout >> 4) + ot) * (Cin >> 4) + kq) * 1024;
      const int ln = ((((hh << 1) | cg) << 4) | (o & 15)) * 8 + j;
      blk[ln] = hi;
      blk[512 + ln] = lo;
      if (tap == ksq - 1) {         // the tenth tap of the last pair: zero weights
        const int lz = ((((2 | cg)) << 4) | (o & 15)) * 8 + j;
        blk[lz] = (_Float16)0.f;
        blk[512 + lz] = (_Float16)0.f;
      }
    } else if (packed & 16) {     // split-fp16 fragments (ksq == 1)
      const int i = e;
      const int ot = o >> 4, kb = i >> 5, j = i & 7, q = (i >> 3) & 3;      // natural k order: k = 8 q + j
      const float sv = v * kSplitScale;
      _Float16 hi, lo;
      cips3d_split16(sv, hi, lo);
      auto* blk = cips3d_g(reinterpret_cast<_Float16*>(wm_)) + ((((int64_t)b * (Cout >> 4) + ot) * (Cin >> 5) + kb) * 1024);
      blk[((q << 4) | (o & 15)) * 8 + j] = hi;
      blk[512 + ((q << 4) | (o & 15)) * 8 + j] = lo;
    } else if (packed & 128) {    // bf16 fragments of v_mfma_f32_16x16x32_bf16 (ksq == 1): the split layout's positions, one plane
      const int i = e;
      const int ot = o >> 4, kb = i >> 5, j = i & 7, q = (i >> 3) & 3;
      const __bf16 r = (__bf16)v;                                            // round to nearest even (the bf16 mode's operand rounding)
      auto* blk = cips3d_g(reinterpret_cast<unsigned short*>(wm_)) + ((((int64_t)b * (Cout >> 4) + ot) * (Cin >> 5) + kb) * 512);
      blk[((q << 4) | (o & 15)) * 8 + j] = __builtin_bit_cast(unsigned short, r);
    } else if (packed & 64) {     // fragments of wm^T (ksq == 1): row = input channel, k = output unit (backward.hip:pack_kernel)
      const int i = e;
      wm[(((int64_t)b * (Cin >> 4) + (i >> 4)) * (Cout >> 4) + (o >> 4)) * 256 + (((o & 3) << 4) | (i & 15)) * 4 + ((o >> 2) & 3)] = v;
    } else if (packed) {
      const int i = ksq == 1 ? e : e / ksq;
      const int tap = ksq == 1 ? 0 : ((packed & 8) ? ksq - 1 - e % ksq : e % ksq);
      const int ot = o >> 4, kq = i >> 4;
      // standard: k-step j of the 16-byte piece, lane quarter q = i & 3.  chained (packed == 2): the roles swap, lane quarter
      // (i >> 2) & 3 and k-step i & 3 -- the order of the MFMA D layout (4 consecutive channels per lane)
      const bool chained = (packed & 7) == 2;
      const int j = chained ? (i & 3) : ((i >> 2) & 3), q = chained ? ((i >> 2) & 3) : (i & 3);
      wm[((((int64_t)b * ksq + tap) * (Cout >> 4) + ot) * (Cin >> 4) + kq) * 256 + ((q << 4) | (o & 15)) * 4 + j] = v;
    } else {
      wm[((int64_t)b * Cout + o) * len + e] = v;
    }
  };
  if (cached) {
#pragma unroll
    for (int m = 0; m < MAXV; ++m) {
      const int e = lane + 64 * m;
      if (e < len) put(e, vreg[m]);
    }
  } else {
    for (int e = lane; e < len; e += 64) put(e, (scale * w[e]) * sb[e / ksq]);
  }
}

__global__ void __launch_bounds__(256) modulate_kernel(const float* __restrict__ W, const float* __restrict__ s,
                                                       int64_t s_stride, float* __restrict__ wm, int B, int Cout,
                                                       int Cin, int ksq, float scale, int demod, int packed) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (int64_t)B * Cout) return;
  const int b = (int)(row / Cout), o = (int)(row % Cout);
  modulate_row(W, s + (int64_t)b * s_stride, wm, b, o, Cout, Cin, ksq, scale, demod, packed, lane);
}

// every conv of the decoder in one launch: grid.x covers the table's rows, grid.y the samples
__global__ void __launch_bounds__(256) modulate_table_kernel(const cips3d_modulate_desc* __restrict__ table, int n_desc,
                                                             int total_rows, float noise_bound) {
  const int lane = threadIdx.x & 63;
  const int grow = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (grow >= total_rows) return;
  const int b = blockIdx.y;
  int lo;
  if (n_desc <= 64) {
    lo = owner_desc(table, n_desc, grow, lane);
  } else {
    lo = 0;
    int hi = n_desc - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (table[mid].row_begin <= grow) lo = mid; else hi = mid - 1;
    }
  }
  const cips3d_modulate_desc d = table[lo];
  if (d.lconst && grow == d.row_begin)
    layer_consts(d.bias, d.n_bias, d.noise_w, noise_bound, sqrtf((float)(d.Cin * d.ksq)), d.fir, d.lconst + b * 4, lane);
  modulate_row(d.W, d.s + (int64_t)b * d.s_stride, d.out, b, grow - d.row_begin, d.Cout, d.Cin, d.ksq, d.scale,
               d.flags & 1, (d.flags & 2) ? (((d.flags & 4) ? 2 : 1) | (d.flags & 248)) : 0, lane,
               d.lconst ? d.lconst + b * 4 + 2 : nullptr);
}

// cips3d_range_consts: the same constants for one layer from the per-op path; cips3d_absmax: amax slots of an existing tensor
__global__ void __launch_bounds__(64) range_consts_kernel(const float* __restrict__ bias, int n_bias, const float* __restrict__ noise_w,
                                                          float noise_bound, const float* __restrict__ noise_amax, float w_gain,
                                                          const float* __restrict__ fir, float* __restrict__ lconst) {
  float* lc = lconst + blockIdx.x * 4;
  if (threadIdx.x == 0) { lc[2] = 0.f; lc[3] = 0.f; }
  if (noise_amax) noise_bound = fmaxf(noise_bound, cips3d_amax_load(noise_amax));
  layer_consts(bias, n_bias, noise_w, noise_bound, w_gain, fir, lc, threadIdx.x);
}

__global__ void __launch_bounds__(256) absmax_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ amax) {
  const int b = blockIdx.y;
  const float* xb = x + (int64_t)b * n;
  float m = 0.f;
  const int64_t n4 = (reinterpret_cast<uintptr_t>(xb) & 15) == 0 ? n / 4 : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(xb)[i];
    m = fmaxf(fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))), m);
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(xb[i]));
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) cips3d_amax_raise(amax + (int64_t)b * CIPS3D_AMAX_FLOATS, m, blockIdx.x * 4 + (threadIdx.x >> 6));
}

}  // namespace

extern "C" int cips3d_modulate_weights(const float* W, const float* s, int64_t s_stride, float* wm, int B, int Cout,
                                       int Cin, int ksq, float scale, int demodulate, void* stream) {
  if (!W || !s || !wm || B < 0 || Cout <= 0 || Cin <= 0 || ksq <= 0) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  // negative ksq is not used; the packed layout is selected with the high bit of `demodulate`
  const int packed = (demodulate & 2) ? (((demodulate & 4) ? 2 : 1) | (demodulate & 248)) : 0;   // bit 3: flipped taps, bit 4: split-fp16, bit 5: split16, bit 6: transposed, bit 7: bf16
  if ((packed & 32) && (ksq != 1 || (packed & 24))) return CIPS3D_E_UNSUPP;
  if ((packed & 64) && (ksq != 1 || (packed & 63) != 1)) return CIPS3D_E_UNSUPP;
  // every ksq == 1 fragment layout indexes 16-channel k-groups (Cin >> 4: plain, chained, split16, transposed); the 32-channel
  // blocks of the split and bf16 forms are checked below.  (Cin % 16 == 8 used to pass: channels 16 kq + 8 .. landed in the next
  // o-tile's block -- in bounds, scrambled)
  if (packed && ksq == 1 && (Cout % 32 != 0 || Cin % 16 != 0)) return CIPS3D_E_UNSUPP;
  if ((packed & 16) && ksq == 1 && ((packed & 7) != 1 || Cin % 32 != 0)) return CIPS3D_E_UNSUPP;
  if ((packed & 16) && ksq != 1 && (ksq != 9 || (packed & ~8) != 17)) return CIPS3D_E_UNSUPP;      // 3x3: PACKED | SPLIT [| FLIP] only
  if ((packed & 128) && (ksq != 1 || (packed & 127) != 1 || Cin % 32 != 0)) return CIPS3D_E_UNSUPP;
  if (packed && ksq != 1 && (ksq != 9 || (packed & 7) != 1 || Cout % 16 != 0 || Cin % 16 != 0)) return CIPS3D_E_UNSUPP;
  const int64_t rows = (int64_t)B * Cout;
  hipLaunchKernelGGL(modulate_kernel, dim3((unsigned)ceil_div<int64_t>(rows, 4)), dim3(256), 0, as_stream(stream), W,
                     s, s_stride, wm, B, Cout, Cin, ksq, scale, demodulate & 1, packed);
  return cips3d_launch_status();
}

extern "C" int cips3d_modulate_table(const cips3d_modulate_desc* table_dev, int n_desc, int total_rows, int B, float noise_bound,
                                     void* stream) {
  if (!table_dev || n_desc <= 0 || total_rows <= 0 || B < 0 || !(noise_bound >= 0.f)) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  hipLaunchKernelGGL(modulate_table_kernel, dim3((unsigned)ceil_div(total_rows, 4), (unsigned)B), dim3(256), 0,
                     as_stream(stream), table_dev, n_desc, total_rows, noise_bound);
  return cips3d_launch_status();
}

__global__ void __launch_bounds__(256) split_words_kernel(const float* __restrict__ x, float k, unsigned* __restrict__ words,
                                                          unsigned* __restrict__ pairs, int64_t n) {
  const float ku = cips3d_uniform(k);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n / 2; i += (int64_t)gridDim.x * 256) {
    words[2 * i] = cips3d_split_word(x[2 * i], ku);
    words[2 * i + 1] = cips3d_split_word(x[2 * i + 1] * k);
    cips3d_split_pair(x[2 * i], x[2 * i + 1], pairs[2 * i], pairs[2 * i + 1]);
  }
}

extern "C" int cips3d_split_words(const float* x, float k, uint32_t* words, uint32_t* pairs, int64_t n, void* stream) {
  if (!x || !words || !pairs || n <= 0 || (n & 1)) return CIPS3D_E_BADARG;
  int64_t blocks = ceil_div<int64_t>(n / 2, 256);
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(split_words_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, k, words, pairs, n);
  return cips3d_launch_status();
}

extern "C" int cips3d_amax_layout(int* slots, int* stride) {
  if (slots) *slots = CIPS3D_AMAX_SLOTS;
  if (stride) *stride = CIPS3D_AMAX_STRIDE;
  return 0;
}

extern "C" int cips3d_absmax(const float* x, int B, int64_t n, float* amax, void* stream) {
  if (!x || !amax || B < 0 || n <= 0) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  hipError_t e = hipMemsetAsync(amax, 0, sizeof(float) * CIPS3D_AMAX_FLOATS * (size_t)B, as_stream(stream));
  if (e != hipSuccess) return (int)e;
  int64_t blocks = ceil_div<int64_t>(n, 256 * 16);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, as_stream(stream), x, n, amax);
  return cips3d_launch_status();
}

extern "C" int cips3d_absmax_raise(const float* x, int B, int64_t n, float* amax, void* stream) {
  if (!x || !amax || B < 0 || n <= 0) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  int64_t blocks = ceil_div<int64_t>(n, 256 * 16);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(absmax_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, as_stream(stream), x, n, amax);
  return cips3d_launch_status();
}

extern "C" int cips3d_range_consts(const float* bias, int n_bias, const float* noise_w, float noise_bound, const float* noise_amax,
                                   float w_gain, const float* fir, float* lconst, int B, void* stream) {
  if (!lconst || B < 0 || n_bias < 0 || (n_bias > 0 && !bias) || !(noise_bound >= 0.f) || !(w_gain >= 0.f)) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  hipLaunchKernelGGL(range_consts_kernel, dim3((unsigned)B), dim3(64), 0, as_stream(stream), bias, n_bias, noise_w, noise_bound,
                     noise_amax, w_gain, fir, lconst);
  return cips3d_launch_status();
}
