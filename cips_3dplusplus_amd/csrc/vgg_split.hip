// The VGG16 conv perceptual loss on split-fp16 products (the `split_fp16` precision mode of perceptual.VGG16ConvLoss; the exact
// fp32 form and everything about the network is vgg.hip).  Convs 1 .. 12 and their data gradients run as implicit GEMMs on
// v_mfma_f32_16x16x32_f16: w x = w_lo x_hi + w_hi x_lo + w_hi x_hi, small terms first, fp32 accumulation -- 16 x the MACs per
// cycle of the fp32 matrix instruction for three products.  Conv 0, its data gradient, the pools, the tap loss and the tap
// gradient are the VALU kernels of vgg_shared.h, the same ones the exact form runs.
//
//   vgg_split_conv_kernel   K step = 32 input channels of one tap; a stage is 32 channels x 9 taps = 9 matrix steps per
//                        accumulator, a layer's chain at most 144 steps (K = 4608 / 32) in a fixed order.
//                        Two workgroup shapes, both 64 output channels and the same K order, so an output's bits do not
//                        depend on the choice: <WP = 4, MT = 4>: four waves on four row groups of a 16 x 16 pixel tile, a wave
//                        holding 64 channels x 4 rows x 16 columns (taken once it alone gives every CU a workgroup);
//                        <WP = 1, MT = 1>: four waves on 4 x 16 channels of a 4 x 16 pixel tile -- four times the workgroups
//                        for the deep, small maps (a 16^2 map of 512 channels is 16 workgroups of the first shape).
//                        After every stage the running accumulators are folded into a second set (as vgg.hip does).
//                        A = weights split ONCE at pack time: [Cout/16][Cin/32][tap][hi | lo][lane][8 fp16] of w 2^-ew, lane
//                        (q, i) holding w[16 ot + i][32 st + 8 q + j][tap] in element j -- one 16-byte load per fragment,
//                        straight from L2, one tap ahead (MT = 4) or a stage at a time in front of the fill (MT = 1).
//                        ew: one power of two per layer from max|w|, found on the device.
//                        B = the halo tile of the stage in LDS: the fill applies the producer's ReLU, scales by 2^-e, splits
//                        and writes hi / lo fp16 as [channel octet][tile pixel][8 channels], so that a lane's B fragment of any
//                        tap is one 16-byte read and the sixteen lanes of a quarter read 256 contiguous bytes.  Zero outside the
//                        image: any H, W >= 1 is correct.  <4, 4>: one buffer of 41 KB, two barriers per stage, two workgroups
//                        on a CU, one's fill under the other's matrix steps.  <1, 1>: two buffers of 14 KB, the next stage's
//                        loads in flight under this stage's matrix steps, one barrier per stage.
//                        Only fp32 pre-ReLU tensors cross HBM, as in the exact form.
//   range                one power of two per (tensor, sample): e with max|.| 2^-e in [2^14, 2^15) (cips3d_split_exp), undone
//                        exactly on the fp32 accumulators.  The maximum is on the device before the consumer launches: the conv
//                        epilogues raise a per-(tensor, sample) word with an integer atomicMax on the bits of |v| (order
//                        independent: same inputs, same bits); the tensors the VALU kernels produce (conv 0's output, the pool
//                        backward's, the deepest tap's gradient) are followed by vgg_absmax_kernel.  The words are zeroed by the
//                        call (cips3d_vgg_split_range_bytes).  Every scale follows the data's exponent, so inputs scaled by a
//                        power of two give outputs scaled by it bit for bit, and a sample's arithmetic does not depend on B.
//
// Roofline: three fp16 products per fp32 product on the 2.5 PFLOP/s fp16 matrix peak are 833 TFLOP/s of fp32-accurate work,
// against 157 TFLOP/s of the fp32 matrix instruction.  The kernels reach a fraction of it: a workgroup fills, waits and multiplies
// in turn, and the deep layers have few workgroups (DESIGN 9.5 has the measured times).
#include "vgg_shared.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef cips3d_h8 h8;

constexpr int SPLIT_BIG_TILE_MIN_WORKGROUPS = 256;      // the MI355X has 256 CUs

struct VggSplitConvArgs {
  const float* x; const u32x4* wp; const float* bias; float* out;
  const float* mask_z;             // data gradient: the kept pre-ReLU tensor of the layer below (shape of out) or NULL
  const float* tap_t; float tap_c; // ... its tap target and 2 w^2, or NULL
  const float* gloss;              // ... the loss' incoming gradient (device scalar)
  const unsigned* x_amax;          // [B] bits of a bound of max|x| of each sample
  const unsigned* w_amax;          // [1] bits of max|w| of the layer
  unsigned* out_amax;              // [B] raised with the bits of max|out| of each sample, or NULL
  int B, Cin, Cout, H, W, relu_in;
};

// acc * 2^e for e in [-254, 254], in two exact steps (each factor a normal power of two)
__device__ static inline float scale_pow2(float v, float s0, float s1) { return v * s0 * s1; }

template <int WP, int MT>
__global__ void __launch_bounds__(256, MT == 1 ? 3 : 2) vgg_split_conv_kernel(VggSplitConvArgs a) {
  constexpr int WMV = 4 / WP;                  // waves along the output channels, 16 MT each
  constexpr int TH = 4 * WP, TC = 18, TR = TH + 2;
  constexpr int NPIX = TR * TC;                // tile pixels
  constexpr int E = 4 * NPIX;                  // (octet, pixel) items of one stage, 16 bytes of hi and of lo each
  constexpr int NU = (E + 255) / 256;          // per thread
  constexpr bool FOLD = true;                  // fold the running accumulators into a second set after every stage
  constexpr bool STAGE_A = MT == 1;            // the small shape: a stage of weights at a time, two halo buffers
  __shared__ u32x4 sT[(STAGE_A ? 2 : 1) * 2 * E];      // [buffer][hi | lo][octet][pixel][8 fp16]

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int q = lane >> 4, jn = lane & 15;
  const int wp = wave % WP, wm = wave / WP;
  const int H = a.H, W = a.W, HW = H * W;
  const int tiles_x = (W + 15) / 16, tiles_y = (H + TH - 1) / TH;
  const int tpi = tiles_x * tiles_y;
  const int b = blockIdx.x / tpi, t_img = blockIdx.x % tpi;
  const int oy0 = (t_img / tiles_x) * TH, ox0 = (t_img % tiles_x) * 16;
  const int m0 = (blockIdx.y * WMV + wm) * (16 * MT);
  const int K = a.Cin, nstage = K >> 5;
  const float* xb = a.x + (int64_t)b * K * HW;
  const bool active = oy0 + wp * 4 < H;        // wave-uniform: a wave whose rows all lie below the image only helps staging

  // ---- the range of this sample's operand and of the layer's weights (wave-uniform scalars)
  const int ex = cips3d_split_exp(__uint_as_float(a.x_amax[b]));
  const int ew = cips3d_split_exp(__uint_as_float(a.w_amax[0]));
  const float x_scale = cips3d_pow2(-ex);
  const int et = ex + ew;
  const float s0 = cips3d_pow2(et >> 1), s1 = cips3d_pow2(et - (et >> 1));

  // ---- halo staging: item e = octet * NPIX + pixel; its source offset inside a 32-channel stage (-1: outside the image)
  int p_src[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int e = tid + 256 * u;
    const int oct = e / NPIX, pix = e % NPIX;
    const int t = pix / TC, m = pix % TC;
    const int iy = oy0 + t - 1, ix = ox0 + m - 1;
    const bool ok = e < E && iy >= 0 && iy < H && ix >= 0 && ix < W;
    p_src[u] = ok ? oct * 8 * HW + iy * W + ix : -1;
  }
  float raw[NU][8];
  auto fill_load = [&](int st) {               // all of a stage's loads in flight
    const float* src = xb + (int64_t)st * 32 * HW;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ps = p_src[u];
      // a scalar base per channel and one 32-bit byte offset per item, opaque to the optimiser: it otherwise keeps the 48
      // 64-bit addresses of a stage in registers through the matrix steps (96 VGPRs, spilled)
      unsigned off = (unsigned)(ps >= 0 ? ps : 0) * 4u;
      asm volatile("" : "+v"(off));
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const char* cj = reinterpret_cast<const char*>(src + (int64_t)j * HW);
        const float v = *reinterpret_cast<const float*>(cj + off);
        raw[u][j] = ps >= 0 ? v : 0.f;
      }
    }
  };
  auto fill_store = [&](u32x4* dst) {          // ReLU, scale, split, LDS
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int e = tid + 256 * u;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (a.relu_in ? fmaxf(raw[u][j], 0.f) : raw[u][j]) * x_scale;
      h8 hi, lo;
      cips3d_split8(v, hi, lo);
      if (e < E) {
        dst[e] = __builtin_bit_cast(u32x4, hi);
        dst[E + e] = __builtin_bit_cast(u32x4, lo);
      }
    }
  };

  // ---- A fragments [Cout/16][Cin/32][tap][hi | lo][64 lanes] of 16 bytes.  MT = 4: one tap ahead (a tap's 48 matrix steps and
  // the CU's other workgroup cover the load), one halo buffer, fill and matrix steps in turn.  MT = 1: a tap is 12 matrix steps,
  // which cover nothing, and the deep layers give a CU one workgroup -- so the stage's nine taps sit in 72 registers, each
  // re-requested for the next stage as soon as its tap has issued, and the next stage's halo loads fly under this stage's matrix
  // steps into the other buffer: one barrier per stage.
  u32x4 ah[MT], al[MT], ah_next[MT], al_next[MT];
  u32x4 sh[STAGE_A ? 9 : 1], sl[STAGE_A ? 9 : 1];
  const unsigned lane16 = lane * 16;
  auto a_load = [&](int st, int tap, u32x4 (&dh)[MT], u32x4 (&dl)[MT]) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      // (a wave-uniform base and a 32-bit lane offset: the scalar-base form of the load, no 64-bit address per fragment)
      const char* p = reinterpret_cast<const char*>(a.wp + (((int64_t)((m0 >> 4) + i) * nstage + st) * 9 + tap) * 128);
      dh[i] = *reinterpret_cast<const u32x4*>(p + lane16);
      dl[i] = *reinterpret_cast<const u32x4*>(p + lane16 + 1024);
    }
  };

  f32x4 acc[MT][4], tot[MT][4];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
      tot[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  auto stage_a_load = [&](int st, int tap) {
    const char* p = reinterpret_cast<const char*>(a.wp + (((int64_t)(m0 >> 4) * nstage + st) * 9 + tap) * 128);
    sh[tap] = *reinterpret_cast<const u32x4*>(p + lane16);
    sl[tap] = *reinterpret_cast<const u32x4*>(p + lane16 + 1024);
  };
  if constexpr (STAGE_A) {
    if (active) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) stage_a_load(0, tap);
    }
    fill_load(0);
    fill_store(sT);
    __syncthreads();
  } else {
    if (active) a_load(0, 0, ah_next, al_next);
  }
  const int frag0 = q * NPIX + (wp * 4) * TC + jn;

#pragma unroll 1
  for (int st = 0; st < nstage; ++st) {
    const bool more = st + 1 < nstage;
    if constexpr (STAGE_A) {
      if (more) fill_load(st + 1);
    } else {
      fill_load(st);
      fill_store(sT);
      __syncthreads();
    }
    const u32x4* cur = sT + (STAGE_A ? (st & 1) * 2 * E : 0) + frag0;
    if (active) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        if constexpr (STAGE_A) {
          ah[0] = sh[tap]; al[0] = sl[tap];
        } else {
#pragma unroll
          for (int i = 0; i < MT; ++i) { ah[i] = ah_next[i]; al[i] = al_next[i]; }
          if (tap < 8) a_load(st, tap + 1, ah_next, al_next);
          else if (more) a_load(st + 1, 0, ah_next, al_next);
        }
        h8 bh[4], bl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          bh[r] = __builtin_bit_cast(h8, cur[(r + ky) * TC + kx]);
          bl[r] = __builtin_bit_cast(h8, cur[E + (r + ky) * TC + kx]);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, al[i]), bh[r], acc[i][r], 0, 0, 0);
            acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ah[i]), bl[r], acc[i][r], 0, 0, 0);
            acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, ah[i]), bh[r], acc[i][r], 0, 0, 0);
          }
        if constexpr (STAGE_A) {
          if (more) stage_a_load(st + 1, tap);
        }
        __builtin_amdgcn_sched_barrier(0);     // a tap's reads stay with its products: hoisted, nine taps of fragments spill
      }
      if (FOLD) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tot[i][r] += acc[i][r];
            acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
    if constexpr (STAGE_A) {
      if (more) fill_store(sT + ((st + 1) & 1) * 2 * E);      // free since the barrier that ended stage st - 1
    }
    __syncthreads();
  }
  if (!active) return;

  // ---- epilogue.  D layout: acc[i][r][e] = out[o = m0 + 16 i + 4 q + e][oy0 + 4 wp + r][ox0 + jn]
  const int ox = ox0 + jn;
  const float gl = a.tap_t ? a.gloss[0] * a.tap_c : 0.f;
  const int64_t ob = (int64_t)b * a.Cout * HW;
  float vmax = 0.f;
  if (ox < W) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oy = oy0 + wp * 4 + r;
      if (oy >= H) continue;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = m0 + 16 * i + 4 * q + e;
          const int64_t idx = ob + (int64_t)o * HW + oy * W + ox;
          float v = scale_pow2(FOLD ? tot[i][r][e] : acc[i][r][e], s0, s1);
          if (a.bias) v += a.bias[o];
          if (a.mask_z) {
            const float z = a.mask_z[idx];
            v = z > 0.f ? v : 0.f;
            if (a.tap_t) v += gl * (z - a.tap_t[idx]);
          }
          a.out[idx] = v;
          vmax = fmaxf(vmax, fabsf(v));
        }
    }
  }
  if (a.out_amax) {
    vmax = cips3d_wave_max_uniform(vmax);
    if (lane == 0) atomicMax(a.out_amax + b, __float_as_uint(vmax));
  }
}

// word[b] = max(word[b], bits of max|x[b][:]|) for x [B][n]; grid (blocks, B).  Non-negative floats order like their bit
// patterns, so the integer maximum is the float one whatever the order of the atomics.
__global__ void __launch_bounds__(256) vgg_absmax_kernel(const float* __restrict__ x, int64_t n, unsigned* __restrict__ word) {
  const float* xb = x + (int64_t)blockIdx.y * n;
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(xb[i]));
  m = cips3d_wave_max_uniform(m);
  if ((threadIdx.x & 63) == 0) atomicMax(word + blockIdx.y, __float_as_uint(m));
}

// [Cout,Cin,3,3] -> both split operand forms, [M/16][K/32][tap][hi | lo][lane = 16 q + i][j] of W(m = 16 mt + i, k = 32 ks + 8 q
// + j, tap) 2^-ew: the forward form W = w[m][k][tap] (M = Cout, K = Cin) and the data-gradient form W = w[k][m][8 - tap]
// (M = Cin, K = Cout: transposed, rotated 180 degrees).  One thread per weight of each form.
__global__ void __launch_bounds__(256) vgg_split_pack_kernel(const float* __restrict__ w, const unsigned* __restrict__ w_amax,
                                                             _Float16* __restrict__ fwd, _Float16* __restrict__ bwd, int Cout,
                                                             int Cin) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9 * Cout * Cin) return;
  const float scale = cips3d_pow2(-cips3d_split_exp(__uint_as_float(w_amax[0])));
  const int j = idx & 7, lane = (idx >> 3) & 63, rest = idx >> 9;
  const int i = lane & 15, q = lane >> 4;
  const int tap = rest % 9, blk = rest / 9;           // blk = mt * (K / 32) + ks
  const int64_t dst = ((int64_t)rest * 2) * 512 + lane * 8 + j;
  {
    const int ks = blk % (Cin >> 5), mt = blk / (Cin >> 5);
    const int o = mt * 16 + i, c = ks * 32 + 8 * q + j;
    _Float16 hi, lo;
    cips3d_split16(w[((int64_t)o * Cin + c) * 9 + tap] * scale, hi, lo);
    fwd[dst] = hi;
    fwd[dst + 512] = lo;
  }
  {
    const int ks = blk % (Cout >> 5), mt = blk / (Cout >> 5);
    const int o = ks * 32 + 8 * q + j, c = mt * 16 + i;
    _Float16 hi, lo;
    cips3d_split16(w[((int64_t)o * Cin + c) * 9 + (8 - tap)] * scale, hi, lo);
    bwd[dst] = hi;
    bwd[dst + 512] = lo;
  }
}

// Both shapes give a workgroup 64 output channels and walk K in the same order, so an output's bits do not depend on the choice.
// The 16 x 16 tile reuses every fragment four times as often; it is taken once it alone gives every CU a workgroup.
int launch_conv(const VggSplitConvArgs& a, hipStream_t s) {
  const int64_t big = (int64_t)a.B * ceil_div(a.H, 16) * ceil_div(a.W, 16) * (a.Cout / 64);
  if (big >= SPLIT_BIG_TILE_MIN_WORKGROUPS) {
    dim3 grid(a.B * ceil_div(a.H, 16) * ceil_div(a.W, 16), a.Cout / 64);
    hipLaunchKernelGGL((vgg_split_conv_kernel<4, 4>), grid, dim3(256), 0, s, a);
  } else {
    dim3 grid(a.B * ceil_div(a.H, 4) * ceil_div(a.W, 16), a.Cout / 64);
    hipLaunchKernelGGL((vgg_split_conv_kernel<1, 1>), grid, dim3(256), 0, s, a);
  }
  return cips3d_launch_status();
}

int launch_absmax(const float* x, int B, int64_t n, unsigned* word, hipStream_t s) {
  const int64_t nb = ceil_div<int64_t>(n, 2048);
  hipLaunchKernelGGL(vgg_absmax_kernel, dim3((unsigned)(nb < 256 ? nb : 256), B), dim3(256), 0, s, x, n, word);
  return cips3d_launch_status();
}

// range words: [2][NCONV][B]: the maxima of the pre-ReLU tensors z_l, then of their gradients
inline unsigned* z_word(const cips3d_vgg_split_io* io, int l) { return static_cast<unsigned*>(io->range) + (int64_t)l * io->io.B; }
inline unsigned* g_word(const cips3d_vgg_split_io* io, int l) {
  return static_cast<unsigned*>(io->range) + (int64_t)(NCONV + l) * io->io.B;
}

int check_ctx_io(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* sio) {
  if (!ctx || !sio || !sio->io.x) return CIPS3D_E_BADARG;
  const cips3d_vgg_io* io = &sio->io;
  if (io->n_convs < 1 || io->n_convs > NCONV) return CIPS3D_E_BADARG;
  const int rc = cips3d_vgg_split_supported(io->B, io->H, io->W);
  if (rc != 0) return rc;
  if (!sio->range || !ctx->w_amax) return CIPS3D_E_BADARG;
  int pool = 0;
  for (int l = 0; l < io->n_convs; ++l) {
    if (!ctx->w_fwd[l] || !ctx->bias[l] || !io->z[l]) return CIPS3D_E_BADARG;
    if (kPoolBefore[l] && !io->pooled[pool++]) return CIPS3D_E_BADARG;
  }
  return 0;
}

int zero_range(const cips3d_vgg_split_io* sio, int first, hipStream_t s) {      // first = 0: the z words, 1: the gradient words
  const size_t half = (size_t)NCONV * sio->io.B * sizeof(unsigned);
  const hipError_t e = hipMemsetAsync(static_cast<char*>(sio->range) + first * half, 0, half, s);
  return e == hipSuccess ? 0 : (int)e;
}

int run_features(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* sio, hipStream_t s) {
  const cips3d_vgg_io* io = &sio->io;
  const int B = io->B;
  int H = io->H, W = io->W, pool = 0;
  int rc = zero_range(sio, 0, s);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(vgg_first_fwd_kernel, dim3(blocks_of((int64_t)B * H * W)), dim3(256), 0, s, io->x,
                     static_cast<const float*>(ctx->w_fwd[0]), ctx->bias[0], io->z[0], B, H, W, io->normalize);
  if ((rc = cips3d_launch_status()) != 0) return rc;
  if (io->n_convs > 1) rc = launch_absmax(io->z[0], B, (int64_t)64 * H * W, z_word(sio, 0), s);
  for (int l = 1; l < io->n_convs && rc == 0; ++l) {
    const float* in = io->z[l - 1];
    int relu_in = 1;
    if (kPoolBefore[l]) {
      H /= 2; W /= 2;
      const int64_t total = (int64_t)B * kChan[l - 1] * H * W;
      hipLaunchKernelGGL(vgg_pool_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, s, in, io->pooled[pool], total, H, W);
      if ((rc = cips3d_launch_status()) != 0) break;
      in = io->pooled[pool++];
      relu_in = 0;
    }
    // (the pooled tensor's maximum is at most max|z_{l-1}|: one word serves both)
    VggSplitConvArgs a = {in, static_cast<const u32x4*>(ctx->w_fwd[l]), ctx->bias[l], io->z[l], nullptr, nullptr, 0.f, nullptr,
                          z_word(sio, l - 1), ctx->w_amax + l, l + 1 < io->n_convs ? z_word(sio, l) : nullptr,
                          B, kChan[l - 1], kChan[l], H, W, relu_in};
    rc = launch_conv(a, s);
  }
  return rc;
}

}  // namespace

extern "C" int cips3d_vgg_split_supported(int B, int H, int W) { return cips3d_vgg_supported(B, H, W); }

extern "C" int64_t cips3d_vgg_split_range_bytes(int B) {
  return B < 1 ? (int64_t)CIPS3D_E_BADARG : (int64_t)2 * NCONV * B * (int64_t)sizeof(unsigned);
}

extern "C" int cips3d_vgg_split_pack(const cips3d_vgg_split_ctx* ctx, const float* const* weights, int n_convs, void* stream) {
  if (!ctx || !weights || n_convs < 1 || n_convs > NCONV) return CIPS3D_E_BADARG;
  if (!ctx->w_amax) return CIPS3D_E_BADARG;
  for (int l = 0; l < n_convs; ++l)
    if (!weights[l] || !ctx->w_fwd[l] || (l > 0 && !ctx->w_bwd[l])) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemcpyAsync(ctx->w_fwd[0], weights[0], 64 * 27 * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(ctx->w_amax, 0, NCONV * sizeof(unsigned), s)) != hipSuccess) return (int)e;
  for (int l = 1; l < n_convs; ++l) {
    const int n = 9 * kChan[l] * kChan[l - 1];
    int rc = launch_absmax(weights[l], 1, n, ctx->w_amax + l, s);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(vgg_split_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, s, weights[l], ctx->w_amax + l,
                       static_cast<_Float16*>(ctx->w_fwd[l]), static_cast<_Float16*>(ctx->w_bwd[l]), kChan[l], kChan[l - 1]);
    if ((rc = cips3d_launch_status()) != 0) return rc;
  }
  return 0;
}

extern "C" int cips3d_vgg_split_features(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* io, void* stream) {
  const int rc = check_ctx_io(ctx, io);
  if (rc != 0) return rc;
  return run_features(ctx, io, as_stream(stream));
}

extern "C" int cips3d_vgg_split_loss_forward(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* sio, void* stream) {
  int rc = check_ctx_io(ctx, sio);
  if (rc != 0) return rc;
  const cips3d_vgg_io* io = &sio->io;
  if (!io->partial || !io->loss || !io->target[io->n_convs - 1]) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  if ((rc = run_features(ctx, sio, s)) != 0) return rc;
  return launch_tap_loss(io, s);
}

extern "C" int cips3d_vgg_split_loss_backward(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* sio, void* stream) {
  int rc = check_ctx_io(ctx, sio);
  if (rc != 0) return rc;
  const cips3d_vgg_io* io = &sio->io;
  const int L = io->n_convs - 1;
  if (!io->gloss || !io->dx || !io->target[L] || !io->g[0] || (L > 0 && !io->g[1])) return CIPS3D_E_BADARG;
  for (int l = 1; l <= L; ++l)
    if (!ctx->w_bwd[l]) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  const int B = io->B;
  int Hs[NCONV], Ws[NCONV];
  for (int l = 0, H = io->H, W = io->W; l <= L; ++l) {
    if (kPoolBefore[l]) { H /= 2; W /= 2; }
    Hs[l] = H; Ws[l] = W;
  }
  auto tap_c = [&](int l) { return 2.f * io->tap_w[l] * io->tap_w[l]; };
  if ((rc = zero_range(sio, 1, s)) != 0) return rc;
  float* cur = io->g[0];
  float* other = io->g[1];
  {   // the deepest tap starts the chain
    const int64_t n = (int64_t)B * kChan[L] * Hs[L] * Ws[L];
    hipLaunchKernelGGL(vgg_tap_grad_kernel, dim3(blocks_of(n)), dim3(256), 0, s, io->z[L], io->target[L], tap_c(L), io->gloss, cur,
                       n);
    if ((rc = cips3d_launch_status()) != 0) return rc;
    if (L > 0 && (rc = launch_absmax(cur, B, n / B, g_word(sio, L), s)) != 0) return rc;
  }
  for (int l = L; l >= 1; --l) {
    // cur = d loss / d z_l  ->  d loss / d z_{l-1}; its maximum goes to g_word(l - 1) when another data gradient reads it
    const float* t = io->target[l - 1];
    unsigned* next_word = l > 1 ? g_word(sio, l - 1) : nullptr;
    const u32x4* wb = static_cast<const u32x4*>(ctx->w_bwd[l]);
    if (!kPoolBefore[l]) {
      VggSplitConvArgs a = {cur, wb, nullptr, other, io->z[l - 1], t, t ? tap_c(l - 1) : 0.f, io->gloss, g_word(sio, l),
                            ctx->w_amax + l, next_word, B, kChan[l], kChan[l - 1], Hs[l], Ws[l], 0};
      if ((rc = launch_conv(a, s)) != 0) return rc;
      float* tmp = cur; cur = other; other = tmp;
    } else {
      VggSplitConvArgs a = {cur, wb, nullptr, other, nullptr, nullptr, 0.f, nullptr, g_word(sio, l), ctx->w_amax + l, nullptr,
                            B, kChan[l], kChan[l - 1], Hs[l], Ws[l], 0};
      if ((rc = launch_conv(a, s)) != 0) return rc;
      const int64_t total = (int64_t)B * kChan[l - 1] * Hs[l] * Ws[l];
      hipLaunchKernelGGL(vgg_pool_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, s, other, io->z[l - 1], t,
                         t ? tap_c(l - 1) : 0.f, io->gloss, cur, total, Hs[l], Ws[l]);
      if ((rc = cips3d_launch_status()) != 0) return rc;
      if (next_word && (rc = launch_absmax(cur, B, (int64_t)kChan[l - 1] * Hs[l - 1] * Ws[l - 1], next_word, s)) != 0) return rc;
    }
  }
  hipLaunchKernelGGL(vgg_first_bwd_kernel, dim3(blocks_of((int64_t)B * io->H * io->W)), dim3(256), 0, s, cur,
                     static_cast<const float*>(ctx->w_fwd[0]), io->dx, B, io->H, io->W, io->normalize);
  return cips3d_launch_status();
}
