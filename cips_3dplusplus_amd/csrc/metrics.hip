// PSNR and SSIM of an image pair on the device: what the reference's `project_wplus` logs through tl2's sk_psnr / sk_ssim
// (/root/reference/exp/cips3d/models/projector_v10.py:1125-1139, 1266-1279), i.e. scikit-image's peak_signal_noise_ratio and
// structural_similarity at their defaults on 8-bit images (data range R = 255, win_size 7, uniform window, K1 = 0.01,
// K2 = 0.03, sample covariance), without the copy to the host.
//
// After the quantisation to 8 bits (cips3d_rgb_to_uint8's arithmetic, done here on load for an fp32 operand) both metrics are
// integer statistics: the squared error is an exact integer, and the five moment sums of a 7 x 7 window -- S_x, S_y, S_xx, S_yy,
// S_xy -- are exact 32-bit integers.  With n = 49 and the window's SSIM multiplied through by n^2 and n (n - 1):
//     S = (2 S_x S_y + n^2 C1) (2 (n S_xy - S_x S_y) + n (n - 1) C2)
//         / ((S_x^2 + S_y^2 + n^2 C1) ((n S_xx - S_x^2) + (n S_yy - S_y^2) + n (n - 1) C2)),   C1 = (K1 R)^2, C2 = (K2 R)^2.
// Every product of sums fits int32 (n S_xy <= 49 * 49 * 255^2 < 2^28).  The integer parts of n^2 C1 = 15612.5025 and
// n (n - 1) C2 = 137644.92 are added as integers, so a factor is: one conversion to fp32 (exact for the first pair, which stays
// below 2^24), one addition of the constant's fraction; then two products and one division: 9 roundings per window, every
// factor of the denominator >= its constant, |S| <= 1.  Equal images give numerator == denominator bit for bit: exactly 1.
//
// metrics_tile_kernel   one workgroup per (image, channel, tile of TH x TW window origins).  It loads the (TH + 6) x (TW + 6)
//                       pixels of both images into LDS as bytes (adding up its own pixels' squared differences on the way),
//                       forms the row sums of 7 per (row, origin column) -- {S_x | S_y << 16, S_xx, S_yy, S_xy} as one 16-byte
//                       LDS word -- then each thread adds 7 rows of them for RPT consecutive origins of one column, evaluates
//                       the windows in fp32 and adds them in a fixed order: RPT values in the thread, the 6-stage butterfly of
//                       the wave, the four waves as (w0 + w1) + (w2 + w3).  One {SSE: uint64, SSIM sum: fp32} partial per
//                       workgroup; no atomics of any kind.
// metrics_finish_kernel one workgroup per image: its partials in a fixed order (SSE in uint64, SSIM in fp64), the mean over
//                       windows and channels, and {SSE: int64, SSIM: float64} into row `row + image` of the caller's record.
// An image's result depends on its own partials only: it is the same to the bit whatever batch it sits in, and run to run.
#include "common.h"

namespace {

constexpr int MT_TH = 32, MT_TW = 64;              // window origins per tile
constexpr int MT_THREADS = 256;
constexpr int MT_WIN = 7, MT_HALO = MT_WIN - 1;
constexpr int MT_ROWS = MT_TH + MT_HALO;           // pixel rows of a tile
constexpr int MT_COLS = MT_TW + MT_HALO;           // pixel columns of a tile
constexpr int MT_WORDS = (MT_COLS + 3) / 4;        // LDS words per pixel row
constexpr int MT_RPT = MT_TH * MT_TW / MT_THREADS; // window origins (consecutive rows of one column) per thread
static_assert(MT_TW == 64 && MT_THREADS == 4 * 64 && MT_TH % 4 == 0, "a wave is one strip of MT_RPT origin rows x 64 columns");
static_assert(4 * MT_WORDS >= MT_TW + 8, "the row-sum pass reads three words from the word of its first pixel");
static_assert((int64_t)MT_ROWS * MT_COLS * 255 * 255 < ((int64_t)1 << 32), "a tile's squared error fits uint32");

struct MtPartial { unsigned long long sse; float ssim; unsigned pad_; };   // 16 bytes per (image, channel, tile)

__device__ static inline unsigned mt_quant(float v) { return cips3d_quant_u8(v); }       // cips3d_rgb_to_uint8's arithmetic (common.h)
template <bool U8>
__device__ static inline unsigned mt_load(const void* __restrict__ img, int64_t i) {
  if (U8) return static_cast<const uint8_t*>(img)[i];
  return mt_quant(static_cast<const float*>(img)[i]);
}
__device__ static inline unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
  return v;
}
// sum over the 7 bytes of {q0, low three bytes of q1} of the products with the same bytes of {r0, r1}
__device__ static inline unsigned mt_dot7(unsigned q0, unsigned q1, unsigned r0, unsigned r1) {
  unsigned s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += ((q0 >> (8 * j)) & 0xffu) * ((r0 >> (8 * j)) & 0xffu);
#pragma unroll
  for (int j = 0; j < 3; ++j) s += ((q1 >> (8 * j)) & 0xffu) * ((r1 >> (8 * j)) & 0xffu);
  return s;
}

template <bool A_U8, bool B_U8>
__global__ void __launch_bounds__(MT_THREADS) metrics_tile_kernel(const void* __restrict__ a, const void* __restrict__ b, int C,
                                                                  int H, int W, int tiles_x, int tiles_y,
                                                                  MtPartial* __restrict__ partial) {
  __shared__ unsigned pa[MT_ROWS][MT_WORDS], pb[MT_ROWS][MT_WORDS];
  __shared__ uint4 rs[MT_ROWS][MT_TW];
  __shared__ float red_f[4];
  __shared__ unsigned red_u[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int plane = (int)blockIdx.x / tiles, t = (int)blockIdx.x % tiles;       // plane = image * C + channel
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int y0 = ty * MT_TH, x0 = tx * MT_TW;
  const int64_t base = (int64_t)plane * H * W;
  // the pixels this tile owns for the squared error: its TH x TW block, and the halo too where no further tile follows
  const int own_rows = ty == tiles_y - 1 ? MT_ROWS : MT_TH, own_cols = tx == tiles_x - 1 ? MT_COLS : MT_TW;

  unsigned sse = 0;
  for (int it = tid; it < MT_ROWS * MT_WORDS; it += MT_THREADS) {
    const int r = it / MT_WORDS, g = it % MT_WORDS, gy = y0 + r;
    unsigned wa = 0, wb = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int lx = 4 * g + k, gx = x0 + lx;
      if (gy < H && gx < W && lx < MT_COLS) {
        const int64_t i = base + (int64_t)gy * W + gx;
        const unsigned va = mt_load<A_U8>(a, i), vb = mt_load<B_U8>(b, i);
        wa |= va << (8 * k);
        wb |= vb << (8 * k);
        if (r < own_rows && lx < own_cols) {
          const int d = (int)va - (int)vb;
          sse += (unsigned)(d * d);
        }
      }
    }
    pa[r][g] = wa;
    pb[r][g] = wb;
  }
  __syncthreads();

  // row sums of 7: lane = origin column, so the 16-byte stores of a wave are consecutive
  for (int it = tid; it < MT_ROWS * MT_TW; it += MT_THREADS) {
    const int r = it / MT_TW, x = it % MT_TW, g = x >> 2, sh = x & 3;
    const unsigned a0 = __builtin_amdgcn_alignbyte(pa[r][g + 1], pa[r][g], sh);
    const unsigned a1 = __builtin_amdgcn_alignbyte(pa[r][g + 2], pa[r][g + 1], sh);
    const unsigned b0 = __builtin_amdgcn_alignbyte(pb[r][g + 1], pb[r][g], sh);
    const unsigned b1 = __builtin_amdgcn_alignbyte(pb[r][g + 2], pb[r][g + 1], sh);
    const unsigned ones = 0x01010101u;
    rs[r][x] = make_uint4(mt_dot7(a0, a1, ones, ones) | (mt_dot7(b0, b1, ones, ones) << 16), mt_dot7(a0, a1, a0, a1),
                          mt_dot7(b0, b1, b0, b1), mt_dot7(a0, a1, b0, b1));
  }
  __syncthreads();

  // column sums of 7 for the RPT origins (rows wave * RPT ..) of column `lane`, the windows in fp32
  const int ox = x0 + lane, oy0 = y0 + wave * MT_RPT;
  unsigned sa = 0, sb = 0, sxx = 0, syy = 0, sxy = 0;
  uint4 e[MT_RPT + MT_HALO];
#pragma unroll
  for (int i = 0; i < MT_RPT + MT_HALO; ++i) e[i] = rs[wave * MT_RPT + i][lane];
#pragma unroll
  for (int i = 0; i < MT_HALO; ++i) { sa += e[i].x & 0xffffu; sb += e[i].x >> 16; sxx += e[i].y; syy += e[i].z; sxy += e[i].w; }
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < MT_RPT; ++k) {
    const uint4 in = e[k + MT_HALO];
    sa += in.x & 0xffffu; sb += in.x >> 16; sxx += in.y; syy += in.z; sxy += in.w;
    if (ox <= W - MT_WIN && oy0 + k <= H - MT_WIN) {
      const int n = MT_WIN * MT_WIN;
      const int p = (int)(sa * sb), qa = (int)(sa * sa), qb = (int)(sb * sb);
      const int cov = n * (int)sxy - p, vx = n * (int)sxx - qa, vy = n * (int)syy - qb;
      const float a1 = (float)(2 * p + 15612) + 0.5025f, d1 = (float)(qa + qb + 15612) + 0.5025f;      // n^2 C1 = 15612.5025
      const float a2 = (float)(2 * cov + 137644) + 0.92f, d2 = (float)(vx + vy + 137644) + 0.92f;      // n (n - 1) C2 = 137644.92
      acc += (a1 * a2) / (d1 * d2);
    }
    const uint4 out = e[k];
    sa -= out.x & 0xffffu; sb -= out.x >> 16; sxx -= out.y; syy -= out.z; sxy -= out.w;
  }
  acc = wave_sum(acc);
  sse = wave_sum_u32(sse);
  if (lane == 0) { red_f[wave] = acc; red_u[wave] = sse; }
  __syncthreads();
  if (tid == 0) {
    MtPartial out;
    out.sse = (unsigned long long)((red_u[0] + red_u[1]) + (red_u[2] + red_u[3]));
    out.ssim = (red_f[0] + red_f[1]) + (red_f[2] + red_f[3]);
    out.pad_ = 0;
    partial[blockIdx.x] = out;
  }
}

__global__ void __launch_bounds__(MT_THREADS) metrics_finish_kernel(const MtPartial* __restrict__ partial, int per_image,
                                                                    double windows, long long* __restrict__ record, int64_t row) {
  __shared__ double sd[MT_THREADS];
  __shared__ unsigned long long se[MT_THREADS];
  const int tid = threadIdx.x;
  const MtPartial* p = partial + (int64_t)blockIdx.x * per_image;
  double s = 0.0;
  unsigned long long q = 0;
  for (int i = tid; i < per_image; i += MT_THREADS) { s += (double)p[i].ssim; q += p[i].sse; }
  sd[tid] = s;
  se[tid] = q;
  __syncthreads();
  for (int off = MT_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) { sd[tid] += sd[tid + off]; se[tid] += se[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    long long* out = record + 2 * (row + (int64_t)blockIdx.x);
    out[0] = (long long)se[0];
    out[1] = __double_as_longlong(sd[0] / windows);
  }
}

struct MtShape { int tiles_x, tiles_y; int64_t blocks; };
static bool mt_shape(int B, int C, int H, int W, MtShape* s) {
  if (B < 1 || C < 1 || H < MT_WIN || W < MT_WIN) return false;
  s->tiles_x = ceil_div(W - MT_HALO, MT_TW);
  s->tiles_y = ceil_div(H - MT_HALO, MT_TH);
  s->blocks = (int64_t)B * C * s->tiles_x * s->tiles_y;
  return s->blocks <= 0x7fffffff && (int64_t)C * s->tiles_x * s->tiles_y <= 0x7fffffff;
}

template <bool A_U8, bool B_U8>
static void mt_launch(const void* a, const void* b, int C, int H, int W, const MtShape& s, MtPartial* partial, hipStream_t st) {
  hipLaunchKernelGGL((metrics_tile_kernel<A_U8, B_U8>), dim3((unsigned)s.blocks), dim3(MT_THREADS), 0, st, a, b, C, H, W,
                     s.tiles_x, s.tiles_y, partial);
}

}  // namespace

extern "C" int cips3d_image_metrics_tile(int* tile_h, int* tile_w) {
  if (tile_h) *tile_h = MT_TH;
  if (tile_w) *tile_w = MT_TW;
  return MT_THREADS;
}

extern "C" int64_t cips3d_image_metrics_workspace_bytes(int B, int C, int H, int W) {
  MtShape s;
  if (!mt_shape(B, C, H, W, &s)) return CIPS3D_E_BADARG;
  return s.blocks * (int64_t)sizeof(MtPartial);
}

extern "C" int cips3d_image_metrics(const void* a, int a_is_u8, const void* b, int b_is_u8, int B, int C, int H, int W,
                                    void* workspace, void* record, int64_t row, void* stream) {
  MtShape s;
  if (!a || !b || !workspace || !record || row < 0 || !mt_shape(B, C, H, W, &s)) return CIPS3D_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(record) & 7)) return CIPS3D_E_UNSUPP;
  if ((!a_is_u8 && (reinterpret_cast<uintptr_t>(a) & 3)) || (!b_is_u8 && (reinterpret_cast<uintptr_t>(b) & 3))) return CIPS3D_E_UNSUPP;
  MtPartial* partial = static_cast<MtPartial*>(workspace);
  hipStream_t st = as_stream(stream);
  if (a_is_u8) {
    if (b_is_u8) mt_launch<true, true>(a, b, C, H, W, s, partial, st);
    else mt_launch<true, false>(a, b, C, H, W, s, partial, st);
  } else {
    if (b_is_u8) mt_launch<false, true>(a, b, C, H, W, s, partial, st);
    else mt_launch<false, false>(a, b, C, H, W, s, partial, st);
  }
  const int per_image = C * s.tiles_x * s.tiles_y;
  const double windows = (double)C * (double)(H - MT_HALO) * (double)(W - MT_HALO);
  hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)B), dim3(MT_THREADS), 0, st, partial, per_image, windows,
                     static_cast<long long*>(record), row);
  return cips3d_launch_status();
}
