// Gaussian-window SSIM of fp32 image pairs as a differentiable loss (Wang et al. 2004; scikit-image's structural_similarity with
// gaussian_weights = True, sigma = 1.5, use_sample_covariance = False): the structural term of flip inversion,
//     loss = weight * mean_i (1 - ssim_i),   ssim_i = the mean of S over the C (H - 10) (W - 10) windows inside image i,
//     S = (2 mux muy + C1) (2 vxy + C2) / ((mux^2 + muy^2 + C1) (vx + vy + C2)),   C1 = (0.01 R)^2, C2 = (0.03 R)^2,
// with the moments taken under the separable 11-tap window g (x) g, g[i] ~ exp(-(i - 5)^2 / 4.5), sum g = 1.  Images are
// continuous fp32 values: nothing is quantised or clamped (csrc/metrics.hip is the 8-bit, uniform-window metric).
//
// Shifted moments.  vx = E[x^2] - mux^2 cancels: on a bright flat region (x ~ 1, vx ~ 1e-5) fp32 loses five digits.  Variances
// and the covariance do not change when a constant is subtracted, so every workgroup takes the moments of x - cx, y - cy with
// cx, cy = the first pixel of ITS tile in each image (pixel (tile_y TH, tile_x TW) of the plane: always inside the image); only
// the means add the constant back.  A flat image then has vx = vy = vxy = 0 exactly, whatever its level.
//
// ssim_tile_kernel    one workgroup per (image, channel, tile of TH x TW window origins).  The (TH + 10) x (TW + 10) pixels of
//                     both images go to LDS as fp32, shifted; the row pass writes the five moment planes {x, y, xx, yy, xy} per
//                     (pixel row, origin column) to LDS; the column pass keeps RPT consecutive origins of one column per thread
//                     in registers.  Both passes are chains of 11 fmas in tap order.  A window is then
//                         vx = fma(-ma, ma, maa), ...;  mux = ma + cx;  A1 = 2 (mux muy) + C1;  B1 = (mux mux + muy muy) + C1;
//                         A2 = 2 vxy + C2;  B2 = (vx + vy) + C2;  S = (A1 A2) / (B1 B2)
//                     (equal images: numerator == denominator bit for bit, S == 1).  The windows are added in a fixed order: RPT
//                     values in the thread, the 6-stage butterfly of the wave, the four waves as (w0 + w1) + (w2 + w3); one
//                     fp32 partial per workgroup.  When a gradient is wanted the kernel also stores, per window, the three
//                     derivative maps the backward needs (below); an optional pointer receives S itself.
// ssim_finish_kernel  one workgroup: per image its partials in fp64 in a fixed order -> ssim[i] (fp64), then the loss (fp32).
//                     ssim[i] depends on image i's partials only: the same bits in any batch.
// ssim_bwd_kernel     one workgroup per (image, channel, tile of TH x TW PIXELS): the transposed ("full") Gaussian convolution
//                     of the three maps, zero outside the valid origins, by the same two passes, then
//                         da(p) = coef gloss[0] (T1(p) + 2 (a(p) - kx) T2(p) + (b(p) - ky) T3(p)).
// No atomics of any kind; value, map and gradient are bit-identical run to run.
//
// The derivative maps.  With Smu, Svx, Svxy the partial derivatives of S with respect to mux, vx and vxy,
//     dS/da(p) = g(p - w) (Smu + 2 (a(p) - mux) Svx + (b(p) - muy) Svxy)            for every window w that holds p.
// a(p) - mux cancels like the variance does, so the maps are stored for the plane's constants kx, ky = the first pixel of the
// plane (image, channel) in a and b:
//     D1 = Smu - 2 (mux - kx) Svx - (muy - ky) Svxy,   D2 = Svx = -S / B2,   D3 = Svxy = 2 A1 / (B1 B2),
//     Smu = (2 / B1) (muy A2 / B2 - mux S),           mux - kx = ma + (cx - kx)
// -- "dS/dmux" with E[x^2] and E[xy] held fixed, for the shifted image a - kx.  Any constant gives the same sum in exact
// arithmetic.
#include <math.h>

#include "common.h"

namespace {

constexpr int SL_TH = 16, SL_TW = 64;              // window origins (forward) / pixels (backward) per tile
constexpr int SL_THREADS = 256;
constexpr int SL_WIN = 11, SL_HALO = SL_WIN - 1;
constexpr int SL_ROWS = SL_TH + SL_HALO;           // staged rows of a tile
constexpr int SL_COLS = SL_TW + SL_HALO;           // staged columns of a tile
constexpr int SL_LD = SL_COLS + 1;                 // odd leading dimension of the staged planes
constexpr int SL_RPT = SL_TH * SL_TW / SL_THREADS; // consecutive rows of one column per thread
static_assert(SL_TW == 64 && SL_THREADS == 4 * 64 && SL_TH % 4 == 0, "a wave is one strip of SL_RPT rows x 64 columns");
static_assert((2 * SL_ROWS * SL_LD + 5 * SL_ROWS * SL_TW + 4) * 4 < 56 * 1024, "two workgroups and more per CU");

struct SlWin { float g[SL_WIN]; };

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, in double, rounded once; symmetric by construction
static SlWin sl_window() {
  double e[SL_HALO / 2 + 1], s = 0.0;
  for (int d = 0; d <= SL_HALO / 2; ++d) {
    e[d] = exp(-(double)(d * d) / (2.0 * 1.5 * 1.5));
    s += d == 0 ? e[d] : 2.0 * e[d];
  }
  SlWin w;
  for (int d = 0; d <= SL_HALO / 2; ++d) w.g[SL_HALO / 2 - d] = w.g[SL_HALO / 2 + d] = (float)(e[d] / s);
  return w;
}

// out[k] = sum_j g[j] col[k + j] for k < SL_RPT: 11 fmas per output, in tap order
__device__ static inline void sl_column(const float* __restrict__ plane, int row0, int lane, const SlWin& win, float (&out)[SL_RPT]) {
  float e[SL_RPT + SL_HALO];
#pragma unroll
  for (int i = 0; i < SL_RPT + SL_HALO; ++i) e[i] = plane[(row0 + i) * SL_TW + lane];
#pragma unroll
  for (int k = 0; k < SL_RPT; ++k) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < SL_WIN; ++j) s = fmaf(win.g[j], e[k + j], s);
    out[k] = s;
  }
}

__global__ void __launch_bounds__(SL_THREADS) ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                               int tiles_x, int tiles_y, SlWin win, float c1, float c2,
                                                               float* __restrict__ partial, float* __restrict__ d1,
                                                               float* __restrict__ d2, float* __restrict__ d3,
                                                               float* __restrict__ map) {
  __shared__ float pa[SL_ROWS * SL_LD], pb[SL_ROWS * SL_LD];
  __shared__ float rs[5][SL_ROWS * SL_TW];
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int plane = (int)blockIdx.x / tiles, t = (int)blockIdx.x % tiles;       // plane = image * C + channel
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int y0 = ty * SL_TH, x0 = tx * SL_TW;                                   // (y0 <= H - 11, x0 <= W - 11: a pixel of the image)
  const int64_t base = (int64_t)plane * H * W;
  const float ka = a[base], kb = b[base];
  const float ca = a[base + (int64_t)y0 * W + x0], cb = b[base + (int64_t)y0 * W + x0];

  for (int it = tid; it < SL_ROWS * SL_COLS; it += SL_THREADS) {
    const int r = it / SL_COLS, c = it % SL_COLS, gy = y0 + r, gx = x0 + c;
    float va = 0.f, vb = 0.f;
    if (gy < H && gx < W) {
      const int64_t i = base + (int64_t)gy * W + gx;
      va = a[i] - ca;
      vb = b[i] - cb;
    }
    pa[r * SL_LD + c] = va;
    pb[r * SL_LD + c] = vb;
  }
  __syncthreads();

  // row pass: lane = origin column, so a wave's LDS reads and writes are consecutive words
  for (int it = tid; it < SL_ROWS * SL_TW; it += SL_THREADS) {
    const int r = it / SL_TW, x = it % SL_TW;
    float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
    for (int k = 0; k < SL_WIN; ++k) {
      const float va = pa[r * SL_LD + x + k], vb = pb[r * SL_LD + x + k], g = win.g[k];
      ma = fmaf(g, va, ma);
      mb = fmaf(g, vb, mb);
      maa = fmaf(g, va * va, maa);
      mbb = fmaf(g, vb * vb, mbb);
      mab = fmaf(g, va * vb, mab);
    }
    rs[0][it] = ma; rs[1][it] = mb; rs[2][it] = maa; rs[3][it] = mbb; rs[4][it] = mab;
  }
  __syncthreads();

  // column pass for the RPT origins (rows wave * RPT ..) of column `lane`, then the windows
  float m[5][SL_RPT];
#pragma unroll
  for (int q = 0; q < 5; ++q) sl_column(rs[q], wave * SL_RPT, lane, win, m[q]);
  const int ox = x0 + lane, oy0 = y0 + wave * SL_RPT;
  const int Ho = H - SL_HALO, Wo = W - SL_HALO;
  const float dca = ca - ka, dcb = cb - kb;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < SL_RPT; ++k) {
    if (ox < Wo && oy0 + k < Ho) {
      const float ma = m[0][k], mb = m[1][k];
      const float vx = fmaf(-ma, ma, m[2][k]), vy = fmaf(-mb, mb, m[3][k]), vxy = fmaf(-ma, mb, m[4][k]);
      const float mux = ma + ca, muy = mb + cb;
      const float A1 = 2.f * (mux * muy) + c1, B1 = (mux * mux + muy * muy) + c1;
      const float A2 = 2.f * vxy + c2, B2 = (vx + vy) + c2;
      const float den = B1 * B2;
      const float S = (A1 * A2) / den;
      acc += S;
      const int64_t o = ((int64_t)plane * Ho + (oy0 + k)) * Wo + ox;
      if (map) map[o] = S;
      if (d1) {
        const float svx = -(S / B2), svxy = (2.f * A1) / den;
        const float smu = (2.f / B1) * fmaf(muy, A2 / B2, -(mux * S));
        const float sa = ma + dca, sb = mb + dcb;                        // mux - kx, muy - ky
        d1[o] = fmaf(-2.f * sa, svx, fmaf(-sb, svxy, smu));
        d2[o] = svx;
        d3[o] = svxy;
      }
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void __launch_bounds__(SL_THREADS) ssim_finish_kernel(const float* __restrict__ partial, int B, int per_image,
                                                                 double windows, double weight, double* __restrict__ ssim,
                                                                 float* __restrict__ loss) {
  __shared__ double sd[SL_THREADS];
  const int tid = threadIdx.x;
  double total = 0.0;                                     // (thread 0's: sum of 1 - ssim_i in image order)
  for (int img = 0; img < B; ++img) {
    const float* p = partial + (int64_t)img * per_image;
    double s = 0.0;
    for (int i = tid; i < per_image; i += SL_THREADS) s += (double)p[i];
    sd[tid] = s;
    __syncthreads();
    for (int off = SL_THREADS / 2; off > 0; off >>= 1) {
      if (tid < off) sd[tid] += sd[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      const double v = sd[0] / windows;
      if (ssim) ssim[img] = v;
      total += 1.0 - v;
    }
    __syncthreads();
  }
  if (tid == 0 && loss) loss[0] = (float)(weight * (total / (double)B));
}

__global__ void __launch_bounds__(SL_THREADS) ssim_bwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int H, int W,
                                                              int tiles_x, int tiles_y, SlWin win, float coef,
                                                              const float* __restrict__ gloss, const float* __restrict__ d1,
                                                              const float* __restrict__ d2, const float* __restrict__ d3,
                                                              float* __restrict__ da) {
  __shared__ float dm[3][SL_ROWS * SL_LD];
  __shared__ float rs[3][SL_ROWS * SL_TW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = tiles_x * tiles_y;
  const int plane = (int)blockIdx.x / tiles, t = (int)blockIdx.x % tiles;
  const int ty = t / tiles_x, tx = t % tiles_x;
  const int y0 = ty * SL_TH, x0 = tx * SL_TW;                                   // first pixel of the tile
  const int Ho = H - SL_HALO, Wo = W - SL_HALO;
  const int64_t base = (int64_t)plane * H * W, obase = (int64_t)plane * Ho * Wo;
  const float ka = a[base], kb = b[base];

  // staged entry (r, c) is the window origin (y0 - 10 + r, x0 - 10 + c); zero outside the valid origins
  for (int it = tid; it < SL_ROWS * SL_COLS; it += SL_THREADS) {
    const int r = it / SL_COLS, c = it % SL_COLS, oy = y0 - SL_HALO + r, ox = x0 - SL_HALO + c;
    float v1 = 0.f, v2 = 0.f, v3 = 0.f;
    if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
      const int64_t i = obase + (int64_t)oy * Wo + ox;
      v1 = d1[i]; v2 = d2[i]; v3 = d3[i];
    }
    dm[0][r * SL_LD + c] = v1; dm[1][r * SL_LD + c] = v2; dm[2][r * SL_LD + c] = v3;
  }
  __syncthreads();

  // pixel column j takes the origins j - dx, dx = 0 .. 10, with weight g[dx] = g[10 - dx]: staged columns j .. j + 10 in tap order
  for (int it = tid; it < SL_ROWS * SL_TW; it += SL_THREADS) {
    const int r = it / SL_TW, x = it % SL_TW;
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int k = 0; k < SL_WIN; ++k) {
      const float g = win.g[k];
      s1 = fmaf(g, dm[0][r * SL_LD + x + k], s1);
      s2 = fmaf(g, dm[1][r * SL_LD + x + k], s2);
      s3 = fmaf(g, dm[2][r * SL_LD + x + k], s3);
    }
    rs[0][it] = s1; rs[1][it] = s2; rs[2][it] = s3;
  }
  __syncthreads();

  float T[3][SL_RPT];
#pragma unroll
  for (int q = 0; q < 3; ++q) sl_column(rs[q], wave * SL_RPT, lane, win, T[q]);
  const float cg = coef * gloss[0];
  const int px = x0 + lane, py0 = y0 + wave * SL_RPT;
#pragma unroll
  for (int k = 0; k < SL_RPT; ++k) {
    if (px < W && py0 + k < H) {
      const int64_t i = base + (int64_t)(py0 + k) * W + px;
      const float sa = a[i] - ka, sb = b[i] - kb;
      da[i] = cg * fmaf(sb, T[2][k], fmaf(2.f * sa, T[1][k], T[0][k]));
    }
  }
}

struct SlShape { int tiles_x, tiles_y, ptiles_x, ptiles_y; int64_t blocks, pblocks, windows; };
static bool sl_shape(int B, int C, int H, int W, SlShape* s) {
  if (B < 1 || C < 1 || H < SL_WIN || W < SL_WIN) return false;
  s->tiles_x = ceil_div(W - SL_HALO, SL_TW);
  s->tiles_y = ceil_div(H - SL_HALO, SL_TH);
  s->ptiles_x = ceil_div(W, SL_TW);
  s->ptiles_y = ceil_div(H, SL_TH);
  s->blocks = (int64_t)B * C * s->tiles_x * s->tiles_y;
  s->pblocks = (int64_t)B * C * s->ptiles_x * s->ptiles_y;
  s->windows = (int64_t)B * C * (H - SL_HALO) * (W - SL_HALO);
  return s->pblocks <= 0x7fffffff && (int64_t)B * C <= 0x7fffffff;
}
static int64_t sl_partial_bytes(const SlShape& s) { return (s.blocks * 4 + 255) / 256 * 256; }

}  // namespace

extern "C" int cips3d_ssim_loss_tile(int* tile_h, int* tile_w) {
  if (tile_h) *tile_h = SL_TH;
  if (tile_w) *tile_w = SL_TW;
  return SL_THREADS;
}

extern "C" int64_t cips3d_ssim_loss_workspace_bytes(int B, int C, int H, int W, int need_grad) {
  SlShape s;
  if (!sl_shape(B, C, H, W, &s)) return CIPS3D_E_BADARG;
  return sl_partial_bytes(s) + (need_grad ? 3 * 4 * s.windows : 0);
}

extern "C" int cips3d_ssim_loss(const float* a, const float* b, int B, int C, int H, int W, float weight, float data_range,
                                void* workspace, int need_grad, float* map, double* ssim, float* loss, void* stream) {
  SlShape s;
  if (!a || !b || !workspace || (!ssim && !loss) || !(data_range > 0.f) || !sl_shape(B, C, H, W, &s)) return CIPS3D_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) || (reinterpret_cast<uintptr_t>(ssim) & 7)) return CIPS3D_E_UNSUPP;
  float* partial = static_cast<float*>(workspace);
  float* d1 = need_grad ? reinterpret_cast<float*>(static_cast<char*>(workspace) + sl_partial_bytes(s)) : nullptr;
  float* d2 = need_grad ? d1 + s.windows : nullptr;
  float* d3 = need_grad ? d2 + s.windows : nullptr;
  const double R = (double)data_range;
  const float c1 = (float)((0.01 * R) * (0.01 * R)), c2 = (float)((0.03 * R) * (0.03 * R));
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)s.blocks), dim3(SL_THREADS), 0, st, a, b, H, W, s.tiles_x, s.tiles_y,
                     sl_window(), c1, c2, partial, d1, d2, d3, map);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(SL_THREADS), 0, st, partial, B, C * s.tiles_x * s.tiles_y,
                     (double)(s.windows / B), (double)weight, ssim, loss);
  return cips3d_launch_status();
}

extern "C" int cips3d_ssim_loss_bwd(const float* a, const float* b, int B, int C, int H, int W, float weight, const void* workspace,
                                    const float* gloss, float* da, void* stream) {
  SlShape s;
  if (!a || !b || !workspace || !gloss || !da || !sl_shape(B, C, H, W, &s)) return CIPS3D_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 15) return CIPS3D_E_UNSUPP;
  const float* d1 = reinterpret_cast<const float*>(static_cast<const char*>(workspace) + sl_partial_bytes(s));
  const float* d2 = d1 + s.windows;
  const float* d3 = d2 + s.windows;
  const float coef = (float)(-(double)weight / (double)s.windows);
  hipLaunchKernelGGL(ssim_bwd_kernel, dim3((unsigned)s.pblocks), dim3(SL_THREADS), 0, as_stream(stream), a, b, H, W, s.ptiles_x,
                     s.ptiles_y, sl_window(), coef, gloss, d1, d2, d3, da);
  return cips3d_launch_status();
}
