// What the two forms of the VGG16 conv perceptual loss share (vgg.hip: exact fp32; vgg_split.hip: split-fp16): the layer
// tables, the VALU kernels around the 3x3 convolutions (conv 0 and its data gradient, the max-pool and its backward, the tap
// gradient, the tap loss) and the launch of the tap loss.  Every translation unit that includes it gets its own copy.
#pragma once
#include "common.h"

namespace {

constexpr int NCONV = CIPS3D_VGG_CONVS;
const int kChan[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int kPoolBefore[NCONV] = {0, 0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0};       // a 2x2 max-pool sits in front of conv l
constexpr int PARTIALS_PER_TAP = 1024;

__device__ static inline float vgg_mean(int c) { return c == 0 ? 0.485f : (c == 1 ? 0.456f : 0.406f); }
__device__ static inline float vgg_std(int c) { return c == 0 ? 0.229f : (c == 1 ? 0.224f : 0.225f); }

// conv 0: x [B,3,H,W] in [-1, 1] (normalize) or already normalised -> z [B,64,H,W].  One thread per pixel; the weight and
// bias indices are wave-uniform (scalar loads).
__global__ void __launch_bounds__(256) vgg_first_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ z, int B, int H,
                                                            int W, int normalize) {
  const int HW = H * W;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * HW) return;
  const int b = (int)(gid / HW), p = (int)(gid % HW), y = p / W, xx = p % W;
  float in[27];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int ty = 0; ty < 3; ++ty)
#pragma unroll
      for (int tx = 0; tx < 3; ++tx) {
        const int iy = y + ty - 1, ix = xx + tx - 1;
        const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
        float v = x[ok ? ((int64_t)b * 3 + c) * HW + iy * W + ix : 0];
        if (normalize) v = ((v + 1.f) * 0.5f - vgg_mean(c)) / vgg_std(c);      // the padding is zero AFTER the normalisation
        in[c * 9 + ty * 3 + tx] = ok ? v : 0.f;
      }
  float* zb = z + (int64_t)b * 64 * HW + p;
#pragma unroll 4
  for (int o = 0; o < 64; ++o) {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc = fmaf(w[o * 27 + k], in[k], acc);
    zb[(int64_t)o * HW] = acc + bias[o];
  }
}

// data gradient of conv 0: g [B,64,H,W] (w.r.t. its pre-ReLU output, already masked) -> dx [B,3,H,W], times 0.5 / std
__global__ void __launch_bounds__(256) vgg_first_bwd_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                            float* __restrict__ dx, int B, int H, int W, int normalize) {
  const int HW = H * W;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (int64_t)B * HW) return;
  const int b = (int)(gid / HW), p = (int)(gid % HW), y = p / W, xx = p % W;
  int off[9];
#pragma unroll
  for (int ty = 0; ty < 3; ++ty)
#pragma unroll
    for (int tx = 0; tx < 3; ++tx) {
      const int iy = y - (ty - 1), ix = xx - (tx - 1);        // the output pixel that read this input through tap (ty, tx)
      off[ty * 3 + tx] = (iy >= 0 && iy < H && ix >= 0 && ix < W) ? iy * W + ix : -1;
    }
  const float* gb = g + (int64_t)b * 64 * HW;
  float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll 2
  for (int o = 0; o < 64; ++o) {
    const float* go = gb + (int64_t)o * HW;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      float v = go[off[t] >= 0 ? off[t] : 0];
      v = off[t] >= 0 ? v : 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] = fmaf(w[o * 27 + c * 9 + t], v, acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
    dx[((int64_t)b * 3 + c) * HW + p] = normalize ? acc[c] * (0.5f / vgg_std(c)) : acc[c];
}

// out [n = B C, H/2, W/2] = max-pool 2x2/2 of relu(z [n, H, W])
__global__ void __launch_bounds__(256) vgg_pool_fwd_kernel(const float* __restrict__ z, float* __restrict__ out, int64_t total,
                                                           int Ho, int Wo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int xo = (int)(gid % Wo);
  const int64_t row = gid / Wo;                       // = n * Ho + yo
  const float* s = z + (row * 2) * (2 * Wo) + 2 * xo;
  const float2 r0 = *reinterpret_cast<const float2*>(s), r1 = *reinterpret_cast<const float2*>(s + 2 * Wo);
  out[gid] = fmaxf(fmaxf(fmaxf(r0.x, r0.y), fmaxf(r1.x, r1.y)), 0.f);
}

// Backward of (ReLU, max-pool) in one pass: gp [n, H/2, W/2] is the gradient of the pooled tensor, z [n, H, W] the kept
// pre-ReLU tensor; out = route(gp) * (z > 0) + gloss 2 w^2 (z - t).  The gradient goes to the first maximum of relu(z) in scan
// order (torch's max_pool2d backward).  Ties only occur at 0 after the ReLU, where the ReLU mask kills the gradient anyway.
__global__ void __launch_bounds__(256) vgg_pool_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ z,
                                                           const float* __restrict__ tap_t, float tap_c,
                                                           const float* __restrict__ gloss, float* __restrict__ out,
                                                           int64_t total, int Ho, int Wo) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int xo = (int)(gid % Wo);
  const int64_t row = gid / Wo;
  const int64_t i0 = (row * 2) * (2 * Wo) + 2 * xo, i1 = i0 + 2 * Wo;
  const float2 z0 = *reinterpret_cast<const float2*>(z + i0), z1 = *reinterpret_cast<const float2*>(z + i1);
  const float zz[4] = {z0.x, z0.y, z1.x, z1.y};
  float m = fmaxf(fmaxf(fmaxf(zz[0], zz[1]), fmaxf(zz[2], zz[3])), 0.f);
  int sel = 3;
#pragma unroll
  for (int k = 2; k >= 0; --k)
    if (fmaxf(zz[k], 0.f) == m) sel = k;
  const float g = gp[gid];
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (k == sel && zz[k] > 0.f) ? g : 0.f;
  if (tap_t) {
    const float gl = gloss[0] * tap_c;
    const float2 t0 = *reinterpret_cast<const float2*>(tap_t + i0), t1 = *reinterpret_cast<const float2*>(tap_t + i1);
    v[0] += gl * (zz[0] - t0.x);
    v[1] += gl * (zz[1] - t0.y);
    v[2] += gl * (zz[2] - t1.x);
    v[3] += gl * (zz[3] - t1.y);
  }
  *reinterpret_cast<float2*>(out + i0) = float2{v[0], v[1]};
  *reinterpret_cast<float2*>(out + i1) = float2{v[2], v[3]};
}

// the deepest tap's gradient, which starts the backward chain: g = gloss 2 w^2 (z - t)
__global__ void __launch_bounds__(256) vgg_tap_grad_kernel(const float* __restrict__ z, const float* __restrict__ t, float c,
                                                           const float* __restrict__ gloss, float* __restrict__ g, int64_t n) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  g[gid] = gloss[0] * c * (z[gid] - t[gid]);
}

__device__ static inline double vgg_block_sum(double s, double* sh) {       // fixed-order tree over 256 threads
  sh[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
    __syncthreads();
  }
  return sh[0];
}

// partial[blockIdx.x] = sum over this workgroup's elements of (z - t)^2, fp64, element -> thread assignment fixed by the grid
__global__ void __launch_bounds__(256) vgg_tap_loss_kernel(const float* __restrict__ z, const float* __restrict__ t, int64_t n,
                                                           double* __restrict__ partial) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float d = z[i] - t[i];
    s += (double)d * (double)d;
  }
  s = vgg_block_sum(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct VggLossFinal { int n_part[NCONV]; float w[NCONV]; };
// loss[0] = sum_l w_l^2 sum partial[l][:], layers in order; one workgroup
__global__ void __launch_bounds__(256) vgg_tap_loss_final_kernel(const double* __restrict__ partial, VggLossFinal f,
                                                                 float* __restrict__ loss) {
  __shared__ double sh[256];
  double total = 0.0;
  for (int l = 0; l < NCONV; ++l) {
    if (f.n_part[l] <= 0) continue;
    double s = 0.0;
    for (int i = threadIdx.x; i < f.n_part[l]; i += 256) s += partial[(int64_t)l * PARTIALS_PER_TAP + i];
    s = vgg_block_sum(s, sh);
    total += (double)f.w[l] * (double)f.w[l] * s;
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)total;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)ceil_div<int64_t>(n, 256); }

// the tap loss of convs 0 .. n_convs - 1 (layers with a target): per-tap partial sums, then loss[0]
int launch_tap_loss(const cips3d_vgg_io* io, hipStream_t s) {
  int rc = 0;
  VggLossFinal f;
  int H = io->H, W = io->W;
  for (int l = 0; l < NCONV; ++l) {
    f.n_part[l] = 0;
    f.w[l] = 0.f;
    if (l >= io->n_convs) continue;
    if (kPoolBefore[l]) { H /= 2; W /= 2; }
    if (!io->target[l]) continue;
    const int64_t n = (int64_t)io->B * kChan[l] * H * W;
    const int nb = (int)(ceil_div<int64_t>(n, 4096) < PARTIALS_PER_TAP ? ceil_div<int64_t>(n, 4096) : PARTIALS_PER_TAP);
    f.n_part[l] = nb;
    f.w[l] = io->tap_w[l];
    hipLaunchKernelGGL(vgg_tap_loss_kernel, dim3(nb), dim3(256), 0, s, io->z[l], io->target[l], n,
                       static_cast<double*>(io->partial) + (int64_t)l * PARTIALS_PER_TAP);
    if ((rc = cips3d_launch_status()) != 0) return rc;
  }
  hipLaunchKernelGGL(vgg_tap_loss_final_kernel, dim3(1), dim3(256), 0, s, static_cast<const double*>(io->partial), f, io->loss);
  return cips3d_launch_status();
}

}  // namespace
