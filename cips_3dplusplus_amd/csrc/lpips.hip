// LPIPS v0.1 (net = 'vgg', spatial = False) on the device: the head on five ReLU taps of the VGG16 trunk of vgg.hip /
// vgg_split.hip.  For one layer, maps za, zb [B,C,H,W] (the trunk's PRE-ReLU outputs) and weights lin [C]:
//     f = relu(z);  n(p) = sqrt(sum_c f[c,p]^2) + 1e-10;  d(p) = sum_c lin[c] (fa[c,p] / na(p) - fb[c,p] / nb(p))^2
// and the layer's value is the mean of d over the pixels; LPIPS is the sum of the five layers' values.
//
// lpips_head_kernel: a workgroup of four waves owns tiles of 64 consecutive pixels of one sample; a lane is a pixel (the channel
// stride is H W, so every load of a wave is 256 contiguous bytes) and wave w walks channels [w C/4, (w + 1) C/4).  Two passes
// over the channels -- the squared norms, then the weighted squared difference of the normalised values -- each combined
// across the four waves through LDS in the order w = 0, 1, 2, 3.  The single-pass expansion of the square is not used: it
// cancels for close images, and identical images must give exactly 0.  A pixel whose channels are all <= 0 has f = 0 and
// n = 1e-10: it contributes 0 / 1e-10 = 0.  Wave 0 writes d(p) to the optional map and adds it, in fp64, to its lane's running
// sum over the workgroup's tiles (tile t of workgroup g: g + t * gridDim.x, fixed by the grid, which depends on H W alone);
// a fixed tree over the 64 lanes gives partial[sample][layer][workgroup].  lpips_final_kernel, one workgroup per sample, adds
// a layer's partials in a fixed order, divides by H W, and writes the five values and their sum (layers in order) into the
// sample's row of the record.  No atomics; a result does not depend on the batch the sample sits in, nor on which of the
// two operands comes from a separate trunk call.
#include "common.h"

namespace {

constexpr int LAYERS = CIPS3D_LPIPS_LAYERS;
constexpr int MAX_PARTS = 2048;                  // workgroups (= partial sums) per (sample, layer)
const int kTapConv[LAYERS] = {1, 3, 6, 9, 12};   // relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
const int kTapChan[LAYERS] = {64, 128, 256, 512, 512};
const int kTapShift[LAYERS] = {0, 1, 2, 3, 4};   // the tap's stride is 1 << shift

__device__ static inline float relu(float v) { return fmaxf(v, 0.f); }

__global__ void __launch_bounds__(256) lpips_head_kernel(const float* __restrict__ za, const float* __restrict__ zb,
                                                         int64_t zb_sample_stride, const float* __restrict__ lin,
                                                         float* __restrict__ map, double* __restrict__ partial,
                                                         int64_t partial_sample_stride, int C, int HW) {
  __shared__ float s_norm[2][4][64];
  __shared__ float s_dist[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const int Cq = C >> 2, c0 = wave * Cq;
  const int n_tiles = (HW + 63) >> 6;
  const float* pa = za + (int64_t)b * C * HW + (int64_t)c0 * HW;
  const float* pb = zb + (int64_t)b * zb_sample_stride + (int64_t)c0 * HW;
  double acc = 0.0;
  for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {       // (uniform over the workgroup: the barriers are safe)
    const int p = tile * 64 + lane;
    const bool live = p < HW;
    const float* qa = pa + (live ? p : 0);
    const float* qb = pb + (live ? p : 0);
    float sa = 0.f, sb = 0.f;
    if (live) {
#pragma unroll 8
      for (int c = 0; c < Cq; ++c) {
        const float fa = relu(qa[(int64_t)c * HW]), fb = relu(qb[(int64_t)c * HW]);
        sa += fa * fa;
        sb += fb * fb;
      }
    }
    s_norm[0][wave][lane] = sa;
    s_norm[1][wave][lane] = sb;
    __syncthreads();
    const float na = sqrtf(((s_norm[0][0][lane] + s_norm[0][1][lane]) + s_norm[0][2][lane]) + s_norm[0][3][lane]) + 1e-10f;
    const float nb = sqrtf(((s_norm[1][0][lane] + s_norm[1][1][lane]) + s_norm[1][2][lane]) + s_norm[1][3][lane]) + 1e-10f;
    float d = 0.f;
    if (live) {
#pragma unroll 8
      for (int c = 0; c < Cq; ++c) {
        const float fa = relu(qa[(int64_t)c * HW]), fb = relu(qb[(int64_t)c * HW]);
        const float t = fa / na - fb / nb;
        d += lin[c0 + c] * (t * t);
      }
    }
    s_dist[wave][lane] = d;
    __syncthreads();
    if (wave == 0 && live) {
      const float dp = ((s_dist[0][lane] + s_dist[1][lane]) + s_dist[2][lane]) + s_dist[3][lane];
      if (map) map[(int64_t)b * HW + p] = dp;
      acc += (double)dp;
    }
  }
  if (wave == 0) {              // a fixed tree over the 64 lanes, in registers
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) acc += __shfl_down(acc, k, 64);
    if (lane == 0) partial[(int64_t)b * partial_sample_stride + blockIdx.x] = acc;
  }
}

struct LpipsFinal { int n_part[LAYERS]; double inv_hw[LAYERS]; };
// out[b * row_stride + first + k] = layer k's mean (the layers with partial sums) and, with_total, out[b * row_stride] = their
// sum in layer order; one workgroup per sample, fixed-order tree over 256 threads
__global__ void __launch_bounds__(256) lpips_final_kernel(const double* __restrict__ partial, LpipsFinal f,
                                                          double* __restrict__ out, int row_stride, int first, int with_total) {
  __shared__ double sh[256];
  const int b = blockIdx.x;
  double total = 0.0;
  for (int k = 0; k < LAYERS; ++k) {
    if (f.n_part[k] <= 0) continue;
    const double* src = partial + ((int64_t)b * LAYERS + k) * MAX_PARTS;
    double s = 0.0;
    for (int i = threadIdx.x; i < f.n_part[k]; i += 256) s += src[i];
    sh[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int j = 128; j > 0; j >>= 1) {
      if ((int)threadIdx.x < j) sh[threadIdx.x] += sh[threadIdx.x + j];
      __syncthreads();
    }
    const double v = sh[0] * f.inv_hw[k];
    __syncthreads();
    if (threadIdx.x == 0) out[(int64_t)b * row_stride + first + k] = v;
    total += v;
  }
  if (with_total && threadIdx.x == 0) out[(int64_t)b * row_stride] = total;
}

inline int parts_of(int64_t HW) { return (int)(ceil_div<int64_t>(HW, 64) < MAX_PARTS ? ceil_div<int64_t>(HW, 64) : MAX_PARTS); }

bool good_channels(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// one layer's head into partial slot `k` of every sample
int launch_head(const float* za, const float* zb, int64_t zb_sample_stride, const float* lin, float* map, double* partial, int k,
                int B, int C, int64_t HW, hipStream_t s) {
  hipLaunchKernelGGL(lpips_head_kernel, dim3(parts_of(HW), B), dim3(256), 0, s, za, zb, zb_sample_stride, lin, map,
                     partial + (int64_t)k * MAX_PARTS, (int64_t)LAYERS * MAX_PARTS, C, (int)HW);
  return cips3d_launch_status();
}

int check_lpips(const cips3d_lpips_io* io, const cips3d_vgg_io* t) {
  if (!io || !t) return CIPS3D_E_BADARG;
  if (io->B < 1 || io->row < 0 || !io->partial || !io->record) return CIPS3D_E_BADARG;
  int n_target = 0;
  for (int k = 0; k < LAYERS; ++k) {
    if (!io->lin[k]) return CIPS3D_E_BADARG;
    n_target += io->target[k] != nullptr;
  }
  if (n_target != 0 && n_target != LAYERS) return CIPS3D_E_BADARG;
  if (t->n_convs != CIPS3D_VGG_CONVS) return CIPS3D_E_BADARG;
  if (t->B != (n_target ? io->B : 2 * io->B)) return CIPS3D_E_BADARG;       // pair form: the trunk's batch is a then b
  return cips3d_lpips_supported(io->B, t->H, t->W);
}

int run_heads(const cips3d_lpips_io* io, const cips3d_vgg_io* t, hipStream_t s) {
  const int B = io->B;
  LpipsFinal f;
  for (int k = 0; k < LAYERS; ++k) {
    const int C = kTapChan[k];
    const int64_t HW = (int64_t)(t->H >> kTapShift[k]) * (t->W >> kTapShift[k]);
    const float* za = t->z[kTapConv[k]];
    const float* zb = io->target[k] ? io->target[k] : za + (int64_t)B * C * HW;
    const int64_t stride = (io->target[k] && io->target_broadcast) ? 0 : (int64_t)C * HW;
    f.n_part[k] = parts_of(HW);
    f.inv_hw[k] = 1.0 / (double)HW;
    const int rc = launch_head(za, zb, stride, io->lin[k], io->map[k], static_cast<double*>(io->partial), k, B, C, HW, s);
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(lpips_final_kernel, dim3(B), dim3(256), 0, s, static_cast<const double*>(io->partial), f,
                     static_cast<double*>(io->record) + io->row * (LAYERS + 1), LAYERS + 1, 1, 1);
  return cips3d_launch_status();
}

}  // namespace

extern "C" int cips3d_lpips_supported(int B, int H, int W) {
  const int rc = cips3d_vgg_supported(B, H, W);
  if (rc != 0) return rc;
  return B > 32767 ? CIPS3D_E_UNSUPP : 0;         // a sample is a grid row of the head; the pair form runs the trunk at 2 B
}

extern "C" int64_t cips3d_lpips_partial_bytes(int B) {
  return B < 1 ? (int64_t)CIPS3D_E_BADARG : (int64_t)B * LAYERS * MAX_PARTS * (int64_t)sizeof(double);
}

extern "C" int cips3d_lpips_head(const float* za, const float* zb, const float* lin, int B, int C, int H, int W, float* map,
                                 void* partial, double* mean, void* stream) {
  if (!za || !zb || !lin || !partial || !mean) return CIPS3D_E_BADARG;
  if (B < 1 || H < 1 || W < 1 || !good_channels(C)) return CIPS3D_E_BADARG;
  const int64_t HW = (int64_t)H * W;
  if (HW > 0x7fffffff - 64 || B > 65535) return CIPS3D_E_UNSUPP;
  hipStream_t s = as_stream(stream);
  int rc = launch_head(za, zb, (int64_t)C * HW, lin, map, static_cast<double*>(partial), 0, B, C, HW, s);
  if (rc != 0) return rc;
  LpipsFinal f = {};
  f.n_part[0] = parts_of(HW);
  f.inv_hw[0] = 1.0 / (double)HW;
  hipLaunchKernelGGL(lpips_final_kernel, dim3(B), dim3(256), 0, s, static_cast<const double*>(partial), f, mean, 1, 0, 0);
  return cips3d_launch_status();
}

extern "C" int cips3d_lpips(const cips3d_vgg_ctx* ctx, const cips3d_lpips_io* io, void* stream) {
  if (!ctx || !io) return CIPS3D_E_BADARG;
  const cips3d_vgg_io* t = static_cast<const cips3d_vgg_io*>(io->trunk);
  int rc = check_lpips(io, t);
  if (rc != 0) return rc;
  if (io->heads_only) {                 // the maps are there already: the trunk's own checks, nothing of it launched
    for (int k = 0; k < LAYERS; ++k)
      if (!t->z[kTapConv[k]]) return CIPS3D_E_BADARG;
  } else if ((rc = cips3d_vgg_features(ctx, t, stream)) != 0) {
    return rc;
  }
  return run_heads(io, t, as_stream(stream));
}

extern "C" int cips3d_lpips_split(const cips3d_vgg_split_ctx* ctx, const cips3d_lpips_io* io, void* stream) {
  if (!ctx || !io) return CIPS3D_E_BADARG;
  const cips3d_vgg_split_io* t = static_cast<const cips3d_vgg_split_io*>(io->trunk);
  int rc = check_lpips(io, t ? &t->io : nullptr);
  if (rc != 0) return rc;
  if (io->heads_only) {
    for (int k = 0; k < LAYERS; ++k)
      if (!t->io.z[kTapConv[k]]) return CIPS3D_E_BADARG;
  } else if ((rc = cips3d_vgg_split_features(ctx, t, stream)) != 0) {
    return rc;
  }
  return run_heads(io, &t->io, as_stream(stream));
}
