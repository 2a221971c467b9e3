// Per-op kernels of the StyleGAN2-style decoder of CIPS-3D++ on gfx950 (reference models/model_v3.py:218-341,418-482).
//
//   cips3d_noise_bias_act    NoiseInjection + bias + leaky-ReLU on their own (generality path)
//   cips3d_torgb             ToRGB (C->3 modulated conv, bias, skip / FIR-upsampled skip add)
//   cips3d_modconv_kxk       direct k x k modulated convolution / stride-2 transpose (generality path)
//   cips3d_torgb_reduce      the fixed-order fold of the ToRGB partial sums of cips3d_modconv1x1_torgb (gemm1x1.hip)
//
// ToRGB and its FIR-upsampled skip are HBM-bound: every kernel reads its input once and writes its output once with
// >= 128-byte row segments.

#include "up2_fir.h"

namespace {

// StyledConv epilogue on its own (generality path): out = lrelu(x + noise_w*noise + bias[c], 0.2)*sqrt(2)
// (NoiseInjection as ONE fused multiply-add in every kernel of the library: `image + weight * noise` of model_v3.py:317-341 with
// one rounding instead of two -- the same value in the fused stages, the chain, the per-layer GEMM and the differentiable forward)
__global__ void __launch_bounds__(256) noise_bias_act_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                             int64_t noise_bstride, const float* __restrict__ nwp,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int B, int C, int64_t HW) {
  const float noise_w = (noise && nwp) ? nwp[0] : 0.f;
  const int64_t total = (int64_t)B * C * HW;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = i % HW;
    const int c = (int)((i / HW) % C);
    const int b = (int)(i / (HW * C));
    const float nz = noise ? noise[(int64_t)b * noise_bstride + n] : 0.f;
    out[i] = lrelu02(fmaf(noise_w, nz, x[i]) + bias[c]) * 1.41421356237309515f;
  }
}

// ------------------------------------------------------------------------------------------------
// ToRGB: 3 x Cin GEMV per pixel on the VALU (HBM-bound: Cin*4 B read per pixel), + bias + skip.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) torgb_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                    const float* __restrict__ bias, const float* __restrict__ skip,
                                                    int skip_up, const float* __restrict__ fir, float* __restrict__ out,
                                                    int B, int Cin, int H, int W) {
  extern __shared__ float s_w[];   // [3][Cin] of this sample
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i < 3 * Cin; i += 256) s_w[i] = wm[(int64_t)b * 3 * Cin + i];
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  const int64_t quads = HW / 4;
  const float* xb = x + (int64_t)b * Cin * HW;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f), g = r, bl = r;
#pragma unroll 4
    for (int i = 0; i < Cin; ++i) {
      const float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)i * HW + q * 4);
      const float w0 = s_w[i], w1 = s_w[Cin + i], w2 = s_w[2 * Cin + i];
      r.x = fmaf(w0, v.x, r.x); r.y = fmaf(w0, v.y, r.y); r.z = fmaf(w0, v.z, r.z); r.w = fmaf(w0, v.w, r.w);
      g.x = fmaf(w1, v.x, g.x); g.y = fmaf(w1, v.y, g.y); g.z = fmaf(w1, v.z, g.z); g.w = fmaf(w1, v.w, g.w);
      bl.x = fmaf(w2, v.x, bl.x); bl.y = fmaf(w2, v.y, bl.y); bl.z = fmaf(w2, v.z, bl.z); bl.w = fmaf(w2, v.w, bl.w);
    }
    float4 res[3] = {r, g, bl};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float4 o = res[c];
      const float bs = bias[c];
      o.x += bs; o.y += bs; o.z += bs; o.w += bs;
      if (skip) {
        if (skip_up) {
          const int oy = (int)((q * 4) / W), ox0 = (int)((q * 4) % W);
          const float* sp = skip + ((int64_t)b * 3 + c) * (H / 2) * (W / 2);
          o.x += up2_tap(sp, H / 2, W / 2, oy, ox0 + 0, fir);
          o.y += up2_tap(sp, H / 2, W / 2, oy, ox0 + 1, fir);
          o.z += up2_tap(sp, H / 2, W / 2, oy, ox0 + 2, fir);
          o.w += up2_tap(sp, H / 2, W / 2, oy, ox0 + 3, fir);
        } else {
          const float4 sv = *reinterpret_cast<const float4*>(skip + ((int64_t)b * 3 + c) * HW + q * 4);
          o.x += sv.x; o.y += sv.y; o.z += sv.z; o.w += sv.w;
        }
      }
      *reinterpret_cast<float4*>(out + ((int64_t)b * 3 + c) * HW + q * 4) = o;
    }
  }
}

// Channel-split variant: a workgroup owns 256/S quads, its S thread slices each reduce Cin/S channels and
// the partial sums meet in LDS.  Keeps every CU busy at low resolution (64^2 x 512 channels is only 1024
// quads) and multiplies the loads in flight per CU at high resolution.
template <int S>
__global__ void __launch_bounds__(256) torgb_split_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                          const float* __restrict__ bias, const float* __restrict__ skip,
                                                          int skip_up, const float* __restrict__ fir,
                                                          float* __restrict__ out, int B, int Cin, int H, int W) {
  constexpr int QB = 256 / S;
  extern __shared__ __attribute__((aligned(16))) float s_mem[];   // [256][12] partials, then [3][Cin] weights
  float* s_part = s_mem;
  float* s_w = s_mem + 256 * 12;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  for (int i = tid; i < 3 * Cin; i += 256) s_w[i] = wm[(int64_t)b * 3 * Cin + i];
  __syncthreads();
  const int64_t HW = (int64_t)H * W;
  const int64_t quads = HW / 4;
  const int ql = tid % QB, sl = tid / QB;
  const int64_t q = (int64_t)blockIdx.x * QB + ql;
  const bool qok = q < quads;
  const float* xb = x + (int64_t)b * Cin * HW + (qok ? q : 0) * 4;
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f), g = r, bl = r;
#pragma unroll 4
  for (int i = sl; i < Cin; i += S) {
    const float4 v = *reinterpret_cast<const float4*>(xb + (int64_t)i * HW);
    const float w0 = s_w[i], w1 = s_w[Cin + i], w2 = s_w[2 * Cin + i];
    r.x = fmaf(w0, v.x, r.x); r.y = fmaf(w0, v.y, r.y); r.z = fmaf(w0, v.z, r.z); r.w = fmaf(w0, v.w, r.w);
    g.x = fmaf(w1, v.x, g.x); g.y = fmaf(w1, v.y, g.y); g.z = fmaf(w1, v.z, g.z); g.w = fmaf(w1, v.w, g.w);
    bl.x = fmaf(w2, v.x, bl.x); bl.y = fmaf(w2, v.y, bl.y); bl.z = fmaf(w2, v.z, bl.z); bl.w = fmaf(w2, v.w, bl.w);
  }
  float4* pp = reinterpret_cast<float4*>(s_part) + (sl * QB + ql) * 3;
  pp[0] = r; pp[1] = g; pp[2] = bl;
  __syncthreads();
  if (tid < QB * 3) {
    const int c = tid / QB, q2 = tid % QB;
    const int64_t qq = (int64_t)blockIdx.x * QB + q2;
    if (qq < quads) {
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int k = 0; k < S; ++k) {
        const float4 v = reinterpret_cast<const float4*>(s_part)[(k * QB + q2) * 3 + c];
        o.x += v.x; o.y += v.y; o.z += v.z; o.w += v.w;
      }
      const float bs = bias[c];
      o.x += bs; o.y += bs; o.z += bs; o.w += bs;
      if (skip) {
        if (skip_up) {
          const int oy = (int)((qq * 4) / W), ox0 = (int)((qq * 4) % W);
          const float* sp = skip + ((int64_t)b * 3 + c) * (H / 2) * (W / 2);
          o.x += up2_tap(sp, H / 2, W / 2, oy, ox0 + 0, fir);
          o.y += up2_tap(sp, H / 2, W / 2, oy, ox0 + 1, fir);
          o.z += up2_tap(sp, H / 2, W / 2, oy, ox0 + 2, fir);
          o.w += up2_tap(sp, H / 2, W / 2, oy, ox0 + 3, fir);
        } else {
          const float4 sv = *reinterpret_cast<const float4*>(skip + ((int64_t)b * 3 + c) * HW + qq * 4);
          o.x += sv.x; o.y += sv.y; o.z += sv.z; o.w += sv.w;
        }
      }
      *reinterpret_cast<float4*>(out + ((int64_t)b * 3 + c) * HW + qq * 4) = o;
    }
  }
}

// any H, W (no 16-byte alignment): one pixel per thread
__global__ void __launch_bounds__(256) torgb_scalar_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                           const float* __restrict__ bias, const float* __restrict__ skip,
                                                           int skip_up, const float* __restrict__ fir,
                                                           float* __restrict__ out, int B, int Cin, int H, int W) {
  const int64_t HW = (int64_t)H * W;
  const int64_t total = (int64_t)B * HW;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(idx / HW);
    const int64_t n = idx % HW;
    const float* xb = x + (int64_t)b * Cin * HW + n;
    const float* w = wm + (int64_t)b * 3 * Cin;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < Cin; ++i) {
      const float v = xb[(int64_t)i * HW];
      acc[0] = fmaf(w[i], v, acc[0]); acc[1] = fmaf(w[Cin + i], v, acc[1]); acc[2] = fmaf(w[2 * Cin + i], v, acc[2]);
    }
    const int oy = (int)(n / W), ox = (int)(n % W);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o = acc[c] + bias[c];
      if (skip) {
        if (skip_up) o += up2_tap(skip + ((int64_t)b * 3 + c) * (H / 2) * (W / 2), H / 2, W / 2, oy, ox, fir);
        else o += skip[((int64_t)b * 3 + c) * HW + n];
      }
      out[((int64_t)b * 3 + c) * HW + n] = o;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// direct k x k (generality path: k = 3 configs, channel counts the MFMA kernel does not tile)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) modconv_kxk_kernel(const float* __restrict__ x, const float* __restrict__ wm,
                                                          float* __restrict__ out, int B, int Cin, int Cout, int H,
                                                          int W, int k, int transpose2, int OH, int OW) {
  const int64_t total = (int64_t)B * Cout * OH * OW;
  const int pad = k / 2;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int ox = (int)(t % OW); t /= OW;
    const int oy = (int)(t % OH); t /= OH;
    const int o = (int)(t % Cout);
    const int b = (int)(t / Cout);
    const float* wrow = wm + ((int64_t)b * Cout + o) * Cin * k * k;
    const float* xb = x + (int64_t)b * Cin * H * W;
    float acc = 0.f;
    for (int i = 0; i < Cin; ++i) {
      const float* xi = xb + (int64_t)i * H * W;
      const float* wi = wrow + i * k * k;
      for (int ky = 0; ky < k; ++ky) {
        int iy;
        if (transpose2) { const int ty = oy - ky; if (ty < 0 || (ty & 1)) continue; iy = ty >> 1; }
        else iy = oy + ky - pad;
        if (iy < 0 || iy >= H) continue;
        for (int kx = 0; kx < k; ++kx) {
          int ix;
          if (transpose2) { const int tx = ox - kx; if (tx < 0 || (tx & 1)) continue; ix = tx >> 1; }
          else ix = ox + kx - pad;
          if (ix < 0 || ix >= W) continue;
          acc = fmaf(xi[(int64_t)iy * W + ix], wi[ky * k + kx], acc);
        }
      }
    }
    out[idx] = acc;
  }
}

}  // namespace

extern "C" int cips3d_noise_bias_act(const float* x, const float* noise, int64_t noise_bstride, const float* noise_w,
                                     const float* bias, float* out, int B, int C, int64_t HW, void* stream) {
  if (!x || !bias || !out || B < 0 || C <= 0 || HW <= 0) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  int64_t blocks = ceil_div<int64_t>((int64_t)B * C * HW, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(noise_bias_act_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, noise,
                     noise_bstride, noise_w, bias, out, B, C, HW);
  return cips3d_launch_status();
}

// out = skip + sum_s part[s] + sum_k bias_k : the fixed-order fold of the ToRGB partial sums written by
// cips3d_modconv1x1_torgb (slots = layers x row blocks, each [B][3][HW]).  One float4 per thread.
struct RgbReduceArgs {
  const float* part; int n_slots; int n_bias; const float* bias[CIPS3D_TORGB_FOLD_MAX]; const float* skip; float* out;
  int64_t n4, HW4, slot_stride;
};

// block = 64 float4 positions x 4 slot groups: group g adds slots g, g+4, ... (independent loads in flight), the groups
// meet in LDS in a fixed order.
__global__ void __launch_bounds__(256) torgb_reduce_kernel(RgbReduceArgs a) {
  __shared__ f32x4 s_p[4][64];
  const int pl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + pl;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (i < a.n4) {
    for (int s0 = g; s0 < a.n_slots; s0 += 16) {
      f32x4 t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        t[u] = s0 + 4 * u < a.n_slots ? *reinterpret_cast<const f32x4*>(a.part + (s0 + 4 * u) * a.slot_stride + i * 4)
                                      : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += t[u][c];
    }
  }
  s_p[g][pl] = v;
  __syncthreads();
  if (g != 0 || i >= a.n4) return;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const f32x4 t = s_p[k][pl];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += t[c];
  }
  const int ch = (int)((i / a.HW4) % 3);
  float bs = 0.f;
  for (int k = 0; k < a.n_bias; ++k) bs += a.bias[k][ch];
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] += bs;
  if (a.skip) {
    const f32x4 sk = *reinterpret_cast<const f32x4*>(a.skip + i * 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += sk[c];
  }
  *reinterpret_cast<f32x4*>(a.out + i * 4) = v;
}

extern "C" int cips3d_torgb_reduce(const float* part, int n_slots, const float* const* biases, int n_bias, const float* skip,
                                   float* out, int B, int64_t HW, void* stream) {
  if (!part || !out || n_slots < 1 || n_bias < 0 || n_bias > CIPS3D_TORGB_FOLD_MAX || (n_bias && !biases) || B < 0 || HW <= 0)
    return CIPS3D_E_BADARG;
  if (HW % 4) return CIPS3D_E_UNSUPP;
  if (B == 0) return 0;
  RgbReduceArgs a{};
  a.part = part; a.n_slots = n_slots; a.n_bias = n_bias;
  for (int k = 0; k < n_bias; ++k) a.bias[k] = biases[k];
  a.skip = skip; a.out = out;
  a.n4 = (int64_t)B * 3 * HW / 4; a.HW4 = HW / 4; a.slot_stride = (int64_t)B * 3 * HW;
  hipLaunchKernelGGL(torgb_reduce_kernel, dim3((unsigned)ceil_div<int64_t>(a.n4, 64)), dim3(256), 0, as_stream(stream), a);
  return cips3d_launch_status();
}

extern "C" int cips3d_torgb(const float* x, const float* wm, const float* bias, const float* skip, int skip_up,
                            const float* fir, float* out, int B, int Cin, int H, int W, void* stream) {
  if (!x || !wm || !bias || !out || B < 0 || Cin <= 0 || H <= 0 || W <= 0) return CIPS3D_E_BADARG;
  if (skip && skip_up && (!fir || (H % 2) || (W % 2))) return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  if (W % 4 != 0) {
    int64_t bs = ceil_div<int64_t>((int64_t)B * H * W, 256);
    if (bs > 16384) bs = 16384;
    hipLaunchKernelGGL(torgb_scalar_kernel, dim3((unsigned)bs), dim3(256), 0, as_stream(stream), x, wm, bias, skip,
                       skip_up, fir, out, B, Cin, H, W);
    return cips3d_launch_status();
  }
  const int64_t quads = (int64_t)H * W / 4;
  {
    const size_t lds = sizeof(float) * (256 * 12 + 3 * (size_t)Cin);
    if (quads <= 32768 && Cin >= 64) {
      hipLaunchKernelGGL(torgb_split_kernel<16>, dim3((unsigned)ceil_div<int64_t>(quads, 16), (unsigned)B), dim3(256), lds,
                         as_stream(stream), x, wm, bias, skip, skip_up, fir, out, B, Cin, H, W);
      return cips3d_launch_status();
    }
    if (Cin >= 16) {
      hipLaunchKernelGGL(torgb_split_kernel<4>, dim3((unsigned)ceil_div<int64_t>(quads, 64), (unsigned)B), dim3(256), lds,
                         as_stream(stream), x, wm, bias, skip, skip_up, fir, out, B, Cin, H, W);
      return cips3d_launch_status();
    }
  }
  int64_t bx = ceil_div<int64_t>(quads, 256);
  if (bx > 4096) bx = 4096;
  hipLaunchKernelGGL(torgb_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), sizeof(float) * 3 * Cin,
                     as_stream(stream), x, wm, bias, skip, skip_up, fir, out, B, Cin, H, W);
  return cips3d_launch_status();
}

extern "C" int cips3d_modconv_kxk(const float* x, const float* wm, float* out, int B, int Cin, int Cout, int H, int W,
                                  int k, int transpose2, void* stream) {
  if (!x || !wm || !out || B < 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || k <= 0 || (k % 2) == 0)
    return CIPS3D_E_BADARG;
  if (B == 0) return 0;
  const int OH = transpose2 ? 2 * H - 1 + k - 1 : H, OW = transpose2 ? 2 * W - 1 + k - 1 : W;
  const int64_t total = (int64_t)B * Cout * OH * OW;
  int64_t blocks = ceil_div<int64_t>(total, 256);
  if (blocks > 65535) blocks = 65535;
  hipLaunchKernelGGL(modconv_kxk_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, wm, out, B, Cin,
                     Cout, H, W, k, transpose2, OH, OW);
  return cips3d_launch_status();
}
