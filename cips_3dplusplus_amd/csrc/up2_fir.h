// Patch loads and the polyphase FIR of the 2x up-sampler (upfirdn2d up=2, pad=(2,1), 4x4 taps), shared by the per-op
// kernels (cips3d_up2_fir_act in gemm1x1.hip, ToRGB's skip in decoder_ops.hip) and the fused up-sampling stage (fused_stage.hip).
#pragma once
#include "mfma_frag.h"

// single tap set for one output pixel; taps come from memory (runtime parity => no register array)
__device__ __forceinline__ float up2_tap(const float* __restrict__ src, int H, int W, int oy, int ox,
                                         const float* __restrict__ fir) {
  // u[y][x] = in[(y-2)/2][(x-2)/2] on even (y-2),(x-2); out = sum_{ky,kx} u[oy+ky][ox+kx] * fir[3-ky][3-kx]
  const int ky0 = oy & 1, kx0 = ox & 1;        // first tap with (oy+ky-2) even
  float acc = 0.f;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int ky = ky0 + 2 * a;
    const int iy = (oy + ky - 2) >> 1;
    if (iy < 0 || iy >= H) continue;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int kx = kx0 + 2 * c;
      const int ix = (ox + kx - 2) >> 1;
      if (ix < 0 || ix >= W) continue;
      acc = fmaf(src[(int64_t)iy * W + ix], fir[15 - (ky * 4 + kx)], acc);
    }
  }
  return acc;
}

// 3 x 4 input patch (rows iy-1..iy+1, columns 2*qx-1..2*qx+2, zero outside the image) of the 2 x 4 output block
// at rows 2*iy, 2*iy+1, columns 4*qx .. 4*qx+3
// (interior variant: the whole patch is inside the image, no predication)
__device__ __forceinline__ void up2_load_interior(const float* __restrict__ src, int W, int iy, int qx, float (&v)[3][4]) {
  const float* row = src + ((iy - 1) * W + 2 * qx);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float2 mid = *reinterpret_cast<const float2*>(row);
    v[r][0] = row[-1]; v[r][1] = mid.x; v[r][2] = mid.y; v[r][3] = row[2];
    row += W;
  }
}

// the same patches from a bf16 array (CIPS3D_Y_BF16: the low-resolution GEMM result stored as bf16): a bf16 is the upper
// half of the fp32 with the same value, the middle pair is one aligned 32-bit load
typedef unsigned short bf16_t;
__device__ __forceinline__ float bf16_f32(unsigned bits) { return __uint_as_float(bits << 16); }
__device__ __forceinline__ void up2_load_interior(const bf16_t* __restrict__ src, int W, int iy, int qx, float (&v)[3][4]) {
  const bf16_t* row = src + ((iy - 1) * W + 2 * qx);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const unsigned mid = *reinterpret_cast<const unsigned*>(row);
    v[r][0] = bf16_f32(row[-1]); v[r][1] = bf16_f32(mid & 0xffffu); v[r][2] = __uint_as_float(mid & 0xffff0000u);
    v[r][3] = bf16_f32(row[2]);
    row += W;
  }
}
__device__ __forceinline__ void up2_load(const bf16_t* __restrict__ src, int H, int W, int iy, int qx, float (&v)[3][4]) {
  const int c = 2 * qx;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = iy - 1 + r;
    const bool yok = (y >= 0) && (y < H);
    const bf16_t* row = src + (yok ? y : 0) * W;
    unsigned mid = 0u;
    if (yok) mid = *reinterpret_cast<const unsigned*>(row + c);
    v[r][1] = bf16_f32(mid & 0xffffu); v[r][2] = __uint_as_float(mid & 0xffff0000u);
    v[r][0] = (yok && c - 1 >= 0) ? bf16_f32(row[c - 1]) : 0.f;
    v[r][3] = (yok && c + 2 < W) ? bf16_f32(row[c + 2]) : 0.f;
  }
}

__device__ __forceinline__ void up2_load(const float* __restrict__ src, int H, int W, int iy, int qx, float (&v)[3][4]) {
  const int c = 2 * qx;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = iy - 1 + r;
    const bool yok = (y >= 0) && (y < H);
    const float* row = src + (yok ? y : 0) * W;
    float2 mid = make_float2(0.f, 0.f);           // middle pair is 8-byte aligned (c even, W even)
    if (yok) mid = *reinterpret_cast<const float2*>(row + c);
    v[r][1] = mid.x; v[r][2] = mid.y;
    v[r][0] = (yok && c - 1 >= 0) ? row[c - 1] : 0.f;
    v[r][3] = (yok && c + 2 < W) ? row[c + 2] : 0.f;
  }
}

// FLAT stages (no up-sampling): the 2 x 4 block itself, rows y, y + 1, columns x .. x + 3 (x % 4 == 0), into rows 0 / 1 of the set
__device__ __forceinline__ void flat_load(const float* __restrict__ src, int W, int y, int x, float (&v)[3][4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(src + ((y + r) * W + x));
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = t[c];
  }
}
__device__ __forceinline__ void flat_load(const bf16_t* __restrict__ src, int W, int y, int x, float (&v)[3][4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const uint2 t = *reinterpret_cast<const uint2*>(src + ((y + r) * W + x));
    v[r][0] = bf16_f32(t.x & 0xffffu); v[r][1] = __uint_as_float(t.x & 0xffff0000u);
    v[r][2] = bf16_f32(t.y & 0xffffu); v[r][3] = __uint_as_float(t.y & 0xffff0000u);
  }
}

// polyphase FIR of the patch; all tap indices are compile-time constants
__device__ __forceinline__ void up2_fir(const float (&v)[3][4], const float (&kf)[16], float (&o)[2][4]) {
#pragma unroll
  for (int py = 0; py < 2; ++py) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int px = j & 1;
      const int col0 = (j + 1) >> 1;                 // j=0 -> v0,v1 ; j=1,2 -> v1,v2 ; j=3 -> v2,v3
      float acc = 0.f;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int ky = py + 2 * a;
        const int r = py + a;                        // py=0: rows iy-1, iy ; py=1: rows iy, iy+1
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) acc = fmaf(v[r][col0 + bb], kf[ky * 4 + px + 2 * bb], acc);
      }
      o[py][j] = acc;
    }
  }
}
