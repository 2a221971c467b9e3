// The fragment vocabulary of the decoder's MFMA kernels (modulate.hip, gemm1x1.hip, decoder_ops.hip, fused_stage.hip,
// chain.hip): vector types of the MFMA operands, the split-fp16 and bf16 operand conversions, the counted-wait immediate.
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// ---- split-fp16 inside the fused up-sampling stage (16-channel k-groups, v_mfma_f32_16x16x16_f16): an activation travels
// through LDS as ONE 32-bit word holding its two halves {fp16 hi (bits 0-15), fp16 lo (bits 16-31)} -- the producer splits
// it once -- and a lane assembles its 4-element fragments from four such words with two v_perm_b32 each.  Weights come
// pre-split from the modulate kernel (CIPS3D_MOD_SPLIT16: per o-tile and k-group [lane][hi x4 | lo x4], the 16 bytes of
// the fp32 fragment they replace), scaled by 2^8.
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float pack_split(float x) { return __uint_as_float(cips3d_split_word(x)); }
// ... of the exact product x * k (k wave-uniform): the activation's sqrt(2) 2^-e rides on the split, two instructions in all
__device__ __forceinline__ float pack_split(float x, float k) { return __uint_as_float(cips3d_split_word(x, k)); }
// four packed words (fragment elements 0..3) -> the hi fragment and the lo fragment
__device__ __forceinline__ void unpack_frag(float p0, float p1, float p2, float p3, h4& hi, h4& lo) {
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const unsigned a0 = __float_as_uint(p0), a1 = __float_as_uint(p1), a2 = __float_as_uint(p2), a3 = __float_as_uint(p3);
  hi = __builtin_bit_cast(h4, u32x2_t{__builtin_amdgcn_perm(a1, a0, 0x05040100u), __builtin_amdgcn_perm(a3, a2, 0x05040100u)});
  lo = __builtin_bit_cast(h4, u32x2_t{__builtin_amdgcn_perm(a1, a0, 0x07060302u), __builtin_amdgcn_perm(a3, a2, 0x07060302u)});
}
// split four fp32 values (fragment elements 0..3) in registers
__device__ __forceinline__ void split_frag(float v0, float v1, float v2, float v3, h4& hi, h4& lo) {
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  unsigned h0, l0, h1, l1;
  cips3d_split_pair(v0, v1, h0, l0);
  cips3d_split_pair(v2, v3, h1, l1);
  hi = __builtin_bit_cast(h4, u32x2_t{h0, h1});
  lo = __builtin_bit_cast(h4, u32x2_t{l0, l1});
}
// the three products of one 16x16x16 block: A fragment word = {hi x4 | lo x4}
__device__ __forceinline__ f32x4 split_mfma16(f32x4 afrag, h4 bh, h4 bl, f32x4 c) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  const h4 ah = __builtin_bit_cast(h4, f32x2_t{afrag[0], afrag[1]});
  const h4 al = __builtin_bit_cast(h4, f32x2_t{afrag[2], afrag[3]});
  c = __builtin_amdgcn_mfma_f32_16x16x16f16(al, bh, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bl, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bh, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 fused_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Split-fp16 GEMM mode (CIPS3D_GEMM_SPLIT): fp32-equivalent products at the fp16 matrix rate.  Every operand is the
// unevaluated sum of two fp16 numbers, x = hi + lo (hi = fp16(x), lo = fp16(x - hi): 22 significant bits in the 4 bytes
// of an fp32); a product is accumulated in fp32 as the three exact fp16 x fp16 products w_lo x_hi + w_hi x_lo + w_hi x_hi
// on v_mfma_f32_16x16x32_f16 (3 x 16 cycles per 16x16x32 block against 8 x 32 cycles of v_mfma_f32_16x16x4_f32).  The
// dropped term and the representation error are ~2^-22 relative per product, below the rounding fp32 accumulation makes
// on the sum (tools/split_probe.py).  Modulated weights (|wm| <= 1 after demodulation) are pre-scaled by
// kSplitScale = 2^8 into fp16's normal range and split by the modulate kernel; activations are split in registers after
// the LDS read; the epilogue undoes the scale exactly.
constexpr float kSplitScale = 256.f, kSplitInv = 1.f / 256.f;
__device__ __forceinline__ void split8(const float (&v)[8], h8& hi, h8& lo) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  unsigned h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) cips3d_split_pair(v[2 * p], v[2 * p + 1], h[p], l[p]);
  hi = __builtin_bit_cast(h8, u32x4_t{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(h8, u32x4_t{l[0], l[1], l[2], l[3]});
}

// bf16 compute mode of the GEMMs (BASELINE config 3: decoder in bf16 with fp32 accumulate).  Storage and data movement
// stay fp32 and identical; only the fragments are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) in registers and fed to
// v_mfma_f32_16x16x16_bf16.  The packed A layout gives lane (o, q) the channels 16kq + 4e + q (e = 0..3) of row o and the
// B-fragment reads give lane (n, q) the same channels of pixel n, so element e of both operands is MFMA k = 4q + e:
// one bf16 MFMA replaces the four fp32 MFMAs of a k-group.
// Two-wide vector conversions compile to one v_cvt_pk_bf16_f32 per pair AND keep the compiler's hazard bookkeeping
// (an inline-asm cvt feeding an MFMA loses the required wait state between the VALU write and the MFMA read: measured
// wrong results).
__device__ __forceinline__ s16x4 pack_bf16(float a0, float a1, float a2, float a3) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t lo = __builtin_convertvector(f32x2_t{a0, a1}, bf16x2_t);
  const bf16x2_t hi = __builtin_convertvector(f32x2_t{a2, a3}, bf16x2_t);
  return __builtin_bit_cast(s16x4, u32x2_t{__builtin_bit_cast(unsigned, lo), __builtin_bit_cast(unsigned, hi)});
}

// s_waitcnt immediate that waits until at most n vector-memory operations of this wave are outstanding
// (gfx9 encoding: vmcnt = imm[3:0] | imm[15:14] << 4; expcnt / lgkmcnt fields left at "no wait")
__device__ __forceinline__ constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }
