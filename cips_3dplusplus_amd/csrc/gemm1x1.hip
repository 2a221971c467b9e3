// The 1x1 ModulatedConv2d of the StyleGAN2-style decoder of CIPS-3D++ on gfx950 (reference models/model_v3.py:218-341).
//
//   cips3d_modconv1x1        the 1x1 ModulatedConv2d as a per-sample GEMM  out[o][n] = sum_i wm[o][i] x[i][n]
//                            on v_mfma_f32_32x32x2_f32, NoiseInjection + FusedLeakyReLU fused in the epilogue
//   cips3d_modconv1x1_actbwd the same GEMM on the transposed weights with the activation backward in the epilogue
//   cips3d_up2_fir_act       k=1 up-sampling conv = low-res GEMM followed by upfirdn2d(up=2, pad=(2,1)) of
//                            its result (pinned by tests/test_oracle_golden.py), fused with
//                            noise + bias + leaky-ReLU
//
// Rooflines: 64^2 / 128^2 layers are MFMA-bound (2*Cin*Cout flop per pixel against (Cin+Cout)*4 B); >= 256^2 layers and
// the FIR up-sampler are HBM-bound: every kernel reads its input once and writes its output once with >= 128-byte row
// segments.

#include "up2_fir.h"

namespace {

// ------------------------------------------------------------------------------------------------
// 1x1 modulated conv as GEMM on v_mfma_f32_16x16x4_f32.  Workgroup tile BM x BN, BK-deep stages through a
// 2-slot LDS ring filled by LDS-DMA (A: packed fragments, linear copy; B: BK rows of BN pixels).
// A wave owns WM o-tiles (16 rows each) x 64 pixels.  Its four 16-pixel column tiles are INTERLEAVED over
// the pixels (lane j of column tile c holds pixel 4*j + c), so ONE ds_read_b128 per k-step delivers the
// B fragments of all four column tiles (a per-MFMA ds_read_b32 made the kernel LDS-issue bound at one
// wave per SIMD), and the epilogue stores 16 bytes per lane.
// ------------------------------------------------------------------------------------------------
struct GemmArgs {
  const float* x; const float* wmp; float* out;
  int B, Cin, Cout; int64_t HW;
  int epilogue; const float* noise; int64_t noise_bstride; const float* noise_w; const float* bias;
  int bf16;                 // GEMM mode: 0 exact fp32, 1 bf16 operands, 2 split-fp16 (pre-split weights)
  int out_bf16;             // the output is stored as bf16 (CIPS3D_Y_BF16: the low-resolution GEMM of an up-sampling stage)
  // optional: the ToRGB that follows this conv, folded into the epilogue.  Every workgroup writes the partial sums of its
  // BM output rows, rgb_part[blockIdx.y][b][3][HW]; cips3d_torgb_reduce adds the row blocks (and layers) in a fixed order.
  const float* rgb_w;       // plain [B][3][Cout] modulated ToRGB weights (no demodulation)
  float* rgb_part;          // [Cout/BM][B][3][HW]
  // range tracking (cips3d_range): split mode splits x * 2^-e, e from the measured maximum of x; any mode records max |out|
  const float* x_amax;      // [B][CIPS3D_AMAX_FLOATS] or NULL (e = 0)
  float* out_amax;          // [B][CIPS3D_AMAX_FLOATS] or NULL
  // activation-backward epilogue (ACTBWD instantiations, cips3d_modconv1x1_actbwd): see cips3d_actbwd in the public header
  cips3d_actbwd ab;
};

// MODE: 0 exact fp32 MFMA, 1 bf16 operands (CIPS3D_GEMM_BF16), 2 split-fp16 (CIPS3D_GEMM_SPLIT; A pre-split by the modulate kernel)
// ACTBWD: the data-gradient GEMM of the one-call decoder backward.  Its result is the gradient w.r.t. the OUTPUT of the
// previous StyledConv; the epilogue turns it into the gradient w.r.t. that layer's pre-activation -- adds the contribution of
// the ToRGB that read the same tensor (a rank-3 update), applies the leaky-ReLU derivative from the stored output's sign --
// and reduces the bias / noise-weight / ToRGB-weight gradients of its rows (backward.hip: act_bwd_kernel + torgb_bwd_kernel,
// which read and wrote the whole tensor once more each).
template <int WM, int WGM, int WGN, int BK, int NS, int MODE = 0, bool ACTBWD = false>
// (the ACTBWD forms with a 2-slot ring -- short contractions, HBM-bound -- are compiled for two 8-wave workgroups per CU:
// 128 VGPRs, a handful of spills outside the K loop)
__global__ void __launch_bounds__(64 * WGM * WGN, (ACTBWD && NS == 2 && BK == 32 && WGM * WGN == 8) ? 4 : 1) modconv1x1_kernel(GemmArgs a) {
  constexpr bool BF16 = MODE == 1;
  constexpr bool SPLIT = MODE == 2;
  constexpr int NW = WGM * WGN;               // waves per workgroup: 8 = two per SIMD, so one wave's DMA issue,
                                              // waits and fragment reads run under the partner's MFMAs
  constexpr int BM = 16 * WM * WGM, BN = 64 * WGN;
  constexpr int A_STAGE = BM * BK;            // floats
  constexpr int B_STAGE = BK * BN;
  constexpr int STAGE = A_STAGE + B_STAGE;
  constexpr int A_PIECES = A_STAGE / 256;     // 1-KiB pieces
  constexpr int B_PIECES = B_STAGE / 256;
  constexpr int PIECES = A_PIECES + B_PIECES;
  constexpr int PW = PIECES / NW;             // LDS-DMA instructions per wave per stage
  constexpr int KQ = BK / 16;                 // A pieces per o-tile per stage
  static_assert(NW == 4 || NW == 8, "four or eight waves");
  static_assert(PIECES % NW == 0, "every wave must issue the same number of DMA pieces (counted vmcnt)");
  static_assert(NS >= 2 && NS <= 4, "ring depth");
  // NS-slot ring, NS-1 stages in flight: the LDS-DMA lands ~1.1 us after issue, so ONE 24 KB stage in
  // flight caps a CU at ~22 GB/s (Little's law) -- below what the MFMA pipe consumes (measured: 63 % of
  // peak at any tile shape).  Waits are counted (vmcnt(N) leaves the younger stages in flight) and the
  // barrier is the raw s_barrier: __syncthreads() would drain every outstanding DMA.
  __shared__ __attribute__((aligned(16))) float lds[NS * STAGE];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int wm_i = wave / WGN, wn_i = wave % WGN;
  const int b = blockIdx.z;
  const int m0 = blockIdx.y * BM;
  // split mode: the activations are split as x * kx, kx = 2^-e with max|x| 2^-e in [2^14, 2^15) (the measured maximum of x;
  // common.h, cips3d_range); the accumulators come back with kin = 2^-8 2^e
  float kx = 1.f, kin = kSplitInv;
  if constexpr (SPLIT) {
    if (a.x_amax) {
      const int e = cips3d_split_exp(cips3d_amax_load(a.x_amax + b * CIPS3D_AMAX_FLOATS));
      kx = cips3d_uniform(cips3d_pow2(-e));
      kin = cips3d_uniform(kSplitInv * cips3d_pow2(e));
    }
  }
  // per-lane index arithmetic in 32 bits (the host refuses max(Cin, Cout) * HW >= 2^31); 64-bit products only in the
  // workgroup-uniform sample bases
  const int n0 = blockIdx.x * BN;
  const int HW = (int)a.HW;
  const int K = a.Cin;
  const int nstage = K / BK;
  const float* xb = a.x + (int64_t)b * K * HW;
  const float* ab = a.wmp + (int64_t)b * a.Cout * K;   // packed: [ot][kq][256]

  auto stage_load = [&](int st) {
    float* dstA = lds + (st % NS) * STAGE;
    float* dstB = dstA + A_STAGE;
    const int k0 = st * BK;
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int piece = j * NW + wave;
      if (piece < A_PIECES) {
        const int ot_l = piece / KQ, kq_l = piece % KQ;
        const float* src = ab + ((((m0 >> 4) + ot_l) * (K >> 4) + (k0 >> 4) + kq_l) * 256 + lane * 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(dstA + piece * 256), 16, 0, 0);
      } else {
        const int pb = piece - A_PIECES;
        const int f = pb * 256 + lane * 4;
        const int row = f / BN, col = f % BN;
        int n = n0 + col;
        if (n > HW - 4) n = HW - 4;                       // clamp: those columns are never stored
        const float* src = xb + ((k0 + row) * HW + n);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(dstB + pb * 256), 16, 0, 0);
      }
    }
  };

  const int q = lane >> 4, jn = lane & 15;
  // epilogue operands first (registers, ordinary loads, consumed only after the main loop)
  const int ncol = n0 + wn_i * 64 + jn * 4;                // this lane's 4 consecutive pixels
  f32x4 nz4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 bias4[WM];
  f32x4 wrgb[WM][3];
  float nw = 0.f;
  f32x4 aby[ACTBWD ? WM : 1][4], abg[3];                     // ACTBWD: the stored output's rows, the ToRGB gradient's pixels
  // With a 2-slot ring the first wait of the loop is vmcnt(0) anyway, so the operand loads go out right AFTER the first
  // stage's DMA (one exposed round trip less per launch).  Deeper rings count their waits in DMA pieces only: there the
  // operands are retired before the prologue.
  constexpr bool OPS_AFTER_PROLOGUE = NS == 2;
  auto load_ops = [&]() {
    if (a.epilogue == 1) {
      if (a.noise && a.noise_w && ncol < HW) {
        nz4 = *reinterpret_cast<const f32x4*>(a.noise + (int64_t)b * a.noise_bstride + ncol);
        nw = a.noise_w[0];
      }
#pragma unroll
      for (int i = 0; i < WM; ++i)
        bias4[i] = *reinterpret_cast<const f32x4*>(a.bias + m0 + (wm_i * WM + i) * 16 + 4 * q);
    }
    if constexpr (ACTBWD) {
      const bool ok = ncol < HW;
      const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
      nz4 = (a.ab.d_noise_w && ok) ? *reinterpret_cast<const f32x4*>(a.noise + (int64_t)b * a.noise_bstride + ncol) : z4;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        abg[ch] = (a.ab.drgb && ok) ? *reinterpret_cast<const f32x4*>(a.ab.drgb + ((int64_t)b * 3 + ch) * HW + ncol) : z4;
#pragma unroll
      for (int i = 0; i < WM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          aby[i][r] = ok ? *reinterpret_cast<const f32x4*>(a.ab.y + ((int64_t)b * a.Cout + m0 + (wm_i * WM + i) * 16 + 4 * q + r) * HW + ncol) : z4;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          wrgb[i][ch] = a.ab.drgb ? *reinterpret_cast<const f32x4*>(a.ab.rgb_w + ((int64_t)b * 3 + ch) * a.Cout + m0 + (wm_i * WM + i) * 16 + 4 * q) : z4;
      }
    }
    if (a.rgb_part) {        // the folded ToRGB's weights of this lane's rows (an epilogue-time load would be an exposed round trip)
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          wrgb[i][ch] = *reinterpret_cast<const f32x4*>(a.rgb_w + (int64_t)b * 3 * a.Cout + ch * a.Cout + m0 + (wm_i * WM + i) * 16 + 4 * q);
    }
  };
  if (!OPS_AFTER_PROLOGUE) {
    load_ops();
    // retire them now so that the counted waits below see DMA pieces only
    if (a.epilogue == 1 || ACTBWD) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }

  f32x4 acc[WM][4];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: NS-1 stages in flight
#pragma unroll
  for (int s0 = 0; s0 < NS - 1; ++s0)
    if (s0 < nstage) stage_load(s0);
  if (OPS_AFTER_PROLOGUE) load_ops();

  for (int st = 0; st < nstage; ++st) {
    // stage st must have landed; stages st+1 .. st+NS-2 (as far as they exist) stay in flight
    int younger = nstage - 1 - st;
    if (younger > NS - 2) younger = NS - 2;
    if (younger >= 2) __builtin_amdgcn_s_waitcnt(vmcnt_imm(2 * PW));
    else if (younger == 1) __builtin_amdgcn_s_waitcnt(vmcnt_imm(PW));
    else __builtin_amdgcn_s_waitcnt(vmcnt_imm(0));
    __builtin_amdgcn_s_barrier();      // every wave's pieces of stage st landed; everyone is done with stage st-1
    if (st + NS - 1 < nstage) stage_load(st + NS - 1);    // refills the slot stage st-1 was read from
    const float* sA = lds + (st % NS) * STAGE;
    const float* sB = sA + A_STAGE + wn_i * 64 + jn * 4;
    // Issue every fragment read of the stage first (12 x ds_read_b128 for BK = 32, WM = 2), then run the MFMAs
    // back to back behind counted lgkmcnt waits: with one wave per SIMD a read-then-wait per MFMA group
    // leaves the matrix pipe idle for an LDS round trip every 16 MFMAs (measured 64 % busy).
    if constexpr (SPLIT) {
      // 32-channel blocks: hi / lo A fragments (pre-split, two 1-KiB pieces per o-tile and block) and eight B rows
      // (channel 32 kb + 8 q + j = fragment element j of lane quarter q), split into hi / lo fragments in registers.
      constexpr int KB = BK / 32;
      static_assert(BK % 32 == 0, "split mode pairs the 16-channel groups");
      h8 ah[KB][WM], al[KB][WM];
      f32x4 b8[KB][8];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int i = 0; i < WM; ++i) {
          ah[kb][i] = *reinterpret_cast<const h8*>(sA + ((wm_i * WM + i) * KQ + 2 * kb) * 256 + lane * 4);
          al[kb][i] = *reinterpret_cast<const h8*>(sA + ((wm_i * WM + i) * KQ + 2 * kb + 1) * 256 + lane * 4);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) b8[kb][j] = *reinterpret_cast<const f32x4*>(sB + (kb * 32 + 8 * q + j) * BN);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v8[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v8[j] = b8[kb][j][c] * kx;
          h8 bh, bl;
          split8(v8, bh, bl);
#pragma unroll
          for (int i = 0; i < WM; ++i) {
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[kb][i], bh, acc[i][c], 0, 0, 0);
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[kb][i], bl, acc[i][c], 0, 0, 0);
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[kb][i], bh, acc[i][c], 0, 0, 0);
          }
        }
    } else {
    f32x4 afr[KQ][WM], bfr[KQ][4];
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq) {
#pragma unroll
      for (int i = 0; i < WM; ++i)
        afr[kq][i] = *reinterpret_cast<const f32x4*>(sA + ((wm_i * WM + i) * KQ + kq) * 256 + lane * 4);
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4)   // k row 16*kq + 4*j4 + q, pixels 4*jn..4*jn+3 = B fragments of the 4 column tiles
        bfr[kq][j4] = *reinterpret_cast<const f32x4*>(sB + (kq * 16 + j4 * 4 + q) * BN);
    }
    __builtin_amdgcn_sched_barrier(0);   // hipcc otherwise sinks each read back in front of its first MFMA
    if (BF16) {
#pragma unroll
      for (int kq = 0; kq < KQ; ++kq) {
        s16x4 ah[WM], bh[4];
#pragma unroll
        for (int i = 0; i < WM; ++i) ah[i] = pack_bf16(afr[kq][i][0], afr[kq][i][1], afr[kq][i][2], afr[kq][i][3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) bh[c] = pack_bf16(bfr[kq][0][c], bfr[kq][1][c], bfr[kq][2][c], bfr[kq][3][c]);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah[i], bh[c], acc[i][c], 0, 0, 0);
      }
    } else {
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4)
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[kq][i][j4], bfr[kq][j4][c], acc[i][c], 0, 0, 0);
    }
    }
    // all LDS reads of this stage retired before the slot can be refilled after the next barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- epilogue.  D layout: acc[i][c][r] = out[o = obase + 4*q + r][pixel ncol + c]
  const bool col_ok = ncol < HW;
  if (!ACTBWD && !col_ok && !a.rgb_part && !a.out_amax) return;
  float* ob = a.out + (int64_t)b * a.Cout * HW + ncol;
  float mx = 0.f;
  float rs[ACTBWD ? WM : 1][4][5];             // ACTBWD row sums of this lane's 4 pixels: bias, noise weight, ToRGB weight x 3
  float prgb[3][4];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int c = 0; c < 4; ++c) prgb[ch][c] = 0.f;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int obase = m0 + (wm_i * WM + i) * 16 + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      if constexpr (SPLIT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] *= kin;                 // exact: the weights carried 2^8, the activations 2^-e
      }
      if (a.epilogue == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = lrelu02(fmaf(nw, nz4[c], v[c]) + bias4[i][r]) * 1.41421356237309515f;
      }
      if constexpr (ACTBWD) {
        const f32x4 yv = aby[i][r];
        float sb = 0.f, sn = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float g = v[c];
          g = fmaf(wrgb[i][0][r], abg[0][c], g);
          g = fmaf(wrgb[i][1][r], abg[1][c], g);
          g = fmaf(wrgb[i][2][r], abg[2][c], g);
          g *= yv[c] > 0.f ? 1.41421356237309515f : 0.2f * 1.41421356237309515f;
          if (!col_ok) g = 0.f;                      // (clamped columns past the image)
          v[c] = g;
          sb += g;
          sn = fmaf(g, nz4[c], sn);
          s0 = fmaf(abg[0][c], yv[c], s0); s1 = fmaf(abg[1][c], yv[c], s1); s2 = fmaf(abg[2][c], yv[c], s2);
        }
        rs[i][r][0] = sb; rs[i][r][1] = sn; rs[i][r][2] = s0; rs[i][r][3] = s1; rs[i][r][4] = s2;
      }
      if (col_ok) {
        mx = fmaxf(fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))), mx);
        if (a.out_bf16)
          cips3d_store_wt8(reinterpret_cast<unsigned short*>(a.out) + (int64_t)b * a.Cout * HW + ncol + (obase + r) * HW,
                           pack_bf16(v[0], v[1], v[2], v[3]));
        else
          cips3d_store_wt16(ob + (obase + r) * HW, v);                // (write-through: common.h)
      }
      if (a.rgb_part) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float wc = wrgb[i][ch][r];
#pragma unroll
          for (int c = 0; c < 4; ++c) prgb[ch][c] = fmaf(wc, v[c], prgb[ch][c]);
        }
      }
    }
  }
  if (a.out_amax) {        // the workgroup's largest |out| raises one slot of the sample's amax array (cips3d_range); the LDS
    // words live in the ring slot the last K stage did not use (a __shared__ array of their own would move the ring)
    const float m = cips3d_workgroup_max(mx, lds + (nstage % NS) * STAGE, wave, lane, NW);
    if (tid == 0) cips3d_amax_raise_if(a.out_amax + b * CIPS3D_AMAX_FLOATS, m, blockIdx.y * gridDim.x + blockIdx.x);
  }
  if constexpr (ACTBWD) {
    // row sums: over the 16 lanes of a DPP row (the 64 pixels of this wave), over the WGN wave columns through LDS, then
    // ONE atomic per (row, quantity) and workgroup, issued as contiguous wave-wide instructions
    __syncthreads();                                  // (every wave is past its last fragment read: the ring is free)
    float* s_rs = lds;                                // [5][WGN][BM]
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          const float t = cips3d_row16_sum(rs[i][r][k]);
          if (jn == 0) s_rs[(k * WGN + wn_i) * BM + (wm_i * WM + i) * 16 + 4 * q + r] = t;
        }
    __syncthreads();
    for (int idx = tid; idx < 5 * BM; idx += 64 * NW) {
      const int k = idx / BM, row = idx % BM;
      float t = 0.f;
#pragma unroll
      for (int w = 0; w < WGN; ++w) t += s_rs[(k * WGN + w) * BM + row];
      const int slot = a.ab.slots > 1 ? (int)(blockIdx.x & (a.ab.slots - 1)) : 0;
      float* dst = k == 0 ? a.ab.d_bias : (k == 1 ? a.ab.d_noise_w : (a.ab.d_rgb_w ? a.ab.d_rgb_w + ((int64_t)b * 3 + (k - 2)) * a.Cout : nullptr));
      if (dst) unsafeAtomicAdd(dst + (int64_t)slot * (k < 2 ? a.ab.slot_stride : a.ab.rgb_slot_stride) + m0 + row, t);
    }
    return;
  }
  if (!a.rgb_part) return;
  // ---- ToRGB partial of this workgroup's BM rows: over the 4 lane quarters by shuffles, over the WGM wave rows through
  // LDS (the ring is free: every wave passed the last stage's lgkmcnt(0) and meets at the barrier below)
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float v = prgb[ch][c];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      prgb[ch][c] = v;
    }
  __syncthreads();
  float* s_red = lds;                                   // [WGM][3][BN]
  const int nloc = wn_i * 64 + jn * 4;
  if (q == 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      *reinterpret_cast<f32x4*>(s_red + (wm_i * 3 + ch) * BN + nloc) = f32x4{prgb[ch][0], prgb[ch][1], prgb[ch][2], prgb[ch][3]};
  }
  __syncthreads();
  if (wm_i == 0 && q < 3 && col_ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < WGM; ++m) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(s_red + (m * 3 + q) * BN + nloc);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] += t[c];
    }
    *reinterpret_cast<f32x4*>(a.rgb_part + ((int64_t)blockIdx.y * a.B + b) * 3 * HW + (q * HW + ncol)) = v;
  }
}

template <int WM, int WGM, int WGN, int BK, int NS>
int launch_gemm_actbwd(const GemmArgs& a, hipStream_t st) {
  constexpr int BM = 16 * WM * WGM, BN = 64 * WGN;
  dim3 grid((unsigned)ceil_div<int64_t>(a.HW, BN), (unsigned)(a.Cout / BM), (unsigned)a.B);
  if (a.bf16 == 2) hipLaunchKernelGGL((modconv1x1_kernel<WM, WGM, WGN, BK, NS, 2, true>), grid, dim3(64 * WGM * WGN), 0, st, a);
  else hipLaunchKernelGGL((modconv1x1_kernel<WM, WGM, WGN, BK, NS, 0, true>), grid, dim3(64 * WGM * WGN), 0, st, a);
  return cips3d_launch_status();
}

template <int WM, int WGM, int WGN, int BK, int NS>
int launch_gemm(const GemmArgs& a, hipStream_t st) {
  constexpr int BM = 16 * WM * WGM, BN = 64 * WGN;
  dim3 grid((unsigned)ceil_div<int64_t>(a.HW, BN), (unsigned)(a.Cout / BM), (unsigned)a.B);
  if (a.bf16 == 2) hipLaunchKernelGGL((modconv1x1_kernel<WM, WGM, WGN, BK, NS, 2>), grid, dim3(64 * WGM * WGN), 0, st, a);
  else if (a.bf16) hipLaunchKernelGGL((modconv1x1_kernel<WM, WGM, WGN, BK, NS, 1>), grid, dim3(64 * WGM * WGN), 0, st, a);
  else hipLaunchKernelGGL((modconv1x1_kernel<WM, WGM, WGN, BK, NS, 0>), grid, dim3(64 * WGM * WGN), 0, st, a);
  return cips3d_launch_status();
}

// ------------------------------------------------------------------------------------------------
// 2x polyphase FIR up-sampler (upfirdn2d up=2, pad=(2,1), 4x4 taps) + noise + bias + leaky-ReLU.
// Each thread produces 4 consecutive output pixels of one row (16-byte store).
// ------------------------------------------------------------------------------------------------
// (Why the second half of a k=1 up-sampling conv sits in its GEMM's file and not in decoder_ops.hip: before it inlines, hipcc
// propagates the constants and ranges of a static helper's arguments over all the helper's call sites in the translation
// unit.  As the only caller of cips3d_workgroup_max in its file this kernel has the helper specialised to its own LDS array
// and thread-id ranges first and comes out with another address computation in front of the reduction's ds_write; beside the
// GEMM's calls it keeps the instructions it always had -- tools/isa_same.py.)
__device__ __forceinline__ void up2_block(const float* __restrict__ src, int H, int W, int iy, int qx,
                                          const float (&kf)[16], float (&o)[2][4]) {
  float v[3][4];
  up2_load(src, H, W, iy, qx, v);
  up2_fir(v, kf, o);
}

__global__ void __launch_bounds__(256) up2_fir_act_kernel(const float* __restrict__ y_lo, const float* __restrict__ fir,
                                                          float* __restrict__ out, int B, int C, int H, int W,
                                                          const float* __restrict__ noise, int64_t noise_bstride,
                                                          const float* __restrict__ nwp, const float* __restrict__ bias,
                                                          float* __restrict__ out_amax) {
  const float noise_w = (noise && nwp) ? nwp[0] : 0.f;
  float mx = 0.f;      // out_amax: the largest |out| of the sample this thread is in (a grid-stride loop may cross samples)
  int mx_b = -1;
  float kf[16];   // flipped taps: kf[ky][kx] = fir[3-ky][3-kx]
#pragma unroll
  for (int i = 0; i < 16; ++i) kf[i] = fir[15 - i];
  const int OW = 2 * W;
  const int qw = W / 2;                                    // 4-pixel output quads per row
  const int64_t total = (int64_t)B * C * H * qw;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int qx = (int)(t % qw); t /= qw;
    const int iy = (int)(t % H); t /= H;
    const int c = (int)(t % C);
    const int b = (int)(t / C);
    const float* src = y_lo + ((int64_t)b * C + c) * H * W;
    const float bs = bias[c];
    if (out_amax && b != mx_b) {        // (rare: at most B - 1 times per thread)
      if (mx_b >= 0) cips3d_amax_raise(out_amax + mx_b * CIPS3D_AMAX_FLOATS, mx, blockIdx.x);
      mx = 0.f;
      mx_b = b;
    }
    float o[2][4];
    up2_block(src, H, W, iy, qx, kf, o);
    float* dst = out + (((int64_t)b * C + c) * 2 * H + 2 * iy) * OW + 4 * qx;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      float4 nz = make_float4(0.f, 0.f, 0.f, 0.f);
      if (noise) nz = *reinterpret_cast<const float4*>(noise + (int64_t)b * noise_bstride + (int64_t)(2 * iy + py) * OW + 4 * qx);
      float4 r;
      r.x = lrelu02(fmaf(noise_w, nz.x, o[py][0]) + bs) * 1.41421356237309515f;
      r.y = lrelu02(fmaf(noise_w, nz.y, o[py][1]) + bs) * 1.41421356237309515f;
      r.z = lrelu02(fmaf(noise_w, nz.z, o[py][2]) + bs) * 1.41421356237309515f;
      r.w = lrelu02(fmaf(noise_w, nz.w, o[py][3]) + bs) * 1.41421356237309515f;
      cips3d_store_wt16(dst + (int64_t)py * OW, r);
      mx = fmaxf(fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fmaxf(fabsf(r.z), fabsf(r.w))), mx);
    }
  }
  if (out_amax) {
    // One atomic per WORKGROUP, and only when it would raise the slot (the slot's current value is peeked first: 16 384
    // workgroups raising 8 lines unconditionally cost more than the absmax pass this replaces).  Lanes that ended in another
    // sample than the workgroup's first (a straddling workgroup: at most B - 1 of them) raise theirs directly.
    __shared__ float s_mx[16];
    __shared__ int s_b;
    if (threadIdx.x == 0) s_b = mx_b;
    __syncthreads();
    const int b0 = s_b;
    if (mx_b >= 0 && mx_b != b0) cips3d_amax_raise(out_amax + mx_b * CIPS3D_AMAX_FLOATS, mx, blockIdx.x);
    const float m = cips3d_workgroup_max(mx_b == b0 ? mx : 0.f, s_mx, threadIdx.x >> 6, threadIdx.x & 63, 4);
    if (threadIdx.x == 0 && b0 >= 0) {
      float* slots = out_amax + b0 * CIPS3D_AMAX_FLOATS;
      cips3d_amax_raise_if(slots, m, blockIdx.x, cips3d_amax_peek(slots, blockIdx.x));
    }
  }
}

}  // namespace

extern "C" int cips3d_modconv1x1_supported(int Cin, int Cout, int64_t HW) {
  // (the kernel keeps intra-sample offsets in 32 bits)
  return (Cin % 32 == 0) && (Cout % 32 == 0) && (HW % 4 == 0) && HW >= 4 &&
         (int64_t)(Cin > Cout ? Cin : Cout) * HW + 256 < ((int64_t)1 << 31);
}

extern "C" int cips3d_modconv1x1(const float* x, const float* wm, float* out, int B, int Cin, int Cout, int64_t HW,
                                 int epilogue, const float* noise, int64_t noise_bstride, const float* noise_w,
                                 const float* bias, const cips3d_range* rg, void* stream) {
  return cips3d_modconv1x1_torgb(x, wm, out, B, Cin, Cout, HW, epilogue, noise, noise_bstride, noise_w, bias, nullptr,
                                 nullptr, nullptr, rg, stream);
}

// The tile of a 1x1 GEMM launch, forward (cips3d_modconv1x1_torgb) or activation-backward (cips3d_modconv1x1_actbwd):
// BM = 16 WM WGM rows (= one row block of the ToRGB partials) x BN = 64 WGN pixels, K stages of BK in a ring of NS slots.
struct GemmTile { int WM, WGM, WGN, BK, NS; };

// small_grid_allowed: the forward GEMM without a ToRGB fold only (the fold's slots are 64 rows or more at these widths)
static GemmTile gemm_tile(int B, int Cin, int Cout, int64_t HW, bool small_grid_allowed) {
  if (Cout >= 256 && Cout % 64 == 0) {
    // 64 x 128 tiles, 8 waves.  A grid that covers at most half of the 256 CUs (the 512 -> 256 low-res GEMM at 64^2: 128 tiles)
    // runs on 32 x 128 tiles of 4 waves instead
    const int64_t tiles = B > 0 && HW > 0 ? (int64_t)B * (Cout / 64) * ceil_div<int64_t>(HW, 128) : 0;
    if (small_grid_allowed && tiles <= 128) return {1, 2, 2, 32, 4};
    // 64-deep stages (half as many stage barriers: 705.9 -> 703.4 us per 1024^2 view, A/B on one box) when K allows
    // ... for a grid of at most ONE workgroup per CU (the 64^2 layers of a single view: 256 tiles).  A larger grid (batch 2 and
    // up: the inversion step) whose shape does not admit the 128-row tile below runs 32-deep stages in a 48 KB ring instead: two
    // workgroups share a CU and one's prologue / epilogue -- a third of a launch, with the L2 port idle -- runs under the other's
    // K loop (inversion step +3.4 %, same box)
    if (tiles <= 256 && Cin % 64 == 0) return {1, 4, 2, 64, 2};
    // a grid of more than one 64 x 128 tile per CU (batch 2 and up: the inversion step): 128 x 128 tiles, 64-deep stages -- half
    // the operand bytes per flop through the L2 port and one workgroup per CU again; the ToRGB partials then come in 128-row
    // blocks.  Inversion step, same box x3: 341.6-343.2 -> 348.8-349.4 steps/s with this form in the forward and the data-gradient
    // GEMM (32-deep in 3 / 4 slots: 347.1-348.7 / 346.9-347.7)
    if (tiles > 256 && Cout % 128 == 0 && Cin % 64 == 0) return {2, 4, 2, 64, 2};
    return {1, 4, 2, 32, 2};
  }
  // Short contractions (K <= 128: the decoder's 128 / 64 / 32-channel layers at 256^2 and above) are HBM-bound streams with
  // two to four K stages: a 2-slot ring (half the LDS) lets a second workgroup share the CU and cover the first one's
  // epilogue loads and stores
  const int ns = Cin <= 128 && Cout < 256 ? 2 : 4;
  if (Cout == 128) return {1, 8, 1, 32, ns};      // all 128 rows: x read once
  if (Cout == 64) return {1, 4, 2, 32, ns};       // 64 x 128
  return {1, 2, 2, 32, ns};                       // 32 x 128 (any Cout % 32 == 0)
}

// row blocks of the ToRGB partial sums: one rgb_part slot each
static int row_blocks(const GemmTile& t, int Cout) { return Cout > 0 ? Cout / (16 * t.WM * t.WGM) : 0; }

extern "C" int cips3d_modconv1x1_torgb_blocks(int B, int Cin, int Cout, int64_t HW) {
  return row_blocks(gemm_tile(B, Cin, Cout, HW, false), Cout);
}

static int launch_gemm_tile(const GemmTile& t, bool actbwd, const GemmArgs& a, hipStream_t st) {
#define GEMM_TILE_CASE(wm, wgm, wgn, bk, ns)                                                    \
  if (t.WM == wm && t.WGM == wgm && t.WGN == wgn && t.BK == bk && t.NS == ns)                   \
    return actbwd ? launch_gemm_actbwd<wm, wgm, wgn, bk, ns>(a, st) : launch_gemm<wm, wgm, wgn, bk, ns>(a, st);
  GEMM_TILE_CASE(1, 2, 2, 32, 4)
  GEMM_TILE_CASE(1, 4, 2, 64, 2)
  GEMM_TILE_CASE(2, 4, 2, 64, 2)
  GEMM_TILE_CASE(1, 4, 2, 32, 2)
  GEMM_TILE_CASE(1, 8, 1, 32, 2)
  GEMM_TILE_CASE(1, 2, 2, 32, 2)
  GEMM_TILE_CASE(1, 8, 1, 32, 4)
  GEMM_TILE_CASE(1, 4, 2, 32, 4)
#undef GEMM_TILE_CASE
  return CIPS3D_E_UNSUPP;      // (not reached: gemm_tile names only the tiles above)
}

extern "C" int cips3d_modconv1x1_torgb(const float* x, const float* wm, float* out, int B, int Cin, int Cout, int64_t HW,
                                       int epilogue, const float* noise, int64_t noise_bstride, const float* noise_w,
                                       const float* bias, const float* rgb_w, float* rgb_part, int* n_row_blocks,
                                       const cips3d_range* rg, void* stream) {
  if ((rgb_w == nullptr) != (rgb_part == nullptr)) return CIPS3D_E_BADARG;
  const GemmTile tile = gemm_tile(B, Cin, Cout, HW, !rgb_part);
  if (n_row_blocks) *n_row_blocks = row_blocks(tile, Cout);
  if (!x || !wm || !out || B < 0 || Cin <= 0 || Cout <= 0 || HW <= 0) return CIPS3D_E_BADARG;
  if ((epilogue & CIPS3D_GEMM_BF16) && (epilogue & CIPS3D_GEMM_SPLIT)) return CIPS3D_E_BADARG;
  const int bf16 = (epilogue & CIPS3D_GEMM_BF16) ? 1 : (epilogue & CIPS3D_GEMM_SPLIT) ? 2 : 0;
  const int out_bf16 = (epilogue & CIPS3D_Y_BF16) ? 1 : 0;
  epilogue &= ~(CIPS3D_GEMM_BF16 | CIPS3D_Y_BF16 | CIPS3D_GEMM_SPLIT);
  if (epilogue != 0 && epilogue != 1) return CIPS3D_E_BADARG;
  if (out_bf16 && (epilogue != 0 || rgb_part)) return CIPS3D_E_BADARG;     // bf16 storage is for the pre-FIR GEMM result only
  if (epilogue == 1 && !bias) return CIPS3D_E_BADARG;
  if (!cips3d_modconv1x1_supported(Cin, Cout, HW)) return CIPS3D_E_UNSUPP;
  if (B == 0) return 0;
  GemmArgs a{x, wm, out, B, Cin, Cout, HW, epilogue, noise, noise_bstride, noise_w, bias, bf16, out_bf16, rgb_w, rgb_part,
             rg ? rg->x_amax : nullptr, rg ? rg->out_amax : nullptr, cips3d_actbwd{}};
  return launch_gemm_tile(tile, false, a, as_stream(stream));
}

extern "C" int cips3d_modconv1x1_actbwd(const float* g, const float* wm_t, float* dpre, int B, int Cin, int Cout, int64_t HW,
                                        int flags, const cips3d_actbwd* ab, const float* noise, int64_t noise_bstride,
                                        const cips3d_range* rg, void* stream) {
  if (!g || !wm_t || !dpre || !ab || !ab->y || B < 0 || Cin <= 0 || Cout <= 0 || HW <= 0) return CIPS3D_E_BADARG;
  if (flags & ~CIPS3D_GEMM_SPLIT) return CIPS3D_E_BADARG;
  if ((ab->drgb == nullptr) != (ab->rgb_w == nullptr) || (ab->d_rgb_w && !ab->drgb)) return CIPS3D_E_BADARG;
  if (ab->d_noise_w && !noise) return CIPS3D_E_BADARG;
  if (ab->slots > 1 && ((ab->slots & (ab->slots - 1)) || ab->slot_stride < Cout || (ab->d_rgb_w && ab->rgb_slot_stride < B * 3 * Cout)))
    return CIPS3D_E_BADARG;
  if (!cips3d_modconv1x1_supported(Cin, Cout, HW)) return CIPS3D_E_UNSUPP;
  if (B == 0) return 0;
  GemmArgs a{g, wm_t, dpre, B, Cin, Cout, HW, 0, noise, noise_bstride, nullptr, nullptr, (flags & CIPS3D_GEMM_SPLIT) ? 2 : 0, 0,
             nullptr, nullptr, rg ? rg->x_amax : nullptr, rg ? rg->out_amax : nullptr, *ab};
  return launch_gemm_tile(gemm_tile(B, Cin, Cout, HW, false), true, a, as_stream(stream));
}

extern "C" int cips3d_up2_fir_act(const float* y_lo, const float* fir, float* out, int B, int C, int H, int W,
                                  const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                                  float* out_amax, void* stream) {
  if (!y_lo || !fir || !out || !bias || B < 0 || C <= 0 || H <= 0 || W <= 0) return CIPS3D_E_BADARG;
  if (W % 2 != 0) return CIPS3D_E_UNSUPP;     // 16-byte output quads
  if (B == 0) return 0;
  const int64_t total = (int64_t)B * C * H * (W / 2);
  int64_t blocks = ceil_div<int64_t>(total, 256);
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(up2_fir_act_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), y_lo, fir, out, B,
                     C, H, W, noise, noise_bstride, noise_w, bias, out_amax);
  return cips3d_launch_status();
}
