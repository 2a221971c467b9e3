// The fused up-sampling stage of the StyleGAN2-style decoder of CIPS-3D++ on gfx950 (reference
// models/model_v3.py:418-482,592-637), with its diagnostic builds CIPS3D_FUSED_AB and CIPS3D_FUSED_STAMPS.
//
//   cips3d_fused_up_conv       one up-sampling (or flat) decoder block in one kernel
//   cips3d_fused_up_conv_next  the same with the next block's low-resolution GEMM chained behind it (C = 64, 128, 256)
//
// (A file of its own has one visible effect on the code: before it inlines, hipcc propagates the ranges of a static helper's
// arguments over all the helper's call sites in the translation unit.  Every call of cips3d_workgroup_max here passes
// lane = tid & 63, so the helper learns 0 <= lane < 64 first; in one file with the 1x1 GEMM, whose lane has no
// known range at that point (lambdas capture it by reference; any such caller in the file has this effect), it did not.  The 24 chained instantiations therefore form the
// LDS address of the next_amax reduction with one v_lshl_add_u32 instead of v_lshrrev_b32 + v_add_u32 / v_lshl_or_b32, once per
// workgroup; nothing else differs -- tools/isa_same.py.)

#include <type_traits>

#include "up2_fir.h"

namespace {

// The patch loads of up2_fir.h (the same loads in the same order) from a workgroup-uniform byte base `ub` and a 32-bit lane
// offset `vo` in bytes: global loads in the saddr form, where a 64-bit pointer per lane costs a sign extension and a
// v_lshl_add_u64 per patch.  T = float | bf16_t.
__device__ __forceinline__ void ld_mid(const float* row, float& m0, float& m1) {
  const float2 m = *reinterpret_cast<const float2*>(row);
  m0 = m.x; m1 = m.y;
}
__device__ __forceinline__ void ld_mid(const bf16_t* row, float& m0, float& m1) {
  const unsigned m = *reinterpret_cast<const unsigned*>(row);
  m0 = bf16_f32(m & 0xffffu); m1 = __uint_as_float(m & 0xffff0000u);
}
__device__ __forceinline__ float ld_one(const float* p) { return *p; }
__device__ __forceinline__ float ld_one(const bf16_t* p) { return bf16_f32(*p); }

// up2_load_interior: `ub + vo` is the middle pair of the first patch row
template <typename T>
__device__ __forceinline__ void up2_load_interior_at(const char* ub, unsigned vo, unsigned row_bytes, float (&v)[3][4]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const T* row = reinterpret_cast<const T*>(ub + vo);
    ld_mid(row, v[r][1], v[r][2]);
    v[r][0] = ld_one(row - 1); v[r][3] = ld_one(row + 2);
    vo += row_bytes;
  }
}

// up2_load (rows and columns outside the image read as zero): `ub + vo` is the channel plane
template <typename T>
__device__ __forceinline__ void up2_load_at(const char* ub, unsigned vo, int H, int W, int iy, int qx, float (&v)[3][4]) {
  const int c = 2 * qx;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int y = iy - 1 + r;
    const bool yok = (y >= 0) && (y < H);
    const T* row = reinterpret_cast<const T*>(ub + (vo + (unsigned)((yok ? y : 0) * W + c) * (unsigned)sizeof(T)));
    float m0 = 0.f, m1 = 0.f;
    if (yok) ld_mid(row, m0, m1);
    v[r][1] = m0; v[r][2] = m1;
    v[r][0] = (yok && c - 1 >= 0) ? ld_one(row - 1) : 0.f;
    v[r][3] = (yok && c + 2 < W) ? ld_one(row + 2) : 0.f;
  }
}

// flat_load: `ub + vo` is the block's first pixel
template <typename T>
__device__ __forceinline__ void flat_load_at(const char* ub, unsigned vo, unsigned row_bytes, float (&v)[3][4]) {
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if constexpr (std::is_same<T, float>::value) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(ub + vo);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[r][c] = t[c];
    } else {
      const uint2 t = *reinterpret_cast<const uint2*>(ub + vo);
      v[r][0] = bf16_f32(t.x & 0xffffu); v[r][1] = __uint_as_float(t.x & 0xffff0000u);
      v[r][2] = bf16_f32(t.y & 0xffffu); v[r][3] = __uint_as_float(t.y & 0xffff0000u);
    }
    vo += row_bytes;
  }
}

// ------------------------------------------------------------------------------------------------
// Fused up-sampling stage:  y_lo --(2x FIR + noise1 + bias1 + lrelu)--> act1 --(1x1 modconv, noise2 + bias2
// + lrelu)--> out2 --(ToRGB + bias + FIR-upsampled skip)--> rgb, one kernel.  act1 (the largest tensor of
// the stage) only ever exists as LDS B-operand stages; out2 is stored only when a later stage needs it
// (never for the last stage, which then writes 12 B per pixel instead of moving ~540 B).
//   workgroup = 8 waves: WGM wave rows cover ALL C output channels (so ToRGB reduces inside the
//   workgroup, deterministically), WGN waves cover WGN image rows of 64 pixels.
//   per 32-channel K stage: every thread builds 2x4-pixel blocks of act1 from a 3x4 patch of y_lo (VALU),
//   writes them to the LDS stage the MFMAs of the next step read; A fragments come straight from L2.
// ------------------------------------------------------------------------------------------------
struct FusedArgs {
  const float* y_lo; const float* fir; const float* noise1; int64_t nbs1; const float* nw1; const float* bias1;
  const float* wm2; const float* noise2; int64_t nbs2; const float* nw2; const float* bias2; float* out2;
  const float* wm_rgb; const float* bias_rgb; const float* skip; int skip_up; float* rgb;
  int B, H, W;   // low-resolution size; the stage outputs 2H x 2W (FLAT: the size of y_lo AND of the outputs)
  int bf16;      // 0: exact fp32; 1: bf16 GEMM operands (CIPS3D_GEMM_BF16); 2: additionally y_lo / y_next are bf16 arrays (CIPS3D_Y_BF16);
                 // 3: fp32-equivalent split-fp16 products (CIPS3D_GEMM_SPLIT; wm2 / wm_next CIPS3D_MOD_SPLIT16-packed)
  // optional (NEXT instantiation): the next stage's low-resolution GEMM y_next = wm_next (C/2 x C, chained pack) out2
  const float* wm_next; float* y_next;
  // range tracking (split mode; cips3d_range): amax of y_lo, the constants of conv1 / conv2; max |y_next| recorded (out2 is
  // not tracked: 64 registers is all the C = 32 stage has -- a split GEMM that reads a stored out2 measures it, cips3d_absmax)
  const float* x_amax; const float* lconst1; const float* lconst2; float* next_amax;
  // next_gain > 0: next_amax does not receive the measured max|y_next| (a workgroup reduction + one atomic per workgroup:
  // 4 us at the 4096 workgroups of the C = 64 stage) but its BOUND next_gain * U2 (next_gain: sqrt(C) for a demodulated next
  // up-conv), written once -- good enough for a consumer that is the last stage of the decoder (cips3d_range)
  float next_gain;
  // FLAT stage (CIPS3D_STAGE_FLAT): a decoder block that does not up-sample -- [StyledConv, StyledConv, ToRGB] at ONE resolution.
  // y_lo is conv1's GEMM result at that resolution, `fir` is unused, the skip image (if any) has the output's size and is added
  // as it is.  Everything behind the first activation is the up-sampling stage's code.
  int flat;
  // What does not depend on the workgroup, worked out once by the launcher (stage_geometry) instead of by every wave of every
  // launch: the tile row length with its shift (a power of two) or reciprocal (anything else), the plane sizes, and the BYTE
  // strides of one sample of every tensor.  A wave's addresses are then one uniform 64-bit base per tensor -- sample, tile, channel
  // group: advanced on the scalar unit -- plus 32-bit lane offsets (the saddr form of the global loads and stores).
  cips3d_stage_geom g;
  int64_t nz1_bs, nz2_bs;   // nbs1 / nbs2 in bytes
};

// What a launch is compiled for (the FEAT template argument of fused_up_conv_kernel; the table of instantiations is stage_forms
// below).  One body with every feature as a run-time branch on a FusedArgs pointer was 74 to 137 basic blocks around the same
// arithmetic, with a group of kernarg loads and a wait per test; a form carries only what its launches do.
enum : int {
  SF_NOISE1 = 1,      // conv1 has a noise map and its weight (both pointers given)
  SF_NOISE2 = 2,      // conv2 likewise
  SF_RGB = 4,         // ToRGB: wm_rgb / bias_rgb / rgb given
  SF_SKIP = 8,        // ... with a skip image of the output's size, added as it is
  SF_SKIP_UP = 16,    // ... with a skip image of the input's size, FIR-up-sampled (never FLAT)
  SF_OUT2 = 32,       // out2 is stored
  SF_RANGED = 64,     // split mode: x_amax and the layers' constants are there, the operands are split under tracked scales
  SF_AMAX = 128,      // chained: the measured max |y_next| raises next_amax
  SF_BOUND = 256,     // chained, ranged: next_amax receives the bound next_gain * U2 instead
  SF_U8 = 512,        // the image leaves as uint8
  SF_GENERIC = 1024   // everything above decided at run time from FusedArgs, as the one body used to
};

// MINW = waves per SIMD the register allocation must leave room for (the per-workgroup chain load -> FIR -> LDS -> MFMA ->
// store is serial, so throughput comes from co-resident workgroups).
#ifndef CIPS3D_FUSED_AB
// timing-only ablations of the fused stages (results garbage; tools/README.md): 1 no scale loads, 2 no y_next record, 4 no ToRGB
// sums (at C = 32, where nothing else reads conv2's output, the compiler then drops conv2 altogether: read that one as "no
// conv2"), 8 no FIR arithmetic, 16 no conv2 epilogue arithmetic, 32 no activation / split of conv1, 64 no patch loads (register
// values instead), 128 no noise / skip loads of the epilogues
#define CIPS3D_FUSED_AB 0
#endif
#ifdef CIPS3D_FUSED_STAMPS
// Diagnostic build only: per-phase cycle sums of wave 0 of every workgroup of the fused up-sampling stages, slot = log2(C) - 5
// (C = 32, 64, 128, 256), accumulated in registers, flushed at the end of the workgroup.
__device__ unsigned long long g_fused_stamps[4][8];
#define FSTAMP(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); fst_[i] += t_ - ftp_; ftp_ = t_; } while (0)
#define FSTAMP_FLUSH() do { if (tid == 0 && (blockIdx.x & 31) == 0) {   /* every 32nd workgroup: the atomics must not become the load */ constexpr int sl_ = C == 32 ? 0 : C == 64 ? 1 : C == 128 ? 2 : 3; \
    for (int i_ = 0; i_ < 7; ++i_) atomicAdd(&g_fused_stamps[sl_][i_], fst_[i_]); atomicAdd(&g_fused_stamps[sl_][7], 1ull); } } while (0)
#else
#define FSTAMP(i)
#define FSTAMP_FLUSH()
#endif

// FEAT: SF_* bits fixed at compile time -- or SF_GENERIC: read from FusedArgs at run time.  The arithmetic, the loads, the stores
// and their order are the same in every form.
template <int C, int WM, int WGM, int WGN, int RW, int BK, int MINW, int PREC, bool NEXT, bool XPREF, bool LATE_OPS, bool FLAT, int FEAT>
__global__ void __launch_bounds__(64 * WGM * WGN, MINW) fused_up_conv_kernel(FusedArgs a) {
  constexpr bool GEN = (FEAT & SF_GENERIC) != 0;
  static_assert(GEN || ((!(FEAT & (SF_SKIP | SF_SKIP_UP | SF_U8)) || (FEAT & SF_RGB)) && !((FEAT & SF_SKIP) && (FEAT & SF_SKIP_UP)) &&
                        (!(FEAT & SF_SKIP_UP) || !FLAT) && (!(FEAT & SF_RANGED) || PREC == 3) && (!(FEAT & (SF_AMAX | SF_BOUND)) || NEXT) &&
                        (!(FEAT & SF_BOUND) || ((FEAT & SF_RANGED) && !(FEAT & SF_AMAX))) && ((FEAT & (SF_OUT2 | SF_RGB)) || NEXT)), "no such form");
  constexpr bool BF16 = PREC == 1 || PREC == 2;  // bf16 MFMA operands, fp32 accumulate
  constexpr bool YB = PREC == 2;                 // y_lo (in) and y_next (out) stored as bf16
  constexpr bool SPLIT = PREC == 3;              // fp32-equivalent split-fp16 products (weights CIPS3D_MOD_SPLIT16-packed)
  typedef typename std::conditional<YB, bf16_t, float>::type ylo_t;
  // A wave covers RW image rows x CW columns (64 pixels, 4 consecutive x per lane); the WGN waves of a
  // workgroup are stacked vertically: pixel tile TH x TW.
  constexpr int NT = 64 * WGM * WGN;
  constexpr int CW = 64 / RW, TH = RW * WGN, TW = CW, BN = TH * TW;
  constexpr int NSTAGE = C / BK, NBUF = NSTAGE > 1 ? 2 : 1, KQ = BK / 16;
  constexpr int LPR = CW / 4;                    // lanes (pixel quads) per image row of the wave tile
  static_assert((WGM * WGN == 8 || WGM * WGN == 4) && 16 * WM * WGM == C && TH % 2 == 0 && C % BK == 0, "tile shape");
  constexpr int NBLK = (TH / 2) * (TW / 4);      // 2x4 blocks per channel in the tile
  constexpr int BPT = BK * NBLK / NT;            // blocks per thread per stage
  static_assert((BK * NBLK) % NT == 0 && BPT >= 1, "block split");
  __shared__ __attribute__((aligned(16))) float sB[NBUF * BK * BN];
  __shared__ __attribute__((aligned(16))) float s_nz1[BN + 8];     // + the stage's scale factors (wave 0 -> everyone)
  // (the last stage has no chained GEMM: its B tile is dead when the ToRGB partials are exchanged, so they take its place --
  // 3 KB of LDS less per workgroup, which with <= 64 VGPRs admits an eighth workgroup per CU)
  __shared__ __attribute__((aligned(16))) float s_red_own[NEXT ? WGM * 3 * BN : 4];
  float* s_red = NEXT ? s_red_own : sB;
  __shared__ __attribute__((aligned(16))) float s_wrgb[3 * C];

  const int tid = threadIdx.x;
#ifdef CIPS3D_FUSED_STAMPS
  unsigned long long fst_[7] = {0, 0, 0, 0, 0, 0, 0}, ftp_ = __builtin_amdgcn_s_memtime();
#endif
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int wm_i = wave / WGN, wn_i = wave % WGN;
  const int q = lane >> 4, jn = lane & 15;
  const int lrow = jn / LPR, lx4 = jn % LPR;
  const int nloc = (wn_i * RW + lrow) * TW + lx4 * 4;     // this lane's first pixel inside the tile
  const int b = blockIdx.z;
  const int H = a.H, W = a.W, OW = FLAT ? W : 2 * W;
  // what the launch does: constants of the form, or (SF_GENERIC) read from the arguments
  const bool noisy1 = (GEN ? (a.noise1 && a.nw1) : (FEAT & SF_NOISE1) != 0) && !(CIPS3D_FUSED_AB & 128);
  const bool noisy2 = (GEN ? (a.noise2 && a.nw2) : (FEAT & SF_NOISE2) != 0) && !(CIPS3D_FUSED_AB & 128);
  const bool to_rgb = GEN ? a.wm_rgb != nullptr : (FEAT & SF_RGB) != 0;
  const bool skip_fir = !FLAT && (GEN ? (a.skip && (a.skip_up & 1)) : (FEAT & SF_SKIP_UP) != 0);
  const bool skip_any = GEN ? a.skip != nullptr : (FEAT & (SF_SKIP | SF_SKIP_UP)) != 0;
  const bool store_out2 = GEN ? a.out2 != nullptr : (FEAT & SF_OUT2) != 0;
  const bool ranged = SPLIT && (GEN ? a.x_amax != nullptr : (FEAT & SF_RANGED) != 0) && !(CIPS3D_FUSED_AB & 1);
  const bool amax_bound = NEXT && (GEN ? (a.next_amax && a.next_gain > 0.f) : (FEAT & SF_BOUND) != 0);
  const bool amax_measured = NEXT && (GEN ? (a.next_amax && !(a.next_gain > 0.f)) : (FEAT & SF_AMAX) != 0) && !(CIPS3D_FUSED_AB & 2);
  const bool rgb_u8 = GEN ? (a.skip_up & 2) != 0 : (FEAT & SF_U8) != 0;
  const int tiles_x = a.g.tiles_x;
  // XCD-aware tile order.  Workgroups go to the 8 XCDs round-robin by linear id, and each XCD has its own L2: in row-major
  // tile order the horizontal neighbours of a tile -- whose FIR halo columns sit in the SAME 128-byte lines as its own
  // first / last columns -- always ran on other XCDs, so every (channel, row) segment pulled three lines through its L2 for
  // one line of unique data (FETCH_SIZE 2.5x the algorithmic bytes at C = 32; tools/calib/fetch_calibrate.hip shows the
  // counter itself is exact for these load widths).  Here XCD k walks the k-th contiguous eighth of the tiles instead:
  // neighbours in both directions share an L2 and are dispatched 8 (resp. 8 * tiles_x) workgroups apart.
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (bid & 7) * (gridDim.x >> 3) + (bid >> 3);
  // bid / tiles_x without a division: a shift where tiles_x is a power of two, else the high word of bid * (2^32 / tiles_x + 1),
  // which is the quotient or one more (stage_geometry; bid < 2^32): one multiply puts it right
  int tile_y;
  if (a.g.tx_shift >= 0) {
    tile_y = bid >> a.g.tx_shift;
  } else {
    tile_y = (int)__umulhi((unsigned)bid, a.g.tx_rcp);
    if (tile_y * tiles_x > bid) --tile_y;
  }
  const int ox0 = (bid - tile_y * tiles_x) * TW, oy0 = tile_y * TH;
  // Index arithmetic stays in 32 bits: 64-bit products only in the workgroup-uniform bases below (the host refuses
  // C * 4HW >= 2^31, so an intra-sample offset in ELEMENTS fits; in bytes it fits where the comments below say why)
  const int HWlo = a.g.HWlo, HWo = a.g.HWo;
  const int oy = oy0 + wn_i * RW + lrow, ox = ox0 + lx4 * 4;
  // ---- addresses: uniform byte bases (scalar registers) + 32-bit lane offsets
  typedef const char* ubase_t;
  constexpr unsigned ES = sizeof(ylo_t);
  // this wave's pixel strip inside the sample (row oy0 + wn_i RW, column ox0) and the lane's place in it
  const int pix_u = (oy0 + wn_i * RW) * OW + ox0;
  const unsigned pix_l = (unsigned)(lrow * OW + lx4 * 4);
  // channel 4 q of a 16-channel group + the lane's pixel: the one lane offset of every out2 / y_next store (r, the group and the
  // tile advance the uniform base).  16 HWo * 4 bytes < 2^32: HWo < 2^31 / C <= 2^26
  const unsigned vo_q = (unsigned)(4 * q * HWo) + pix_l;

  // scale factors of the split operands (cips3d_range); set right before the first patch_store below
  float kact1 = 1.41421356237309515f, k2in = kSplitInv, kact2 = 1.41421356237309515f, kback2 = 1.f, kyn = kSplitInv;

  float nw1_u = 0.f;                        // NoiseInjection.weight of conv1 (applied where the tile is read)
  // the layer's range constants (uniform addresses: scalar loads -- as long as they are read in FRONT of the LDS-DMA below)
  float c10_u = 0.f, c11_u = 0.f, c20_u = 0.f, c21a_u = 0.f, c21b_u = 0.f;
  if constexpr (SPLIT) {
    if (ranged) {
      const float* l1 = a.lconst1 + b * 4;
      c10_u = l1[0]; c11_u = l1[1];
      if (NEXT) {
        const float* l2 = a.lconst2 + b * 4;
        c20_u = l2[0]; c21a_u = l2[1]; c21b_u = l2[2];
      }
    }
  }
  // Everything that does not depend on a barrier is requested first: conv2's first A fragments, its noise / bias.
  // packed [ot][kq][256]: this wave row's WM tiles, 16 bytes per lane
  const ubase_t ab = reinterpret_cast<ubase_t>(a.wm2) + ((int64_t)b * C * C + wm_i * WM * (C / 16) * 256) * 4;
  const unsigned vo_a = lane * 16;
  f32x4 afr_next[KQ][WM];
#pragma unroll
  for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
    for (int i = 0; i < WM; ++i)
      afr_next[kq][i] = *reinterpret_cast<const f32x4*>(ab + (i * (C / 16) + kq) * 1024 + vo_a);
  // LATE (single-stage kernels, C = BK): the epilogue's operands are requested after the MFMAs instead of up front -- 24
  // registers that buy a sixth resident wave per SIMD
  constexpr bool LATE = LATE_OPS;
  f32x4 nz2 = {0.f, 0.f, 0.f, 0.f};
  float nw2_u = 0.f;                        // NoiseInjection.weight of conv2 (applied by the FMA that adds the noise)
  f32x4 bias4[WM];
  auto load_epilogue_ops = [&]() {
    if (noisy2) {
      nz2 = *reinterpret_cast<const f32x4*>(reinterpret_cast<ubase_t>(a.noise2) + ((int64_t)b * a.nz2_bs + (int64_t)pix_u * 4) + pix_l * 4u);
      nw2_u = a.nw2[0];
    }
    const ubase_t bb = reinterpret_cast<ubase_t>(a.bias2) + wm_i * WM * 64;
#pragma unroll
    for (int i = 0; i < WM; ++i) bias4[i] = *reinterpret_cast<const f32x4*>(bb + i * 64 + (unsigned)q * 16u);
  };
  if (!LATE) load_epilogue_ops();

  float kf[16];   // flipped taps
#pragma unroll
  for (int i = 0; i < 16; ++i) kf[i] = FLAT ? 0.f : a.fir[15 - i];
  // the lanes that will finish a colour channel (wave row 0, quarter = channel) fetch their skip operands now
  const bool rgb_lane = to_rgb && wm_i == 0 && q < 3;
  float skp[3][4];
  f32x4 skv = {0.f, 0.f, 0.f, 0.f};
  float rgb_bias = 0.f;
  auto load_skip_ops = [&]() {
    if (rgb_lane) {
      rgb_bias = a.bias_rgb[q];
      if (skip_any && !(CIPS3D_FUSED_AB & 128)) {
        const ubase_t sb = reinterpret_cast<ubase_t>(a.skip) + (int64_t)b * a.g.skip_bs;
        // (lane offsets: colour plane q of the low-resolution image, resp. of the output-sized one plus the lane's pixel -- 3 planes)
        if (skip_fir) up2_load_at<float>(sb, (unsigned)(q * HWlo) * 4u, H, W, oy >> 1, ox >> 2, skp);
        else skv = *reinterpret_cast<const f32x4*>(sb + (int64_t)pix_u * 4 + ((unsigned)(q * HWo) + pix_l) * 4u);
      }
    }
  };
  if (!LATE) load_skip_ops();

  // FIR patches of one K stage: loaded early (before the MFMAs that precede their use), filtered late.  Tiles whose
  // low-resolution window (rows oy0/2-1 .. oy0/2+TH/2, columns ox0/2-1 .. ox0/2+TW/2) lies inside the image take loads
  // without edge predication (workgroup-uniform branch; 87 % of the tiles at 1024^2).
  const bool interior = FLAT || (oy0 / 2 >= 1 && oy0 / 2 + TH / 2 < H && ox0 / 2 >= 1 && ox0 / 2 + TW / 2 < W);
  // Two patch register sets when the K loop has >= 3 stages and it pays (C = 256): the patches of stage
  // st + 2 are requested at the START of stage st and filtered at the END of stage st + 1 -- two stages of lead.  With one
  // stage of lead (the form C = 64 keeps) a stage lasted as long as a patch round trip: in-kernel stamps (tools/
  // fused_stamps.py) showed 5.6k cycles per stage at C = 256 for 1.5k cycles of matrix work.
  constexpr bool DEEP = NSTAGE >= 3 && C >= 256;   // same-box A/B: C = 256 24.4 -> 22.9 us; C = 128 (252 VGPRs with it) 25.2 -> 25.5: off there
  float pv[BPT][3][4], pw[BPT][3][4];
  // Thread tid builds block tid % NBLK of channel tid / NBLK + u NT / NBLK of the stage (u < BPT): the lane's part of a patch
  // address -- its channel among the first NT / NBLK, its block's place in the tile -- is the same in every stage and for every
  // u; stage, u, sample and the tile's origin advance the uniform base.  In bytes the lane's part stays below
  // (NT / NBLK) HWlo ES <= 2^32: 16 channels (64 at C = 256) of a plane of fewer than 2^31 / C elements.
  static_assert(NT % NBLK == 0 && (int64_t)(NT / NBLK) * 4 * (((int64_t)1 << 31) / C) <= ((int64_t)1 << 32), "32-bit patch offsets");
  constexpr int CPU_ = NT / NBLK;                                  // channels per u
  const int p_ch = tid / NBLK, p_by = (tid % NBLK) / (TW / 4), p_qx = tid % (TW / 4);
  const unsigned row_lo = (unsigned)W * ES;
  const ubase_t ylo_b = reinterpret_cast<ubase_t>(a.y_lo) + (int64_t)b * a.g.ylo_bs;
  // (tile origins: the first patch row oy0 / 2 - 1 and column ox0 / 2 of an interior tile; row oy0, column ox0 of a flat one)
  const int64_t tile_lo = FLAT ? ((int64_t)oy0 * W + ox0) * ES : ((int64_t)(oy0 / 2 - 1) * W + ox0 / 2) * ES;
  const unsigned vo_p = (unsigned)(p_ch * HWlo) * ES + (FLAT ? (unsigned)(2 * p_by * W + 4 * p_qx) : (unsigned)(p_by * W + 2 * p_qx)) * ES;
  const unsigned vo_pe = (unsigned)(p_ch * HWlo) * ES;             // edge tiles: rows and columns clamped per load (up2_load_at)
  auto patch_load_into = [&](int st, float (&pset)[BPT][3][4]) {
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const ubase_t src = ylo_b + (int64_t)((st * BK + u * CPU_) * HWlo) * ES;
      if constexpr (CIPS3D_FUSED_AB & 64) {        // no patch loads: what the latency chain behind them costs
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) pset[u][r][c] = __int_as_float(0x3c000000 + ((tid + st + r * 4 + c) << 8));
      } else
      if constexpr (FLAT) flat_load_at<ylo_t>(src + tile_lo, vo_p, row_lo, pset[u]);
      else if (interior) up2_load_interior_at<ylo_t>(src + tile_lo, vo_p, row_lo, pset[u]);
      else up2_load_at<ylo_t>(src, vo_pe, H, W, oy0 / 2 + p_by, ox0 / 4 + p_qx, pset[u]);
    }
  };
  auto patch_load = [&](int st) { patch_load_into(st, pv); };
  auto patch_store_from = [&](int st, float* dst, float (&pset)[BPT][3][4]) {
#pragma unroll
    for (int u = 0; u < BPT; ++u) {
      const int ch = p_ch + u * CPU_, by = p_by, qx = p_qx;
      float o[2][4];
      if constexpr (FLAT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { o[0][c] = pset[u][0][c]; o[1][c] = pset[u][1][c]; }
      } else if constexpr (CIPS3D_FUSED_AB & 8) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { o[0][c] = pset[u][0][c] + pset[u][1][c]; o[1][c] = pset[u][1][c] + pset[u][2][c]; }
      } else {
        up2_fir(pset[u], kf, o);
      }
      const float bs = *reinterpret_cast<const float*>(reinterpret_cast<ubase_t>(a.bias1) + (st * BK + u * CPU_) * 4 + (unsigned)p_ch * 4u);
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        const f32x4 nz = *reinterpret_cast<const f32x4*>(s_nz1 + (2 * by + py) * TW + qx * 4);
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          // (the tile holds the raw noise, its weight rides in the FMA: see noise_bias_act_kernel)
          const float on = fmaf(nw1_u, nz[c], o[py][c]);
          v[c] = (CIPS3D_FUSED_AB & 32) ? on : lrelu02(on + bs);
        }
        if constexpr (SPLIT && !(CIPS3D_FUSED_AB & 32)) {          // split once here (with the activation's gain and range scale: cips3d_split_word);
#pragma unroll                          // every wave row reads the packed halves
          for (int c = 0; c < 4; ++c) v[c] = pack_split(v[c], kact1);
        } else {
#pragma unroll
          for (int c = 0; c < 4; ++c) v[c] *= kact1;
        }
        *reinterpret_cast<f32x4*>(dst + ch * BN + (2 * by + py) * TW + qx * 4) = v;
      }
    }
  };
  auto patch_store = [&](int st, float* dst) { patch_store_from(st, dst, pv); };
  // Round 5: the first conv's noise tile and the ToRGB rows have to be in LDS at the first barrier.  Loaded where they were stored
  // -- behind the range block, `load -> wait -> LDS store` each -- they were two more dependent round trips of every workgroup's
  // prologue (three in all, with the patches + amax slots).  Now they travel by LDS-DMA, requested with the first patches: no
  // registers (the C = 32 / 64 stages have none to spare: five more live values spilled 34 / 20), no wait of their own -- the one
  // vmcnt(0) in front of the first barrier covers them, the patches and the range slots.  The tile holds the RAW noise; its weight
  // rides in the FMA that adds it (patch_store).  The request sits BEHIND the uniform loads of the prologue (FIR taps, biases): an
  // LDS-DMA counts as a memory write for the compiler, and uniform loads behind one are no longer scalar loads -- issued at the very
  // top, the 16 taps alone came back in vector registers and the C = 32 / 64 stages spilled 43 / 34.
  // The first patches go out in FRONT of the LDS-DMA requests: behind them, the compiler waited for vmcnt(0) -- the A fragments, the
  // noise tile, the ToRGB rows, all from a cold L2 -- before it reused the DMAs' address registers for the patch addresses.  Same
  // box (rocprofv3 / unprofiled bench, variants interleaved): C = 32 stage 38.5 -> 37.3 us, the view 0.3481 -> 0.3474 ms.
  // (Measured with it and NOT kept: the patch rows as register quads from the load to the FIR, all of a stage's patches under ONE
  // interior / edge branch -- the interior path then issues its six 16-byte loads back to back with no wait between them, where
  // today every row's load is waited for before its middle pair is copied to an even register pair -- 39.1 / 32.9 / 25.1 / 23.1 us
  // for C = 32 / 64 / 128 / 256 against 37.3 / 32.3 / 23.3 / 21.5: the co-resident workgroups cover those waits, the quads cost
  // registers and copies in the K loop.)
  patch_load(0);
  if (DEEP) patch_load_into(1, pw);          // stage s's patches live in set s & 1 (pv: even, pw: odd)
  const bool have_nz = noisy1;
  if (have_nz) nw1_u = a.nw1[0];
  if (wave == 0) {                        // BN / 4 <= 64 lanes (BN = 128 in every instantiation): one wave's worth of 16-byte pieces
    static_assert(BN / 4 <= 64 && (3 * C) % 4 == 0, "one LDS-DMA instruction per tile");
    if (lane < BN / 4) {
      if (have_nz) {
        const int r = lane / (TW / 4), x4 = lane % (TW / 4);
        const ubase_t nb = reinterpret_cast<ubase_t>(a.noise1) + ((int64_t)b * a.nz1_bs + ((int64_t)oy0 * OW + ox0) * 4);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(nb + (unsigned)(r * OW + x4 * 4) * 4u),
                                         (__attribute__((address_space(3))) void*)s_nz1, 16, 0, 0);
      } else {
        *reinterpret_cast<f32x4*>(s_nz1 + lane * 4) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  if (to_rgb) {                           // 3 C floats = 3 C / 4 pieces of 16 bytes, 64 per wave-instruction
    const ubase_t wb = reinterpret_cast<ubase_t>(a.wm_rgb) + (int64_t)b * (3 * C * 4);
#pragma unroll
    for (int p0 = 0; p0 < 3 * C / 4; p0 += 64 * WGM * WGN) {
      const int pbase = p0 + wave * 64;   // (wave-uniform LDS base: the hardware adds lane * 16)
      if (pbase < 3 * C / 4 && pbase + lane < 3 * C / 4)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wb + pbase * 16 + vo_a),
                                         (__attribute__((address_space(3))) void*)(s_wrgb + pbase * 4), 16, 0, 0);
    }
  }

  // Range of the split operands (cips3d_range, common.h).  act1 is split as act1 2^-e1, e1 from the bound
  // U1 = c1 max|y_lo| + c0 (conv1's constants: FIR gain, noise, bias); conv2's accumulators come back with 2^-8 2^e1.  In the
  // chained form out2 is split as out2 2^-e2, U2 = c1' U1 + c0' (conv2's constants), and y_next comes back with 2^-8 2^e2.
  // Both powers of two ride on the sqrt(2) of the activations: no instruction per value.  Wave 0 makes them -- ONE vector load
  // for the amax slots (lane = slot), issued here with the tile's first loads and waited for with them at the barrier below;
  // as scalar loads in front of the first patch_store their latency was exposed: +2.9 us at C = 32 -- and leaves them behind
  // the noise tile for everyone.

  if constexpr (SPLIT) {
    if (ranged && wave == 0) {
      const float t = lane < CIPS3D_AMAX_SLOTS ? a.x_amax[b * CIPS3D_AMAX_FLOATS + lane * CIPS3D_AMAX_STRIDE] : 0.f;
      float c10 = c10_u, c11 = c11_u, c20 = 0.f, c21 = 0.f;
      if (NEXT) { c20 = c20_u; c21 = fmaxf(c21a_u, 1.41421356237309515f * c21b_u); }
      // (FLAT: x_amax is the maximum of conv1's GEMM RESULT -- what the FIR's gain multiplies in the up-sampling form; the row
      // gain of a plain StyledConv's constants is relative to that conv's INPUT)
      if (FLAT) c11 = 1.41421356237309515f;
      const float m_in = cips3d_wave_max_uniform(t);
      const float u1 = fmaf(c11, m_in, c10);
      const int e1 = cips3d_split_exp(u1);
      f32x4 sc = {1.41421356237309515f * cips3d_pow2(-e1), kSplitInv * cips3d_pow2(e1), 1.41421356237309515f, 1.f};
      if (NEXT) {
        const float u2 = fmaf(c21, u1, c20);
        const int e2 = cips3d_split_exp(u2);
        sc[2] = 1.41421356237309515f * cips3d_pow2(-e2);
        sc[3] = cips3d_pow2(e2);
        // the bound of |y_next| instead of its measured maximum (see FusedArgs::next_gain): slot 0, once per sample
        if (amax_bound && blockIdx.x == 0 && lane == 0) a.next_amax[b * CIPS3D_AMAX_FLOATS] = a.next_gain * u2 * 1.000001f;
      }
      if (lane == 0) *reinterpret_cast<f32x4*>(s_nz1 + BN) = sc;
    }
  }
  // noise of the first conv for this tile, ToRGB weights: on their way since the top of the kernel
  __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0): this wave's LDS-DMA pieces (and, needed right behind the barrier anyway, its patches)
  __syncthreads();

  f32x4 acc[WM][4];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  FSTAMP(0);        // operand requests, noise staged, first barrier
  if constexpr (SPLIT) {      // the scale factors wave 0 left behind the noise tile (below), now wave-uniform registers
    if (ranged) {
      const f32x4 sc = *reinterpret_cast<const f32x4*>(s_nz1 + BN);
      kact1 = cips3d_uniform(sc[0]);
      k2in = cips3d_uniform(sc[1]);
      if (NEXT) {
        kact2 = cips3d_uniform(sc[2]);
        kback2 = cips3d_uniform(sc[3]);
        kyn = cips3d_uniform(kSplitInv * kback2);
      }
    }
  }

  patch_store(0, sB);
  __syncthreads();
  FSTAMP(1);        // FIR + activation + split of stage 0 into LDS (waits for its patches), barrier
#pragma unroll (DEEP ? NSTAGE : 1)
  for (int st = 0; st < NSTAGE; ++st) {
    const float* cur = sB + (NBUF > 1 ? (st & 1) : 0) * BK * BN + nloc;
    f32x4 afr[KQ][WM];
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
      for (int i = 0; i < WM; ++i) afr[kq][i] = afr_next[kq][i];
    if (st + 1 < NSTAGE) {   // next stage's operands travel under this stage's MFMAs
#pragma unroll
      for (int kq = 0; kq < KQ; ++kq)
#pragma unroll
        for (int i = 0; i < WM; ++i)
          afr_next[kq][i] = *reinterpret_cast<const f32x4*>(ab + (i * (C / 16) + (st + 1) * KQ + kq) * 1024 + vo_a);
      if (!DEEP) patch_load(st + 1);
    }
    if (DEEP && st + 2 < NSTAGE) {           // set st & 1 was filtered into LDS at the end of stage st - 1: free
      if (st & 1) patch_load_into(st + 2, pw);
      else patch_load_into(st + 2, pv);
    }
#pragma unroll
    for (int kq = 0; kq < KQ; ++kq) {
      if (BF16) {
        f32x4 b4[4];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) b4[j4] = *reinterpret_cast<const f32x4*>(cur + (kq * 16 + j4 * 4 + q) * BN);
        s16x4 ah[WM], bh[4];
#pragma unroll
        for (int i = 0; i < WM; ++i) ah[i] = pack_bf16(afr[kq][i][0], afr[kq][i][1], afr[kq][i][2], afr[kq][i][3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) bh[c] = pack_bf16(b4[0][c], b4[1][c], b4[2][c], b4[3][c]);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah[i], bh[c], acc[i][c], 0, 0, 0);
      } else if constexpr (SPLIT) {
        f32x4 b4[4];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) b4[j4] = *reinterpret_cast<const f32x4*>(cur + (kq * 16 + j4 * 4 + q) * BN);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          h4 bh, bl;
          unpack_frag(b4[0][c], b4[1][c], b4[2][c], b4[3][c], bh, bl);
#pragma unroll
          for (int i = 0; i < WM; ++i) acc[i][c] = split_mfma16(afr[kq][i], bh, bl, acc[i][c]);
        }
      } else {
#pragma unroll
      for (int j4 = 0; j4 < 4; ++j4) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(cur + (kq * 16 + j4 * 4 + q) * BN);
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            acc[i][c] = fused_mfma(afr[kq][i][j4], b4[c], acc[i][c]);
      }
      }
    }
    if (NBUF > 1 && st + 1 < NSTAGE) {
      if (DEEP && ((st + 1) & 1)) patch_store_from(st + 1, sB + ((st + 1) & 1) * BK * BN, pw);
      else patch_store(st + 1, sB + ((st + 1) & 1) * BK * BN);
    }
    __syncthreads();
  }

  FSTAMP(2);        // K loop (conv2 MFMAs, next stage's patches)
  // ---- epilogue of conv2: this lane holds channels o = (wm_i*WM+i)*16 + 4q + r at pixels (oy, ox .. ox+3)
  if (LATE) { load_epilogue_ops(); load_skip_ops(); }
  float prgb[3][4];
  float mxn = 0.f;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int c = 0; c < 4; ++c) prgb[ch][c] = 0.f;
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int obase = (wm_i * WM + i) * 16 + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      f32x4 v = {acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      if constexpr (SPLIT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] *= k2in;                // exact: conv2's weights carried 2^8, act1 2^-e1
      }
      // (chained split form: v = out2 2^-e2 from here on -- the B operand of the next GEMM; the ToRGB sums are scaled back once)
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = (CIPS3D_FUSED_AB & 16) ? v[c] : lrelu02(fmaf(nw2_u, nz2[c], v[c]) + bias4[i][r]) * kact2;
      if (NEXT) {   // keep the activated value where the accumulator was: it is the next GEMM's B operand
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c][r] = v[c];
      }
      if (store_out2) {
        // (uniform: sample, the wave's strip, channel 16 (wm_i WM + i) + r; the lane adds its channel quarter and pixel, vo_q)
        f32x4* dst = reinterpret_cast<f32x4*>(reinterpret_cast<char*>(a.out2) +
                                              ((int64_t)b * a.g.out2_bs + ((int64_t)((wm_i * WM + i) * 16 + r) * HWo + pix_u) * 4) + vo_q * 4u);
        if constexpr (NEXT && SPLIT) *dst = f32x4{v[0] * kback2, v[1] * kback2, v[2] * kback2, v[3] * kback2};
        else *dst = v;
      }
      if (to_rgb && !(CIPS3D_FUSED_AB & 4)) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float w = s_wrgb[ch * C + obase + r];
#pragma unroll
          for (int c = 0; c < 4; ++c) prgb[ch][c] = fmaf(w, v[c], prgb[ch][c]);
        }
      }
    }
  }
  FSTAMP(3);        // conv2 epilogue (noise, bias, leaky ReLU, ToRGB partial sums, out2 store)
  // ---- NEXT: the next stage's low-resolution GEMM y_next = Wn out2 from the registers.  acc[i][c][r] is channel
  // 16 (wm_i WM + i) + 4 q + r of pixel c: with Wn in the chained pack that IS the B operand of k-step r of k-group
  // (wm_i WM + i).  Each wave row covers its own WM k-groups (split K); rows 1.. park their partial in the (now free) B
  // stages and row 0 adds them in order and stores.
  constexpr int OTN = NEXT ? C / 32 : 1;           // o-tiles of the C/2 output channels
  // Wide stage (C = 256: eight wave rows over the same 64 pixels, eight output tiles): split K would need a 224 KB
  // exchange of partials.  Instead the ACTIVATIONS are exchanged: in two rounds half of the wave rows drop their 32
  // channels into the dead B stages (32 KB, lane-linear: the lane that produced a k-step's fragment is the lane that
  // needs it), and every wave accumulates ITS output tile over the full K.
  constexpr bool XCHG = NEXT && XPREF && OTN % WGM == 0 && WGM % 2 == 0;
  if (XCHG) {
    constexpr int GR = (WGM / 2) * WM;             // k-groups (16 channels) per round
    constexpr int TPW = XCHG ? OTN / WGM : 1;      // output tiles per wave
    static_assert(!XCHG || WGN * GR * 4 * 256 <= NBUF * BK * BN, "half of the activations must fit the B stages");
    const ubase_t an = reinterpret_cast<ubase_t>(a.wm_next) + ((int64_t)b * (C / 2) * C + wm_i * TPW * (C / 16) * 256) * 4;
    float* sx = sB + wn_i * GR * 4 * 256 + lane * 4;            // this pixel set's exchange area
    f32x4 accx[TPW][4];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
      for (int c = 0; c < 4; ++c) accx[tp][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
      f32x4 af[TPW][GR];
#pragma unroll
      for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
        for (int gl = 0; gl < GR; ++gl)
          af[tp][gl] = *reinterpret_cast<const f32x4*>(an + (tp * (C / 16) + rd * GR + gl) * 1024 + vo_a);
      if (wm_i / (WGM / 2) == rd) {
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            *reinterpret_cast<f32x4*>(sx + (((wm_i % (WGM / 2)) * WM + i) * 4 + r) * 256) =
                SPLIT ? f32x4{pack_split(acc[i][0][r]), pack_split(acc[i][1][r]), pack_split(acc[i][2][r]), pack_split(acc[i][3][r])}
                      : f32x4{acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
      }
      __syncthreads();
#pragma unroll
      for (int gl = 0; gl < GR; ++gl) {
        f32x4 bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bv[r] = *reinterpret_cast<const f32x4*>(sx + (gl * 4 + r) * 256);
        if (BF16) {
          s16x4 bh[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) bh[c] = pack_bf16(bv[0][c], bv[1][c], bv[2][c], bv[3][c]);
#pragma unroll
          for (int tp = 0; tp < TPW; ++tp) {
            const s16x4 ah = pack_bf16(af[tp][gl][0], af[tp][gl][1], af[tp][gl][2], af[tp][gl][3]);
#pragma unroll
            for (int c = 0; c < 4; ++c) accx[tp][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, bh[c], accx[tp][c], 0, 0, 0);
          }
        } else if constexpr (SPLIT) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            h4 bh, bl;
            unpack_frag(bv[0][c], bv[1][c], bv[2][c], bv[3][c], bh, bl);
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp) accx[tp][c] = split_mfma16(af[tp][gl], bh, bl, accx[tp][c]);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
              for (int c = 0; c < 4; ++c)
                accx[tp][c] = fused_mfma(af[tp][gl][r], bv[r][c], accx[tp][c]);
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
      char* ynb = reinterpret_cast<char*>(a.y_next) + ((int64_t)b * a.g.ynext_bs + ((int64_t)((wm_i * TPW + tp) * 16) * HWo + pix_u) * ES);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ys = SPLIT ? kyn : 1.f;                  // the chained weights carried 2^8 as well, out2 2^-e2
        const f32x4 yv = {accx[tp][0][r] * ys, accx[tp][1][r] * ys, accx[tp][2][r] * ys, accx[tp][3][r] * ys};
        mxn = fmaxf(fmaxf(fmaxf(fabsf(yv[0]), fabsf(yv[1])), fmaxf(fabsf(yv[2]), fabsf(yv[3]))), mxn);
        ylo_t* yn = reinterpret_cast<ylo_t*>(ynb + (int64_t)(r * HWo) * ES + vo_q * ES);
        if constexpr (YB) cips3d_store_wt8(yn, pack_bf16(yv[0], yv[1], yv[2], yv[3]));
        else cips3d_store_wt16(yn, yv);
      }
    }
    if (amax_measured) {     // the workgroup's largest |y_next| raises one slot of the sample's amax array; s_nz1 is dead (K loop over)
      static_assert(!NEXT || 4 * WGM * WGN <= BN, "the reduction words fit the noise tile");
      const float m = cips3d_workgroup_max(mxn, s_nz1, wave, lane, WGM * WGN);
      if (tid == 0) cips3d_amax_raise_if(a.next_amax + b * CIPS3D_AMAX_FLOATS, m, blockIdx.x);
    }
  }
  f32x4 accn[OTN][4];
  if (NEXT && !XCHG) {
    static_assert(!NEXT || XCHG || (WGM - 1) * WGN * OTN * 4 * 64 * 4 <= NBUF * BK * BN * 4, "split-K partials must fit the B stages");
    const ubase_t an = reinterpret_cast<ubase_t>(a.wm_next) + ((int64_t)b * (C / 2) * C + wm_i * WM * 256) * 4;      // packed [ot'][kq][256]
    f32x4 afn[OTN][WM];
#pragma unroll
    for (int t = 0; t < OTN; ++t)
#pragma unroll
      for (int i = 0; i < WM; ++i)
        afn[t][i] = *reinterpret_cast<const f32x4*>(an + (t * (C / 16) + i) * 1024 + vo_a);
#pragma unroll
    for (int t = 0; t < OTN; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c) accn[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      if (BF16) {
        s16x4 bh[4], ah[OTN];
#pragma unroll
        for (int c = 0; c < 4; ++c) bh[c] = pack_bf16(acc[i][c][0], acc[i][c][1], acc[i][c][2], acc[i][c][3]);
#pragma unroll
        for (int t = 0; t < OTN; ++t) ah[t] = pack_bf16(afn[t][i][0], afn[t][i][1], afn[t][i][2], afn[t][i][3]);
#pragma unroll
        for (int t = 0; t < OTN; ++t)
#pragma unroll
          for (int c = 0; c < 4; ++c) accn[t][c] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah[t], bh[c], accn[t][c], 0, 0, 0);
      } else if constexpr (SPLIT) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          h4 bh, bl;
          split_frag(acc[i][c][0], acc[i][c][1], acc[i][c][2], acc[i][c][3], bh, bl);
#pragma unroll
          for (int t = 0; t < OTN; ++t) accn[t][c] = split_mfma16(afn[t][i], bh, bl, accn[t][c]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int t = 0; t < OTN; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c)
              accn[t][c] = fused_mfma(afn[t][i][r], acc[i][c][r], accn[t][c]);
      }
    }
    if (wm_i > 0) {
      float* sp = sB + ((((wm_i - 1) * WGN + wn_i) * OTN * 4) * 256 + lane * 4);
#pragma unroll
      for (int t = 0; t < OTN; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) *reinterpret_cast<f32x4*>(sp + (t * 4 + c) * 256) = accn[t][c];
    }
  }
  FSTAMP(4);        // chained next-stage GEMM (MFMAs)
  if (!to_rgb && !NEXT) { FSTAMP_FLUSH(); return; }
  // ---- ToRGB: reduce over the 4 lane quarters, then over the WGM wave rows through LDS
  if (to_rgb) {
    // Quarter q ends up with colour channel q of the wave's four pixels, in the order the shuffles added them ((q0 + q1) + (q2 +
    // q3): same bits).  v_permlane16_swap exchanges the odd 16-lane rows of its first operand with the even rows of the second,
    // v_permlane32_swap the upper half of the first with the lower half of the second: two colours share a register after
    // the first step, all three after the second -- 3 swaps + 3 adds per pixel where the ds_bpermute form spent 6 + 6.
    // (not at C = 32: the swaps work in place on both operands, the copies do not fit that instantiation's 64 registers)
    if constexpr (MINW >= 8) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float v = prgb[ch][c];
          v += __shfl_xor(v, 16, 64);
          v += __shfl_xor(v, 32, 64);
          prgb[ch][c] = (NEXT && SPLIT) ? v * kback2 : v;
        }
      if (q == 0) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          *reinterpret_cast<f32x4*>(s_red + (wm_i * 3 + ch) * BN + nloc) =
              f32x4{prgb[ch][0], prgb[ch][1], prgb[ch][2], prgb[ch][3]};
      }
    } else {
    f32x4 tot;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const auto rg = __builtin_amdgcn_permlane16_swap(__float_as_uint(prgb[0][c]), __float_as_uint(prgb[1][c]), false, false);
      const auto bb = __builtin_amdgcn_permlane16_swap(__float_as_uint(prgb[2][c]), __float_as_uint(prgb[2][c]), false, false);
      const float p = __uint_as_float(rg[0]) + __uint_as_float(rg[1]);        // [R01, G01, R23, G23] by quarter
      const float u = __uint_as_float(bb[0]) + __uint_as_float(bb[1]);        // [B01, B01, B23, B23]
      const auto h = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(u), false, false);
      const float v = __uint_as_float(h[0]) + __uint_as_float(h[1]);          // [R, G, B, B]
      tot[c] = (NEXT && SPLIT) ? v * kback2 : v;
    }
    if (q < 3) *reinterpret_cast<f32x4*>(s_red + (wm_i * 3 + q) * BN + nloc) = tot;
    }
  }
  __syncthreads();
  if (NEXT && !XCHG && wm_i == 0) {
#pragma unroll
    for (int m = 1; m < WGM; ++m) {
      const float* sp = sB + ((((m - 1) * WGN + wn_i) * OTN * 4) * 256 + lane * 4);
#pragma unroll
      for (int t = 0; t < OTN; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const f32x4 pv4 = *reinterpret_cast<const f32x4*>(sp + (t * 4 + c) * 256);
#pragma unroll
          for (int r = 0; r < 4; ++r) accn[t][c][r] += pv4[r];
        }
    }
    char* ynb = reinterpret_cast<char*>(a.y_next) + ((int64_t)b * a.g.ynext_bs + (int64_t)pix_u * ES);
#pragma unroll
    for (int t = 0; t < OTN; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ys = SPLIT ? kyn : 1.f;
        const f32x4 yv = {accn[t][0][r] * ys, accn[t][1][r] * ys, accn[t][2][r] * ys, accn[t][3][r] * ys};
        mxn = fmaxf(fmaxf(fmaxf(fabsf(yv[0]), fabsf(yv[1])), fmaxf(fabsf(yv[2]), fabsf(yv[3]))), mxn);
        ylo_t* yn = reinterpret_cast<ylo_t*>(ynb + (int64_t)((t * 16 + r) * HWo) * ES + vo_q * ES);
        if constexpr (YB) cips3d_store_wt8(yn, pack_bf16(yv[0], yv[1], yv[2], yv[3]));
        else cips3d_store_wt16(yn, yv);
      }
  }
  if (NEXT && !XCHG && amax_measured) {     // (only wave row 0 stored: the other rows bring 0)
    const float m = cips3d_workgroup_max(mxn, s_nz1, wave, lane, WGM * WGN);
    if (tid == 0) cips3d_amax_raise_if(a.next_amax + b * CIPS3D_AMAX_FLOATS, m, blockIdx.x);
  }
  FSTAMP(5);        // partial exchange of the chained GEMM / ToRGB through LDS, y_next store
  if (!to_rgb) { FSTAMP_FLUSH(); return; }
  if (rgb_lane) {                     // quarter q finishes colour channel q
    const int ch = q;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < WGM; ++m) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(s_red + (m * 3 + ch) * BN + nloc);
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] += t[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] += rgb_bias;
    if (skip_any) {
      if (skip_fir) {
        float so[2][4];
        up2_fir(skp, kf, so);
        const int py = oy & 1;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += py ? so[1][c] : so[0][c];
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] += skv[c];
      }
    }
    // (uniform: sample and the wave's strip; the lane adds its colour plane and pixel)
    char* rb = reinterpret_cast<char*>(a.rgb) + (int64_t)b * a.g.rgb_bs;
    const unsigned vo_rgb = (unsigned)(ch * HWo) + pix_l;
    if (rgb_u8) {
      // CIPS3D_RGB_U8: the image leaves as uint8 -- cips3d_rgb_to_uint8's arithmetic (clamp to [-1, 1], (c + 1) 127.5, round to
      // nearest even) on the value that would have been stored: the multi-view loop's img_tensor_to_pil step
      // (render_video_web_v10.py:1825-1826) without the fp32 image's round trip through memory
      unsigned pk = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) pk |= cips3d_quant_u8(v[c]) << (8 * c);
      *reinterpret_cast<unsigned*>(rb + (int64_t)pix_u + vo_rgb) = pk;
    } else {
      cips3d_store_wt16(reinterpret_cast<float*>(rb + (int64_t)pix_u * 4 + vo_rgb * 4u), v);
    }
  }
  FSTAMP(6);        // rgb: bias, FIR of the skip, store
  FSTAMP_FLUSH();
}

// ---- the instantiations of fused_up_conv_kernel.  Seven base shapes: C, WM, WGM, WGN, RW, BK, MINW | NEXT, XPREF, LATE.
template <int C_, int WM_, int WGM_, int WGN_, int RW_, int BK_, int MINW_, bool NEXT_, bool XPREF_, bool LATE_>
struct StageBase {
  static constexpr int C = C_, WM = WM_, WGM = WGM_, WGN = WGN_, RW = RW_, BK = BK_, MINW = MINW_;
  static constexpr bool NEXT = NEXT_, XPREF = XPREF_, LATE = LATE_;
};
// tile shapes / register budgets picked by sweep on MI355X (profiles/r01_i_*): time per stage in the comment
// C = 32 (one K stage): with the epilogue's operands (noise2, bias2, skip patch) requested after the MFMAs instead of up
// front the kernel needs 71 instead of 93 registers: seven instead of five resident waves per SIMD, -6 us at 1024^2
// (round 5, what bounds it: 503.6 VALU instructions per wave x 32 768 waves = 64.5 k issue cycles per SIMD = 30.7 us of its
// 37.3 -- the stage is VALU-issue bound.  With no arithmetic (-DCIPS3D_FUSED_AB=60) 201.7 VALU / 26.2 us, with no loads either
// (252) 136.8 VALU / 16.7 us.  Not the wave launch rate: a wave that owns all 32 channels of its 64 pixels (<32, 2, 1, 4, 1, 32,
// 4>: half the waves, no cross-wave ToRGB exchange) takes 39.6 against 39.4 us on one box, eight waves per workgroup 41.0.  The
// conv2 epilogue written as channel-pair v_pk_*_f32 by hand: 37.4 against 37.5 -- hipcc's SLP pass had packed it already.)
typedef StageBase<32, 1, 2, 2, 1, 32, 8, false, false, true> SB_32U;   // 2 rows x 64, 4 waves             46 us @1024^2
typedef StageBase<64, 2, 2, 2, 1, 16, 4, false, false, false> SB_64U;   // 2 rows x 64, 4 waves, BK 16      42 us @512^2
typedef StageBase<128, 4, 2, 4, 1, 32, 2, false, false, false> SB_128U;   // 4 rows x 64                      33 us @256^2
typedef StageBase<256, 2, 8, 1, 2, 64, 2, false, false, false> SB_256U;   // 2 rows x 32: 256 workgroups at 128^2
// chained (cips3d_fused_up_conv_chains(C)).  C = 128: 2 rows x 64 with four waves (512 workgroups) beats the unchained kernel's
// 4 x 64 / eight waves by 3 us once the chained GEMM is in (sweep on one box, whole-view time)
// XPREF, how the stage's activations reach the chained GEMM: exchanged through LDS, every wave owning output tiles over the
// full K (C = 256: the only form that fits; C = 64: -2.7 us per view against split K), or split K over the wave rows
// with the partials added through LDS (C = 128: a tie, kept)
// LATE: epilogue operands requested after the MFMAs -- at C = 64 / 128 that removes the spills of the chained form, -2 us /
// neutral; at C = 256 it measured +1 us and stays off
typedef StageBase<64, 2, 2, 2, 1, 16, 4, true, true, true> SB_64C;
typedef StageBase<128, 4, 2, 2, 1, 32, 2, true, false, true> SB_128C;
typedef StageBase<256, 2, 8, 1, 2, 64, 2, true, true, false> SB_256C;
// Forms: what cips3d_decoder_steps plus the stage call of forward.hip produce for the shipped generators (FFHQ 128^2 .. 1024^2 on
// a 64^2 NeRF: up-sampling stages C = 256 -> 128 -> 64 chained and C = 32 last, the blocks above the image size flat) -- both noise
// maps, ToRGB with the skip image, no out2; fp32 / bf16 / bf16 storage with no range pointers, split with the range workspace, where
// the stage in front of the last one (C = 64) publishes the bound of |y_next| and the others measure it; the last stage with an
// fp32 or a uint8 image -- each compiled apart; everything else the entry points accept (no noise map, no skip, out2 stored, no
// ToRGB, the split mode without a workspace, ...) runs on the one generic form of its base, precision and kind.  stage_form()
// looks a launch up; a launch that no row takes is CIPS3D_E_UNSUPP and nothing is enqueued.
typedef void (*stage_kernel_t)(FusedArgs);
struct StageForm { int C, next, flat, prec, feat; stage_kernel_t kernel; };
template <class B, int PREC, bool FLAT, int FEAT>
constexpr StageForm stage_form_row() {
  return {B::C, B::NEXT, FLAT, PREC, FEAT,
          fused_up_conv_kernel<B::C, B::WM, B::WGM, B::WGN, B::RW, B::BK, B::MINW, PREC, B::NEXT, B::XPREF, B::LATE, FLAT, FEAT>};
}
#define STAGE_FORM(B, PREC, FLAT, FEAT) stage_form_row<B, PREC, FLAT, FEAT>()
constexpr int SF_LAYER = SF_NOISE1 | SF_NOISE2 | SF_RGB;
// the shipped forms of one precision; RG: the range bits of the split mode (else 0), MEAS / BND: ... of a chained stage
#define STAGE_FORMS_UP(PREC, RG, MEAS, BND)                                                                           \
  STAGE_FORM(SB_256C, PREC, false, SF_LAYER | SF_SKIP_UP | RG | MEAS),   /* 64^2 -> 128^2                  */ \
  STAGE_FORM(SB_128C, PREC, false, SF_LAYER | SF_SKIP_UP | RG | MEAS),   /* 128^2 -> 256^2                 */ \
  STAGE_FORM(SB_64C, PREC, false, SF_LAYER | SF_SKIP_UP | RG | BND),     /* 256^2 -> 512^2, feeds the last */ \
  STAGE_FORM(SB_32U, PREC, false, SF_LAYER | SF_SKIP_UP | RG),           /* 512^2 -> 1024^2: the image     */ \
  STAGE_FORM(SB_32U, PREC, false, SF_LAYER | SF_SKIP_UP | RG | SF_U8)
// (flat blocks of a smaller image.  Compiled apart for the default precision and for bf16 storage only: with the rows of plain
// bf16 and exact fp32 as well this file compiled longer than nerf.hip, the floor of the build -- those run on the generic forms)
#define STAGE_FORMS_FLAT(PREC, RG, MEAS, BND)                                                                         \
  STAGE_FORM(SB_128C, PREC, true, SF_LAYER | SF_SKIP | RG | MEAS), STAGE_FORM(SB_64C, PREC, true, SF_LAYER | SF_SKIP | RG | BND), \
  STAGE_FORM(SB_32U, PREC, true, SF_LAYER | SF_SKIP | RG), STAGE_FORM(SB_32U, PREC, true, SF_LAYER | SF_SKIP | RG | SF_U8)
#define STAGE_GENERIC(B)                                                                                                                 \
  STAGE_FORM(B, 0, false, SF_GENERIC), STAGE_FORM(B, 1, false, SF_GENERIC), STAGE_FORM(B, 2, false, SF_GENERIC),                \
  STAGE_FORM(B, 3, false, SF_GENERIC), STAGE_FORM(B, 0, true, SF_GENERIC), STAGE_FORM(B, 1, true, SF_GENERIC),                  \
  STAGE_FORM(B, 2, true, SF_GENERIC), STAGE_FORM(B, 3, true, SF_GENERIC)
const StageForm stage_forms[] = {
    STAGE_FORMS_UP(0, 0, 0, 0),
    STAGE_FORMS_UP(1, 0, 0, 0),
    STAGE_FORMS_UP(2, 0, 0, 0), STAGE_FORMS_FLAT(2, 0, 0, 0),
    STAGE_FORMS_UP(3, SF_RANGED, SF_AMAX, SF_BOUND), STAGE_FORMS_FLAT(3, SF_RANGED, SF_AMAX, SF_BOUND),
    STAGE_GENERIC(SB_32U), STAGE_GENERIC(SB_64U), STAGE_GENERIC(SB_128U), STAGE_GENERIC(SB_256U),
    STAGE_GENERIC(SB_64C), STAGE_GENERIC(SB_128C), STAGE_GENERIC(SB_256C),
};
#undef STAGE_GENERIC
#undef STAGE_FORMS_FLAT
#undef STAGE_FORMS_UP
#undef STAGE_FORM

// what a launch does, as SF_* bits (the kernel's generic form reads the same from FusedArgs)
int stage_features(const FusedArgs& a) {
  const bool rgb = a.wm_rgb != nullptr, next = a.wm_next != nullptr, ranged = a.bf16 == 3 && a.x_amax;
  const bool bound = next && a.next_amax && a.next_gain > 0.f;
  return ((a.noise1 && a.nw1) ? SF_NOISE1 : 0) | ((a.noise2 && a.nw2) ? SF_NOISE2 : 0) | (rgb ? SF_RGB : 0) |
         ((rgb && a.skip) ? ((!a.flat && (a.skip_up & 1)) ? SF_SKIP_UP : SF_SKIP) : 0) | (a.out2 ? SF_OUT2 : 0) | (ranged ? SF_RANGED : 0) |
         ((next && a.next_amax && !bound) ? SF_AMAX : 0) | ((bound && ranged) ? SF_BOUND : 0) | ((rgb && (a.skip_up & 2)) ? SF_U8 : 0);
}

// The form of a launch: the row compiled for exactly what it does, else the generic row of its base, else NULL.  (A bound that
// nobody would write -- next_gain > 0 without the range workspace -- is no feature: such a launch records nothing, as before.)
const StageForm* stage_form(int C, const FusedArgs& a) {
  const int feat = stage_features(a), next = a.wm_next != nullptr;
  const StageForm* generic = nullptr;
  for (const StageForm& f : stage_forms) {
    if (f.C != C || f.next != next || f.flat != a.flat || f.prec != a.bf16) continue;
    if (f.feat & SF_GENERIC) generic = &f;
    else if (f.feat == feat) return &f;
  }
  return generic;
}

// the launch-invariant part of FusedArgs (see there and cips3d_stage_geom); BN = 128 pixels per workgroup in every form
int stage_geometry(int C, bool chained, int H, int W, int skip_up, cips3d_stage_geom* g) {
  const bool flat = (skip_up & CIPS3D_STAGE_FLAT) != 0;
  if (!(flat ? cips3d_fused_flat_conv_supported(C, H, W) : cips3d_fused_up_conv_supported(C, H, W))) return CIPS3D_E_UNSUPP;
  if (chained && !cips3d_fused_up_conv_chains(C)) return CIPS3D_E_UNSUPP;
  // (RW, WGN, waves of the base shapes above)
  const int rw = C == 256 ? 2 : 1, wgn = C == 256 ? 1 : (C == 128 && !chained) ? 4 : 2, waves = C <= 64 || (C == 128 && chained) ? 4 : 8;
  const int up = flat ? 1 : 2, OH = up * H, OW = up * W;
  *g = cips3d_stage_geom{};
  g->tile_h = rw * wgn; g->tile_w = 64 / rw; g->threads = 64 * waves;
  g->tiles_x = OW / g->tile_w; g->tiles_y = OH / g->tile_h;
  g->tx_shift = -1;
  for (int s = 0; s < 31; ++s)
    if (g->tiles_x == (1 << s)) g->tx_shift = s;
  g->tx_rcp = g->tiles_x > 1 ? (uint32_t)((((uint64_t)1 << 32) / (uint64_t)g->tiles_x) + 1) : 0u;    // (tiles_x = 1: shift 0)
  g->HWlo = H * W; g->HWo = OH * OW;
  const int64_t es = (skip_up & CIPS3D_Y_BF16) ? 2 : 4;
  g->ylo_bs = (int64_t)C * g->HWlo * es;
  g->out2_bs = (int64_t)C * g->HWo * 4;
  g->ynext_bs = (int64_t)(C / 2) * g->HWo * es;
  g->rgb_bs = (int64_t)3 * g->HWo * ((skip_up & CIPS3D_RGB_U8) ? 1 : 4);
  g->skip_bs = (int64_t)3 * ((!flat && (skip_up & 1)) ? g->HWlo : g->HWo) * 4;
  return 0;
}

}  // namespace

extern "C" int cips3d_fused_stage_geometry(int C, int chained, int H, int W, int skip_up, cips3d_stage_geom* geom) {
  if (!geom || H <= 0 || W <= 0) return CIPS3D_E_BADARG;
  return stage_geometry(C, chained != 0, H, W, skip_up, geom);
}

#ifdef CIPS3D_FUSED_STAMPS
extern "C" int cips3d_debug_read_fused_stamps(unsigned long long* out32) {
  hipDeviceSynchronize();
  hipMemcpyFromSymbol(out32, HIP_SYMBOL(g_fused_stamps), 256);
  unsigned long long z[32] = {0};
  hipMemcpyToSymbol(HIP_SYMBOL(g_fused_stamps), z, 256);
  return 0;
}
#endif

extern "C" int cips3d_fused_up_conv_supported(int C, int H, int W) {
  // (the kernel keeps intra-sample offsets in 32 bits: C * 2H * 2W must stay below 2^31)
  return (C == 32 || C == 64 || C == 128 || C == 256) && W % 32 == 0 && H % 2 == 0 && H >= 2 &&
         (int64_t)C * 4 * H * W < ((int64_t)1 << 31);
}

extern "C" int cips3d_fused_flat_conv_supported(int C, int H, int W) {
  // the same tiles over an H x W output: 64 pixels per wave row, up to 4 image rows per workgroup
  return (C == 32 || C == 64 || C == 128 || C == 256) && W % 64 == 0 && H % 4 == 0 && H >= 4 &&
         (int64_t)C * H * W < ((int64_t)1 << 31);
}

extern "C" int cips3d_fused_up_conv(const float* y_lo, const float* fir, const float* noise1, int64_t noise1_bstride,
                                    const float* noise_w1, const float* bias1, const float* wm2, const float* noise2,
                                    int64_t noise2_bstride, const float* noise_w2, const float* bias2, float* out2,
                                    const float* wm_rgb, const float* bias_rgb, const float* skip, int skip_up,
                                    float* rgb, int B, int C, int H, int W, const cips3d_range* rg, void* stream) {
  return cips3d_fused_up_conv_next(y_lo, fir, noise1, noise1_bstride, noise_w1, bias1, wm2, noise2, noise2_bstride, noise_w2,
                                   bias2, out2, wm_rgb, bias_rgb, skip, skip_up, rgb, nullptr, nullptr, B, C, H, W, rg, stream);
}

extern "C" int cips3d_fused_up_conv_chains(int C) { return C == 64 || C == 128 || C == 256; }

extern "C" int cips3d_fused_up_conv_next(const float* y_lo, const float* fir, const float* noise1, int64_t noise1_bstride,
                                         const float* noise_w1, const float* bias1, const float* wm2, const float* noise2,
                                         int64_t noise2_bstride, const float* noise_w2, const float* bias2, float* out2,
                                         const float* wm_rgb, const float* bias_rgb, const float* skip, int skip_up,
                                         float* rgb, const float* wm_next, float* y_next, int B, int C, int H, int W,
                                         const cips3d_range* rg, void* stream) {
  const int flat = (skip_up & CIPS3D_STAGE_FLAT) ? 1 : 0;
  if (!y_lo || (!fir && !flat) || !bias1 || !wm2 || !bias2 || B < 0 || H <= 0 || W <= 0) return CIPS3D_E_BADARG;
  if (flat && (skip_up & 1)) return CIPS3D_E_BADARG;           // a flat stage's skip image has the output's size
  if ((wm_next == nullptr) != (y_next == nullptr)) return CIPS3D_E_BADARG;
  if (wm_next && !cips3d_fused_up_conv_chains(C)) return CIPS3D_E_UNSUPP;
  if (!out2 && !wm_rgb && !wm_next) return CIPS3D_E_BADARG;
  if (wm_rgb && (!bias_rgb || !rgb)) return CIPS3D_E_BADARG;
  if (!(flat ? cips3d_fused_flat_conv_supported(C, H, W) : cips3d_fused_up_conv_supported(C, H, W))) return CIPS3D_E_UNSUPP;
  if (B == 0) return 0;
  FusedArgs a{y_lo, fir, noise1, noise1_bstride, noise_w1, bias1, wm2, noise2, noise2_bstride, noise_w2, bias2, out2,
              wm_rgb, bias_rgb, skip, (skip_up & 1) | ((skip_up & CIPS3D_RGB_U8) ? 2 : 0), rgb, B, H, W,
              (skip_up & CIPS3D_GEMM_SPLIT) ? 3 : (skip_up & CIPS3D_GEMM_BF16) ? ((skip_up & CIPS3D_Y_BF16) ? 2 : 1) : 0, wm_next,
              y_next, rg ? rg->x_amax : nullptr, rg ? rg->lconst : nullptr, rg ? rg->lconst2 : nullptr,
              rg ? rg->next_amax : nullptr, rg ? rg->next_gain : 0.f, flat};
  // split mode with range tracking: the bound of act1 needs conv1's constants, the chained form conv2's as well
  if ((skip_up & CIPS3D_GEMM_SPLIT) && rg && rg->x_amax && (!rg->lconst || (wm_next && !rg->lconst2))) return CIPS3D_E_BADARG;
  if ((skip_up & CIPS3D_Y_BF16) && !(skip_up & CIPS3D_GEMM_BF16)) return CIPS3D_E_BADARG;   // bf16 storage implies bf16 operands
  if ((skip_up & CIPS3D_GEMM_SPLIT) && (skip_up & CIPS3D_GEMM_BF16)) return CIPS3D_E_BADARG;
  if (const int rc = stage_geometry(C, wm_next != nullptr, H, W, skip_up, &a.g)) return rc;
  a.nz1_bs = noise1_bstride * 4;
  a.nz2_bs = noise2_bstride * 4;
  const StageForm* f = stage_form(C, a);
  if (!f) return CIPS3D_E_UNSUPP;
  hipLaunchKernelGGL(f->kernel, dim3((unsigned)(a.g.tiles_x * a.g.tiles_y), 1, (unsigned)B), dim3((unsigned)a.g.threads), 0,
                     as_stream(stream), a);
  return cips3d_launch_status();
}

