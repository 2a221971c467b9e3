// Shared by the NeRF point-MLP kernels (nerf.hip: forward render; nerf_bwd_fused.hip: recompute + backward; nerf_sdf_grad.hip):
// operand fragment types, the task shape (NerfTaskShape: the one statement of groups / tasks_per_view / chunk that the render,
// the fused backward and the stash size share), the LDS weight ring, the split-fp16 conversion -- and the FORWARD LAYER itself:
// first_layer (3 -> H on the VALU) and mfma_layer (H -> H on the matrix cores, FiLM / sine epilogue, accumulator stash).  The
// render kernel and the backward's forward recompute (nerf_stash_kernel) both instantiate these two, so the accumulators either
// of them writes to the stash come from one text; they differ only in the view layer's sink (ViewComposite / ViewGdot below).
// See nerf.hip's header for the work decomposition and the arithmetic.
// A translation unit that wants the in-kernel stamps of a diagnostic build defines STAMP, STAMP_FLUSH, STAMP_PARAM and STAMP_ARG
// before it includes this header (nerf.hip under -DCIPS3D_STAMPS); otherwise they are nothing.
#pragma once
#include <type_traits>
#include "common.h"
#include "nerf_geom.h"

#ifndef STAMP
#define STAMP(i)
#define STAMP_FLUSH()
#define STAMP_PARAM
#define STAMP_ARG
#endif

// The staged FiLM table carries gamma' / 2 pi and c / 2 pi, so that the epilogue's FMA yields the
// sine argument in revolutions and v_sin_f32(fract(.)) takes it as it is -- one multiplication less per activation.  The extra
// rounding (of gamma' / 2 pi, once per table entry) perturbs the argument by |x| 2^-24 relative, the size of an ulp of gamma.
#define FILM_UNIT 0.159154943091895336f
#define FILM_SIN sin_revolutions

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));    // one MFMA 16x16x32 operand fragment (8 fp16 = 4 VGPRs)
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

constexpr int RAYS = 16;    // rays per wave task
constexpr int WAVES = 8;    // waves (tasks) per workgroup

struct NerfArgs {
  cips3d_nerf_params p;
  int groups;          // ray groups of 16 per view
  int tasks_per_view;  // groups * n_chunks rounded up to a multiple of WAVES
  int chunk;           // samples per chunk (uniform trip count)
  int fuse_finish;     // the workgroup's eight chunk waves combine their partials in LDS and write the final maps
  int pad_;             // (keeps the 8-byte alignment of what follows explicit)
  float t_end, t_step; // nerf_linspace_consts (nerf_geom.h), computed on the host (kernel arguments are
                       // re-readable scalars; computed in the kernel they ended up as spilled VGPR copies)
};

// The task shape of a launch: NerfArgs, FusedArgs and cips3d_nerf_bwd_fused_stash_floats take it from here, so that the kernel
// that fills the stash, the kernel that reads it and the caller that sizes it agree on its rows.
// (64-bit: the stash size is asked for before anything has checked the shape)
struct NerfTaskShape {
  int64_t groups;          // ray groups of 16 per view
  int64_t tasks_per_view;  // groups * n_chunks rounded up to a multiple of WAVES
  int64_t chunk;           // samples per chunk
  template <class Args>
  void to(Args& a) const { a.groups = (int)groups; a.tasks_per_view = (int)tasks_per_view; a.chunk = (int)chunk; }
};
inline NerfTaskShape nerf_task_shape(int64_t n_rays, int n_samples, int n_chunks) {
  const int64_t groups = ceil_div<int64_t>(n_rays, RAYS);
  return {groups, ceil_div<int64_t>(groups * n_chunks, WAVES) * WAVES, ceil_div(n_samples, n_chunks)};
}

// LDS floats of the render kernel: slab ring (or the 8 x 16 x H partial exchange of the fused finish, whichever is
// larger) + per-view tables (which double as the 8 x 8 x 16 scalar exchange once the last sample is done)
// pitch of one ray's partial in the exchange: H + 4 floats, so that the 16 rays of a wave start 16 bytes apart in the bank
// pattern (at pitch H every ray of a quarter hit the same banks: 8-way conflicts on the writes, 16-way on the combining reads)
__host__ __device__ constexpr int nerf_xf_pitch(int H) { return H + 4; }
__host__ __device__ constexpr int nerf_ring_floats(int H, int TPS, bool fuse) {
  return (fuse && WAVES * RAYS * nerf_xf_pitch(H) > 2 * 16 * H * TPS) ? WAVES * RAYS * nerf_xf_pitch(H) : 2 * 16 * H * TPS;
}


// ------------------------------------------------------------------------------------------------
// LDS-DMA of one weight slab (SLAB floats, linear copy, 1 KiB per wave-instruction)
// ------------------------------------------------------------------------------------------------
// one 1 KiB piece (the wave's 64 lanes x 16 bytes) of a linear copy global -> LDS
__device__ __forceinline__ void stage_piece(const float* __restrict__ gsrc, float* lds_dst, int piece, int lane) {
  // uniform base (SGPR pair, advanced on the scalar unit) + a 32-bit lane offset: the saddr form of the instruction.  With
  // a per-lane 64-bit pointer every piece needed a v_lshl_add_u64 into the same register pair first, and a wave's eight
  // DMA issues of a step ran one behind the other's address arithmetic
  const char* ub = reinterpret_cast<const char*>(gsrc + piece * 256);
  unsigned vo = lane * 16;
  // (both opaque: the optimiser otherwise re-associates the lane offset into the base, or hoists its zero extension out
  // of the block, where instruction selection no longer sees the base + zext(offset) shape the saddr form needs)
  asm volatile("" : "+s"(ub), "+v"(vo));
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)(ub + vo),
      (__attribute__((address_space(3))) void*)(lds_dst + piece * 256), 16, 0, 0);
}
template <int SLAB, int NW = WAVES>
__device__ __forceinline__ void stage_slab(const float* __restrict__ gsrc, float* lds_dst, int wave, int lane) {
  constexpr int PIECES = SLAB * 4 / 1024;
  constexpr int PER_WAVE = (PIECES + NW - 1) / NW;
#pragma unroll
  for (int j = 0; j < PER_WAVE; ++j) {
    const int piece = j * NW + wave;
    if (PIECES % NW == 0 || piece < PIECES) stage_piece(gsrc, lds_dst, piece, lane);
  }
}

// Per-wave streaming state of the weight ring.
struct Ring {
  const float* packed;   // global base of the packed stream (one sample's worth, repeated)
  float* lds;            // 2 slots
  int seq;               // slabs consumed so far
  int seq_end;           // total slabs this workgroup will consume
  int per_sample;        // slabs per sample
};

// x = hi + lo with hi = fp16(x), lo = fp16(x - hi): 22 significant bits in the 4 bytes of an fp32
__device__ __forceinline__ void split2(float x, _Float16& hi, _Float16& lo) {
  cips3d_split16(x, hi, lo);
}
// eight fp32 values (units 4q..4q+3 of tile 2m, then of tile 2m+1) -> the hi / lo B fragments of k-block m
// (cips3d_split_pair: one conversion and two v_fma_mix per two values instead of four instructions and a pack per value)
__device__ __forceinline__ void split8(const float (&v)[8], h8& hi, h8& lo) {
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  unsigned h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) cips3d_split_pair(v[2 * p], v[2 * p + 1], h[p], l[p]);
  hi = __builtin_bit_cast(h8, u32x4_t{h[0], h[1], h[2], h[3]});
  lo = __builtin_bit_cast(h8, u32x4_t{l[0], l[1], l[2], l[3]});
}

// ------------------------------------------------------------------------------------------------
// The forward layer
// ------------------------------------------------------------------------------------------------
// LDS floats of the per-view tables behind the ring: the FiLM table [L][2][H] + w_first^T, view-direction columns, sigma head, rgb head
__host__ __device__ constexpr int nerf_table_floats(int H, int L) { return L * 2 * H + 10 * H; }

// eight fp32 activations -> the (hi, lo) B fragments of a k-block; F32: their bits, as they are (see mfma_layer)
template <bool F32>
__device__ __forceinline__ void put8(const float (&v)[8], h8& hi, h8& lo) {
  if constexpr (F32) {
    hi = __builtin_bit_cast(h8, f32x4{v[0], v[1], v[2], v[3]});
    lo = __builtin_bit_cast(h8, f32x4{v[4], v[5], v[6], v[7]});
  } else {
    split8(v, hi, lo);
  }
}

// Layer 0: 3 -> H, in D layout, written as the B fragments of the first MFMA layer.  `sigma_here`: there is no hidden MFMA layer
// (D == 1), this is h_D and the sigma head's partial sum is taken from its fp32 values.
template <int NT, bool F32>
__device__ __forceinline__ void first_layer(h8 (&Oh)[NT / 2], h8 (&Ol)[NT / 2], float& sdf, bool sigma_here, const float* s_film,
                                            const float* s_w0, const float* s_ws, float nx, float ny, float nz, int q4o) {
  constexpr int H = NT * 16;
#pragma unroll
  for (int m = 0; m < NT / 2; ++m) {
    float v8[8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const int o4 = (2 * m + hf) * 16 + q4o;
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(s_film + o4);
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(s_film + H + o4);
      const f32x4 wx = *reinterpret_cast<const f32x4*>(s_w0 + o4);
      const f32x4 wy = *reinterpret_cast<const f32x4*>(s_w0 + H + o4);
      const f32x4 wz = *reinterpret_cast<const f32x4*>(s_w0 + 2 * H + o4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pre = fmaf(wz[i], nz, fmaf(wy[i], ny, wx[i] * nx));
        v8[hf * 4 + i] = FILM_SIN(fmaf(g4[i], pre, c4[i]));
      }
      if (sigma_here) {
        const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) sdf = fmaf(ws4[i], v8[hf * 4 + i], sdf);
      }
    }
    put8<F32>(v8, Oh[m], Ol[m]);
  }
}

// Where the view layer's features f go (the only thing the render and the recompute do differently with a layer):
template <int NT>
struct ViewComposite {              // render: FA += w f, the sample's share of the composited feature map
  static constexpr bool GDOT = false;
  float (&FA)[NT * 4];
  float w;
};
struct ViewGdot {                   // recompute: gdot += <dF[:, ray], f>, what the compositing backward needs of the features
  static constexpr bool GDOT = true;
  const float* dF_ray;
  float& gdot;
};
struct ViewNone {};                 // (a hidden layer)

// One MFMA layer for the wave's 16 points (split-fp16 products, fp32 accumulation; see nerf.hip's header).
//   hidden layer (View = ViewNone):  Y = sin(gamma' * (W' X) + c)     gamma' = gamma 2^-s, W' = 2^s W (s_film holds gamma')
//   view layer (VIEW, any other View): f = sin(gamma' * (W' X + Wd' v) + c);  f -> view (above);  rgb head partial sums += Wc f
//   last (hidden layers): Y is h_D, the sigma head's partial sum  sdf_acc += Ws . Y  is taken from the epilogue's fp32 values
// The caller guarantees slab `seq` is resident in slot (seq & 1); every slab step prefetches seq+1
// while multiplying and ends with wait + barrier.
// F32: the exact-fp32 instantiation (Generator.set_precision("fp32_exact"); cips3d_nerf_params.packed32): the same slabs, ring
// and register images hold fp32 -- a 1 KiB piece is a 16 x 16 block of W where the split stream has one plane of a 16 x 32
// block, (Xh[m], Xl[m]) are the bits of the fp32 activations of o-tiles 2m, 2m + 1 (the MFMA D layout IS the B operand of
// v_mfma_f32_16x16x4_f32: k-step r of k-quarter q <-> unit 16 T + 4 q + r), eight 32-cycle MFMAs per (tile, k-block) where the
// split kernel issues three 16-cycle ones.  Two waves per SIMD as in the split kernel: one wave's sine epilogue runs under
// the other's matrix block (a one-wave-per-SIMD form of the same arithmetic measured 252 us; this one: see DESIGN).
template <int NT, int TPS, bool STASH, bool F32 = false, class View>
__device__ __forceinline__ void mfma_layer(const h8 (&Xh)[NT / 2], const h8 (&Xl)[NT / 2], h8 (&Yh)[NT / 2], h8 (&Yl)[NT / 2],
                                           View view, float (&chead)[3], float& sdf_acc, bool last,
                                           Ring& ring, const float* film_l, const float* s_wd, const float* s_wc,
                                           const float* s_ws, float vx, float vy, float vz, float* stash_l, int wave, int lane, int q4o STAMP_PARAM) {
  constexpr bool VIEW = !std::is_same<View, ViewNone>::value;
  constexpr bool GDOT = std::is_same<View, ViewGdot>::value;
  constexpr int H = NT * 16;
  constexpr int TILE = 16 * H;          // floats (= 4-byte hi/lo pairs) of one o-tile's A fragments
  constexpr int SLAB = TILE * TPS;
  constexpr int STEPS = NT / TPS;
  constexpr int R = TPS * 4;            // output values produced per step
  constexpr int MB = NT / 2;            // 32-unit k-blocks of the layer input
  constexpr int BPS = TPS / 2;          // k-blocks of the NEXT layer's input a step completes
  static_assert(TPS % 2 == 0 && NT % TPS == 0, "a slab step must complete whole 32-unit blocks");
  // The slab steps of a layer are fully unrolled (with 96 fp16 MFMAs per step instead of 256 fp32 ones the whole kernel is
  // ~40 KB of code): the step index is a constant, results go straight to their final registers (the rolled loop of the
  // fp32 kernel had to rotate Yh / Yl / FA by 48 moves per step; unrolling measured 107.6 -> 101.0 us).
  // Epilogue stagger.  Waves w and w + WAVES/2 share a SIMD and meet at every slab barrier; with the barrier after the
  // FiLM/sine epilogue both would run its VALU instructions together while the matrix pipe idles.  The upper half of the
  // waves takes the step barrier BEFORE its epilogue instead, which then overlaps the partner wave's next-step MFMAs.  Either
  // position is after this wave's last read of slot (seq&1) and before its next stage_slab into it.
  // In-kernel stamps of this scheme (tools/run_kernel.py nerf on a -DCIPS3D_STAMPS build): the two matrix blocks of a SIMD
  // run together (~2.9k cycles for 192 MFMAs = the pipe is full), then the lower wave's epilogue (~1.3k) with the pipe idle;
  // a step is ~6.4k cycles.  Tried: a true half-period offset (two barriers per step, the upper half one barrier behind, so
  // that one wave's matrix block always faces the other's epilogue): correct, but 127 us instead of 97 -- a matrix block
  // that has the SIMD to itself is bound by its own A-fragment reads (8 x [8 ds_read_b128 -> wait -> 12 MFMAs]; the second
  // wave is what hides that latency today), and double-buffering the fragments needs 32 registers the kernel does not have.
  const bool late_epilogue = __builtin_amdgcn_readfirstlane(wave) >= WAVES / 2;
#pragma unroll
  for (int sl = 0; sl < STEPS; ++sl) {
    if (ring.seq + 1 < ring.seq_end) {
      const int nxt = (ring.seq + 1) % ring.per_sample;
      stage_slab<SLAB>(ring.packed + (int64_t)nxt * SLAB, ring.lds + ((ring.seq + 1) & 1) * SLAB, wave, lane);
    }
    STAMP(8);    // (in-layer stamps: the phase before the first one of a layer is charged to slot 12 / 11 of the previous step)
    const float* slab = ring.lds + (ring.seq & 1) * SLAB;
    const int o_base = sl * (TPS * 16) + q4o;          // this lane's first output unit of the step
    f32x4 acc[TPS];
    // (opaque per step: as loop invariants the operand copies of vx, vy, vz were hoisted out of the sample loop and spilled)
    float vxo = vx, vyo = vy, vzo = vz;
    if (VIEW) asm volatile("" : "+v"(vxo), "+v"(vyo), "+v"(vzo));
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) {
      const int o4 = o_base + tt * 16;
      if (VIEW) {       // view-direction columns (pre-scaled by 2^s at staging) straight into the accumulator
        const f32x4 wx = *reinterpret_cast<const f32x4*>(s_wd + o4);
        const f32x4 wy = *reinterpret_cast<const f32x4*>(s_wd + H + o4);
        const f32x4 wz = *reinterpret_cast<const f32x4*>(s_wd + 2 * H + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[tt][i] = fmaf(wz[i], vzo, fmaf(wy[i], vyo, wx[i] * vxo));
      } else {
        acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    // Matrix block, software-pipelined over half k-blocks.  History, all measured: 8 reads -> wait -> 12 MFMAs per k-block
    // (the form of the fp32 kernel) left each wave bound by 8 LDS round trips per step -- ~3.2k cycles for 1.5k of its own
    // matrix work (in-kernel stamps) -- 92.0 us; the next half's 4 reads requested before the current half's 6 MFMAs, through
    // the compiler (which drains lgkmcnt to 0 at every wait, the fresh prefetch included) 89.2 us; the wait provoked in FRONT
    // of the next reads (below) 87.3 us, matrix block ~2.0k cycles per step.
    // (nerf_bwd_fused.hip's mfma_step is this block as a function, for the backward's rolled steps; calling it from here
    // changed the render kernels' code, so the block stays spelled out)
    {
      constexpr int HT = TPS / 2;
      h8 fh[2][HT], fl[2][HT];
      auto load_half = [&](int buf, int m, int half) {
#pragma unroll
        for (int t = 0; t < HT; ++t) {
          const int tt = half * HT + t;
          fh[buf][t] = *reinterpret_cast<const h8*>(slab + tt * TILE + ((2 * m) * 64 + lane) * 4);
          fl[buf][t] = *reinterpret_cast<const h8*>(slab + tt * TILE + ((2 * m + 1) * 64 + lane) * 4);
        }
      };
      load_half(0, 0, 0);
#pragma unroll
      for (int g = 0; g < 2 * MB; ++g) {
        const int m = g >> 1, half = g & 1, cur = g & 1;
#pragma unroll
        for (int t = 0; t < HT; ++t) asm volatile("" : "+v"(fh[cur][t]), "+v"(fl[cur][t]));
        if (g + 1 < 2 * MB) load_half(cur ^ 1, (g + 1) >> 1, (g + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (F32) {      // fh / fl: the fp32 fragments of the k-block's two 16-unit halves; k ascending, the bit-exact chain
          const f32x4 x0 = __builtin_bit_cast(f32x4, Xh[m]), x1 = __builtin_bit_cast(f32x4, Xl[m]);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < HT; ++t)
              acc[half * HT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, fh[cur][t])[r], x0[r],
                                                                        acc[half * HT + t], 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < HT; ++t)
              acc[half * HT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(__builtin_bit_cast(f32x4, fl[cur][t])[r], x1[r],
                                                                        acc[half * HT + t], 0, 0, 0);
        } else {
#pragma unroll
        for (int t = 0; t < HT; ++t)
          acc[half * HT + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl[cur][t], Xh[m], acc[half * HT + t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < HT; ++t)
          acc[half * HT + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[cur][t], Xl[m], acc[half * HT + t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < HT; ++t)
          acc[half * HT + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh[cur][t], Xh[m], acc[half * HT + t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    STAMP(9);    // matrix block
    if (late_epilogue) {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's piece of slab seq+1 has landed
      __syncthreads();
    }
    STAMP(10);   // late waves: step barrier
    float res[R];
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) {
      const int o4 = o_base + tt * 16;
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(film_l + o4);
      const f32x4 c4 = *reinterpret_cast<const f32x4*>(film_l + H + o4);
      if constexpr (VIEW) {
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(s_wc + o4);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(s_wc + H + o4);
        const f32x4 w2 = *reinterpret_cast<const f32x4*>(s_wc + 2 * H + o4);
        f32x4 d4;
        if constexpr (GDOT) d4 = *reinterpret_cast<const f32x4*>(view.dF_ray + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float f = FILM_SIN(fmaf(g4[i], acc[tt][i], c4[i]));
          if constexpr (GDOT) view.gdot = fmaf(d4[i], f, view.gdot);
          else res[tt * 4 + i] = fmaf(view.w, f, view.FA[sl * R + tt * 4 + i]);
          chead[0] = fmaf(w0[i], f, chead[0]);
          chead[1] = fmaf(w1[i], f, chead[1]);
          chead[2] = fmaf(w2[i], f, chead[2]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) res[tt * 4 + i] = FILM_SIN(fmaf(g4[i], acc[tt][i], c4[i]));
        if (last) {     // h_D: sigma head partial (volume_renderer.py:148) from the fp32 values, before they are split
          const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
          for (int i = 0; i < 4; ++i) sdf_acc = fmaf(ws4[i], res[tt * 4 + i], sdf_acc);
        }
      }
    }
    // The sink pass would otherwise move the sines below the barrier that follows (undoing the stagger): make
    // the results opaque here.
    if constexpr (!GDOT) {
#pragma unroll
      for (int k = 0; k < R; ++k) asm volatile("" : "+v"(res[k]));
    } else {
      asm volatile("" : "+v"(view.gdot));
    }
    if (VIEW) asm volatile("" : "+v"(chead[0]), "+v"(chead[1]), "+v"(chead[2]));
    // fully unrolled steps: the step index is a constant, results go to their final places
    if constexpr (VIEW) {
      if constexpr (!GDOT) {
#pragma unroll
        for (int k = 0; k < R; ++k) view.FA[sl * R + k] = res[k];
      }
    } else {
#pragma unroll
      for (int bb = 0; bb < BPS; ++bb) {
        float v8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = res[(2 * bb) * 4 + j];
        put8<F32>(v8, Yh[sl * BPS + bb], Yl[sl * BPS + bb]);
      }
    }
    STAMP(11);   // epilogue
    // slab seq+1 has landed for every wave before anyone reads it / before slot (seq&1) is reused
    if (!late_epilogue) {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)  (expcnt/lgkmcnt untouched)
      __syncthreads();
    }
    STAMP(12);   // early waves: step barrier
    if constexpr (STASH) {
      // differentiable forward and forward recompute: the step's accumulators in register order [sl * TPS + tt][lane][4], for
      // nerf_bwd_kernel.  Issued after the step barrier, so that no store acknowledgement is waited for at it.
#pragma unroll
      for (int tt = 0; tt < TPS; ++tt) *reinterpret_cast<f32x4*>(stash_l + ((sl * TPS + tt) * 64 + lane) * 4) = acc[tt];
    }
    ++ring.seq;
  }
}


}  // namespace
