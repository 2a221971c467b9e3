// Eikonal and minimal-surface losses of the SDF head with their gradient to the FiLM table, on gfx950: the reference's two
// generator-side regularisers (exp/stylesdf/losses.py:13-24 applied to autograd.grad(sdf, pts, create_graph=True),
// cips3d/nerf_utils.py:221-228) as ONE kernel that runs the forward-mode pass of nerf_sdf_grad.hip and then a reverse sweep over it.
//
//   L = lam_e mean((|g| - 1)^2) + lam_m mean(exp(-beta_ms |sdf|)),    g = d sdf / d pts,   mean over the M = B R N points
//
// Forward (the arithmetic of nerf_sdf_grad.hip, same column layout: 4 points x {value, t_x, t_y, t_z} per 16-column MFMA tile).
// With s = 2 / (far - near), FiLM rows (gamma_l, beta_l), c_l = gamma_l b_l + beta_l:
//   layer 0         p_0 = W0 p_n,       A_0^j = W0[:, j] s
//   layer l >= 1    p_l = W_l x_{l-1},  A_l^j = W_l T_{l-1}^j
//   z_l = gamma_l p_l + c_l,  x_l = sin z_l,  T_l^j = cos z_l gamma_l A_l^j,    sdf = w_s . x_{D-1} + b_s,  g_j = w_s . T_{D-1}^j
// Seeds:  gbar = lam_e 2 (|g| - 1) / |g| g / M (0 where |g| = 0),  sbar = -lam_m beta_ms sign(sdf) exp(-beta_ms |sdf|) / M.
// Reverse, from xbar = sbar w_s, Tbar^j = gbar_j w_s, for l = D-1 .. 0, Q = sum_j Tbar^j A_l^j:
//   zbar = xbar cos z_l - Q sin z_l gamma_l
//   dgamma_l += sum_points zbar (p_l + b_l) + Q cos z_l,     dbeta_l += sum_points zbar
//   l > 0:  xbar <- W_l^T (zbar gamma_l),  Tbar^j <- W_l^T (Tbar^j cos z_l gamma_l)
// The FiLM table is the render kernel's plain one (gamma, beta as stored, no 2 pi folded in): dfilm is taken with respect to its
// entries.  The view layer is not part of the SDF: its row of dfilm is written as zeros.  No gradient to the points, the camera or
// the renderer's own weights.
//
// Work decomposition.  As nerf_sdf_grad.hip: one 512-thread workgroup walks a grid-stride sequence of 32-point steps of one view,
// the eight waves share the weight slabs through the 2-slot LDS-DMA ring.  Per step the ring carries the (D-1) x 4 slabs of the
// exact-fp32 stream `packed32` for the forward sweep and then the same number of slabs of `packed32_t` -- the same packing of the
// transposed matrices, layers in reverse order -- for the reverse sweep.  The forward sweep writes every layer's accumulators
// (p_l on the value lanes, A_l^j on the tangent lanes: 4 H floats per point and layer) to a scratch area private to the
// workgroup; each lane reads back only what it wrote itself, so no ordering between lanes is needed.  In the reverse sweep the
// epilogue of the matrix step that completes xbar / Tbar for 64 units of layer l - 1 applies that layer's reverse formulas to them
// at once, so that it overlaps the partner wave's matrix block like the forward epilogue does.
//
// Reductions: no floating-point atomics.  dgamma / dbeta accumulate per (workgroup, wave, point slot) in a workspace array that
// only the owning value lane reads and writes (plain stores on the first step, read-add-write afterwards: padded points carry zero
// seeds and add exact zeros).  The two loss sums are per-lane fp64, folded over a workgroup in fixed order through LDS.  A second
// launch sums the slots and the workgroups in fixed order: values and dfilm are bit-identical from run to run (for one grid, i.e.
// one device and one workspace size).
//
// Arithmetic: all products on v_mfma_f32_16x16x4_f32, k ascending; sine and cosine share sin_accurate's Cody-Waite reduction
// (the polynomials of nerf_sdf_grad.hip's film_sincos).
#include <atomic>

#include "common.h"
#include "nerf_mlp.h"

namespace {

constexpr int GPTS = 4;              // points per wave step
constexpr int WG_PTS = GPTS * WAVES; // points per workgroup step
constexpr int NTH = WAVES * 64;
constexpr int EIK_NT = 16, EIK_TPS = 4, EIK_H = EIK_NT * 16;

struct EikArgs {
  cips3d_nerf_params p;
  const float* packed32_t;   // [(D-1)][H*H]: packed32's packing of W_l^T, l = D-1 .. 1
  float* scratch;            // [wg][D][NT][NTH][4]   the forward sweep's accumulators
  float* acc;                // [wg][D][2][WAVES][NT][GPTS][16]   dgamma / dbeta per point slot
  double* loss_part;         // [wg][2]
  int points;                // per view: R * N
  int wgs_per_view;
  int iters;                 // steps per workgroup (uniform over the grid)
  int values_only;
  float t_end, t_step;       // nerf_linspace_consts (nerf_geom.h)
  float lam_e, lam_m, beta_ms, inv_m;
};

// sin(x) and cos(x) from one reduction: nerf_sdf_grad.hip's film_sincos with both polynomials returned
__device__ __forceinline__ void sin_cos(float x, float& sn, float& cs) {
  const float INV_PI = 0.318309886183790672f;
  const float PI_HI = 3.14159274101257324f;
  const float PI_LO = -8.74227765734758577e-8f;
  const float k = rintf(x * INV_PI);
  float r = fmaf(k, -PI_HI, x);
  r = fmaf(k, -PI_LO, r);
  const float s = r * r;
  float p = fmaf(s, -2.3889859e-08f, 2.7525562e-06f);
  p = fmaf(p, s, -1.9840874e-04f);
  p = fmaf(p, s, 8.3333310e-03f);
  p = fmaf(p, s, -1.6666667e-01f);
  const float ys = fmaf(r * s, p, r);
  float c = fmaf(s, -1.1470745597729725e-11f, 2.08767569878681e-09f);
  c = fmaf(c, s, -2.7557319223985893e-07f);
  c = fmaf(c, s, 2.4801587301587302e-05f);
  c = fmaf(c, s, -1.3888888888888889e-03f);
  c = fmaf(c, s, 4.1666666666666664e-02f);
  c = fmaf(c, s, -0.5f);
  const float yc = fmaf(c, s, 1.f);
  const int sign = (int)k << 31;
  sn = __int_as_float(__float_as_int(ys) ^ sign);
  cs = __int_as_float(__float_as_int(yc) ^ sign);
}

// sin(x) on the value lanes, cos(x) on the tangent lanes (the forward sweep needs one of them per lane: one select, no divergence)
__device__ __forceinline__ float sin_or_cos(float x, bool tangent) {
  float sn, cs;
  sin_cos(x, sn, cs);
  return __int_as_float(tangent ? __float_as_int(cs) : __float_as_int(sn));
}

// DPP within the quad of a point's four columns: lane 0's value in all four; the sum of the four in all four (fixed order)
template <int CTRL>
__device__ __forceinline__ float quad_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float quad_first(float v) { return quad_dpp<0x00>(v); }
__device__ __forceinline__ float quad_sum(float v) {
  v += quad_dpp<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  return v + quad_dpp<0x4E>(v); // quad_perm [2, 3, 0, 1]
}

// FiLM rows of layer l at units o4 .. o4 + 3: (gamma, gamma * bias + beta), from the staged table or from memory
template <int H, bool FILM_LDS>
__device__ __forceinline__ void film_rows(const float* s_film, const float* film_b, const float* layer_bias, int l, int o4, f32x4& g4,
                                          f32x4& c4) {
  if constexpr (FILM_LDS) {
    g4 = *reinterpret_cast<const f32x4*>(s_film + (l * 2) * H + o4);
    c4 = *reinterpret_cast<const f32x4*>(s_film + (l * 2 + 1) * H + o4);
  } else {
    g4 = *reinterpret_cast<const f32x4*>(film_b + (l * 2) * H + o4);
    const f32x4 bt = *reinterpret_cast<const f32x4*>(film_b + (l * 2 + 1) * H + o4);
    const f32x4 lb = *reinterpret_cast<const f32x4*>(layer_bias + l * H + o4);
#pragma unroll
    for (int i = 0; i < 4; ++i) c4[i] = fmaf(g4[i], lb[i], bt[i]);
  }
}

// The ring of a step: `fwd_slabs` slabs of packed32, then (gradient calls) as many of packed32_t
struct EikRing {
  const float* fwd;
  const float* rev;
  float* lds;
  int seq, seq_end;
  int per_step;     // fwd_slabs or 2 * fwd_slabs
  int fwd_slabs;
  template <int SLAB>
  __device__ __forceinline__ const float* slab_src(int s) const {
    const int n = s % per_step;
    return n < fwd_slabs ? fwd + (int64_t)n * SLAB : rev + (int64_t)(n - fwd_slabs) * SLAB;
  }
};

// One H x H matrix layer for the wave's 16 columns, in mfma_layer's slab protocol (nerf_mlp.h): slab `seq` is resident in slot
// seq & 1, every step prefetches seq + 1 while multiplying and ends with wait + barrier; the upper half of the waves takes the
// barrier in front of its epilogue.  epi(sl, acc) consumes the step's TPS accumulator tiles (output units 64 sl + 16 tt + 4 q + i);
// post(sl, acc) runs behind both barriers (global stores whose acknowledgement nobody should wait for at the barrier).
template <int NT, int TPS, class Epi, class Post>
__device__ __forceinline__ void matrix_layer(const f32x4 (&X)[NT], EikRing& ring, int wave, int lane, Epi&& epi, Post&& post) {
  constexpr int H = NT * 16;
  constexpr int TILE = 16 * H;
  constexpr int SLAB = TILE * TPS;
  constexpr int STEPS = NT / TPS;
  const bool late_epilogue = __builtin_amdgcn_readfirstlane(wave) >= WAVES / 2;
#pragma unroll
  for (int sl = 0; sl < STEPS; ++sl) {
    if (ring.seq + 1 < ring.seq_end)
      stage_slab<SLAB>(ring.template slab_src<SLAB>(ring.seq + 1), ring.lds + ((ring.seq + 1) & 1) * SLAB, wave, lane);
    const float* slab = ring.lds + (ring.seq & 1) * SLAB;
    f32x4 acc[TPS];
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      f32x4 fr[2][TPS];
      auto load_tile = [&](int buf, int T) __attribute__((always_inline)) {
#pragma unroll
        for (int tt = 0; tt < TPS; ++tt) fr[buf][tt] = *reinterpret_cast<const f32x4*>(slab + tt * TILE + (T * 64 + lane) * 4);
      };
      load_tile(0, 0);
#pragma unroll
      for (int T = 0; T < NT; ++T) {
        const int cur = T & 1;
#pragma unroll
        for (int tt = 0; tt < TPS; ++tt) asm volatile("" : "+v"(fr[cur][tt]));
        if (T + 1 < NT) load_tile(cur ^ 1, T + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)        // k ascending
#pragma unroll
          for (int tt = 0; tt < TPS; ++tt)
            acc[tt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[cur][tt][r], X[T][r], acc[tt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if (late_epilogue) {
      __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's piece of slab seq + 1 has landed
      __syncthreads();
    }
    epi(sl, acc);
    if (!late_epilogue) {
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
    post(sl, acc);
    ++ring.seq;
  }
}

// XG: explicit sample points (cips3d_nerf_params.x_pts) instead of camera-generated rays
template <int NT, int TPS, bool XG, bool FILM_LDS>
__global__ void __launch_bounds__(NTH, 2) nerf_eikonal_kernel(EikArgs a) {
  constexpr int H = NT * 16;
  constexpr int SLAB = 16 * H * TPS;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const cips3d_nerf_params& P = a.p;
  const int D = P.depth;
  float* ringmem = lds;                                   // 2 * SLAB
  float* s_film = ringmem + 2 * SLAB;                     // [D][2][H] (FILM_LDS)
  float* s_w0 = s_film + (FILM_LDS ? D * 2 * H : 0);      // [3][H] first-layer weights, transposed
  float* s_ws = s_w0 + 3 * H;                             // [H]    sigma head

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int qd = lane >> 4;
  const int kind = lane & 3;                              // 0: value column, 1..3: d / dx, dy, dz
  const bool tangent = kind != 0;
  const bool grads = a.values_only == 0;                  // uniform

  const int b = blockIdx.x / a.wgs_per_view;              // uniform over the workgroup
  const int wv = blockIdx.x - b * a.wgs_per_view;
  const int N = P.n_samples;
  const int S = P.img_size;
  const int R = P.n_rays > 0 ? P.n_rays : S * S;
  const float* film_b = P.film + (int64_t)b * (D + 1) * 2 * H;
  // this lane's pieces of the workgroup's private areas
  float* scr0 = a.scratch + ((int64_t)blockIdx.x * D * NT * NTH + tid) * 4;                        // + (l * NT + T) * NTH * 4
  float* accp0 = a.acc + (int64_t)blockIdx.x * D * 2 * (WAVES * NT * GPTS * 16) +
                (wave * NT * GPTS + ((lane >> 2) & 3)) * 16 + 4 * qd;   // + ((l * 2 + j) * WAVES * NT + T) * GPTS * 16

  if constexpr (FILM_LDS) {
    for (int i = tid; i < D * H; i += NTH) {
      const int l = i / H, o = i - l * H;
      const float gm = film_b[(l * 2) * H + o], bt = film_b[(l * 2 + 1) * H + o], lb = P.layer_bias[i];
      s_film[(l * 2) * H + o] = gm;
      s_film[(l * 2 + 1) * H + o] = fmaf(gm, lb, bt);
    }
  }
  for (int i = tid; i < 3 * H; i += NTH) {
    const int k = i / H, o = i - k * H;
    s_w0[i] = P.w_first[o * 3 + k];
  }
  for (int i = tid; i < H; i += NTH) s_ws[i] = P.w_sigma[i];
  const float b_sigma = P.b_sigma[0];

  const float nearv = P.near_[b], farv = P.far_[b];
  const float span = cips3d_uniform(farv - nearv);
  const NerfDepths zs{nearv, farv, a.t_end, a.t_step, N};

  EikRing ring;
  ring.fwd = P.packed32;
  ring.rev = a.packed32_t;
  ring.lds = ringmem;
  ring.seq = 0;
  ring.fwd_slabs = (D - 1) * (NT / TPS);
  ring.per_step = grads ? 2 * ring.fwd_slabs : ring.fwd_slabs;
  ring.seq_end = a.iters * ring.per_step;
  if (ring.seq_end > 0) stage_slab<SLAB>(ring.fwd, ringmem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  double sum_e = 0.0, sum_m = 0.0;      // this lane's loss sums (value lanes of quarter 0)

  for (int it = 0; it < a.iters; ++it) {
    // ---- the lane's point (nerf_sdf_grad.hip): steps past the end are computed on the last point with zero seeds
    const int64_t p64 = ((int64_t)wv + (int64_t)it * a.wgs_per_view) * WG_PTS + wave * GPTS + ((lane >> 2) & 3);
    const bool live = p64 < a.points;
    const int pt = live ? (int)p64 : a.points - 1;
    float ptx, pty, ptz;
    if constexpr (XG) {
      const float* pp = P.x_pts + ((int64_t)b * a.points + pt) * 3;
      ptx = pp[0]; pty = pp[1]; ptz = pp[2];
    } else {
      const int ray = pt / N, sk = pt - ray * N;
      const float focal = P.focals[b];
      const float* cw = P.cam_poses + 12 * b;
      const NerfCamRay cam = nerf_cam_ray(focal, cw, S, ray);
      const float z0 = zs.zbase(sk);
      const float z = P.perturb_u ? zs.zoffset(z0, zs.zbase(sk + 1), P.perturb_u[(int64_t)b * R + ray]) : z0;
      ptx = cw[3] + cam.dx * z; pty = cw[7] + cam.dy * z; ptz = cw[11] + cam.dz * z;
    }
    const float nx = ptx * 2.f / span, ny = pty * 2.f / span, nz = ptz * 2.f / span;
    const float dn = 2.f / span;                          // d p_n / d p
    // (opaque zero in every table offset of the iteration: keeps the loop-invariant tables out of registers, as in nerf.hip)
    int opq = 0;
    asm volatile("" : "+v"(opq));
    const int q4o = 4 * qd + opq;
    // (and the lane's private-area pointers: hoisted, their per-tile addresses were 52 spilled registers)
    float* scr = scr0;
    float* accp = accp0;
    asm volatile("" : "+v"(scr), "+v"(accp));

    f32x4 X[NT], Y[NT];
    float head = 0.f;         // this lane's partial of w_sigma . column
    // ---- forward, layer 0: 3 -> H on the VALU, straight into the D layout
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      const int o4 = T * 16 + q4o;
      f32x4 g4, c4;
      film_rows<H, FILM_LDS>(s_film, film_b, P.layer_bias, 0, o4, g4, c4);
      const f32x4 wx = *reinterpret_cast<const f32x4*>(s_w0 + o4);
      const f32x4 wy = *reinterpret_cast<const f32x4*>(s_w0 + H + o4);
      const f32x4 wz = *reinterpret_cast<const f32x4*>(s_w0 + 2 * H + o4);
      f32x4 res, pre4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pre = fmaf(wz[i], nz, fmaf(wy[i], ny, wx[i] * nx));
        const float f = sin_or_cos(fmaf(g4[i], pre, c4[i]), tangent);
        const float wk = kind == 1 ? wx[i] : (kind == 2 ? wy[i] : wz[i]);
        pre4[i] = tangent ? wk * dn : pre;
        res[i] = tangent ? (g4[i] * f) * (wk * dn) : f;
      }
      if (D == 1) {
        const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) head = fmaf(ws4[i], res[i], head);
      }
      if (grads) *reinterpret_cast<f32x4*>(scr + (int64_t)T * NTH * 4) = pre4;
      X[T] = res;
    }
    // ---- forward, hidden layers 1 .. D-1
    for (int l = 1; l < D; ++l) {
      const bool last = l == D - 1;
      matrix_layer<NT, TPS>(
          X, ring, wave, lane,
          [&](int sl, f32x4(&acc)[TPS]) __attribute__((always_inline)) {
#pragma unroll
            for (int tt = 0; tt < TPS; ++tt) {
              const int o4 = sl * (TPS * 16) + tt * 16 + q4o;
              f32x4 g4, c4;
              film_rows<H, FILM_LDS>(s_film, film_b, P.layer_bias, l, o4, g4, c4);
              f32x4 res;
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const float av = quad_first(acc[tt][i]);
                const float f = sin_or_cos(fmaf(g4[i], av, c4[i]), tangent);
                res[i] = tangent ? (g4[i] * f) * acc[tt][i] : f;
              }
              if (last) {
                const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
                for (int i = 0; i < 4; ++i) head = fmaf(ws4[i], res[i], head);
              }
              asm volatile("" : "+v"(res));      // (keeps the activations above the barrier that follows: the stagger)
              Y[sl * TPS + tt] = res;
            }
          },
          [&](int sl, f32x4(&acc)[TPS]) __attribute__((always_inline)) {
            if (grads) {
#pragma unroll
              for (int tt = 0; tt < TPS; ++tt)
                *reinterpret_cast<f32x4*>(scr + ((int64_t)l * NT + sl * TPS + tt) * NTH * 4) = acc[tt];
            }
          });
#pragma unroll
      for (int T = 0; T < NT; ++T) X[T] = Y[T];
    }
    // ---- head and losses: sdf on the value lanes, g_j on the tangent lanes, |g| over the quad
    head += __shfl_xor(head, 16, 64);
    head += __shfl_xor(head, 32, 64);
    const float sdf = quad_first(head) + b_sigma;
    const float nrm = sqrtf(quad_sum(tangent ? head * head : 0.f));
    const float em = expf(-a.beta_ms * fabsf(sdf));
    if (live && qd == 0 && !tangent) {
      sum_e += (double)((nrm - 1.f) * (nrm - 1.f));
      sum_m += (double)em;
    }
    if (!grads) continue;       // uniform

    // ---- seeds: the column's scalar times w_sigma
    float seed;
    {
      const float ge = nrm > 0.f ? (a.lam_e * 2.f * (nrm - 1.f) / nrm) * head * a.inv_m : 0.f;
      const float sg = sdf > 0.f ? 1.f : (sdf < 0.f ? -1.f : 0.f);
      const float sb = -(a.lam_m * a.beta_ms) * sg * em * a.inv_m;
      seed = live ? (tangent ? ge : sb) : 0.f;
    }
    // The reverse formulas of layer l at units o4 .. o4 + 3: xb = xbar (value lanes) / Tbar^j (tangent lanes) -> the column of
    // the next transposed product, zbar gamma / Tbar^j cos z gamma; the value lanes add their point's share of dgamma, dbeta
    auto reverse_units = [&](int l, int T, const f32x4& xb) __attribute__((always_inline)) -> f32x4 {
      const int o4 = T * 16 + q4o;
      f32x4 g4, c4;
      film_rows<H, FILM_LDS>(s_film, film_b, P.layer_bias, l, o4, g4, c4);
      const f32x4 pa = *reinterpret_cast<const f32x4*>(scr + ((int64_t)l * NT + T) * NTH * 4);
      f32x4 u, dg, db;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float av = quad_first(pa[i]);
        float sn, cs;
        sin_cos(fmaf(g4[i], av, c4[i]), sn, cs);
        const float Q = quad_sum(tangent ? xb[i] * pa[i] : 0.f);
        const float zb = xb[i] * cs - (Q * sn) * g4[i];
        dg[i] = Q * cs;       // + zbar (p + b) below
        db[i] = zb;
        u[i] = (tangent ? xb[i] * cs : zb) * g4[i];
      }
      if (!tangent) {
        const f32x4 lb = *reinterpret_cast<const f32x4*>(P.layer_bias + l * H + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) dg[i] = fmaf(db[i], pa[i] + lb[i], dg[i]);
        float* ag = accp + ((int64_t)(l * 2) * WAVES * NT + T) * (GPTS * 16);
        float* ab = ag + (int64_t)WAVES * NT * GPTS * 16;
        if (it > 0) {
          const f32x4 og = *reinterpret_cast<const f32x4*>(ag), ob = *reinterpret_cast<const f32x4*>(ab);
#pragma unroll
          for (int i = 0; i < 4; ++i) { dg[i] += og[i]; db[i] += ob[i]; }
        }
        *reinterpret_cast<f32x4*>(ag) = dg;
        *reinterpret_cast<f32x4*>(ab) = db;
      }
      return u;
    };
    // ---- reverse, layer D-1 from the seeds
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + T * 16 + q4o);
      f32x4 xb;
#pragma unroll
      for (int i = 0; i < 4; ++i) xb[i] = seed * ws4[i];
      X[T] = reverse_units(D - 1, T, xb);
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- reverse, W_l^T for l = D-1 .. 1: the step that completes 64 units of layer l - 1 applies that layer's formulas
    for (int l = D - 1; l >= 1; --l) {
      matrix_layer<NT, TPS>(
          X, ring, wave, lane,
          [&](int sl, f32x4(&acc)[TPS]) __attribute__((always_inline)) {
#pragma unroll
            for (int tt = 0; tt < TPS; ++tt) {
              f32x4 u = reverse_units(l - 1, sl * TPS + tt, acc[tt]);
              asm volatile("" : "+v"(u));
              Y[sl * TPS + tt] = u;
              __builtin_amdgcn_sched_barrier(0);      // one tile at a time: the four tiles' loads hoisted together spilled
            }
          },
          [&](int, f32x4(&)[TPS]) __attribute__((always_inline)) {});
#pragma unroll
      for (int T = 0; T < NT; ++T) X[T] = Y[T];
    }
  }

  // ---- the workgroup's loss sums, folded in fixed order: 4 value lanes of quarter 0 per wave, 8 waves
  __syncthreads();
  double* s_loss = reinterpret_cast<double*>(ringmem);
  if (qd == 0 && !tangent) {
    const int slot = wave * GPTS + (lane >> 2);
    s_loss[slot * 2] = sum_e;
    s_loss[slot * 2 + 1] = sum_m;
  }
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int i = 0; i < WG_PTS; ++i) s += s_loss[i * 2 + tid];
    a.loss_part[(int64_t)blockIdx.x * 2 + tid] = s;
  }
}

// Second launch: dfilm[b][l][j][o] = the sum of the view's workgroups and their 32 point slots in fixed order (the view layer's
// row: zeros); block 0 also sums the workgroups' fp64 loss partials into the two means.
__global__ void __launch_bounds__(256) nerf_eikonal_reduce_kernel(const float* __restrict__ acc, const double* __restrict__ loss_part,
                                                                  float* __restrict__ dfilm, double* __restrict__ loss_out, int B,
                                                                  int D, int wgs_per_view, double inv_m) {
  constexpr int H = EIK_H, NT = EIK_NT;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    double s = 0.0;
    for (int w = 0; w < B * wgs_per_view; ++w) s += loss_part[(int64_t)w * 2 + threadIdx.x];
    loss_out[threadIdx.x] = s * inv_m;
  }
  if (!dfilm || i >= B * (D + 1) * 2 * H) return;
  const int o = i % H, j = (i / H) % 2, l = (i / (2 * H)) % (D + 1), b = i / (2 * H * (D + 1));
  float s = 0.f;
  if (l < D) {
    const int T = o >> 4, within = o & 15;
    for (int w = 0; w < wgs_per_view; ++w) {
      const float* base = acc + (int64_t)(b * wgs_per_view + w) * D * 2 * (WAVES * NT * GPTS * 16) +
                          (int64_t)(l * 2 + j) * (WAVES * NT * GPTS * 16) + T * (GPTS * 16) + within;
      for (int wave = 0; wave < WAVES; ++wave) {
        const float* pw = base + wave * (NT * GPTS * 16);
        s += (pw[0] + pw[16]) + (pw[32] + pw[48]);
      }
    }
  }
  dfilm[i] = s;
}

constexpr size_t eik_lds_bytes(int H, int TPS, int D, bool film_lds) {
  return sizeof(float) * ((size_t)2 * 16 * H * TPS + (film_lds ? (size_t)D * 2 * H : 0) + 4 * (size_t)H);
}

template <int NT, int TPS, bool XG, bool FILM_LDS>
int launch_eikonal_x(const EikArgs& a, hipStream_t st) {
  constexpr int H = NT * 16;
  const size_t lds_bytes = eik_lds_bytes(H, TPS, a.p.depth, FILM_LDS);
  if (lds_bytes > 160 * 1024) return CIPS3D_E_UNSUPP;
  // the attribute is per device and the flag is shared by host threads (launch_render_x)
  static std::atomic<unsigned long long> attr_set{0};
  int dev_id = 0;
  if (hipError_t e = hipGetDevice(&dev_id); e != hipSuccess) return (int)e;
  const unsigned long long bit = 1ull << (dev_id & 63);
  if (dev_id >= 64 || !(attr_set.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nerf_eikonal_kernel<NT, TPS, XG, FILM_LDS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL((nerf_eikonal_kernel<NT, TPS, XG, FILM_LDS>), dim3((unsigned)(a.p.B * a.wgs_per_view)), dim3(NTH), lds_bytes, st, a);
  return cips3d_launch_status();
}

// bytes of one workgroup's share of the workspace: scratch + point-slot accumulators (gradient calls) + the two fp64 loss partials
constexpr int64_t eik_scratch_floats(int D) { return (int64_t)D * EIK_NT * NTH * 4; }
constexpr int64_t eik_acc_floats(int D) { return (int64_t)D * 2 * WAVES * EIK_NT * GPTS * 16; }
int64_t eik_wg_bytes(int D, bool values_only) {
  return 16 + (values_only ? 0 : 4 * (eik_scratch_floats(D) + eik_acc_floats(D)));
}

}  // namespace

extern "C" int cips3d_nerf_eikonal_supported(int hidden, int depth) { return hidden == EIK_H && depth >= 1 && depth <= 64 ? 1 : 0; }

extern "C" int64_t cips3d_nerf_eikonal_workspace_bytes(int hidden, int depth, int workgroups, int values_only) {
  if (!cips3d_nerf_eikonal_supported(hidden, depth) || workgroups < 1) return 0;
  return (int64_t)workgroups * eik_wg_bytes(depth, values_only != 0);
}

extern "C" int cips3d_nerf_eikonal_loss(const cips3d_nerf_params* p, const float* packed32_t, float lambda_eikonal,
                                        float lambda_minimal_surface, float beta_ms, int values_only, void* workspace,
                                        int64_t workspace_bytes, double* loss_out, float* dfilm_out, void* stream) {
  if (!p || !loss_out || !workspace || workspace_bytes <= 0) return CIPS3D_E_BADARG;
  const cips3d_nerf_params& P = *p;
  if (P.B < 0 || P.img_size <= 0 || P.n_samples <= 0 || P.depth < 1 || P.hidden <= 0) return CIPS3D_E_BADARG;
  if (!cips3d_nerf_eikonal_supported(P.hidden, P.depth)) return CIPS3D_E_UNSUPP;
  const bool vo = values_only != 0;
  if (!vo && !dfilm_out) return CIPS3D_E_BADARG;
  if (!P.near_ || !P.far_ || !P.w_first || !P.film || !P.layer_bias || !P.w_sigma || !P.b_sigma ||
      (P.depth > 1 && (!P.packed32 || (!vo && !packed32_t))))
    return CIPS3D_E_BADARG;
  if (P.x_pts ? P.n_rays <= 0 : (!P.cam_poses || !P.focals || P.n_rays != 0)) return CIPS3D_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return CIPS3D_E_BADARG;
  if (P.B == 0) return CIPS3D_E_BADARG;                    // a mean over no points
  const int64_t points = (int64_t)(P.n_rays > 0 ? (int64_t)P.n_rays : (int64_t)P.img_size * P.img_size) * P.n_samples;
  if (points > 0x7fffffff) return CIPS3D_E_UNSUPP;
  int dev_id = 0, cus = 0;
  if (hipError_t e = hipGetDevice(&dev_id); e != hipSuccess) return (int)e;
  if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id); e != hipSuccess) return (int)e;
  if (cus < 1) cus = 1;
  // one workgroup per compute unit, as many as the workspace has room for, at least one per view
  const int64_t per_wg = eik_wg_bytes(P.depth, vo);
  const int64_t room = workspace_bytes / per_wg;
  if (room < P.B) return CIPS3D_E_BADARG;
  const int64_t steps = ceil_div<int64_t>(points, WG_PTS);
  int64_t wpv = ceil_div<int64_t>(cus, P.B);
  if (wpv > room / P.B) wpv = room / P.B;
  if (wpv > steps) wpv = steps;
  EikArgs a;
  a.p = P;
  a.packed32_t = packed32_t;
  a.points = (int)points;
  a.iters = (int)ceil_div<int64_t>(steps, wpv);
  a.wgs_per_view = (int)ceil_div<int64_t>(steps, a.iters);
  const int64_t wgs = (int64_t)P.B * a.wgs_per_view;
  if (wgs > 0x7fffffff) return CIPS3D_E_UNSUPP;
  a.values_only = vo ? 1 : 0;
  // workspace: [scratch of every workgroup][accumulators of every workgroup][loss partials]
  float* wsf = static_cast<float*>(workspace);
  a.scratch = wsf;
  a.acc = wsf + (vo ? 0 : wgs * eik_scratch_floats(P.depth));
  a.loss_part = reinterpret_cast<double*>(a.acc + (vo ? 0 : wgs * eik_acc_floats(P.depth)));
  nerf_linspace_consts(P.n_samples, a.t_end, a.t_step);
  a.lam_e = lambda_eikonal;
  a.lam_m = lambda_minimal_surface;
  a.beta_ms = beta_ms;
  const double inv_m = 1.0 / ((double)P.B * (double)points);
  a.inv_m = (float)inv_m;
  hipStream_t st = as_stream(stream);
  int rc;
  if (eik_lds_bytes(EIK_H, EIK_TPS, P.depth, true) <= 160 * 1024)
    rc = P.x_pts ? launch_eikonal_x<EIK_NT, EIK_TPS, true, true>(a, st) : launch_eikonal_x<EIK_NT, EIK_TPS, false, true>(a, st);
  else
    rc = P.x_pts ? launch_eikonal_x<EIK_NT, EIK_TPS, true, false>(a, st) : launch_eikonal_x<EIK_NT, EIK_TPS, false, false>(a, st);
  if (rc != 0) return rc;
  const int total = P.B * (P.depth + 1) * 2 * EIK_H;
  hipLaunchKernelGGL(nerf_eikonal_reduce_kernel, dim3((unsigned)(vo ? 1 : ceil_div(total, 256))), dim3(256), 0, st, a.acc, a.loss_part,
                     vo ? nullptr : dfilm_out, loss_out, P.B, P.depth, a.wgs_per_view, inv_m);
  return cips3d_launch_status();
}
