// Gradient of the SDF head with respect to the sample points, g = d sdf / d pts, on gfx950: the reference's eikonal term
// (autograd.grad(sdf, pts, ones), cips3d/nerf_utils.py:221-228, volume_renderer.py:223-226) as a forward-mode pass through the
// FiLM-SIREN trunk, fused in one kernel.  `pts` are the un-normalised world points, so the per-view factor 2 / (far - near) of
// normalize_points is part of g.
//
// Forward mode.  Per point the kernel carries the value h and the three tangents t_x, t_y, t_z = d h / d pts through the trunk.
// With s = 2 / (far - near), p_n = s p and the FiLM rows (gamma_l, beta_l) of the render kernel's table:
//   layer 0         a = W0 p_n + b0;   h = sin(gamma a + beta);   t_k = gamma cos(gamma a + beta) (.) W0[:, k] s
//   layer 1..D-1    a = W h + b;  u_k = W t_k;   h = sin(gamma a + beta);   t_k = gamma cos(gamma a + beta) (.) u_k
//   head            sdf = w_sigma . h + b_sigma;   g_k = w_sigma . t_k
// The view layer and the rgb head are not part of it.
//
// Work decomposition.  A hidden layer is the render kernel's GEMM Y^T = W X^T with FOUR B columns per point {h, t_x, t_y, t_z}:
// the 16 columns of a v_mfma_f32_16x16x4_f32 tile are 4 points x 4 columns, lane l holds column (l & 15) = point (l >> 2) & 3,
// kind l & 3 (0: value, 1..3: tangent), and the quarters l >> 4 are the four k-slices, exactly as in nerf.hip: the D layout of one
// layer is the B operand of the next, X and Y are 64 registers each.  In the epilogue a tangent lane needs the pre-activation of
// its point's value lane: a DPP quad broadcast.  One wave works on 4 points per step, a 512-thread workgroup on 32; the eight waves
// share the weight slabs of the exact-fp32 stream (cips3d_nerf_pack_weights32: the `packed32` of the render kernel) through the
// same 2-slot LDS-DMA ring and walk a grid-stride sequence of steps of one view, so that every wave of a workgroup meets every
// slab barrier.  Points are independent: no atomics, no cross-wave sums, results do not depend on the grid.
//
// Arithmetic.  Tangents are unbounded (|g| reaches tens at depth 8), unlike the sines the split-fp16 scheme of the render kernel
// relies on: the matrix products run on the exact fp32 instruction, k ascending as in the render kernel's exact instantiation.
// The activation is sin_accurate's Cody-Waite reduction by pi, then its odd polynomial on the value lanes and an even polynomial
// for the cosine of the SAME reduced argument on the tangent lanes (one select, no divergence).
#include <atomic>

#include "common.h"
#include "nerf_mlp.h"

namespace {

constexpr int GPTS = 4;              // points per wave step
constexpr int WG_PTS = GPTS * WAVES; // points per workgroup step

struct SdfGradArgs {
  cips3d_nerf_params p;
  float* grad;          // [B, points, 3]
  int points;           // per view: R * N
  int wgs_per_view;
  int iters;            // steps per workgroup (uniform over the grid)
  int pad_;
  float t_end, t_step;  // nerf_linspace_consts (nerf_geom.h)
};

// sin(x) on the value lanes (bit for bit sin_accurate), cos(x) on the tangent lanes: the same two-constant Cody-Waite reduction
// x = k pi + r, |r| <= pi/2, then the odd degree-11 polynomial of sin_accurate or the even degree-14 Taylor polynomial of the cosine
// (truncation (pi/2)^16 / 16! = 7e-11) on r, and the sign (-1)^k both share.
__device__ __forceinline__ float film_sincos(float x, bool tangent) {
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
  const float y = tangent ? yc : ys;
  return __int_as_float(__float_as_int(y) ^ ((int)k << 31));
}

// the value of quad lane 0 (the point's value column) in all four lanes of the quad
__device__ __forceinline__ float quad_first(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x00, 0xf, 0xf, true));
}

// FiLM rows of layer l at units o4 .. o4 + 3: (gamma, gamma * bias + beta).  FILM_LDS: from the staged table; else (networks
// whose table does not fit beside the ring) from the global arrays
template <int H, bool FILM_LDS>
__device__ __forceinline__ void film_rows(const float* s_film, const float* __restrict__ film_b, const float* __restrict__ layer_bias, int l,
                                          int o4, f32x4& g4, f32x4& c4) {
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

// One hidden layer for the wave's 16 columns: Y = act(W X), X / Y in the MFMA D layout (X[T][r] = unit 16 T + 4 q + r).  The slab
// protocol is mfma_layer's (nerf_mlp.h): slab `seq` is resident in slot seq & 1, every step prefetches seq + 1 while multiplying
// and ends with wait + barrier; the upper half of the waves takes the barrier in front of its epilogue, so that it runs under
// the partner wave's next matrix block.
template <int NT, int TPS, bool FILM_LDS>
__device__ __forceinline__ void grad_layer(const f32x4 (&X)[NT], f32x4 (&Y)[NT], float& head, bool last, Ring& ring, int l,
                                           const float* s_film, const float* __restrict__ film_b, const float* __restrict__ layer_bias,
                                           const float* s_ws, bool tangent, int wave, int lane, int q4o) {
  constexpr int H = NT * 16;
  constexpr int TILE = 16 * H;
  constexpr int SLAB = TILE * TPS;
  constexpr int STEPS = NT / TPS;
  const bool late_epilogue = __builtin_amdgcn_readfirstlane(wave) >= WAVES / 2;
#pragma unroll
  for (int sl = 0; sl < STEPS; ++sl) {
    if (ring.seq + 1 < ring.seq_end) {
      const int nxt = (ring.seq + 1) % ring.per_sample;
      stage_slab<SLAB>(ring.packed + (int64_t)nxt * SLAB, ring.lds + ((ring.seq + 1) & 1) * SLAB, wave, lane);
    }
    const float* slab = ring.lds + (ring.seq & 1) * SLAB;
    const int o_base = sl * (TPS * 16) + q4o;
    f32x4 acc[TPS];
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
    // matrix block, software-pipelined over the input tiles: the next tile's A fragments are requested before this tile's MFMAs
    {
      f32x4 fr[2][TPS];
      auto load_tile = [&](int buf, int T) {
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
        for (int r = 0; r < 4; ++r)        // k ascending: the chain of the render kernel's exact instantiation
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
#pragma unroll
    for (int tt = 0; tt < TPS; ++tt) {
      const int o4 = o_base + tt * 16;
      f32x4 g4, c4;
      film_rows<H, FILM_LDS>(s_film, film_b, layer_bias, l, o4, g4, c4);
      f32x4 res;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float a = quad_first(acc[tt][i]);                 // the point's pre-activation (the value lane's own accumulator)
        const float f = film_sincos(fmaf(g4[i], a, c4[i]), tangent);
        res[i] = tangent ? (g4[i] * f) * acc[tt][i] : f;
      }
      if (last) {       // h_D and its tangents: the head's partial sums, from the values the next layer would read
        const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) head = fmaf(ws4[i], res[i], head);
      }
      // (opaque: the sink pass would otherwise move the activations below the barrier that follows and undo the stagger)
      asm volatile("" : "+v"(res));
      Y[sl * TPS + tt] = res;
    }
    if (!late_epilogue) {
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
    ++ring.seq;
  }
}

// XG: explicit sample points (cips3d_nerf_params.x_pts) instead of camera-generated rays
template <int NT, int TPS, bool XG, bool FILM_LDS>
__global__ void __launch_bounds__(WAVES * 64, 2) nerf_sdf_grad_kernel(SdfGradArgs a) {
  constexpr int H = NT * 16;
  constexpr int SLAB = 16 * H * TPS;
  constexpr int NTH = WAVES * 64;
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

  const int b = blockIdx.x / a.wgs_per_view;              // uniform over the workgroup
  const int wv = blockIdx.x - b * a.wgs_per_view;
  const int N = P.n_samples;
  const int S = P.img_size;
  const int R = P.n_rays > 0 ? P.n_rays : S * S;
  const float* film_b = P.film + (int64_t)b * (D + 1) * 2 * H;

  // ---- per-view tables: s_film[l] = (gamma, gamma * bias_l + beta), the FMA form of the render kernel's table
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

  Ring ring;
  ring.packed = P.packed32;
  ring.lds = ringmem;
  ring.seq = 0;
  ring.per_sample = (D - 1) * (NT / TPS);
  ring.seq_end = a.iters * ring.per_sample;
  if (ring.seq_end > 0) stage_slab<SLAB>(ring.packed, ringmem, wave, lane);
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();

  for (int it = 0; it < a.iters; ++it) {
    // ---- the lane's point: p = ray * N + sample of view b ([B, R, N] order); steps past the end are computed on the last point
    // and store nothing (every wave must meet the slab barriers)
    const int64_t p64 = ((int64_t)wv + (int64_t)it * a.wgs_per_view) * WG_PTS + wave * GPTS + ((lane >> 2) & 3);
    const bool live = p64 < a.points;
    const int pt = live ? (int)p64 : a.points - 1;
    float ptx, pty, ptz;
    if constexpr (XG) {
      const float* pp = P.x_pts + ((int64_t)b * a.points + pt) * 3;
      ptx = pp[0]; pty = pp[1]; ptz = pp[2];
    } else {
      // the render kernel's ray and offset sampling (nerf_geom.h)
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
    // Opaque zero folded into every table offset of this iteration: the tables are loop-invariant and LICM would otherwise
    // hoist their registers out of the loop (nerf.hip)
    int opq = 0;
    asm volatile("" : "+v"(opq));
    const int q4o = 4 * qd + opq;

    f32x4 X[NT], Y[NT];
    float head = 0.f;         // this lane's partial of w_sigma . column
    // ---- layer 0: 3 -> H on the VALU, straight into the D layout
#pragma unroll
    for (int T = 0; T < NT; ++T) {
      const int o4 = T * 16 + q4o;
      f32x4 g4, c4;
      film_rows<H, FILM_LDS>(s_film, film_b, P.layer_bias, 0, o4, g4, c4);
      const f32x4 wx = *reinterpret_cast<const f32x4*>(s_w0 + o4);
      const f32x4 wy = *reinterpret_cast<const f32x4*>(s_w0 + H + o4);
      const f32x4 wz = *reinterpret_cast<const f32x4*>(s_w0 + 2 * H + o4);
      f32x4 res;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float pre = fmaf(wz[i], nz, fmaf(wy[i], ny, wx[i] * nx));
        const float f = film_sincos(fmaf(g4[i], pre, c4[i]), tangent);
        const float wk = kind == 1 ? wx[i] : (kind == 2 ? wy[i] : wz[i]);
        res[i] = tangent ? (g4[i] * f) * (wk * dn) : f;
      }
      if (D == 1) {
        const f32x4 ws4 = *reinterpret_cast<const f32x4*>(s_ws + o4);
#pragma unroll
        for (int i = 0; i < 4; ++i) head = fmaf(ws4[i], res[i], head);
      }
      X[T] = res;
    }
    // ---- hidden layers 1 .. D-1
    for (int l = 1; l < D; ++l) {
      grad_layer<NT, TPS, FILM_LDS>(X, Y, head, l == D - 1, ring, l, s_film, film_b, P.layer_bias, s_ws, tangent, wave, lane, q4o);
#pragma unroll
      for (int T = 0; T < NT; ++T) X[T] = Y[T];
    }
    // ---- head: the four k-quarters of the column, then sdf = . + b_sigma on the value lanes
    head += __shfl_xor(head, 16, 64);
    head += __shfl_xor(head, 32, 64);
    if (live && qd == 0) {
      int t_o = threadIdx.x;                    // (opaque: the output index is re-derived, not kept across the layers)
      asm volatile("" : "+v"(t_o));
      const int64_t po = (int64_t)b * a.points +
                         (((int64_t)wv + (int64_t)it * a.wgs_per_view) * WG_PTS + (t_o >> 6) * GPTS + ((t_o >> 2) & 3));
      const int ko = t_o & 3;
      if (ko == 0) {
        if (P.sdf) P.sdf[po] = head + b_sigma;
      } else {
        a.grad[po * 3 + (ko - 1)] = head;
      }
    }
  }
}

constexpr size_t sdf_grad_lds_bytes(int H, int TPS, int D, bool film_lds) {
  return sizeof(float) * ((size_t)2 * 16 * H * TPS + (film_lds ? (size_t)D * 2 * H : 0) + 4 * (size_t)H);
}

template <int NT, int TPS, bool XG, bool FILM_LDS>
int launch_sdf_grad_x(const SdfGradArgs& a, hipStream_t st) {
  constexpr int H = NT * 16;
  const size_t lds_bytes = sdf_grad_lds_bytes(H, TPS, a.p.depth, FILM_LDS);
  if (lds_bytes > 160 * 1024) return CIPS3D_E_UNSUPP;
  // the attribute is per device and the flag is shared by host threads (launch_render_x)
  static std::atomic<unsigned long long> attr_set{0};
  int dev_id = 0;
  if (hipError_t e = hipGetDevice(&dev_id); e != hipSuccess) return (int)e;
  const unsigned long long bit = 1ull << (dev_id & 63);
  if (dev_id >= 64 || !(attr_set.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&nerf_sdf_grad_kernel<NT, TPS, XG, FILM_LDS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return (int)e;
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL((nerf_sdf_grad_kernel<NT, TPS, XG, FILM_LDS>), dim3((unsigned)(a.p.B * a.wgs_per_view)), dim3(WAVES * 64),
                     lds_bytes, st, a);
  return cips3d_launch_status();
}

template <int NT, int TPS>
int launch_sdf_grad(const SdfGradArgs& a, hipStream_t st) {
  // the FiLM table sits in LDS beside the two slabs while it fits (depth <= 14 at hidden 256); deeper networks read its rows
  // from memory in the epilogues
  if (sdf_grad_lds_bytes(NT * 16, TPS, a.p.depth, true) <= 160 * 1024)
    return a.p.x_pts ? launch_sdf_grad_x<NT, TPS, true, true>(a, st) : launch_sdf_grad_x<NT, TPS, false, true>(a, st);
  return a.p.x_pts ? launch_sdf_grad_x<NT, TPS, true, false>(a, st) : launch_sdf_grad_x<NT, TPS, false, false>(a, st);
}

}  // namespace

extern "C" int cips3d_nerf_sdf_grad_supported(int hidden, int depth) { return hidden == 256 && depth >= 1 && depth <= 64 ? 1 : 0; }

extern "C" int cips3d_nerf_sdf_grad(const cips3d_nerf_params* p, float* grad, void* stream) {
  if (!p || !grad) return CIPS3D_E_BADARG;
  const cips3d_nerf_params& P = *p;
  if (P.B < 0 || P.img_size <= 0 || P.n_samples <= 0 || P.depth < 1 || P.hidden <= 0) return CIPS3D_E_BADARG;
  if (!cips3d_nerf_sdf_grad_supported(P.hidden, P.depth)) return CIPS3D_E_UNSUPP;
  if (!P.near_ || !P.far_ || !P.w_first || !P.film || !P.layer_bias || !P.w_sigma || !P.b_sigma || (P.depth > 1 && !P.packed32))
    return CIPS3D_E_BADARG;
  if (P.x_pts ? P.n_rays <= 0 : (!P.cam_poses || !P.focals || P.n_rays != 0)) return CIPS3D_E_BADARG;
  if (P.B == 0) return 0;
  const int64_t points = (int64_t)(P.n_rays > 0 ? (int64_t)P.n_rays : (int64_t)P.img_size * P.img_size) * P.n_samples;
  if (points > 0x7fffffff) return CIPS3D_E_UNSUPP;
  int dev_id = 0, cus = 0;
  if (hipError_t e = hipGetDevice(&dev_id); e != hipSuccess) return (int)e;
  if (hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev_id); e != hipSuccess) return (int)e;
  if (cus < 1) cus = 1;
  SdfGradArgs a;
  a.p = P;
  a.grad = grad;
  a.points = (int)points;
  // one workgroup per compute unit (the ring takes most of its LDS), each walking `iters` steps of 32 points of one view
  const int64_t steps = ceil_div<int64_t>(points, WG_PTS);
  int64_t wpv = ceil_div<int64_t>(cus, P.B);
  if (wpv > steps) wpv = steps;
  a.iters = (int)ceil_div<int64_t>(steps, wpv);
  a.wgs_per_view = (int)ceil_div<int64_t>(steps, a.iters);
  if ((int64_t)P.B * a.wgs_per_view > 0x7fffffff) return CIPS3D_E_UNSUPP;
  a.pad_ = 0;
  nerf_linspace_consts(P.n_samples, a.t_end, a.t_step);
  return launch_sdf_grad<16, 4>(a, as_stream(stream));
}
