// Composited surface normals and the Phong-shaded geometry frame of a rendered view (cips3d_nerf_normals).
//
//   normal_raw[b,:,r] = sum_i w_i grad[b,r,i,:]     w = the compositing weights of nerf_utils.py:276-286 (the render
//                                                   kernel's rays, depths and compositing step: csrc/nerf_geom.h),
//                                                   grad = d sdf / d pts of csrc/nerf_sdf_grad.hip
//   normal = normal_raw / max(|normal_raw|, 1e-12)  (F.normalize)
//   shade  = the mesh frames' Phong (csrc/shade.h) at p = xyz[b,:,r], seen from `eye`, lit from `light`
//
// sdf and grad have the sample index innermost, so lanes span SAMPLES: a ray is a segment of W = 2^k >= N lanes (64 / W rays
// per wave), or, for N > 64, one wave walking chunks of 64 samples with the transmittance carried across.  The transmittance
// T_i = prod_{j<i} (1 - alpha_j + 1e-10) is a SHIFTED exclusive prefix product over the segment (lane i starts from its left
// neighbour's factor, lane 0 from 1): no division by the own factor and no log-space subtraction, either of which would
// cancel against the 1e10 last interval.  The weighted sum is a butterfly over the segment.  Every ray's operation order is
// fixed by N alone: no atomics, bit-reproducible, independent of the grid.  Accurate expf / powf throughout.
#include "common.h"
#include "nerf_geom.h"
#include "shade.h"

namespace {

constexpr int NRM_WAVES = 4;

struct NormalsArgs {
  cips3d_normals_params p;
  int64_t rays;              // B * R
  int R;
  float t_end, t_step;       // nerf_linspace_consts (nerf_geom.h)
};

template <int W, bool XG>
__global__ void __launch_bounds__(NRM_WAVES * 64) nerf_normals_kernel(NormalsArgs a) {
  const cips3d_normals_params& P = a.p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int RPW = 64 / W;                       // rays per wave step
  const int seg = lane / W, s0 = lane - seg * W;    // ray within the step, sample within the chunk
  const int N = P.n_samples, R = a.R, S = P.img_size;
  const int n_chunks = (N + W - 1) / W;             // 1 unless N > 64
  const float beta = P.sigmoid_beta[0];
  const int64_t groups = (a.rays + RPW - 1) / RPW;
  for (int64_t g = (int64_t)blockIdx.x * NRM_WAVES + wave; g < groups; g += (int64_t)gridDim.x * NRM_WAVES) {
    const int64_t bray = g * RPW + seg;
    const bool ray_live = bray < a.rays;
    const int64_t brc = ray_live ? bray : a.rays - 1;      // dead segments recompute the last ray and store nothing
    const int b = (int)(brc / R);
    const int ray = (int)(brc - (int64_t)b * R);
    const float nearv = P.near_ ? P.near_[b] : 0.f, farv = P.far_ ? P.far_[b] : 0.f;
    float dx, dy, dz, u = 0.f;
    if constexpr (XG) {
      dx = P.x_rays_d[brc * 3]; dy = P.x_rays_d[brc * 3 + 1]; dz = P.x_rays_d[brc * 3 + 2];
    } else {
      // the render kernel's ray direction (nerf_geom.h)
      const NerfCamRay cam = nerf_cam_ray(P.focals[b], P.cam_poses + 12 * b, S, ray);
      dx = cam.dx; dy = cam.dy; dz = cam.dz;
      if (P.perturb_u) u = P.perturb_u[brc];
    }
    const float dnorm = nerf_norm3(dx, dy, dz);
    const NerfDepths zs{nearv, farv, a.t_end, a.t_step, N};
    auto zsample = [&](int k) -> float {
      if constexpr (XG) {
        return P.x_z_vals[brc * N + k];
      } else {
        return zs.z(k, P.perturb_u != nullptr, u);
      }
    };

    float carry = 1.f, ax = 0.f, ay = 0.f, az = 0.f;
    for (int c = 0; c < n_chunks; ++c) {
      const int sk = c * W + s0;
      const bool live = sk < N;
      float f = 1.f, alpha = 0.f, gx = 0.f, gy = 0.f, gz = 0.f;
      if (live) {
        const int64_t pt = brc * N + sk;
        const float sdf = P.sdf[pt];
        const float* gp = P.grad + pt * 3;
        gx = gp[0]; gy = gp[1]; gz = gp[2];
        const float delta = (sk < N - 1 ? zsample(sk + 1) - zsample(sk) : NERF_DZ_LAST) * dnorm;
        alpha = nerf_alpha(nerf_sdf_density(sdf, beta), delta);
        f = nerf_keep(alpha);
      }
      // shifted exclusive prefix product over the segment
      float x = __shfl_up(f, 1, W);
      if (s0 == 0) x = 1.f;
#pragma unroll
      for (int off = 1; off < W; off <<= 1) {
        const float y = __shfl_up(x, off, W);
        if (s0 >= off) x *= y;
      }
      const float w = alpha * (carry * x);
      ax += w * gx; ay += w * gy; az += w * gz;
      if (n_chunks > 1) carry *= __shfl(x, W - 1, W) * __shfl(f, W - 1, W);
    }
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
      ax += __shfl_xor(ax, off, W);
      ay += __shfl_xor(ay, off, W);
      az += __shfl_xor(az, off, W);
    }
    if (s0 != 0 || !ray_live) continue;
    const int64_t o3 = (int64_t)b * 3 * R + ray;
    if (P.normal_raw) { P.normal_raw[o3] = ax; P.normal_raw[o3 + R] = ay; P.normal_raw[o3 + 2 * (int64_t)R] = az; }
    float nx = ax, ny = ay, nz = az;
    normalize3(nx, ny, nz);
    if (P.normal) { P.normal[o3] = nx; P.normal[o3 + R] = ny; P.normal[o3 + 2 * (int64_t)R] = nz; }
    if (P.shade || P.shade_u8) {
      const float px = P.xyz[o3], py = P.xyz[o3 + R], pz = P.xyz[o3 + 2 * (int64_t)R];
      float lx = P.light[3 * b] - px, ly = P.light[3 * b + 1] - py, lz = P.light[3 * b + 2] - pz;
      float vx = P.eye[3 * b] - px, vy = P.eye[3 * b + 1] - py, vz = P.eye[3 * b + 2] - pz;
      const float sh = phong_white(nx, ny, nz, lx, ly, lz, vx, vy, vz, P.ka, P.kd, P.ks, P.shininess);
      if (P.shade) P.shade[brc] = sh;
      if (P.shade_u8) {
        const uint8_t q = unit_to_u8(sh);
        P.shade_u8[o3] = q; P.shade_u8[o3 + R] = q; P.shade_u8[o3 + 2 * (int64_t)R] = q;
      }
    }
  }
}

template <int W>
int launch_normals(const NormalsArgs& a, hipStream_t st) {
  constexpr int RPW = 64 / W;
  const int64_t groups = ceil_div<int64_t>(a.rays, RPW);
  const int grid = (int)std::min<int64_t>(ceil_div<int64_t>(groups, NRM_WAVES), 1 << 16);
  if (a.p.x_z_vals)
    hipLaunchKernelGGL((nerf_normals_kernel<W, true>), dim3(grid), dim3(NRM_WAVES * 64), 0, st, a);
  else
    hipLaunchKernelGGL((nerf_normals_kernel<W, false>), dim3(grid), dim3(NRM_WAVES * 64), 0, st, a);
  return cips3d_launch_status();
}

}  // namespace

extern "C" int cips3d_nerf_normals(const cips3d_normals_params* p, void* stream) {
  if (!p) return CIPS3D_E_BADARG;
  const cips3d_normals_params& P = *p;
  if (!P.sdf || !P.grad || !P.sigmoid_beta || P.B < 0 || P.n_samples < 1) return CIPS3D_E_BADARG;
  if (!P.normal_raw && !P.normal && !P.shade && !P.shade_u8) return CIPS3D_E_BADARG;
  if ((P.shade || P.shade_u8) && (!P.xyz || !P.eye || !P.light)) return CIPS3D_E_BADARG;
  const bool xg = P.x_z_vals != nullptr;
  if (xg ? (!P.x_rays_d || P.n_rays <= 0) : (!P.cam_poses || !P.focals || !P.near_ || !P.far_ || P.img_size <= 0 || P.n_rays != 0))
    return CIPS3D_E_BADARG;
  if (P.B == 0) return 0;
  NormalsArgs a;
  a.p = P;
  const int64_t R = xg ? (int64_t)P.n_rays : (int64_t)P.img_size * P.img_size;
  a.rays = (int64_t)P.B * R;
  if (R > INT32_MAX || a.rays > INT32_MAX) return CIPS3D_E_UNSUPP;
  a.R = (int)R;
  nerf_linspace_consts(P.n_samples, a.t_end, a.t_step);
  hipStream_t st = as_stream(stream);
  const int N = P.n_samples;
  if (N <= 1) return launch_normals<1>(a, st);
  if (N <= 2) return launch_normals<2>(a, st);
  if (N <= 4) return launch_normals<4>(a, st);
  if (N <= 8) return launch_normals<8>(a, st);
  if (N <= 16) return launch_normals<16>(a, st);
  if (N <= 32) return launch_normals<32>(a, st);
  return launch_normals<64>(a, st);
}
