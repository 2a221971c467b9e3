// The per-ray geometry of the NeRF half, stated ONCE (reference: Render.get_rays_in_world / get_z_vals and the densities of
// volume_integration, cips3d/nerf_utils.py:18-121, 276-297): pixel -> camera direction -> world direction, the view direction, |rays_d|, the
// torch.linspace(0, 1 - 1/N, N) constants, the un-perturbed depth of a sample and its offset-sampled form, the sigmoid and the
// SDF density.  Every kernel that recomputes a ray instead of reading it takes these expressions from here -- the render kernel
// (nerf.hip), both backwards (nerf_bwd.hip, nerf_bwd_fused.hip), the SDF gradient (nerf_sdf_grad.hip), the normals
// (nerf_normals.hip) and the stand-alone Render.* ops (render_ops.hip) -- because they must agree BIT FOR BIT: the fused backward
// refills the forward's stash, the materialised one recomposites with the forward's delta, the normals weight samples with the
// render kernel's z, and the stand-alone ops are what the fused kernel does in registers.  So must what they do with a sample
// once they have its density (nerf_utils.py:264-307; at the end of this file): the compositing step, and its per-sample adjoint
// for the two compositing kernels of the backward.  fp32, contraction off, the association written out: change an expression
// here and it changes everywhere at once.
#pragma once
#include "common.h"

namespace {

// torch.linspace(0, 1 - 1/N, N): last value and step.  The hot kernels take them as kernel arguments (see NerfArgs, nerf_mlp.h).
__host__ __device__ __forceinline__ void nerf_linspace_consts(int N, float& t_end, float& t_step) {
  t_end = (float)(1.0 - 1.0 / (double)N);
  t_step = N > 1 ? t_end / (float)(N - 1) : 0.f;
}

__device__ __forceinline__ float nerf_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }
// with_sdf density (nerf_utils.py:276-286), and F.softplus of the raw density (:288-297; torch's threshold 20: identity above it)
__device__ __forceinline__ float nerf_sdf_density(float sdf, float beta) { return nerf_sigmoid(-sdf / beta) / beta; }
__device__ __forceinline__ float nerf_softplus(float v) { return v > 20.f ? v : log1pf(expf(v)); }
// The render kernel's softplus (nerf.hip; every other kernel uses nerf_softplus): the library log1pf / expf held enough temporaries
// to spill four registers of the kernel's default (with_sdf) path, so it takes the hardware exp and log behind its uniform
// branch.  log(1 + e) alone is 0 once e = exp(v) < 2^-24 (v < -16.6), yet the last sample of a ray (delta = 1e10) still has
// alpha = 1 - exp(-e 1e10 |d|) ~ 1 down to v ~ -21: an empty ray of a density model lost its background weight.  Below
// e = 2^-12 the series e - e^2 / 2 (relative error < e^2 / 3 = 2e-8) takes over; above it the rounding of 1 + e costs sigma at
// most 2^-24 absolute: nothing for a sample of finite delta, and the last sample's alpha is 1 there anyway (sigma 1e10 > 2e6).
// tests/test_gpu_nerf_fwd.py holds it to fp64 at biases -20 .. +25 of the density head.
__device__ __forceinline__ float nerf_softplus_hw(float v) {
  if (v > 20.f) return v;
  const float e = __expf(v);
  return e < 0x1p-12f ? fmaf(-0.5f * e, e, e) : __logf(1.f + e);
}

__device__ __forceinline__ float nerf_norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// Sample depths of one view.
struct NerfDepths {
  float nearv, farv, t_end, t_step;
  int N;
  // un-perturbed depth of sample k (linspace evaluated symmetrically around the midpoint, as torch); k == N gives `far`
  __device__ __forceinline__ float zbase(int k) const {
    if (k >= N) return farv;
    const float t = (k < N / 2) ? t_step * (float)k : t_end - t_step * (float)(N - 1 - k);
    return nearv * (1.f - t) + farv * t;
  }
  // offset sampling (nerf_utils.py:88-96): one uniform u per ray moves every sample the same fraction towards the next (z1)
  __device__ static __forceinline__ float zoffset(float z0, float z1, float u) { return z0 + (z1 - z0) * u; }
  // depth of sample k of a ray (a kernel that reads u only when there is one spells this line itself, with the read as zoffset's
  // last argument)
  __device__ __forceinline__ float z(int k, bool has_u, float u) const {
    const float z0 = zbase(k);
    return has_u ? zoffset(z0, zbase(k + 1), u) : z0;
  }
};

// Ray of pixel `ray` = row * S + column of a view with focal length focals[b] and pose cw = cam_poses + 12 b
// (nerf_utils.py:38-66): direction in the camera frame (dc*) and in the world (d*).  The origin is (cw[3], cw[7], cw[11]).
struct NerfCamRay {
  float dcx, dcy, dcz, dx, dy, dz;
};
__device__ __forceinline__ NerfCamRay nerf_cam_ray(float focal, const float* cw, int S, int ray) {
  NerfCamRay c;
  const int pi = ray / S, pj = ray - pi * S;
  const float px = (float)pj + 0.5f, py = (float)pi + 0.5f;
  c.dcx = (px - (float)S * 0.5f) / focal;
  c.dcy = -(py - (float)S * 0.5f) / focal;
  c.dcz = -1.f;
  c.dx = (c.dcx * cw[0] + c.dcy * cw[1]) + c.dcz * cw[2];
  c.dy = (c.dcx * cw[4] + c.dcy * cw[5]) + c.dcz * cw[6];
  c.dz = (c.dcx * cw[8] + c.dcy * cw[9]) + c.dcz * cw[10];
  return c;
}

// F.normalize (eps 1e-12) of the camera-frame direction (static_viewdirs) or of the world direction; returns the clamped length
__device__ __forceinline__ float nerf_viewdir(const NerfCamRay& c, int static_viewdirs, float& vx, float& vy, float& vz) {
  const float rx = static_viewdirs ? c.dcx : c.dx, ry = static_viewdirs ? c.dcy : c.dy, rz = static_viewdirs ? c.dcz : c.dz;
  const float vnorm = fmaxf(nerf_norm3(rx, ry, rz), 1e-12f);
  vx = rx / vnorm; vy = ry / vnorm; vz = rz / vnorm;
  return vnorm;
}

// Everything about one camera ray.  Fields a kernel does not read cost nothing once this is inlined.
struct RayGeom {
  float ox, oy, oz, dx, dy, dz, dcx, dcy, dcz, vx, vy, vz, vnorm, dnorm, nearv, farv, u, t_end, t_step;
  int N, has_u;
  __device__ __forceinline__ NerfDepths depths() const { return NerfDepths{nearv, farv, t_end, t_step, N}; }
  __device__ __forceinline__ float zbase(int k) const { return depths().zbase(k); }
  __device__ __forceinline__ float z(int k) const { return depths().z(k, has_u, u); }
};

__device__ __forceinline__ RayGeom ray_geom(const float* cam_poses, const float* focals, const float* near_, const float* far_,
                                            const float* perturb_u, int S, int N, int static_viewdirs, int b, int ray,
                                            float t_end, float t_step) {
  RayGeom r;
  const float focal = focals[b];
  r.nearv = near_[b]; r.farv = far_[b];
  const float* cw = cam_poses + 12 * b;
  const NerfCamRay c = nerf_cam_ray(focal, cw, S, ray);
  r.dcx = c.dcx; r.dcy = c.dcy; r.dcz = c.dcz;
  r.dx = c.dx; r.dy = c.dy; r.dz = c.dz;
  r.ox = cw[3]; r.oy = cw[7]; r.oz = cw[11];
  r.vnorm = nerf_viewdir(c, static_viewdirs, r.vx, r.vy, r.vz);
  r.dnorm = nerf_norm3(r.dx, r.dy, r.dz);
  r.has_u = perturb_u != nullptr;
  r.u = r.has_u ? perturb_u[(int64_t)b * S * S + ray] : 0.f;
  r.N = N;
  r.t_end = t_end; r.t_step = t_step;
  return r;
}

// ---- Compositing.  dz_k = z_{k+1} - z_k, delta_k = dz_k |rays_d|, e_k = exp(-sigma_k delta_k), alpha_k = 1 - e_k,
// f_k = (1 - alpha_k) + 1e-10, T_k = prod_{j<k} f_j, w_k = alpha_k T_k.  Helpers take loaded values and the density sigma (which
// softplus a raw density goes through is the call site's choice); the products and sums along a ray stay with each kernel, whose
// order they are.  dz_k of the last sample is NERF_DZ_LAST, scaled by |rays_d| like every other: a call site writes
// k < N - 1 ? z_{k+1} - z_k : NERF_DZ_LAST  around its own loads, so that z_{k+1} is read only where there is one.
constexpr float NERF_DZ_LAST = 1e10f;
__device__ __forceinline__ float nerf_atten(float sigma, float delta) { return expf(-sigma * delta); }               // e_k
__device__ __forceinline__ float nerf_alpha(float sigma, float delta) { return 1.f - nerf_atten(sigma, delta); }
__device__ __forceinline__ float nerf_keep(float alpha) { return (1.f - alpha) + 1e-10f; }                           // f_k

// Upstreams of a ray's geometry maps (nerf_utils.py:329-336): m = d loss / d mask[0], (x, y, z) = the effective adjoint of xyz
struct GeoAdj { float x, y, z, m; };

// One sample of the compositing backward (nerf_bwd.hip): what the forward made of it and every per-sample factor of the adjoint,
// from G_k = d loss / d w_k and S_k = sum_{j>k} w_j G_j.  raw (with_sdf = False, nerf_utils.py:288-297): v is the raw density,
// sigma = softplus(v), d sigma / d v = sg = sigmoid(v); else v is the sdf, sg = sigmoid(-v / beta), sigma = sg / beta.
struct NerfSampleAdj {
  bool raw;
  float beta, v, delta, sg, sigma, e, alpha, keep, s0, s1, s2;   // s*: the rgb sigmoids
  // g = <d feature map, feature_k>, d* = d thumbnail (rgb_map = -1 + 2 sum_k w_k s_k)
  __device__ __forceinline__ float G(float g, float d0, float d1, float d2) const { return g + 2.f * (d0 * s0 + d1 * s1 + d2 * s2); }
  // the geometry upstreams' share of G_k: <xbar, p_k> + [k == N-1] mbar, p_k the world point the forward composites
  __device__ static __forceinline__ float G_geo(float Gk, const GeoAdj& ga, float px, float py, float pz, bool last) {
    Gk += (ga.x * px + ga.y * py) + ga.z * pz;
    return last ? Gk + ga.m : Gk;
  }
  __device__ __forceinline__ float dalpha(float Tk, float Gk, float Sk) const { return Tk * Gk - Sk / keep; }
  __device__ __forceinline__ float dsigma(float dalpha) const { return dalpha * delta * e; }
  __device__ __forceinline__ float ddnorm(float dalpha) const { return dalpha * sigma * e; }   // d |rays_d| = sum_k ddnorm_k dz_k
  __device__ __forceinline__ float dsdf(float dsigma) const { return raw ? dsigma * sg : dsigma * (-sg * (1.f - sg) / (beta * beta)); }
  // d sigma / d beta (with_sdf only): d sigmoid_beta = sum_k dsigma_k dbeta_k
  __device__ __forceinline__ float dbeta() const { return (sg * (1.f - sg) * v / beta - sg) / (beta * beta); }
  __device__ static __forceinline__ float drgb(float wk, float d, float s) { return 2.f * wk * d * s * (1.f - s); }   // d rgb logit
};
__device__ __forceinline__ NerfSampleAdj nerf_sample_adj(bool raw, float beta, float v, float delta, float c0, float c1, float c2) {
  NerfSampleAdj a;
  a.raw = raw; a.beta = beta; a.v = v; a.delta = delta;
  a.sg = raw ? nerf_sigmoid(v) : nerf_sigmoid(-v / beta);
  a.sigma = raw ? nerf_softplus(v) : a.sg / beta;
  a.e = nerf_atten(a.sigma, a.delta);
  a.alpha = 1.f - a.e;
  a.keep = nerf_keep(a.alpha);
  a.s0 = nerf_sigmoid(c0); a.s1 = nerf_sigmoid(c1); a.s2 = nerf_sigmoid(c2);
  return a;
}

}  // namespace
