// cips3d_camera_axis_angle / _bwd: the free camera of the axis-angle projector (reference models/projector_axis_angle.py with
// Camera.get_camera2world, cips3d/nerf_utils.py:439-463): pose = [exp([rot]x) | trans / max(|trans|, 1e-12)], focal / near / far
// as cips3d_camera_params makes them.  One thread per view, a few hundred flops each -- launch-latency bound, so the rotation
// is evaluated in fp64 and rounded once: every inversion starts at rot = 0 exactly, where the fp32 closed forms of the
// derivative cancel to nothing.
//
//   s = |rot|^2, K = [rot]x, R = I + a(s) K + b(s) K^2,  a = sin t / t,  b = (1 - cos t) / t^2 = 1/2 (sin(t/2) / (t/2))^2
//   dR / d r_i = 2 r_i (a' K + b' K^2) + a E_i + b (E_i K + K E_i),   E_i = [e_i]x
//   a' = (cos t - a) / 2s,  b' = (a - 2b) / 2s    (cos t = 1 - s b)
// Below s = SERIES_S the four functions are their Taylor series in s (ten terms: the first one left out is < 1e-19 there);
// above it the quotients lose 12 / s ulps at most to cancellation (5e-15 at the threshold), so the branches meet within a few
// fp64 roundings.  At rot = 0 this gives R = I exactly and dR / d r_i = E_i.
#include "common.h"

namespace {

constexpr double SERIES_S = 0.25;

struct RotCoef { double a, b, da, db; };

// sum_n c_n s^n with c_n = (-1)^n / (2n + k0)! -- and its derivative -- by recurrence on the term
__device__ __forceinline__ void series(double s, int k0, double c0, double& f, double& df) {
  double term = c0;       // c_n s^n
  double coef = c0;       // c_n
  double spow = 1.0;      // s^(n-1) for the derivative
  f = c0;
  df = 0.0;
#pragma unroll
  for (int n = 1; n <= 10; ++n) {
    const double den = (double)((2 * n + k0 - 1) * (2 * n + k0));
    coef = -coef / den;
    term = -term * s / den;
    f += term;
    df += (double)n * coef * spow;
    spow *= s;
  }
}

__device__ __forceinline__ RotCoef rot_coef(double s) {
  RotCoef c;
  if (s < SERIES_S) {
    series(s, 1, 1.0, c.a, c.da);      // 1/(2n+1)!
    series(s, 2, 0.5, c.b, c.db);      // 1/(2n+2)!
  } else {
    const double t = sqrt(s), h = 0.5 * t, q = sin(h) / h;
    c.a = sin(t) / t;
    c.b = 0.5 * q * q;
    c.da = ((1.0 - s * c.b) - c.a) / (2.0 * s);
    c.db = (c.a - 2.0 * c.b) / (2.0 * s);
  }
  return c;
}

struct M3 { double m[3][3]; };
__device__ __forceinline__ M3 skew(double x, double y, double z) {
  return M3{{{0.0, -z, y}, {z, 0.0, -x}, {-y, x, 0.0}}};
}
__device__ __forceinline__ M3 mul(const M3& A, const M3& Bm) {
  M3 C;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C.m[i][j] = (A.m[i][0] * Bm.m[0][j] + A.m[i][1] * Bm.m[1][j]) + A.m[i][2] * Bm.m[2][j];
  return C;
}
__device__ __forceinline__ double dot9(const M3& A, const M3& Bm) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) s += A.m[i][j] * Bm.m[i][j];
  return s;
}

__global__ void camera_axis_angle_kernel(const float* __restrict__ rot, const float* __restrict__ trans,
                                         const float* __restrict__ fov_deg, float fov_s, float dist_radius, int img_size, int B,
                                         float* __restrict__ extr, float* __restrict__ focal, float* __restrict__ near_,
                                         float* __restrict__ far_) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  // (focal / near / far: the expressions of camera_kernel, camera.hip -- the same bits for the same field of view)
  const float fov = (fov_deg ? fov_deg[b] : fov_s) * 3.14159265358979323846f / 180.f;
  focal[b] = 0.5f * (float)img_size / tanf(fov);
  near_[b] = 1.f - dist_radius;
  far_[b] = 1.f + dist_radius;
  const double rx = rot[3 * b], ry = rot[3 * b + 1], rz = rot[3 * b + 2];
  const RotCoef c = rot_coef((rx * rx + ry * ry) + rz * rz);
  const M3 K = skew(rx, ry, rz), K2 = mul(K, K);
  const double tx = trans[3 * b], ty = trans[3 * b + 1], tz = trans[3 * b + 2];
  const double tn = fmax(sqrt((tx * tx + ty * ty) + tz * tz), 1e-12);
  const double t[3] = {tx / tn, ty / tn, tz / tn};
  float* e = extr + 12 * b;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) e[4 * i + j] = (float)(((i == j ? 1.0 : 0.0) + c.a * K.m[i][j]) + c.b * K2.m[i][j]);
    e[4 * i + 3] = (float)t[i];
  }
}

__global__ void camera_axis_angle_bwd_kernel(const float* __restrict__ rot, const float* __restrict__ trans,
                                             const float* __restrict__ fov_deg, float fov_s, int img_size,
                                             const float* __restrict__ dextr, const float* __restrict__ dfocal, int B,
                                             float* __restrict__ drot, float* __restrict__ dtrans, float* __restrict__ dfov) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double gr[3] = {0.0, 0.0, 0.0}, gt[3] = {0.0, 0.0, 0.0};
  if (dextr != nullptr) {
    const float* g = dextr + 12 * b;
    M3 G;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) G.m[i][j] = g[4 * i + j];
    const double r[3] = {rot[3 * b], rot[3 * b + 1], rot[3 * b + 2]};
    const RotCoef c = rot_coef((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    const M3 K = skew(r[0], r[1], r[2]), K2 = mul(K, K);
    const double radial = 2.0 * (c.da * dot9(G, K) + c.db * dot9(G, K2));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const M3 E = skew(i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0);
      const M3 EK = mul(E, K), KE = mul(K, E);
      gr[i] = (r[i] * radial + c.a * dot9(G, E)) + c.b * (dot9(G, EK) + dot9(G, KE));
    }
    // F.normalize: t / max(|t|, eps); below the clamp the denominator is a constant
    const double t[3] = {trans[3 * b], trans[3 * b + 1], trans[3 * b + 2]};
    const double gv[3] = {g[3], g[7], g[11]};
    const double n = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (n > 1e-12) {
      const double u[3] = {t[0] / n, t[1] / n, t[2] / n};
      const double d = (u[0] * gv[0] + u[1] * gv[1]) + u[2] * gv[2];
#pragma unroll
      for (int i = 0; i < 3; ++i) gt[i] = (gv[i] - u[i] * d) / n;
    } else {
#pragma unroll
      for (int i = 0; i < 3; ++i) gt[i] = gv[i] / 1e-12;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    drot[3 * b + i] = (float)gr[i];
    dtrans[3 * b + i] = (float)gt[i];
  }
  if (dfov != nullptr) {
    double gf = 0.0;
    if (dfocal != nullptr) {      // focal = S/2 cot x, x = fov pi / 180:  d focal / d fov = -S/2 / sin^2 x * pi / 180
      const double k = 3.14159265358979323846 / 180.0;
      const double sx = sin((double)(fov_deg ? fov_deg[b] : fov_s) * k);
      gf = (double)dfocal[b] * (-0.5 * (double)img_size / (sx * sx)) * k;
    }
    dfov[b] = (float)gf;
  }
}

}  // namespace

extern "C" int cips3d_camera_axis_angle(const float* rot, const float* trans, const float* fov_deg, float fov_deg_scalar,
                                        float dist_radius, int img_size, int B, float* extrinsics, float* focal, float* near_,
                                        float* far_, void* stream) {
  if (B == 0) return 0;
  if (!rot || !trans || !extrinsics || !focal || !near_ || !far_ || B < 0 || img_size <= 0) return CIPS3D_E_BADARG;
  hipLaunchKernelGGL(camera_axis_angle_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), rot, trans, fov_deg,
                     fov_deg_scalar, dist_radius, img_size, B, extrinsics, focal, near_, far_);
  return cips3d_launch_status();
}

extern "C" int cips3d_camera_axis_angle_bwd(const float* rot, const float* trans, const float* fov_deg, float fov_deg_scalar,
                                            int img_size, const float* dextrinsics, const float* dfocal, int B, float* drot,
                                            float* dtrans, float* dfov, void* stream) {
  if (B == 0) return 0;
  if (!rot || !trans || !drot || !dtrans || B < 0 || img_size <= 0) return CIPS3D_E_BADARG;
  hipLaunchKernelGGL(camera_axis_angle_bwd_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, as_stream(stream), rot, trans, fov_deg,
                     fov_deg_scalar, img_size, dextrinsics, dfocal, B, drot, dtrans, dfov);
  return cips3d_launch_status();
}
