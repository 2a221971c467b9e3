// The shade of the geometry frames, stated ONCE: the composited-normal frame of a rendered view (nerf_normals.hip) and the frames
// of the exported mesh (mesh_raster.hip, mesh_color.hip, mesh_texture.hip) are shown side by side and must shade alike.
#pragma once
#include "common.h"

namespace {

// F.normalize of a 3-vector (eps 1e-12)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
  const float n = fmaxf(sqrtf((x * x + y * y) + z * z), 1e-12f);
  x /= n; y /= n; z /= n;
}

// pytorch3d's Phong for a white vertex colour: unit normal n, vectors l to the light and v to the eye (normalised here)
__device__ __forceinline__ float phong_white(float nx, float ny, float nz, float lx, float ly, float lz, float vx, float vy,
                                             float vz, float ka, float kd, float ks, float shininess) {
  normalize3(lx, ly, lz);
  normalize3(vx, vy, vz);
  const float cs = (nx * lx + ny * ly) + nz * lz;
  const float rx = 2.f * cs * nx - lx, ry = 2.f * cs * ny - ly, rz = 2.f * cs * nz - lz;
  const float vr = fmaxf((vx * rx + vy * ry) + vz * rz, 0.f);
  const float spec = cs > 0.f ? powf(vr, shininess) : 0.f;
  return (ka + kd * fmaxf(cs, 0.f)) + ks * spec;
}

// a shade or colour in [0, 1] (clamped) -> byte, half rounds up
__device__ __forceinline__ uint8_t unit_to_u8(float x) { return (uint8_t)floorf(255.f * fminf(fmaxf(x, 0.f), 1.f) + 0.5f); }

}  // namespace
