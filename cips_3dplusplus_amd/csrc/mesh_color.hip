// Vertex colours of the exported mesh from the generator's own renders (cips3d_mesh_vertex_colors), and the coloured mesh frame
// (cips3d_mesh_albedo_frame).  The reference exports a grey surface (exp/cips3d/utils.py:206-224) and draws it white
// (add_textures, utils.py:260-308); this is the gather that project_noise's correspondence allows in the other direction.
//
//   colours  per vertex, one thread, views in ascending order: the rasteriser's own projection of the vertex (workspace) picks
//            the pixel whose key says which depth the view sees there; a visible, front-facing vertex takes the bilinear sample
//            of that view's image with weight (n . d)^power.  No atomics, no LDS: a vertex's sums are its thread's registers,
//            so the result is independent of the grid and bit-reproducible
//   albedo   per (view, pixel): shade x colour of the resolve pass's maps -> uint8
//
// The library builds with -ffp-contract=off, so every expression below rounds as written (the contract: include/cips3d_hip.h).
#include "mesh_raster.h"

namespace {

// one channel of images[k] at the four taps
__device__ __forceinline__ float mc_bilinear(const float* __restrict__ img, int64_t r0, int64_t r1, int x0, int x1, float fx, float fy) {
  const float top = (1.f - fx) * img[r0 + x0] + fx * img[r0 + x1];
  const float bot = (1.f - fx) * img[r1 + x0] + fx * img[r1 + x1];
  return (1.f - fy) * top + fy * bot;
}

__global__ void __launch_bounds__(MR_THREADS) mc_vertex_kernel(cips3d_mesh_color_params P, const float* __restrict__ cams,
                                                               const float4* __restrict__ proj) {
  const int S = P.S, R = P.R, V = P.V;
  const float fs = (float)(S - 1), fr = (float)(R - 1);
  const int64_t SS = (int64_t)S * S, RR = (int64_t)R * R;
  for (int64_t vi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; vi < V; vi += (int64_t)gridDim.x * blockDim.x) {
    const float px = P.verts[3 * vi], py = P.verts[3 * vi + 1], pz = P.verts[3 * vi + 2];
    const float nx = P.normals[3 * vi], ny = P.normals[3 * vi + 1], nz = P.normals[3 * vi + 2];
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum = 0.f;
    int seen = 0;
    for (int k = 0; k < P.n_views; ++k) {
      const float4 q = proj[(int64_t)k * V + vi];
      if (!(q.w > 0.f)) continue;                                     // behind znear (or NaN)
      const float cj = rintf(q.x), ci = rintf(q.y);
      if (!(cj >= 0.f && cj <= fs && ci >= 0.f && ci <= fs)) continue;      // off the frame (or NaN)
      const unsigned long long key = P.keys[(int64_t)k * SS + (int64_t)(int)ci * S + (int)cj];
      const float zstar = key == MR_EMPTY ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
      if (!(q.z <= zstar + P.depth_tol)) continue;
      const float* cm = cams + (int64_t)k * MR_CAM_FLOATS;
      float dx = cm[0] - px, dy = cm[1] - py, dz = cm[2] - pz;
      normalize3(dx, dy, dz);
      const float c = (nx * dx + ny * dy) + nz * dz;
      if (!(c > 0.f)) continue;
      ++seen;
      float w = c;
      for (int e = 1; e < P.power; ++e) w *= c;
      if (!(w > 0.f)) continue;                                       // (the power underflowed)
      const float u = fminf(fmaxf((q.x + 0.5f) * (float)R / (float)S - 0.5f, 0.f), fr);
      const float v = fminf(fmaxf((q.y + 0.5f) * (float)R / (float)S - 0.5f, 0.f), fr);
      const float fx0 = floorf(u), fy0 = floorf(v);
      const int x0 = (int)fx0, y0 = (int)fy0;
      const int x1 = min(x0 + 1, R - 1), y1 = min(y0 + 1, R - 1);
      const float fx = u - fx0, fy = v - fy0;
      const float* img = P.images + (int64_t)k * 3 * RR;
      const int64_t r0 = (int64_t)y0 * R, r1 = (int64_t)y1 * R;
      acc0 += w * mc_bilinear(img, r0, r1, x0, x1, fx, fy);
      acc1 += w * mc_bilinear(img + RR, r0, r1, x0, x1, fx, fy);
      acc2 += w * mc_bilinear(img + 2 * RR, r0, r1, x0, x1, fx, fy);
      wsum += w;
    }
    if (P.colors) {
      const bool any = wsum > 0.f;
      P.colors[3 * vi] = any ? acc0 / wsum : P.fill;
      P.colors[3 * vi + 1] = any ? acc1 / wsum : P.fill;
      P.colors[3 * vi + 2] = any ? acc2 / wsum : P.fill;
    }
    if (P.weight) P.weight[vi] = wsum;
    if (P.seen) P.seen[vi] = seen;
  }
}

__global__ void __launch_bounds__(MR_THREADS) mc_albedo_kernel(const int32_t* __restrict__ face, const float* __restrict__ shade,
                                                               const float* __restrict__ attr, uint8_t* __restrict__ out,
                                                               int n_views, int S) {
  const int64_t SS = (int64_t)S * S, total = (int64_t)n_views * SS;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int view = (int)(idx / SS);
    const int64_t o = (int64_t)view * 3 * SS + (idx - (int64_t)view * SS);
    const bool hit = face[idx] >= 0;
    const float sh = shade[idx];
    for (int c = 0; c < 3; ++c) {
      uint8_t q = 255;                                // the reference's white background
      if (hit) q = unit_to_u8(sh * (attr[o + c * SS] + 1.f) / 2.f);
      out[o + c * SS] = q;
    }
  }
}

}  // namespace

extern "C" int cips3d_mesh_vertex_colors(const cips3d_mesh_color_params* p, void* stream) {
  if (!p) return CIPS3D_E_BADARG;
  const cips3d_mesh_color_params& P = *p;
  const int e = mr_check(P.V, 0, P.n_views, P.S);
  if (e == CIPS3D_E_BADARG || P.R < 1 || P.power < 1 || P.power > 8) return CIPS3D_E_BADARG;
  if (!P.workspace || !P.keys || (!P.colors && !P.weight && !P.seen)) return CIPS3D_E_BADARG;
  if (P.V > 0 && (!P.verts || !P.normals || (P.n_views > 0 && !P.images))) return CIPS3D_E_BADARG;
  if (e || P.R > 16384) return CIPS3D_E_UNSUPP;
  if (P.V == 0) return 0;
  const MrWorkspace m = mr_workspace(const_cast<void*>(P.workspace), P.n_views);
  hipLaunchKernelGGL(mc_vertex_kernel, dim3(mr_grid(P.V)), dim3(MR_THREADS), 0, as_stream(stream), P, m.cams, m.proj);
  return cips3d_launch_status();
}

extern "C" int cips3d_mesh_albedo_frame(const int32_t* face, const float* shade, const float* attr, uint8_t* out, int n_views,
                                        int S, void* stream) {
  const int e = mr_check(0, 0, n_views, S);
  if (e == CIPS3D_E_BADARG || !face || !shade || !attr || !out) return CIPS3D_E_BADARG;
  if (e) return e;
  if (n_views == 0) return 0;
  hipLaunchKernelGGL(mc_albedo_kernel, dim3(mr_grid((int64_t)n_views * S * S)), dim3(MR_THREADS), 0, as_stream(stream), face, shade,
                     attr, out, n_views, S);
  return cips3d_launch_status();
}
