// A texture atlas for the exported mesh (cips3d_mesh_fill_colors, cips3d_mesh_texture_bake, cips3d_mesh_textured_frame): an
// extension, like the vertex colours it grows from (mesh_color.hip; the reference exports a grey surface).
//
//   fill   grows colours from the vertices some view saw into those none saw, ring by ring.  A ring is two launches: per face,
//          every unfilled corner takes the colours of the corners filled before this ring as 64-bit integer atomic adds of
//          q(x) = rintf(x 2^20) (integer sums do not depend on arrival order: the result is exact and bit-reproducible); per
//          vertex, the mean becomes the colour.  The host enqueues all `iters` rings without looking at the device; a ring that
//          fills nothing leaves its flag at zero, and every later launch returns on that flag
//   bake   per atlas texel, one thread: the texel's surface point and normal from the atlas layout (mesh_texture.h), then, views
//          in ascending order, the vertex colours' gather at that point.  No atomics: independent of the grid, bit-reproducible
//   frame  per (view, pixel): the resolve pass's face and barycentrics -> a bilinear fetch inside the face's own texels -> uint8
//
// No LDS.  The library builds with -ffp-contract=off, so every expression below rounds as written.
#include "mesh_texture.h"

namespace {

// The projection of a point by the derived camera c [MR_CAM_FLOATS] into an S x S frame -> (x_p, y_p, z, 1/z; 1/z = -1: dropped
// by znear).  This restates the body of mr_vertex_kernel (mesh_raster.hip) expression by expression: calling one shared device
// function from that kernel changed its instruction schedule, and the rasteriser's code objects are kept as they are.
__device__ __forceinline__ float4 mt_project_point(float px, float py, float pz, const float* __restrict__ c, int S) {
  const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
  const float vx = (dx * c[3] + dy * c[4]) + dz * c[5];
  const float vy = (dx * c[6] + dy * c[7]) + dz * c[8];
  const float vz = (dx * c[9] + dy * c[10]) + dz * c[11];
  const float s = c[12], znear = c[13];
  const float half = 0.5f * (float)S;
  float4 o;
  o.x = (1.f - s * vx / vz) * half - 0.5f;
  o.y = (1.f - s * vy / vz) * half - 0.5f;
  o.z = vz;
  o.w = (vz >= znear && vz > 0.f) ? 1.f / vz : -1.f;      // NaN: dropped
  return o;
}

// one channel of a map of row pitch folded into r0 / r1, at the four taps
__device__ __forceinline__ float mt_bilinear(const float* __restrict__ img, int64_t r0, int64_t r1, int x0, int x1, float fx, float fy) {
  const float top = (1.f - fx) * img[r0 + x0] + fx * img[r0 + x1];
  const float bot = (1.f - fx) * img[r1 + x0] + fx * img[r1 + x1];
  return (1.f - fy) * top + fy * bot;
}

// ------------------------------------------------------------------------------------------------ fill
constexpr float MT_Q = 1048576.f;                   // 2^20

__global__ void __launch_bounds__(MR_THREADS) mt_fill_init_kernel(const float* __restrict__ colors, const float* __restrict__ weight,
                                                                  float* __restrict__ out, int32_t* __restrict__ filled,
                                                                  int32_t* __restrict__ flags, int V) {
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    out[3 * v] = colors[3 * v]; out[3 * v + 1] = colors[3 * v + 1]; out[3 * v + 2] = colors[3 * v + 2];
    filled[v] = weight[v] > 0.f ? 0 : -1;
    if (v == 0) flags[0] = 1;                       // "ring 0 filled something": ring 1 runs
  }
}

__global__ void __launch_bounds__(MR_THREADS) mt_fill_face_kernel(const int32_t* __restrict__ faces, int F, int V,
                                                                  const float* __restrict__ col, const int32_t* __restrict__ filled,
                                                                  unsigned long long* __restrict__ sums,
                                                                  const int32_t* __restrict__ flags, int ring) {
  if (flags[ring - 1] == 0) return;                 // the ring before filled nothing: neither will this one
  for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
    int id[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    if ((unsigned)id[0] >= (unsigned)V || (unsigned)id[1] >= (unsigned)V || (unsigned)id[2] >= (unsigned)V) continue;
    bool has[3];
    long long q[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      has[k] = filled[id[k]] >= 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) q[k][c] = has[k] ? (long long)rintf(col[3 * (int64_t)id[k] + c] * MT_Q) : 0;
    }
    if (has[0] == has[1] && has[1] == has[2]) continue;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (has[a]) continue;
      const int b0 = (a + 1) % 3, b1 = (a + 2) % 3;
      const long long n = (long long)has[b0] + (long long)has[b1];         // (>= 1 here)
      unsigned long long* s = sums + 4 * (int64_t)id[a];
#pragma unroll
      for (int c = 0; c < 3; ++c) atomicAdd(s + c, (unsigned long long)(q[b0][c] + q[b1][c]));
      atomicAdd(s + 3, (unsigned long long)n);
    }
  }
}

__global__ void __launch_bounds__(MR_THREADS) mt_fill_vertex_kernel(float* __restrict__ col, int32_t* __restrict__ filled,
                                                                    unsigned long long* __restrict__ sums, int32_t* __restrict__ flags,
                                                                    int V, int ring) {
  if (flags[ring - 1] == 0) return;
  bool any = false;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    if (filled[v] >= 0) continue;
    unsigned long long* s = sums + 4 * v;
    const long long n = (long long)s[3];
    if (n <= 0) continue;
    const double den = (double)n * 1048576.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      col[3 * v + c] = (float)((double)(long long)s[c] / den);
      s[c] = 0;
    }
    s[3] = 0;
    filled[v] = ring;
    any = true;
  }
  if (any) flags[ring] = 1;                         // (every writer stores the same value)
}

// ------------------------------------------------------------------------------------------------ bake
__global__ void __launch_bounds__(MR_THREADS) mt_bake_kernel(cips3d_mesh_texture_params P, const float* __restrict__ cams) {
  const int T = P.T, S = P.S, R = P.R, V = P.V;
  const int Wt = P.cols * (T + 1);
  const int64_t HW = (int64_t)Wt * (P.rows * T);
  const float fs = (float)(S - 1), fr = (float)(R - 1);
  const int64_t SS = (int64_t)S * S, RR = (int64_t)R * R;
  const unsigned long long* __restrict__ keys = reinterpret_cast<const unsigned long long*>(P.keys);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < HW; idx += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(idx / Wt), x = (int)(idx - (int64_t)y * Wt);
    const MtTexel t = mt_texel(x, y, T, P.cols);
    float o0 = P.fill, o1 = P.fill, o2 = P.fill, wsum = 0.f;
    int seen = 0;
    int i0 = 0, i1 = 0, i2 = 0;
    bool owned = t.face < P.F;
    if (owned) {
      i0 = P.faces[3 * t.face]; i1 = P.faces[3 * t.face + 1]; i2 = P.faces[3 * t.face + 2];
      owned = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;      // as the rasteriser skips it
    }
    if (owned) {
      float b0, b1, b2;
      mt_bary(t.li, t.lj, T, b0, b1, b2);
      const float* p0 = P.verts + 3 * (int64_t)i0; const float* p1 = P.verts + 3 * (int64_t)i1; const float* p2 = P.verts + 3 * (int64_t)i2;
      const float* n0 = P.normals + 3 * (int64_t)i0; const float* n1 = P.normals + 3 * (int64_t)i1; const float* n2 = P.normals + 3 * (int64_t)i2;
      const float px = (b0 * p0[0] + b1 * p1[0]) + b2 * p2[0], py = (b0 * p0[1] + b1 * p1[1]) + b2 * p2[1],
                  pz = (b0 * p0[2] + b1 * p1[2]) + b2 * p2[2];
      float nx = (b0 * n0[0] + b1 * n1[0]) + b2 * n2[0], ny = (b0 * n0[1] + b1 * n1[1]) + b2 * n2[1],
            nz = (b0 * n0[2] + b1 * n1[2]) + b2 * n2[2];
      normalize3(nx, ny, nz);
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
      // from the projection on: cips3d_mesh_vertex_colors' contract, as mc_vertex_kernel (mesh_color.hip) states it
      for (int k = 0; k < P.n_views; ++k) {
        const float* cm = cams + (int64_t)k * MR_CAM_FLOATS;
        const float4 q = mt_project_point(px, py, pz, cm, S);
        if (!(q.w > 0.f)) continue;                                     // behind znear (or NaN)
        const float cj = rintf(q.x), ci = rintf(q.y);
        if (!(cj >= 0.f && cj <= fs && ci >= 0.f && ci <= fs)) continue;      // off the frame (or NaN)
        const unsigned long long key = keys[(int64_t)k * SS + (int64_t)(int)ci * S + (int)cj];
        const float zstar = key == MR_EMPTY ? __builtin_inff() : __uint_as_float((unsigned)(key >> 32));
        if (!(q.z <= zstar + P.depth_tol)) continue;
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
        acc0 += w * mt_bilinear(img, r0, r1, x0, x1, fx, fy);
        acc1 += w * mt_bilinear(img + RR, r0, r1, x0, x1, fx, fy);
        acc2 += w * mt_bilinear(img + 2 * RR, r0, r1, x0, x1, fx, fy);
        wsum += w;
      }
      if (wsum > 0.f) {
        o0 = acc0 / wsum; o1 = acc1 / wsum; o2 = acc2 / wsum;
      } else if (P.vertex_colors && P.filled[i0] >= 0 && P.filled[i1] >= 0 && P.filled[i2] >= 0) {
        const float* c0 = P.vertex_colors + 3 * (int64_t)i0; const float* c1 = P.vertex_colors + 3 * (int64_t)i1;
        const float* c2 = P.vertex_colors + 3 * (int64_t)i2;
        o0 = (b0 * c0[0] + b1 * c1[0]) + b2 * c2[0];
        o1 = (b0 * c0[1] + b1 * c1[1]) + b2 * c2[1];
        o2 = (b0 * c0[2] + b1 * c1[2]) + b2 * c2[2];
      }
    }
    if (P.texture) { P.texture[idx] = o0; P.texture[HW + idx] = o1; P.texture[2 * HW + idx] = o2; }
    if (P.weight) P.weight[idx] = wsum;
    if (P.seen) P.seen[idx] = seen;
  }
}

// ------------------------------------------------------------------------------------------------ frame
__global__ void __launch_bounds__(MR_THREADS) mt_frame_kernel(const int32_t* __restrict__ face, const float* __restrict__ bary,
                                                              const float* __restrict__ shade, const float* __restrict__ tex,
                                                              uint8_t* __restrict__ out, int n_views, int S, int F, int T, int cols,
                                                              int rows) {
  const int64_t SS = (int64_t)S * S, total = (int64_t)n_views * SS;
  const int Wt = cols * (T + 1);
  const int64_t HW = (int64_t)Wt * (rows * T);
  const float m = (float)(T - 2);
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int view = (int)(idx / SS);
    const int64_t o = (int64_t)view * 3 * SS + (idx - (int64_t)view * SS);
    const int f = face[idx];
    const bool hit = f >= 0 && f < F;
    uint8_t q0 = 255, q1 = 255, q2 = 255;             // the reference's white background
    if (hit) {
      const float b1 = fminf(fmaxf(bary[3 * idx + 1], 0.f), 1.f);
      const float b2 = fminf(fmaxf(bary[3 * idx + 2], 0.f), 1.f - b1);
      // the point b0 uv0 + b1 uv1 + b2 uv2 of the face's UV triangle (mt_corner_uv), fetched bilinearly at (x - 1/2, y - 1/2): in
      // the face's lattice that is (fx, fy) = (b1 m, b2 m), and the four taps are lattice texels (i0 + {0,1}, j0 + {0,1}).
      // fy <= fl(m - fx) keeps i + j of a tap of non-zero weight at m + 1 or below, the face's own gutter, whatever b1 m + b2 m
      // rounds to.  The upper face's lattice is the lower one's mirrored: the same weights, texel (T - i, T - 1 - j)
      const float fx = b1 * m, fy = fminf(b2 * m, m - fx);
      const float fi = floorf(fx), fj = floorf(fy);
      const int i0 = (int)fi, j0 = (int)fj;
      const float wx = fx - fi, wy = fy - fj;
      int ox, oy;
      mt_origin(f, T, cols, ox, oy);
      int xa, xb, ya, yb;
      if (!(f & 1)) { xa = ox + i0; xb = xa + 1; ya = oy + j0; yb = ya + 1; }
      else { xa = ox + T - i0; xb = xa - 1; ya = oy + T - 1 - j0; yb = ya - 1; }
      // i0 + 1 <= m + 1 = T - 1 and j0 + 1 <= T - 1: every tap lies inside the cell, so inside the atlas
      const int64_t r0 = (int64_t)ya * Wt, r1 = (int64_t)yb * Wt;
      const float sh = shade[idx];
      const float c0 = mt_bilinear(tex, r0, r1, xa, xb, wx, wy), c1 = mt_bilinear(tex + HW, r0, r1, xa, xb, wx, wy),
                  c2 = mt_bilinear(tex + 2 * HW, r0, r1, xa, xb, wx, wy);
      q0 = unit_to_u8(sh * (c0 + 1.f) / 2.f);
      q1 = unit_to_u8(sh * (c1 + 1.f) / 2.f);
      q2 = unit_to_u8(sh * (c2 + 1.f) / 2.f);
    }
    out[o] = q0; out[o + SS] = q1; out[o + 2 * SS] = q2;
  }
}

int64_t mt_fill_bytes(int64_t V) { return ceil_div<int64_t>(V * 32 + (int64_t)(MT_MAX_ITERS + 1) * 4, 256) * 256; }

}  // namespace

extern "C" int cips3d_mesh_atlas_layout(int64_t F, int T, int cols_in, int32_t* cols, int32_t* rows, int32_t* width, int32_t* height) {
  if (F < 0 || T < MT_T_MIN || T > MT_T_MAX || cols_in < 0 || !cols || !rows || !width || !height) return CIPS3D_E_BADARG;
  if (F > INT32_MAX) return CIPS3D_E_UNSUPP;
  const int c = cols_in > 0 ? cols_in : mt_default_cols(F, T);
  const int64_t r = mt_rows(F, c);
  if ((int64_t)c * (T + 1) > MT_ATLAS_MAX || r * T > MT_ATLAS_MAX) return CIPS3D_E_UNSUPP;
  *cols = c; *rows = (int32_t)r; *width = c * (T + 1); *height = (int32_t)r * T;
  return 0;
}

extern "C" int cips3d_mesh_atlas_uv(int64_t F, int T, int cols, float* uv_host) {
  if (F < 0 || T < MT_T_MIN || T > MT_T_MAX || cols < 1 || (F > 0 && !uv_host)) return CIPS3D_E_BADARG;
  for (int64_t f = 0; f < F; ++f) mt_corner_uv(f, T, cols, uv_host + 6 * f);
  return 0;
}

extern "C" int cips3d_mesh_atlas_texels(int64_t F, int T, int cols, int rows, int32_t* face_host, float* bary_host,
                                        uint8_t* gutter_host) {
  const int e = mt_atlas_check(F, T, cols, rows);
  if (e) return e;
  const int Wt = cols * (T + 1), Ht = rows * T;
  for (int y = 0; y < Ht; ++y)
    for (int x = 0; x < Wt; ++x) {
      const int64_t idx = (int64_t)y * Wt + x;
      const MtTexel t = mt_texel(x, y, T, cols);
      const bool owned = t.face < F;
      if (face_host) face_host[idx] = owned ? (int32_t)t.face : -1;
      if (gutter_host) gutter_host[idx] = owned && t.gutter;
      if (bary_host) {
        float b0 = 0.f, b1 = 0.f, b2 = 0.f;
        if (owned) mt_bary(t.li, t.lj, T, b0, b1, b2);
        bary_host[3 * idx] = b0; bary_host[3 * idx + 1] = b1; bary_host[3 * idx + 2] = b2;
      }
    }
  return 0;
}

extern "C" int64_t cips3d_mesh_fill_workspace_bytes(int64_t V) {
  if (V < 0) return CIPS3D_E_BADARG;
  if (V > INT32_MAX) return CIPS3D_E_UNSUPP;
  return mt_fill_bytes(V);
}

extern "C" int cips3d_mesh_fill_colors(const float* colors, const float* weight, const int32_t* faces, int64_t V, int64_t F, int iters,
                                       float* colors_out, int32_t* filled, void* workspace, void* stream) {
  if (V < 0 || F < 0 || iters < 0 || iters > MT_MAX_ITERS) return CIPS3D_E_BADARG;
  if (V > 0 && F > 0 && (!colors || !weight || !faces || !colors_out || !filled || !workspace)) return CIPS3D_E_BADARG;
  if (colors_out && colors_out == colors) return CIPS3D_E_BADARG;
  if (V > INT32_MAX || F > INT32_MAX) return CIPS3D_E_UNSUPP;
  if (V == 0 || F == 0) return 0;
  hipStream_t st = as_stream(stream);
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  int32_t* flags = reinterpret_cast<int32_t*>(sums + 4 * V);
  if (hipMemsetAsync(workspace, 0, (size_t)mt_fill_bytes(V), st) != hipSuccess) return cips3d_launch_status();
  hipLaunchKernelGGL(mt_fill_init_kernel, dim3(mr_grid(V)), dim3(MR_THREADS), 0, st, colors, weight, colors_out, filled, flags, (int)V);
  int rc = cips3d_launch_status();
  for (int ring = 1; ring <= iters && rc == 0; ++ring) {
    hipLaunchKernelGGL(mt_fill_face_kernel, dim3(mr_grid(F)), dim3(MR_THREADS), 0, st, faces, (int)F, (int)V, colors_out, filled, sums,
                       flags, ring);
    hipLaunchKernelGGL(mt_fill_vertex_kernel, dim3(mr_grid(V)), dim3(MR_THREADS), 0, st, colors_out, filled, sums, flags, (int)V, ring);
    rc = cips3d_launch_status();
  }
  return rc;
}

extern "C" int cips3d_mesh_texture_bake(const cips3d_mesh_texture_params* p, void* stream) {
  if (!p) return CIPS3D_E_BADARG;
  const cips3d_mesh_texture_params& P = *p;
  const int e = mr_check(P.V, P.F, P.n_views, P.S);
  const int a = mt_atlas_check(P.F, P.T, P.cols, P.rows);
  if (e == CIPS3D_E_BADARG || a == CIPS3D_E_BADARG || P.R < 1 || P.power < 1 || P.power > 8) return CIPS3D_E_BADARG;
  if (!P.workspace || !P.keys || (!P.texture && !P.weight && !P.seen)) return CIPS3D_E_BADARG;
  if ((P.vertex_colors == nullptr) != (P.filled == nullptr)) return CIPS3D_E_BADARG;
  if (P.V > 0 && P.F > 0 && (!P.verts || !P.normals || !P.faces || (P.n_views > 0 && !P.images))) return CIPS3D_E_BADARG;
  if (e || a || P.R > 16384) return CIPS3D_E_UNSUPP;
  if (P.V == 0 || P.F == 0) return 0;
  const MrWorkspace m = mr_workspace(const_cast<void*>(P.workspace), P.n_views);
  const int64_t texels = (int64_t)P.cols * (P.T + 1) * P.rows * P.T;
  hipLaunchKernelGGL(mt_bake_kernel, dim3(mr_grid(texels)), dim3(MR_THREADS), 0, as_stream(stream), P, m.cams);
  return cips3d_launch_status();
}

extern "C" int cips3d_mesh_textured_frame(const int32_t* face, const float* bary, const float* shade, const float* texture, uint8_t* out,
                                          int n_views, int S, int64_t F, int T, int cols, int rows, void* stream) {
  const int e = mr_check(0, F, n_views, S);
  const int a = mt_atlas_check(F, T, cols, rows);
  if (e == CIPS3D_E_BADARG || a == CIPS3D_E_BADARG || !face || !bary || !shade || !out || (F > 0 && !texture)) return CIPS3D_E_BADARG;
  if (e || a) return CIPS3D_E_UNSUPP;
  if (n_views == 0 || F == 0) return 0;
  hipLaunchKernelGGL(mt_frame_kernel, dim3(mr_grid((int64_t)n_views * S * S)), dim3(MR_THREADS), 0, as_stream(stream), face, bary, shade,
                     texture, out, n_views, S, (int)F, T, cols, rows);
  return cips3d_launch_status();
}
