// Hard z-buffer rasteriser for the exported mesh (cips3d_mesh_rasterize / cips3d_mesh_resolve): nearest face per pixel,
// perspective-correct barycentrics, both windings, no blending.  The reference gets this from pytorch3d
// (exp/cips3d/utils.py:260-308 create_cameras / create_mesh_renderer; models/model_v3.py:344-415 project_noise).
//
//   camera   per view, one thread: (azim, elev, fov_deg, dist, znear) -> eye, the three axes, s = 1 / tan(fov / 2)
//   vertex   per (view, vertex): pixel-space position, view depth z and 1 / z; a vertex with z < znear is marked
//   face     per (view, face): bounding box clamped to the frame; a small box is walked by its thread, a large one by the
//            whole wave (the lanes stride the box, one large face of the wave at a time); every covered pixel takes a 64-bit
//            atomicMin of (fp32 bits of z) << 32 | face.  z > 0, so the bits order like the depths; an integer minimum does
//            not depend on arrival order: the buffer is bit-reproducible and independent of the grid, equal depths go to
//            the lower face index
//   resolve  per (view, pixel): decodes the winner, recomputes the barycentrics with the face pass's own expressions and
//            writes the maps
//
// Pixel space: x_p = (1 - x_n) S / 2 - 1/2, so that the centre of pixel (row i, column j) is (j, i).  Edge functions are
// cross products of the corners RELATIVE TO THE PIXEL CENTRE: the two faces of a shared edge evaluate exactly negated
// values, so a pixel centre is never lost between them (and is drawn by both only when the value is exactly zero).
// No LDS, no scratch; the library builds with -ffp-contract=off, so every expression below rounds as written.
#include "mesh_raster.h"          // the workspace layout, MR_EMPTY, mr_check, mr_grid: shared with mesh_color.hip; shade.h

namespace {

constexpr int MR_WAVE_BOX = 64;                     // boxes of more pixels than this go to the wave path

__global__ void __launch_bounds__(64) mr_camera_kernel(const float* __restrict__ cams_in, float* __restrict__ cams, int n_views) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n_views) return;
  const float az = cams_in[5 * v], el = cams_in[5 * v + 1], fov = cams_in[5 * v + 2], dist = cams_in[5 * v + 3];
  const float ce = cosf(el);
  const float cx = dist * (ce * sinf(az)), cy = dist * sinf(el), cz = dist * (ce * cosf(az));
  const float cn = sqrtf((cx * cx + cy * cy) + cz * cz);
  const float zx = -cx / cn, zy = -cy / cn, zz = -cz / cn;
  // x_ax = normalize((0,1,0) x z_ax) = normalize((zz, 0, -zx))
  const float xn = sqrtf(zz * zz + zx * zx);
  const float xx = zz / xn, xy = 0.f, xz = -zx / xn;
  // y_ax = z_ax x x_ax
  const float yx = zy * xz - zz * xy, yy = zz * xx - zx * xz, yz = zx * xy - zy * xx;
  float* o = cams + (int64_t)v * MR_CAM_FLOATS;
  o[0] = cx; o[1] = cy; o[2] = cz;
  o[3] = xx; o[4] = xy; o[5] = xz;
  o[6] = yx; o[7] = yy; o[8] = yz;
  o[9] = zx; o[10] = zy; o[11] = zz;
  o[12] = 1.f / tanf(fov * 0.00872664625997164788f);      // fov_deg * pi / 360
  o[13] = cams_in[5 * v + 4];
  o[14] = 0.f; o[15] = 0.f;
}

__global__ void __launch_bounds__(MR_THREADS) mr_vertex_kernel(const float* __restrict__ verts, int V, const float* __restrict__ cams,
                                                               int n_views, int S, float4* __restrict__ proj) {
  const int64_t total = (int64_t)n_views * V;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int view = (int)(idx / V);
    const int64_t vi = idx - (int64_t)view * V;
    const float* c = cams + (int64_t)view * MR_CAM_FLOATS;
    const float dx = verts[3 * vi] - c[0], dy = verts[3 * vi + 1] - c[1], dz = verts[3 * vi + 2] - c[2];
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
    proj[idx] = o;
  }
}

// one face of one view, as both passes see it
struct MrFace {
  float4 a, b, c;
  float area;
};

__device__ __forceinline__ bool mr_load_face(const int32_t* __restrict__ faces, int64_t f, int V, const float4* __restrict__ proj,
                                             MrFace& t) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  t.a = proj[i0]; t.b = proj[i1]; t.c = proj[i2];
  if (t.a.w <= 0.f || t.b.w <= 0.f || t.c.w <= 0.f) return false;       // a vertex behind znear drops the whole face
  t.area = (t.b.x - t.a.x) * (t.c.y - t.a.y) - (t.c.x - t.a.x) * (t.b.y - t.a.y);
  return fabsf(t.area) > 0.f;                                          // zero area (or NaN): skipped
}

// screen-space barycentrics of pixel centre (px, py); true when the face covers it
__device__ __forceinline__ bool mr_bary(const MrFace& t, float px, float py, float& b0, float& b1, float& b2) {
  const float ax = t.a.x - px, ay = t.a.y - py, bx = t.b.x - px, by = t.b.y - py, cx = t.c.x - px, cy = t.c.y - py;
  const float e0 = bx * cy - cx * by, e1 = cx * ay - ax * cy, e2 = ax * by - bx * ay;
  const bool in = t.area > 0.f ? (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) : (e0 <= 0.f && e1 <= 0.f && e2 <= 0.f);
  b0 = e0 / t.area; b1 = e1 / t.area; b2 = e2 / t.area;
  return in;
}

__device__ __forceinline__ float mr_depth(const MrFace& t, float b0, float b1, float b2) {
  return 1.f / ((b0 * t.a.w + b1 * t.b.w) + b2 * t.c.w);
}

__device__ __forceinline__ void mr_shade_pixel(const MrFace& t, int col, int row, unsigned f, unsigned long long* __restrict__ krow0,
                                               int S) {
  float b0, b1, b2;
  if (!mr_bary(t, (float)col, (float)row, b0, b1, b2)) return;
  const float z = mr_depth(t, b0, b1, b2);
  if (!(z > 0.f)) return;                            // (cannot happen for finite inputs: every 1/z_k > 0)
  atomicMin(krow0 + (int64_t)row * S + col, (unsigned long long)__float_as_uint(z) << 32 | f);
}

// clamped bounding box; false when empty
__device__ __forceinline__ bool mr_box(const MrFace& t, int S, int& x0, int& x1, int& y0, int& y1) {
  const float fs = (float)(S - 1);
  const float lx = fminf(fminf(t.a.x, t.b.x), t.c.x), hx = fmaxf(fmaxf(t.a.x, t.b.x), t.c.x);
  const float ly = fminf(fminf(t.a.y, t.b.y), t.c.y), hy = fmaxf(fmaxf(t.a.y, t.b.y), t.c.y);
  if (!(hx >= 0.f && lx <= fs && hy >= 0.f && ly <= fs)) return false;      // off the frame (or NaN)
  x0 = (int)fmaxf(ceilf(lx), 0.f); x1 = (int)fminf(floorf(hx), fs);
  y0 = (int)fmaxf(ceilf(ly), 0.f); y1 = (int)fminf(floorf(hy), fs);
  return x0 <= x1 && y0 <= y1;
}

__global__ void __launch_bounds__(MR_THREADS) mr_face_kernel(const int32_t* __restrict__ faces, int F, int V, int n_views, int S,
                                                             const float4* __restrict__ proj, unsigned long long* __restrict__ keys) {
  const int lane = threadIdx.x & 63;
  const int64_t total = (int64_t)n_views * F;
  const int64_t padded = ceil_div<int64_t>(total, 64) * 64;           // whole waves stay in the loop together
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < padded; idx += (int64_t)gridDim.x * blockDim.x) {
    bool large = false;
    if (idx < total) {
      const int view = (int)(idx / F);
      const int64_t f = idx - (int64_t)view * F;
      MrFace t;
      int x0, x1, y0, y1;
      if (mr_load_face(faces, f, V, proj + (int64_t)view * V, t) && mr_box(t, S, x0, x1, y0, y1)) {
        if ((int64_t)(x1 - x0 + 1) * (y1 - y0 + 1) > MR_WAVE_BOX) {
          large = true;
        } else {
          unsigned long long* k0 = keys + (int64_t)view * S * S;
          for (int r = y0; r <= y1; ++r)
            for (int c = x0; c <= x1; ++c) mr_shade_pixel(t, c, r, (unsigned)f, k0, S);
        }
      }
    }
    // the wave's large faces, one at a time, every lane striding the box
    unsigned long long m = __ballot(large);
    while (m) {
      const int src = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t widx = idx - lane + src;
      const int view = (int)(widx / F);
      const int64_t f = widx - (int64_t)view * F;
      MrFace t;
      int x0, x1, y0, y1;
      if (!mr_load_face(faces, f, V, proj + (int64_t)view * V, t) || !mr_box(t, S, x0, x1, y0, y1)) continue;   // (wave-uniform)
      unsigned long long* k0 = keys + (int64_t)view * S * S;
      const int bw = x1 - x0 + 1;
      const int64_t npix = (int64_t)bw * (y1 - y0 + 1);
      for (int64_t q = lane; q < npix; q += 64) {
        const int r = (int)(q / bw);
        mr_shade_pixel(t, x0 + (int)(q - (int64_t)r * bw), y0 + r, (unsigned)f, k0, S);
      }
    }
  }
}

__global__ void __launch_bounds__(MR_THREADS) mr_resolve_kernel(cips3d_mesh_resolve_params P, const float* __restrict__ cams,
                                                                const float4* __restrict__ proj) {
  const int S = P.S, V = P.V;
  const int64_t SS = (int64_t)S * S, total = (int64_t)P.n_views * SS;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int view = (int)(idx / SS);
    const int64_t pix = idx - (int64_t)view * SS;
    const int row = (int)(pix / S), col = (int)(pix - (int64_t)row * S);
    const unsigned long long key = P.keys[idx];
    MrFace t;
    int64_t f = (int64_t)(key & 0xffffffffull);
    bool hit = key != MR_EMPTY && f < P.F && mr_load_face(P.faces, f, V, proj + (int64_t)view * V, t);
    float w0 = -1.f, w1 = -1.f, w2 = -1.f, z = -1.f;
    if (hit) {
      float b0, b1, b2;
      mr_bary(t, (float)col, (float)row, b0, b1, b2);
      z = mr_depth(t, b0, b1, b2);
      w0 = (b0 * t.a.w) * z; w1 = (b1 * t.b.w) * z; w2 = (b2 * t.c.w) * z;
    }
    if (P.face) P.face[idx] = hit ? (int32_t)f : -1;
    if (P.zbuf) P.zbuf[idx] = hit ? __uint_as_float((unsigned)(key >> 32)) : -1.f;
    if (P.bary) { P.bary[3 * idx] = w0; P.bary[3 * idx + 1] = w1; P.bary[3 * idx + 2] = w2; }
    int i0 = 0, i1 = 0, i2 = 0;
    if (hit) { i0 = P.faces[3 * f]; i1 = P.faces[3 * f + 1]; i2 = P.faces[3 * f + 2]; }
    if (P.attr_out) {
      const int C = P.n_attr;
      for (int c = 0; c < C; ++c) {
        const int64_t o = ((int64_t)view * C + c) * SS + pix;
        float v;
        if (hit) v = (w0 * P.attr[(int64_t)i0 * C + c] + w1 * P.attr[(int64_t)i1 * C + c]) + w2 * P.attr[(int64_t)i2 * C + c];
        else v = P.base ? P.base[o] : P.fill;
        P.attr_out[o] = v;
      }
    }
    if (P.shade || P.shade_u8) {
      float sh = 1.f;                                 // the reference's white background
      if (hit) {
        const float* n0 = P.normals + 3 * (int64_t)i0; const float* n1 = P.normals + 3 * (int64_t)i1; const float* n2 = P.normals + 3 * (int64_t)i2;
        const float* p0 = P.verts + 3 * (int64_t)i0; const float* p1 = P.verts + 3 * (int64_t)i1; const float* p2 = P.verts + 3 * (int64_t)i2;
        float nx = (w0 * n0[0] + w1 * n1[0]) + w2 * n2[0], ny = (w0 * n0[1] + w1 * n1[1]) + w2 * n2[1],
              nz = (w0 * n0[2] + w1 * n1[2]) + w2 * n2[2];
        const float px = (w0 * p0[0] + w1 * p1[0]) + w2 * p2[0], py = (w0 * p0[1] + w1 * p1[1]) + w2 * p2[1],
                    pz = (w0 * p0[2] + w1 * p1[2]) + w2 * p2[2];
        normalize3(nx, ny, nz);
        const float* cm = cams + (int64_t)view * MR_CAM_FLOATS;
        float lx = P.light[3 * view] - px, ly = P.light[3 * view + 1] - py, lz = P.light[3 * view + 2] - pz;
        float vx = cm[0] - px, vy = cm[1] - py, vz = cm[2] - pz;
        sh = phong_white(nx, ny, nz, lx, ly, lz, vx, vy, vz, P.ka, P.kd, P.ks, P.shininess);
      }
      if (P.shade) P.shade[idx] = sh;
      if (P.shade_u8) {
        const uint8_t q = unit_to_u8(sh);
        const int64_t o = (int64_t)view * 3 * SS + pix;
        P.shade_u8[o] = q; P.shade_u8[o + SS] = q; P.shade_u8[o + 2 * SS] = q;
      }
    }
  }
}

}  // namespace

extern "C" int64_t cips3d_mesh_raster_workspace_bytes(int64_t V, int64_t F, int n_views, int S) {
  const int e = mr_check(V, F, n_views, S);
  if (e) return e;
  return ceil_div<int64_t>((int64_t)n_views * MR_CAM_FLOATS * 4, 256) * 256 + (int64_t)n_views * V * (int64_t)sizeof(float4) + 256;
}

extern "C" int cips3d_mesh_rasterize(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* cams,
                                     int n_views, int S, void* workspace, uint64_t* keys, void* stream) {
  const int e = mr_check(V, F, n_views, S);
  if (e) return e;
  if (!cams || !workspace || !keys || (V > 0 && !verts) || (F > 0 && !faces)) return CIPS3D_E_BADARG;
  if (n_views == 0) return 0;
  hipStream_t st = as_stream(stream);
  const MrWorkspace m = mr_workspace(workspace, n_views);
  if (hipMemsetAsync(keys, 0xff, (size_t)n_views * S * S * sizeof(uint64_t), st) != hipSuccess) return cips3d_launch_status();
  hipLaunchKernelGGL(mr_camera_kernel, dim3(ceil_div(n_views, 64)), dim3(64), 0, st, cams, m.cams, n_views);
  int rc = cips3d_launch_status();
  if (rc || V == 0 || F == 0) return rc;
  hipLaunchKernelGGL(mr_vertex_kernel, dim3(mr_grid((int64_t)n_views * V)), dim3(MR_THREADS), 0, st, verts, (int)V, m.cams, n_views,
                     S, m.proj);
  rc = cips3d_launch_status();
  if (rc) return rc;
  hipLaunchKernelGGL(mr_face_kernel, dim3(mr_grid((int64_t)n_views * F)), dim3(MR_THREADS), 0, st, faces, (int)F, (int)V, n_views, S,
                     m.proj, reinterpret_cast<unsigned long long*>(keys));
  return cips3d_launch_status();
}

extern "C" int cips3d_mesh_resolve(const cips3d_mesh_resolve_params* p, void* stream) {
  if (!p) return CIPS3D_E_BADARG;
  const cips3d_mesh_resolve_params& P = *p;
  const int e = mr_check(P.V, P.F, P.n_views, P.S);
  if (e) return e;
  if (!P.workspace || !P.keys || (P.F > 0 && (!P.faces || !P.verts))) return CIPS3D_E_BADARG;
  if (P.attr_out && (P.n_attr < 1 || (P.F > 0 && !P.attr))) return CIPS3D_E_BADARG;
  if ((P.shade || P.shade_u8) && (!P.light || (P.F > 0 && !P.normals))) return CIPS3D_E_BADARG;
  if (P.n_views == 0) return 0;
  const MrWorkspace m = mr_workspace(const_cast<void*>(P.workspace), P.n_views);
  hipLaunchKernelGGL(mr_resolve_kernel, dim3(mr_grid((int64_t)P.n_views * P.S * P.S)), dim3(MR_THREADS), 0, as_stream(stream), P,
                     m.cams, m.proj);
  return cips3d_launch_status();
}
