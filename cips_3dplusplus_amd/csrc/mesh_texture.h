// The texture atlas of the exported mesh, stated once for the host and every kernel of mesh_texture.hip (the contract:
// include/cips3d_hip.h, cips3d_mesh_texture_bake).  Pure arithmetic, no unwrap: faces 2c and 2c + 1 share cell c, a block of
// (T + 1) x T texels at column c % cols, row c / cols of the atlas.  With m = T - 2, a texel at local (i, j), d = i + j:
//   d <= m      face 2c, owned:      lattice (i, j)
//   d == m + 1  face 2c, gutter:     lattice (i - 1/2, j - 1/2)
//   d == m + 2  face 2c + 1, gutter: lattice (i' - 1/2, j' - 1/2),   i' = T - i, j' = T - 1 - j
//   d >= m + 3  face 2c + 1, owned:  lattice (i', j')
// and barycentrics b1 = clamp(li / m, 0, 1), b2 = clamp(lj / m, 0, 1), b0 = max(0, (1 - b1) - b2).  Every face owns
// T (T - 1) / 2 texels and T gutter texels; a texel whose face is >= F is unowned.  The lattice point (li, lj) of the lower
// face sits at the centre of texel (li, lj) of the cell, that of the upper face at the centre of texel (T - li, T - 1 - lj):
// a bilinear fetch anywhere inside a face's triangle touches, with non-zero weight, only texels of that face (mt_fetch).
#pragma once
#include "mesh_raster.h"

namespace {

constexpr int MT_T_MIN = 3, MT_T_MAX = 64;
constexpr int MT_ATLAS_MAX = 16384;                 // texels per side
constexpr int MT_MAX_ITERS = 4096;                  // rings of cips3d_mesh_fill_colors

// the default number of cell columns: the smallest that makes the atlas at least as wide as it is tall
inline int mt_default_cols(int64_t F, int T) {
  const int64_t cells = (F + 1) / 2;
  int64_t cols = 1;
  while (cols * cols * (T + 1) < cells * T) ++cols;         // ceil(sqrt(cells T / (T + 1))) in integers; cols <= ~47000
  return (int)cols;
}

inline int64_t mt_rows(int64_t F, int cols) { return ceil_div<int64_t>((F + 1) / 2, cols); }

// 0, or the error code, for an atlas of `cols` x `rows` cells of T texels that has to hold F faces
inline int mt_atlas_check(int64_t F, int T, int cols, int rows) {
  if (F < 0 || T < MT_T_MIN || T > MT_T_MAX || cols < 1 || rows < 0 || (int64_t)cols * rows < (F + 1) / 2) return CIPS3D_E_BADARG;
  if ((int64_t)cols * (T + 1) > MT_ATLAS_MAX || (int64_t)rows * T > MT_ATLAS_MAX) return CIPS3D_E_UNSUPP;
  return 0;
}

struct MtTexel {
  int64_t face;     // may be >= F: unowned
  float li, lj;     // the lattice point
  int gutter;
};

__host__ __device__ inline MtTexel mt_texel(int x, int y, int T, int cols) {
  const int cx = x / (T + 1), i = x - cx * (T + 1);
  const int cy = y / T, j = y - cy * T;
  const int64_t c = (int64_t)cy * cols + cx;
  const int d = i + j, m = T - 2;
  MtTexel t;
  if (d <= m + 1) {
    t.face = 2 * c; t.gutter = d == m + 1;
    t.li = (float)i; t.lj = (float)j;
  } else {
    t.face = 2 * c + 1; t.gutter = d == m + 2;
    t.li = (float)(T - i); t.lj = (float)(T - 1 - j);
  }
  if (t.gutter) { t.li -= 0.5f; t.lj -= 0.5f; }
  return t;
}

__host__ __device__ inline void mt_bary(float li, float lj, int T, float& b0, float& b1, float& b2) {
  const float m = (float)(T - 2);
  b1 = fminf(fmaxf(li / m, 0.f), 1.f);
  b2 = fminf(fmaxf(lj / m, 0.f), 1.f);
  b0 = fmaxf(0.f, (1.f - b1) - b2);
}

// the cell's origin in texels
__host__ __device__ inline void mt_origin(int64_t f, int T, int cols, int& ox, int& oy) {
  const int64_t c = f >> 1;
  ox = (int)(c % cols) * (T + 1);
  oy = (int)(c / cols) * T;
}

// corner UVs of face f in continuous texel coordinates (the centre of texel k is k + 1/2): uv = (x0, y0, x1, y1, x2, y2)
__host__ __device__ inline void mt_corner_uv(int64_t f, int T, int cols, float* uv) {
  int ox, oy;
  mt_origin(f, T, cols, ox, oy);
  const float m = (float)(T - 2);
  if (!(f & 1)) {
    const float x = (float)ox + 0.5f, y = (float)oy + 0.5f;
    uv[0] = x; uv[1] = y; uv[2] = x + m; uv[3] = y; uv[4] = x; uv[5] = y + m;
  } else {
    const float x = (float)(ox + T) + 0.5f, y = (float)(oy + T) - 0.5f;
    uv[0] = x; uv[1] = y; uv[2] = x - m; uv[3] = y; uv[4] = x; uv[5] = y - m;
  }
}

}  // namespace
