// What the mesh rasteriser (mesh_raster.hip) shares with the passes that read its workspace (mesh_color.hip): the layout of
// the workspace, the empty key and the size limits of every entry point; and, through shade.h, the shade and its byte.
#pragma once
#include <algorithm>

#include "common.h"
#include "shade.h"

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_CAM_FLOATS = 16;                   // eye(3) x_ax(3) y_ax(3) z_ax(3) s znear pad(2)
constexpr unsigned long long MR_EMPTY = ~0ull;

struct MrWorkspace {
  float* cams;      // [n, MR_CAM_FLOATS]
  float4* proj;     // [n, V]: x_p, y_p, z, 1/z (1/z = -1: dropped by znear)
};

MrWorkspace mr_workspace(void* ws, int n_views) {
  MrWorkspace m;
  m.cams = static_cast<float*>(ws);
  m.proj = reinterpret_cast<float4*>(static_cast<char*>(ws) + ceil_div<int64_t>((int64_t)n_views * MR_CAM_FLOATS * 4, 256) * 256);
  return m;
}

// 0, or the error code, for the sizes every entry point takes
int mr_check(int64_t V, int64_t F, int n_views, int S) {
  if (V < 0 || F < 0 || n_views < 0 || S < 1) return CIPS3D_E_BADARG;
  // vertex and face ids are int32 (the key's low word holds the face id, `face` is int32); S bounds the pixel-space floats
  if (V > INT32_MAX || F > INT32_MAX || S > 16384 || n_views > 65536) return CIPS3D_E_UNSUPP;
  return 0;
}

int mr_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div<int64_t>(items, MR_THREADS), 1 << 16)); }

}  // namespace
