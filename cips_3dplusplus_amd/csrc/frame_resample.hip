// Pillow's 8-bit image resampling on the device, bit for bit: PIL.Image.resize(size, BOX | BILINEAR | BICUBIC | LANCZOS) of every
// channel of planar uint8 images (Pillow's src/libImaging/Resample.c: ImagingResampleHorizontal_8bpc / ...Vertical_8bpc).  It is
// what the reference's demo pages do to every frame on the host -- `pil_utils.pil_resize` of the thumbnail and the geometry
// picture before `merge_image_pil` (render_video_web_v10.py:1825-1890), `load_pil_crop_resize` of an inversion's target.
//
// The host makes the tables in float64 (cips_3dplusplus_amd/frames.py: resample_coeffs): per output index a window (xmin, n) and
// n coefficients k = round(w 2^22).  Everything here is integer:
//     pixel = clamp((2^21 + sum_x p[xmin + x] k_x) >> 22, 0, 255)        (arithmetic shift)
// in plain 32-bit multiply-adds.  The width matters, the order does not.  Pillow's own bound keeps the sum inside int32: 8 bits of
// pixel, 22 of coefficient, and the two bits left over hold the over- and undershoot of the filters with negative lobes (the
// normalised |w| of a window sum to less than 2) -- PRECISION_BITS = 32 - 8 - 2 there; it is not re-derived at run time.  The
// horizontal pass runs first and its rounded, clamped uint8 result is what the vertical pass reads; an axis whose size does
// not change is not filtered (ksize 0).  No atomics, no floating point apart from the optional quantise-on-load of an fp32
// [-1, 1] source (cips3d_quant_u8, common.h: cips3d_rgb_to_uint8's arithmetic).
//
// rs_horiz_kernel / rs_vert_kernel   one pass each, a thread per four consecutive output bytes of a row (one dword store where the
//                                    output's pointer and pitches allow, byte stores otherwise and at a row's end).  One behind
//                                    the other through a uint8 workspace they are the two-launch route; the pass of an axis that
//                                    does not change is skipped (the other one then writes the output itself; neither changes:
//                                    the horizontal kernel's unfiltered path copies / quantises).
// rs_fused_kernel                    both passes in one launch: a workgroup owns an output tile of RS_TILE_H x RS_TILE_W, stages
//                                    the input rows x columns its taps reach into LDS (dword loads where the source's pointer
//                                    and pitches allow, the bytes of a row's ragged end one by one), runs the horizontal pass
//                                    for its columns into LDS as rounded uint8 and the vertical pass from there: the
//                                    intermediate picture never goes to memory.  It takes the shapes where both axes change
//                                    (a single pass has no intermediate to keep on chip) and whose reach fits
//                                    (rs_fused_plan: at most RS_MAX_STAGE_ROWS rows, RS_LDS_BYTES of LDS); the two-launch route
//                                    takes the rest (strong down-scaling).  Same bytes either way.
// Every kernel walks its work items in a loop: the grid is one-dimensional and never above RS_MAX_BLOCKS.
// LDS traffic is bytes inside dwords: the staged rows and the intermediate are written a dword per lane (consecutive lanes,
// consecutive banks); the horizontal taps read single bytes, neighbouring lanes mostly the same or the next dword (a broadcast
// or a conflict-free read), the vertical taps read one dword for four outputs.  A tile's coefficients sit in LDS with their row
// stride ksize, which is odd (2 ceil(support) + 1): lanes on consecutive outputs never share a bank.
#include <atomic>

#include "common.h"
#include "frame_resample.h"

namespace {

struct RsArgs {
  const void* src; uint8_t* dst;
  const int2* bx; const int* cx; const int2* by; const int* cy;
  int64_t s_row, s_ch, s_img;         // source pitches in elements (bytes or floats)
  int64_t d_row, d_ch, d_img;         // destination pitches in bytes
  int64_t total;                      // work items of the launch
  int C, H, W, oh, ow, kx, ky;        // H x W: the pass's input; oh x ow: its output
  int tiles_x, tiles_y, cap_rows, sp; // fused route: tiles per plane, staged rows and their pitch in bytes
  int src_dword, dst_dword;           // the source / destination may be read / written as aligned dwords
};

__device__ static inline unsigned rs_clip8(int acc) {
  const int v = acc >> RS_PRECISION_BITS;
  return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
template <bool F32>
__device__ static inline unsigned rs_load(const void* __restrict__ src, int64_t i) {
  if (F32) return cips3d_quant_u8(static_cast<const float*>(src)[i]);
  return static_cast<const uint8_t*>(src)[i];
}
// four packed bytes to p, of which the first `valid` belong to the row
__device__ static inline void rs_store4(uint8_t* __restrict__ p, unsigned pk, int valid, int dword) {
  if (dword && valid >= 4) {
    *reinterpret_cast<unsigned*>(p) = pk;
  } else {
    for (int j = 0; j < 4 && j < valid; ++j) p[j] = (uint8_t)(pk >> (8 * j));
  }
}

// work item = (plane, row y of H, quad of the ow output columns)
template <bool F32>
__global__ void __launch_bounds__(RS_THREADS) rs_horiz_kernel(RsArgs a) {
  const int quads = (a.ow + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < a.total; it += stride) {
    const int xq = (int)(it % quads);
    const int64_t t = it / quads;
    const int y = (int)(t % a.H), plane = (int)(t / a.H);
    const int img = plane / a.C, ch = plane % a.C;
    const int64_t srow = img * a.s_img + ch * a.s_ch + y * a.s_row;
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = xq * 4 + j;
      if (x >= a.ow) break;
      unsigned v;
      if (a.kx == 0) {
        v = rs_load<F32>(a.src, srow + x);
      } else {
        const int2 b = a.bx[x];
        const int* __restrict__ c = a.cx + (int64_t)x * a.kx;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int k = 0; k < b.y; ++k) acc += (int)rs_load<F32>(a.src, srow + b.x + k) * c[k];
        v = rs_clip8(acc);
      }
      pk |= v << (8 * j);
    }
    rs_store4(a.dst + img * a.d_img + ch * a.d_ch + y * a.d_row + xq * 4, pk, a.ow - xq * 4, a.dst_dword);
  }
}

// work item = (plane, output row y of oh, quad of the W = ow columns)
template <bool F32>
__global__ void __launch_bounds__(RS_THREADS) rs_vert_kernel(RsArgs a) {
  const int quads = (a.ow + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < a.total; it += stride) {
    const int xq = (int)(it % quads);
    const int64_t t = it / quads;
    const int y = (int)(t % a.oh), plane = (int)(t / a.oh);
    const int img = plane / a.C, ch = plane % a.C;
    const int valid = min(4, a.ow - xq * 4);
    const int2 b = a.by[y];
    const int* __restrict__ c = a.cy + (int64_t)y * a.ky;
    const int64_t s0 = img * a.s_img + ch * a.s_ch + xq * 4;
    int acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
    for (int k = 0; k < b.y; ++k) {
      const int64_t i = s0 + (int64_t)(b.x + k) * a.s_row;
      unsigned w = 0;
      if (!F32 && a.src_dword && valid == 4) {
        w = *reinterpret_cast<const unsigned*>(static_cast<const uint8_t*>(a.src) + i);
      } else {
        for (int j = 0; j < valid; ++j) w |= rs_load<F32>(a.src, i + j) << (8 * j);
      }
      const int ck = c[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += (int)((w >> (8 * j)) & 0xffu) * ck;
    }
    unsigned pk = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk |= rs_clip8(acc[j]) << (8 * j);
    rs_store4(a.dst + img * a.d_img + ch * a.d_ch + y * a.d_row + xq * 4, pk, valid, a.dst_dword);
  }
}

// LDS of the fused route: staged input rows | intermediate rows | the tile's x and y coefficients | its x and y windows
struct RsLds { int mid, cx, cy, bx, by, total; };
__host__ __device__ static inline RsLds rs_lds_layout(int cap_rows, int sp, int kx, int ky) {
  RsLds l;
  int o = (cap_rows * sp + 15) & ~15;
  l.mid = o; o += cap_rows * RS_TILE_W;
  l.cx = o;  o += RS_TILE_W * kx * 4;
  l.cy = o;  o += RS_TILE_H * ky * 4;
  l.bx = o;  o += RS_TILE_W * 8;
  l.by = o;  o += RS_TILE_H * 8;
  l.total = o;
  return l;
}

// work item = (plane, tile row, tile column)
template <bool F32>
__global__ void __launch_bounds__(RS_THREADS) rs_fused_kernel(RsArgs a) {
  extern __shared__ __align__(16) unsigned char rs_lds[];
  const RsLds L = rs_lds_layout(a.cap_rows, a.sp, a.kx, a.ky);
  unsigned* const s_stage_w = reinterpret_cast<unsigned*>(rs_lds);
  const uint8_t* const s_stage = rs_lds;
  unsigned* const s_mid_w = reinterpret_cast<unsigned*>(rs_lds + L.mid);
  int* const s_cx = reinterpret_cast<int*>(rs_lds + L.cx);
  int* const s_cy = reinterpret_cast<int*>(rs_lds + L.cy);
  int2* const s_bx = reinterpret_cast<int2*>(rs_lds + L.bx);
  int2* const s_by = reinterpret_cast<int2*>(rs_lds + L.by);
  const int tid = threadIdx.x;
  const int tiles = a.tiles_x * a.tiles_y;
  const int spw = a.sp >> 2;
  for (int64_t work = blockIdx.x; work < a.total; work += gridDim.x) {
    const int plane = (int)(work / tiles), t = (int)(work % tiles);
    const int img = plane / a.C, ch = plane % a.C;
    const int y0 = (t / a.tiles_x) * RS_TILE_H, x0 = (t % a.tiles_x) * RS_TILE_W;
    const int th = min(RS_TILE_H, a.oh - y0), tw = min(RS_TILE_W, a.ow - x0);
    for (int i = tid; i < tw * a.kx; i += RS_THREADS) s_cx[i] = a.cx[(int64_t)x0 * a.kx + i];
    for (int i = tid; i < th * a.ky; i += RS_THREADS) s_cy[i] = a.cy[(int64_t)y0 * a.ky + i];
    if (tid < tw) s_bx[tid] = a.bx[x0 + tid];
    if (tid < th) s_by[tid] = a.by[y0 + tid];
    // the input window of the tile: the windows' ends grow with the output index, so the first and the last output bound it
    const int2 yf = a.by[y0], yl = a.by[y0 + th - 1], xf = a.bx[x0], xl = a.bx[x0 + tw - 1];
    const int r0 = yf.x, nr = min(yl.x + yl.y - r0, a.cap_rows);
    const int c1 = xl.x + xl.y;                                   // <= W
    const int c0a = a.src_dword ? (xf.x & ~3) : xf.x;
    const int nc = min(c1 - c0a, a.sp), nwords = (nc + 3) >> 2;
    const int nwf = a.src_dword ? min(nwords, (a.W - c0a) >> 2) : 0;      // dwords that lie inside the row
    const int64_t sbase = img * a.s_img + ch * a.s_ch + (int64_t)r0 * a.s_row + c0a;
    for (int it = tid; it < nr * nwords; it += RS_THREADS) {
      const int r = it / nwords, w = it % nwords;
      const int64_t i = sbase + r * a.s_row + 4 * w;
      unsigned word = 0;
      if (!F32 && w < nwf) {
        word = *reinterpret_cast<const unsigned*>(static_cast<const uint8_t*>(a.src) + i);
      } else {
        for (int j = 0; j < 4; ++j)
          if (c0a + 4 * w + j < c1) word |= rs_load<F32>(a.src, i + j) << (8 * j);
      }
      s_stage_w[r * spw + w] = word;
    }
    __syncthreads();
    for (int it = tid; it < nr * RS_QUADS; it += RS_THREADS) {
      const int r = it / RS_QUADS, xq = it % RS_QUADS;
      unsigned pk = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = xq * 4 + j;
        if (x >= tw) break;
        const int2 b = s_bx[x];
        const uint8_t* __restrict__ p = s_stage + r * a.sp + (b.x - c0a);
        const int* __restrict__ c = s_cx + x * a.kx;
        int acc = 1 << (RS_PRECISION_BITS - 1);
        for (int k = 0; k < b.y; ++k) acc += (int)p[k] * c[k];
        pk |= rs_clip8(acc) << (8 * j);
      }
      s_mid_w[r * RS_QUADS + xq] = pk;
    }
    __syncthreads();
    for (int it = tid; it < th * RS_QUADS; it += RS_THREADS) {
      const int y = it / RS_QUADS, xq = it % RS_QUADS;
      if (xq * 4 >= tw) continue;
      const int2 b = s_by[y];
      const int off = b.x - r0;
      const int* __restrict__ c = s_cy + y * a.ky;
      int acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
      for (int k = 0; k < b.y; ++k) {
        const unsigned w = s_mid_w[(off + k) * RS_QUADS + xq];
        const int ck = c[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += (int)((w >> (8 * j)) & 0xffu) * ck;
      }
      unsigned pk = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) pk |= rs_clip8(acc[j]) << (8 * j);
      rs_store4(a.dst + img * a.d_img + ch * a.d_ch + (int64_t)(y0 + y) * a.d_row + x0 + xq * 4, pk, tw - xq * 4, a.dst_dword);
    }
    __syncthreads();              // the next tile overwrites the tables and the staged rows
  }
}

// Rows (columns) of the input that T consecutive outputs reach, at the most: the windows' ends are int(center -+ support + 0.5)
// with centers (T - 1) I / O apart and support <= (ksize - 1) / 2, so the span is at most ceil((T - 1) I / O) + ksize - 1; one
// more for the rounding of the centers.
static int rs_reach(int I, int O, int T, int ksize) {
  const int64_t t = T < O ? T : O;
  const int64_t r = ((t - 1) * I + O - 1) / O + ksize;
  return (int)(r < I ? r : I);
}

struct RsFusedPlan { int ok, cap_rows, sp, lds; };
static RsFusedPlan rs_fused_plan(int H, int W, int oh, int ow, int kx, int ky) {
  RsFusedPlan p = {0, 0, 0, 0};
  if (kx <= 0 || ky <= 0) return p;
  p.cap_rows = rs_reach(H, oh, RS_TILE_H, ky);
  if (p.cap_rows > RS_MAX_STAGE_ROWS) return p;
  p.sp = (rs_reach(W, ow, RS_TILE_W, kx) + 3 + 3) & ~3;        // + 3: the window's start moves down to a dword boundary
  const int64_t words = (int64_t)RS_TILE_W * kx + (int64_t)RS_TILE_H * ky;
  if (words * 4 > RS_LDS_BYTES || (int64_t)p.cap_rows * (p.sp + RS_TILE_W) > RS_LDS_BYTES) return p;
  p.lds = rs_lds_layout(p.cap_rows, p.sp, kx, ky).total;
  p.ok = p.lds <= RS_LDS_BYTES;
  return p;
}

static unsigned rs_blocks(int64_t items) {
  const int64_t b = ceil_div<int64_t>(items, RS_THREADS);
  return (unsigned)(b < RS_MAX_BLOCKS ? b : RS_MAX_BLOCKS);
}

static bool rs_aligned4(const void* p, int64_t a, int64_t b, int64_t c) {
  return ((reinterpret_cast<uintptr_t>(p) | (uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 3) == 0;
}

template <bool F32>
static int rs_launch_fused(const RsArgs& a, int lds, hipStream_t st) {
  // the attribute is per device and the flag is shared by host threads
  static std::atomic<unsigned long long> attr_set{0};
  int dev_id = 0;
  if (hipError_t e = hipGetDevice(&dev_id); e != hipSuccess) return (int)e;
  const unsigned long long bit = 1ull << (dev_id & 63);
  if (dev_id >= 64 || !(attr_set.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&rs_fused_kernel<F32>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, RS_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    attr_set.fetch_or(bit, std::memory_order_release);
  }
  const unsigned blocks = (unsigned)(a.total < RS_MAX_BLOCKS ? a.total : RS_MAX_BLOCKS);
  hipLaunchKernelGGL(rs_fused_kernel<F32>, dim3(blocks), dim3(RS_THREADS), (size_t)lds, st, a);
  return cips3d_launch_status();
}

}  // namespace

extern "C" int cips3d_resample_tile(int* tile_h, int* tile_w, int* max_stage_rows) {
  if (tile_h) *tile_h = RS_TILE_H;
  if (tile_w) *tile_w = RS_TILE_W;
  if (max_stage_rows) *max_stage_rows = RS_MAX_STAGE_ROWS;
  return RS_THREADS;
}

extern "C" int cips3d_resample_route(int H, int W, int oh, int ow, int ksize_x, int ksize_y) {
  if (H < 1 || W < 1 || oh < 1 || ow < 1 || ksize_x < 0 || ksize_y < 0) return CIPS3D_E_BADARG;
  if ((ksize_x == 0) != (W == ow) || (ksize_y == 0) != (H == oh)) return CIPS3D_E_BADARG;
  return rs_fused_plan(H, W, oh, ow, ksize_x, ksize_y).ok ? CIPS3D_RESAMPLE_FUSED : CIPS3D_RESAMPLE_TWO_LAUNCH;
}

// the route a call takes: the shape's own (cips3d_resample_route), or a forced one where both axes are filtered
static int rs_resolve_route(int H, int W, int oh, int ow, int kx, int ky, int route) {
  const int r = cips3d_resample_route(H, W, oh, ow, kx, ky);
  if (r < 0 || route == CIPS3D_RESAMPLE_AUTO || route == r) return r;
  if (route == CIPS3D_RESAMPLE_TWO_LAUNCH && r == CIPS3D_RESAMPLE_FUSED) return route;
  return route == CIPS3D_RESAMPLE_FUSED ? CIPS3D_E_UNSUPP : CIPS3D_E_BADARG;
}

extern "C" int64_t cips3d_resample_workspace_bytes(int n, int C, int H, int W, int oh, int ow, int ksize_x, int ksize_y,
                                                   int route) {
  if (n < 0 || C < 0) return CIPS3D_E_BADARG;
  const int r = rs_resolve_route(H, W, oh, ow, ksize_x, ksize_y, route);
  if (r < 0) return r;
  if (r != CIPS3D_RESAMPLE_TWO_LAUNCH || !ksize_x || !ksize_y) return 0;       // a skipped pass: no intermediate
  return (int64_t)n * C * H * ((ow + 3) & ~3);
}

extern "C" int cips3d_resample_u8(const void* src, int n, int C, int H, int W, int64_t src_row_pitch, int64_t src_channel_pitch,
                                  int64_t src_image_pitch, uint8_t* dst, int oh, int ow, int64_t dst_row_pitch,
                                  int64_t dst_channel_pitch, int64_t dst_image_pitch, const int32_t* bounds_x,
                                  const int32_t* coeffs_x, int ksize_x, const int32_t* bounds_y, const int32_t* coeffs_y,
                                  int ksize_y, int src_is_f32, void* workspace, int64_t workspace_bytes, int route,
                                  void* stream) {
  if (n < 0 || C < 0) return CIPS3D_E_BADARG;
  const int r = rs_resolve_route(H, W, oh, ow, ksize_x, ksize_y, route);
  if (r < 0) return r;
  if ((int64_t)n * C == 0) return 0;
  if (!src || !dst || (ksize_x && (!bounds_x || !coeffs_x)) || (ksize_y && (!bounds_y || !coeffs_y))) return CIPS3D_E_BADARG;
  if (src_row_pitch < W || dst_row_pitch < ow || src_channel_pitch < 0 || src_image_pitch < 0 || dst_channel_pitch < 0 ||
      dst_image_pitch < 0)
    return CIPS3D_E_BADARG;
  if ((int64_t)n * C > INT32_MAX) return CIPS3D_E_UNSUPP;
  if (src_is_f32 && (reinterpret_cast<uintptr_t>(src) & 3)) return CIPS3D_E_UNSUPP;
  const hipStream_t st = as_stream(stream);
  const int64_t planes = (int64_t)n * C;
  RsArgs a = {};
  a.src = src; a.dst = dst;
  a.bx = reinterpret_cast<const int2*>(bounds_x); a.cx = coeffs_x;
  a.by = reinterpret_cast<const int2*>(bounds_y); a.cy = coeffs_y;
  a.s_row = src_row_pitch; a.s_ch = src_channel_pitch; a.s_img = src_image_pitch;
  a.d_row = dst_row_pitch; a.d_ch = dst_channel_pitch; a.d_img = dst_image_pitch;
  a.C = C; a.H = H; a.W = W; a.oh = oh; a.ow = ow; a.kx = ksize_x; a.ky = ksize_y;
  a.src_dword = !src_is_f32 && rs_aligned4(src, src_row_pitch, src_channel_pitch, src_image_pitch);
  a.dst_dword = rs_aligned4(dst, dst_row_pitch, dst_channel_pitch, dst_image_pitch);
  const int64_t quads = (ow + 3) >> 2;
  if (r == CIPS3D_RESAMPLE_TWO_LAUNCH && !ksize_y) {       // the vertical pass is skipped (neither axis changes: the unfiltered copy)
    a.total = planes * H * quads;
    if (src_is_f32) hipLaunchKernelGGL(rs_horiz_kernel<true>, dim3(rs_blocks(a.total)), dim3(RS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(rs_horiz_kernel<false>, dim3(rs_blocks(a.total)), dim3(RS_THREADS), 0, st, a);
    return cips3d_launch_status();
  }
  if (r == CIPS3D_RESAMPLE_TWO_LAUNCH && !ksize_x) {       // the horizontal pass is skipped
    a.total = planes * oh * quads;
    if (src_is_f32) hipLaunchKernelGGL(rs_vert_kernel<true>, dim3(rs_blocks(a.total)), dim3(RS_THREADS), 0, st, a);
    else hipLaunchKernelGGL(rs_vert_kernel<false>, dim3(rs_blocks(a.total)), dim3(RS_THREADS), 0, st, a);
    return cips3d_launch_status();
  }
  if (r == CIPS3D_RESAMPLE_FUSED) {
    const RsFusedPlan p = rs_fused_plan(H, W, oh, ow, ksize_x, ksize_y);
    a.tiles_x = ceil_div(ow, RS_TILE_W); a.tiles_y = ceil_div(oh, RS_TILE_H);
    a.cap_rows = p.cap_rows; a.sp = p.sp;
    a.total = planes * a.tiles_x * a.tiles_y;
    return src_is_f32 ? rs_launch_fused<true>(a, p.lds, st) : rs_launch_fused<false>(a, p.lds, st);
  }
  // two launches: horizontal into the workspace (rows padded to dwords), vertical from there
  const int64_t wp = (ow + 3) & ~3;
  if (!workspace || workspace_bytes < planes * H * wp) return CIPS3D_E_BADARG;
  if (reinterpret_cast<uintptr_t>(workspace) & 3) return CIPS3D_E_UNSUPP;
  RsArgs h = a;
  h.dst = static_cast<uint8_t*>(workspace);
  h.d_row = wp; h.d_ch = (int64_t)H * wp; h.d_img = (int64_t)C * H * wp; h.dst_dword = 1;
  h.total = planes * H * quads;
  if (src_is_f32) hipLaunchKernelGGL(rs_horiz_kernel<true>, dim3(rs_blocks(h.total)), dim3(RS_THREADS), 0, st, h);
  else hipLaunchKernelGGL(rs_horiz_kernel<false>, dim3(rs_blocks(h.total)), dim3(RS_THREADS), 0, st, h);
  if (int e = cips3d_launch_status()) return e;
  RsArgs v = a;
  v.src = workspace; v.W = ow;
  v.s_row = h.d_row; v.s_ch = h.d_ch; v.s_img = h.d_img; v.src_dword = 1;
  v.total = planes * oh * quads;
  hipLaunchKernelGGL(rs_vert_kernel<false>, dim3(rs_blocks(v.total)), dim3(RS_THREADS), 0, st, v);
  return cips3d_launch_status();
}
