// Two terms of the flip-inversion step loss (reference: /root/reference/exp/cips3d/models/projector_v10.py) as HIP kernels.
//
// 1. The noise regulariser (:1183-1195, StyleGAN2's multi-scale autocorrelation penalty).  For every noise buffer v [B,1,S,S] and
//    every level n_0 = v, n_{l+1} = avg_pool2d(n_l, 2) down to and including the first level with side <= 8:
//        reg += mean(n_l * roll(n_l, 1, dim 3))^2 + mean(n_l * roll(n_l, 1, dim 2))^2        (circular rolls)
//    The torch expression is ~10 launches per level forward and as many again in autograd's backward.  Here the whole LIST of
//    buffers is (per 32 buffers) at most four launches forward and one backward, whatever the number of buffers and levels:
//      nr_pyramid_kernel   levels 1 .. 6 of every buffer from 64 x 64 tiles of level 0 (run a second time on level 6 for the
//                          buffers with more than seven levels: sides above 512)
//      nr_partial_kernel   per-workgroup partial sums of the two products of every level (4096 elements per workgroup)
//      nr_finish_kernel    the partials of each level in a fixed order -> the 2 x levels means (kept for the backward) and
//                          weight * sum mean^2 on the device
//      nr_bwd_kernel       d/dv = gloss * weight * sum_l 4^-l nearest_upsample(g_l),
//                          g_l = 2 m_w / count_l (left + right neighbour) + 2 m_h / count_l (upper + lower neighbour)
//    No float atomics: every sum runs in a fixed order, so value and gradient are bit-reproducible.  Circular neighbours are
//    read from global memory (the buffer or its pyramid), never from a tile.
//
// 2. The mask blending (:1164-1167, mask of :268-273): synth * m + synth.detach() * (1 - m) with m = the bicubic up-sampling
//    (torch's: align_corners = False, A = -0.75, border-clamped taps, no clamping of the result) of 1 - mask from the
//    thumbnail's resolution.  One kernel forward, one backward (g * m); each evaluates m from the [B,1,h,w] mask on the fly, so
//    the full-resolution mask is never written.
#include "common.h"

namespace {

constexpr int NR_MAX = 32;            // buffers per launch (kernel-argument budget: 32 x 48 B + prefix sums)
constexpr int NR_MAX_LEVELS = 13;     // level 0 + two pyramid passes of six pooling steps
constexpr int NR_STEPS = 6;           // pooling steps of one pyramid pass: a 64 x 64 source tile down to one value
constexpr int NR_TILE = 1 << NR_STEPS;
constexpr int NR_CHUNK = 4096;        // elements per workgroup of the partial pass (256 threads x 16)
constexpr int NR_FINISH_WAVES = 16;

struct NrBuf {
  const float* v;
  float* d;
  int B, S, L;
  int part;             // index of this buffer's first partial pair
  int64_t pyr;          // float offset of its level 1 in the workspace
  int mean;             // index of its level 0 in the means table
  int pad_;
};
struct NrArgs {
  NrBuf b[NR_MAX];
  int blk_begin[NR_MAX + 1];          // exclusive prefix sums of the workgroups per buffer, for the launch at hand
  int n;
};

__host__ __device__ static inline int nr_levels(int S) {
  int L = 1;
  while (S > 8) { S >>= 1; ++L; }
  return L;
}
// float offset of level l >= 1 from the start of the buffer's pyramid
__host__ __device__ static inline int64_t nr_level_off(int B, int S, int l) {
  int64_t o = 0;
  for (int j = 1; j < l; ++j) { const int64_t s = S >> j; o += (int64_t)B * s * s; }
  return o;
}
__host__ __device__ static inline int nr_level_blocks(int B, int s) { return (int)(((int64_t)B * s * s + NR_CHUNK - 1) / NR_CHUNK); }

__device__ static inline int nr_owner(const NrArgs& a) {
  int ei = 0;
  while (ei + 1 < a.n && (int)blockIdx.x >= a.blk_begin[ei + 1]) ++ei;          // (uniform: <= 32 scalar compares)
  return ei;
}
__device__ static inline const float* nr_level_ptr(const NrBuf& E, const float* ws, int l) {
  return l == 0 ? E.v : ws + E.pyr + nr_level_off(E.B, E.S, l);
}

// levels src_level + 1 .. src_level + 6 (as far as the buffer has them) from one 64 x 64 tile of level src_level
__global__ void __launch_bounds__(256) nr_pyramid_kernel(NrArgs a, float* __restrict__ ws, int src_level) {
  __shared__ float lds[1024 + 256 + 64 + 16 + 4 + 1];
  const int ei = nr_owner(a);
  const NrBuf E = a.b[ei];
  const int local = (int)blockIdx.x - a.blk_begin[ei];
  const int Ss = E.S >> src_level;
  const int tiles = ceil_div(Ss, NR_TILE);
  const int b = local / (tiles * tiles), t = local % (tiles * tiles), ty = t / tiles, tx = t % tiles;
  const int steps = min(NR_STEPS, E.L - 1 - src_level);
  const float* src = nr_level_ptr(E, ws, src_level) + (int64_t)b * Ss * Ss;
  {
    const int So = Ss >> 1;
    float* dst = ws + E.pyr + nr_level_off(E.B, E.S, src_level + 1) + (int64_t)b * So * So;
    for (int idx = threadIdx.x; idx < 1024; idx += 256) {
      const int oy = idx >> 5, ox = idx & 31, gy = ty * 32 + oy, gx = tx * 32 + ox;
      if (gy < So && gx < So) {
        const float* p = src + (int64_t)(2 * gy) * Ss + 2 * gx;
        const float val = ((p[0] + p[1]) + (p[Ss] + p[Ss + 1])) * 0.25f;
        lds[idx] = val;
        dst[(int64_t)gy * So + gx] = val;
      }
    }
  }
  int prev_off = 0;
  for (int j = 1; j < steps; ++j) {           // (block-uniform trip count)
    __syncthreads();
    const int sp = NR_TILE >> j, so = sp >> 1, Sj = Ss >> (j + 1);
    const int out_off = prev_off + sp * sp;
    float* dst = ws + E.pyr + nr_level_off(E.B, E.S, src_level + j + 1) + (int64_t)b * Sj * Sj;
    for (int idx = threadIdx.x; idx < so * so; idx += 256) {
      const int oy = idx / so, ox = idx % so, gy = ty * so + oy, gx = tx * so + ox;
      if (gy < Sj && gx < Sj) {               // (valid output => its four sources were valid outputs of the previous step)
        const float* p = lds + prev_off + (2 * oy) * sp + 2 * ox;
        const float val = ((p[0] + p[1]) + (p[sp] + p[sp + 1])) * 0.25f;
        lds[out_off + idx] = val;
        dst[(int64_t)gy * Sj + gx] = val;
      }
    }
    prev_off = out_off;
  }
}

// the level of buffer E that owns the buffer-local workgroup `local` of the partial pass: -> level, side; local -> level-local
__device__ static inline int nr_level_of_block(const NrBuf& E, int& local, int& s) {
  int l = 0;
  s = E.S;
  while (l + 1 < E.L) {
    const int nb = nr_level_blocks(E.B, s);
    if (local < nb) break;
    local -= nb; ++l; s >>= 1;
  }
  return l;
}

__global__ void __launch_bounds__(256) nr_partial_kernel(NrArgs a, const float* __restrict__ ws, float* __restrict__ partial) {
  __shared__ float red[2][4];
  const int ei = nr_owner(a);
  const NrBuf E = a.b[ei];
  const int in_buf = (int)blockIdx.x - a.blk_begin[ei];
  int local = in_buf, s;
  const int l = nr_level_of_block(E, local, s);
  const float* src = nr_level_ptr(E, ws, l);
  const int64_t cnt = (int64_t)E.B * s * s, base = (int64_t)local * NR_CHUNK;
  float sw = 0.f, sh = 0.f;
#pragma unroll 4
  for (int it = 0; it < NR_CHUNK / 256; ++it) {
    const int64_t i = base + it * 256 + threadIdx.x;
    if (i < cnt) {
      const int x = (int)(i % s), y = (int)((i / s) % s);
      const float v = src[i];
      sw = fmaf(v, src[x == 0 ? i + (s - 1) : i - 1], sw);                          // roll(n, 1, dim 3)[x] = n[x - 1]
      sh = fmaf(v, src[y == 0 ? i + (int64_t)(s - 1) * s : i - s], sh);             // roll(n, 1, dim 2)[y] = n[y - 1]
    }
  }
  sw = wave_sum(sw); sh = wave_sum(sh);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[0][w] = sw; red[1][w] = sh; }
  __syncthreads();
  if (threadIdx.x < 2)
    partial[(int64_t)(E.part + in_buf) * 2 + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// one workgroup of 16 waves; wave w takes the levels w, w + 16, ... of the launch's buffers (flat numbering), sums each level's
// partials in a fixed order (lane i takes partials i, i + 64, ...; then the wave butterfly) and keeps the two means
__global__ void __launch_bounds__(64 * NR_FINISH_WAVES) nr_finish_kernel(NrArgs a, const float* __restrict__ partial,
                                                                         float* __restrict__ means, float weight,
                                                                         float* __restrict__ loss, int accumulate) {
  __shared__ float red[NR_FINISH_WAVES];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int total = 0;
  for (int i = 0; i < a.n; ++i) total += a.b[i].L;
  float acc = 0.f;
  for (int f = w; f < total; f += NR_FINISH_WAVES) {
    int ei = 0, l = f;
    while (l >= a.b[ei].L) { l -= a.b[ei].L; ++ei; }
    const NrBuf E = a.b[ei];
    int p0 = E.part, s = E.S;
    for (int j = 0; j < l; ++j) { p0 += nr_level_blocks(E.B, s); s >>= 1; }
    const int nb = nr_level_blocks(E.B, s);
    float sw = 0.f, sh = 0.f;
    for (int i = lane; i < nb; i += 64) { sw += partial[(int64_t)(p0 + i) * 2]; sh += partial[(int64_t)(p0 + i) * 2 + 1]; }
    sw = wave_sum(sw); sh = wave_sum(sh);
    const double cnt = (double)E.B * s * s;
    const float mw = (float)((double)sw / cnt), mh = (float)((double)sh / cnt);
    if (lane == 0) { means[(E.mean + l) * 2] = mw; means[(E.mean + l) * 2 + 1] = mh; }
    acc += mw * mw + mh * mh;
  }
  if (lane == 0) red[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < NR_FINISH_WAVES; ++i) t += red[i];
    loss[0] = accumulate ? loss[0] + weight * t : weight * t;
  }
}

// V = 4: the thread owns four consecutive columns (S % 4 == 0); V = 1: one element
template <int V>
__device__ static inline void nr_bwd_body(const NrBuf& E, int local, const float* __restrict__ ws, const float* __restrict__ means,
                                          float scale) {
  const int S = E.S, per_row = S / V;
  const int64_t unit = (int64_t)local * 256 + threadIdx.x, units = (int64_t)E.B * S * per_row;
  if (unit >= units) return;
  const int x0 = (int)(unit % per_row) * V, y0 = (int)((unit / per_row) % S), b = (int)(unit / ((int64_t)per_row * S));
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  float inv4 = 1.f;
  int s = S;
  for (int l = 0; l < E.L; ++l) {
    const float* n = nr_level_ptr(E, ws, l) + (int64_t)b * s * s;
    const float k = scale * 2.f * inv4 / (float)((int64_t)E.B * s * s);
    const float cw = k * means[(E.mean + l) * 2], ch = k * means[(E.mean + l) * 2 + 1];
    const int p = y0 >> l, pu = p == 0 ? s - 1 : p - 1, pd = p == s - 1 ? 0 : p + 1;
    float g = 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const int q = (x0 + e) >> l;
      if (e == 0 || q != ((x0 + e - 1) >> l)) {
        const int ql = q == 0 ? s - 1 : q - 1, qr = q == s - 1 ? 0 : q + 1;
        const float* row = n + (int64_t)p * s;
        g = cw * (row[ql] + row[qr]) + ch * (n[(int64_t)pu * s + q] + n[(int64_t)pd * s + q]);
      }
      acc[e] += g;
    }
    inv4 *= 0.25f;
    s >>= 1;
  }
  float* d = E.d + ((int64_t)b * S + y0) * S + x0;
  if (V == 4 && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
    *reinterpret_cast<float4*>(d) = make_float4(acc[0], acc[V > 1 ? 1 : 0], acc[V > 2 ? 2 : 0], acc[V > 3 ? 3 : 0]);
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = acc[e];
  }
}

__global__ void __launch_bounds__(256) nr_bwd_kernel(NrArgs a, const float* __restrict__ ws, const float* __restrict__ means,
                                                     float weight, const float* __restrict__ gloss) {
  const int ei = nr_owner(a);
  const NrBuf E = a.b[ei];
  const int local = (int)blockIdx.x - a.blk_begin[ei];
  const float scale = weight * gloss[0];
  if (E.S % 4 == 0) nr_bwd_body<4>(E, local, ws, means, scale);
  else nr_bwd_body<1>(E, local, ws, means, scale);
}

struct NrLayout { int64_t pyr_floats; int64_t part_pairs; int64_t levels; };

static bool nr_supported(int B, int S) {
  if (B < 1 || S < 1) return false;
  for (int s = S; s > 8; s >>= 1)
    if (s & 1) return false;
  if (nr_levels(S) > NR_MAX_LEVELS) return false;
  return (int64_t)B * S * S < ((int64_t)1 << 40);
}

// fills the workspace offsets of bufs[0 .. K) into out (when given); false: an unsupported buffer or a workspace beyond int range
static bool nr_layout(const cips3d_noise_buf* bufs, int K, NrBuf* out, NrLayout* lay) {
  int64_t pyr = 0, part = 0, lev = 0;
  for (int i = 0; i < K; ++i) {
    const int B = bufs[i].B, S = bufs[i].S;
    if (!nr_supported(B, S)) return false;
    const int L = nr_levels(S);
    if (out) out[i] = NrBuf{bufs[i].v, bufs[i].d, B, S, L, (int)part, pyr, (int)lev, 0};
    pyr += nr_level_off(B, S, L);
    for (int l = 0; l < L; ++l) part += nr_level_blocks(B, S >> l);
    lev += L;
    if (part > 0x3fffffff || lev > 0x3fffffff) return false;
  }
  *lay = NrLayout{pyr, part, lev};
  return true;
}

// ------------------------------------------------------------------------------------------------------------ mask blending
// torch's bicubic coefficients (aten/native/UpSample.h, A = -0.75) for the fractional offset t
__device__ static inline void bicubic_coeffs(float t, float (&c)[4]) {
  const float A = -0.75f;
  const float x0 = t + 1.f, x3 = (1.f - t) + 1.f, x2 = 1.f - t;
  c[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  c[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  c[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  c[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}
// destination index d -> first tap index and coefficients; source coordinate inv_f * (d + 0.5) - 0.5
__device__ static inline int bicubic_taps(int d, float inv_f, float (&c)[4]) {
  const float src = inv_f * ((float)d + 0.5f) - 0.5f;
  const float fl = floorf(src);
  bicubic_coeffs(src - fl, c);
  return (int)fl - 1;
}
__device__ static inline int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// BWD = false: out = x m + x (1 - m);  BWD = true: out = x m (x = the incoming gradient).  A thread takes up to four
// consecutive pixels of one row, for all C channels.
template <bool BWD>
__global__ void __launch_bounds__(256) mask_blend_kernel(const float* __restrict__ x, const float* __restrict__ mask,
                                                         float* __restrict__ out, int B, int C, int H, int W, int Hm, int Wm,
                                                         float inv_f) {
  const int per_row = ceil_div(W, 4);
  const int64_t unit = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (unit >= (int64_t)B * H * per_row) return;
  const int x0 = (int)(unit % per_row) * 4, y = (int)((unit / per_row) % H), b = (int)(unit / ((int64_t)per_row * H));
  const float* mb = mask + (int64_t)b * Hm * Wm;
  float cy[4], m[4];
  const int iy = bicubic_taps(y, inv_f, cy);
  const int nx = min(4, W - x0);
  for (int e = 0; e < nx; ++e) {
    float cx[4], r[4];
    const int ix = bicubic_taps(x0 + e, inv_f, cx);
    int col[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) col[j] = clampi(ix + j, Wm - 1);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float* row = mb + (int64_t)clampi(iy + i, Hm - 1) * Wm;
      r[i] = (1.f - row[col[0]]) * cx[0] + (1.f - row[col[1]]) * cx[1] + (1.f - row[col[2]]) * cx[2] + (1.f - row[col[3]]) * cx[3];
    }
    m[e] = r[0] * cy[0] + r[1] * cy[1] + r[2] * cy[2] + r[3] * cy[3];
  }
  for (int e = nx; e < 4; ++e) m[e] = 0.f;
  auto f = [](float v, float mm) { return BWD ? v * mm : v * mm + v * (1.f - mm); };
  for (int c = 0; c < C; ++c) {
    const int64_t o = (((int64_t)b * C + c) * H + y) * W + x0;
    if (nx == 4 && ((reinterpret_cast<uintptr_t>(x + o) | reinterpret_cast<uintptr_t>(out + o)) & 15) == 0) {
      const float4 v = *reinterpret_cast<const float4*>(x + o);
      *reinterpret_cast<float4*>(out + o) = make_float4(f(v.x, m[0]), f(v.y, m[1]), f(v.z, m[2]), f(v.w, m[3]));
    } else {
      for (int e = 0; e < nx; ++e) out[o + e] = f(x[o + e], m[e]);
    }
  }
}

template <bool BWD>
static int mask_blend_launch(const float* x, const float* mask, float* out, int B, int C, int H, int W, int f, void* stream) {
  if (!x || !mask || !out || B < 1 || C < 1 || H < 1 || W < 1 || f < 1 || H % f || W % f) return CIPS3D_E_BADARG;
  const int64_t units = (int64_t)B * H * ceil_div(W, 4), blocks = ceil_div<int64_t>(units, 256);
  if (blocks > 0x7fffffff) return CIPS3D_E_BADARG;
  hipLaunchKernelGGL(mask_blend_kernel<BWD>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), x, mask, out, B, C, H, W,
                     H / f, W / f, (float)(1.0 / (double)f));
  return cips3d_launch_status();
}

}  // namespace

extern "C" int cips3d_noise_reg_supported(int B, int S) { return nr_supported(B, S) ? 1 : 0; }

extern "C" int cips3d_noise_reg_launches(int K, int max_S, int backward) {
  if (K < 1 || max_S < 1) return 0;
  const int chunks = ceil_div(K, NR_MAX);
  if (backward) return chunks;
  const int L = nr_levels(max_S);
  return chunks * (2 + (L > 1 ? 1 : 0) + (L - 1 > NR_STEPS ? 1 : 0));
}

extern "C" int64_t cips3d_noise_reg_workspace(const cips3d_noise_buf* bufs, int K) {
  NrLayout lay;
  if (!bufs || K < 1 || !nr_layout(bufs, K, nullptr, &lay)) return CIPS3D_E_BADARG;
  return 4 * (lay.pyr_floats + 2 * lay.part_pairs + 2 * lay.levels);
}

namespace {
struct NrPlan {
  NrBuf* bufs;
  NrLayout lay;
  float* ws; float* partial; float* means;
};
// kind 0 / 1: pyramid pass from level 0 / NR_STEPS; 2: partial sums; 3: backward
static int nr_blocks_of(const NrBuf& E, int kind) {
  if (kind <= 1) {
    const int src = kind * NR_STEPS;
    if (E.L - 1 <= src) return 0;
    const int t = ceil_div(E.S >> src, NR_TILE);
    return E.B * t * t;
  }
  if (kind == 2) {
    int n = 0;
    for (int l = 0; l < E.L; ++l) n += nr_level_blocks(E.B, E.S >> l);
    return n;
  }
  const int64_t units = (int64_t)E.B * E.S * (E.S % 4 == 0 ? E.S / 4 : E.S);
  return (int)ceil_div<int64_t>(units, 256);
}
static int nr_fill(NrArgs& a, const NrBuf* bufs, int n, int kind) {
  int blocks = 0;
  a.n = 0;
  for (int i = 0; i < n; ++i) {
    const int nb = nr_blocks_of(bufs[i], kind);
    if (nb == 0) continue;
    a.b[a.n] = bufs[i];
    a.blk_begin[a.n++] = blocks;
    blocks += nb;
  }
  a.blk_begin[a.n] = blocks;
  return blocks;
}
}  // namespace

extern "C" int cips3d_noise_reg(const cips3d_noise_buf* bufs, int K, float weight, void* workspace, float* loss, void* stream) {
  if (!bufs || K < 1 || !workspace || !loss) return CIPS3D_E_BADARG;
  for (int i = 0; i < K; ++i)
    if (!bufs[i].v) return CIPS3D_E_BADARG;
  NrBuf* all = new NrBuf[K];
  NrLayout lay;
  if (!nr_layout(bufs, K, all, &lay)) { delete[] all; return CIPS3D_E_BADARG; }
  float* ws = static_cast<float*>(workspace);
  float* partial = ws + lay.pyr_floats;
  float* means = partial + 2 * lay.part_pairs;
  int rc = 0;
  for (int first = 0; first < K && rc == 0; first += NR_MAX) {
    const int n = K - first < NR_MAX ? K - first : NR_MAX;
    NrArgs a;
    for (int kind = 0; kind <= 1; ++kind) {
      const int blocks = nr_fill(a, all + first, n, kind);
      if (blocks > 0) hipLaunchKernelGGL(nr_pyramid_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, ws, kind * NR_STEPS);
    }
    // (the partial pass numbers its partials by E.part + the workgroup's index within the buffer: independent of blk_begin)
    const int blocks = nr_fill(a, all + first, n, 2);
    hipLaunchKernelGGL(nr_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, ws, partial);
    hipLaunchKernelGGL(nr_finish_kernel, dim3(1), dim3(64 * NR_FINISH_WAVES), 0, as_stream(stream), a, partial, means, weight, loss,
                       first > 0 ? 1 : 0);
    rc = cips3d_launch_status();
  }
  delete[] all;
  return rc;
}

extern "C" int cips3d_noise_reg_bwd(const cips3d_noise_buf* bufs, int K, float weight, const void* workspace, const float* gloss,
                                    void* stream) {
  if (!bufs || K < 1 || !workspace || !gloss) return CIPS3D_E_BADARG;
  for (int i = 0; i < K; ++i)
    if (!bufs[i].v || !bufs[i].d) return CIPS3D_E_BADARG;
  NrBuf* all = new NrBuf[K];
  NrLayout lay;
  if (!nr_layout(bufs, K, all, &lay)) { delete[] all; return CIPS3D_E_BADARG; }
  const float* ws = static_cast<const float*>(workspace);
  const float* means = ws + lay.pyr_floats + 2 * lay.part_pairs;
  int rc = 0;
  for (int first = 0; first < K && rc == 0; first += NR_MAX) {
    const int n = K - first < NR_MAX ? K - first : NR_MAX;
    NrArgs a;
    const int blocks = nr_fill(a, all + first, n, 3);
    hipLaunchKernelGGL(nr_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), a, ws, means, weight, gloss);
    rc = cips3d_launch_status();
  }
  delete[] all;
  return rc;
}

extern "C" int cips3d_mask_blend(const float* x, const float* mask, float* out, int B, int C, int H, int W, int f, void* stream) {
  return mask_blend_launch<false>(x, mask, out, B, C, H, W, f, stream);
}

extern "C" int cips3d_mask_blend_bwd(const float* g, const float* mask, float* dx, int B, int C, int H, int W, int f, void* stream) {
  return mask_blend_launch<true>(g, mask, dx, B, C, H, W, f, stream);
}
