// VGG16 conv perceptual loss of flip inversion (reference exp/cips3d/models/vgg_per_loss.py:203-334, used twice per step by
// models/projector_v10.py:131-151, 1170-1174): the 13 dense 3x3 convolutions of torchvision's vgg16.features with frozen,
// batch-shared weights, ReLU, 2x2/2 max-pools, taps at pre-ReLU conv outputs, sum_k w_k^2 sum (f_k - t_k)^2, and the data
// gradient back to the image.  No weight gradient exists.
//
//   vgg_conv3x3_kernel   plain conv, padding 1, as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32: every product is
//                        one fmaf).  The batch is folded into the pixel-tile index: one launch per layer whatever B is, and a
//                        tile's arithmetic does not depend on B (a B = 2 call equals two B = 1 calls bit for bit).
//                        A = packed weights [tap][Cout/16][Cin/16][lane][4] straight from L2, one tap ahead;
//                        B = an LDS halo tile of 16 input channels x (TH + 2) x 18, double buffered, filled with bounds-checked
//                        scalar loads (zero outside the image -- any H, W >= 1 is correct, tiles need not divide them), with the
//                        producer's ReLU applied in the load (relu_in): only PRE-ReLU tensors are ever written, they are the
//                        taps and they are what the backward keeps.
//                        Two workgroup shapes: WP = 4: four waves on four row groups of a 16 x 16 pixel tile, 64 output
//                        channels; WP = 1: four waves on 4 x 64 output channels of a 4 x 16 tile (maps below 16 rows, all of
//                        which have >= 256 channels).  A wave holds 64 channels x 4 rows x 16 columns = 64 accumulator registers;
//                        after every K stage (16 channels x 9 taps = 144 products) the running accumulators are folded into a second
//                        set, so no fmaf chain is longer than 144 however wide the layer is (K = 9 Cin reaches 4608).
//                        The same kernel is the data gradient: weights packed transposed (Cin <-> Cout) and rotated 180 degrees,
//                        no bias, and an epilogue that multiplies by the sign mask of the kept pre-ReLU tensor of the layer
//                        below and adds that layer's tap gradient gloss 2 w^2 (z - t), which is therefore never materialised
//                        (only the deepest tap's is: it starts the chain).
//   vgg_first_*          Cin = 3 forward / Cout = 3 data gradient on the VALU (27-term dot products; 0.2 % of the arithmetic),
//                        with the input normalisation ((x + 1) / 2 - mean) / std and its backward factor 0.5 / std folded in.
//   vgg_pool_*           max-pool of relu(z); its backward routes to the first maximum in scan order as torch does, applies the
//                        ReLU mask and adds the tap gradient.  Ties between maxima only occur at 0 after the ReLU, where the
//                        ReLU mask kills the gradient anyway.
//   vgg_tap_loss_*       per-workgroup fp64 partial sums of (z - t)^2 in a fixed order, then one workgroup adds every tap's
//                        partials in a fixed order: no atomics, same inputs -> same bits.
//
// Roofline: MFMA-bound.  2 * 9 * Cin * Cout flop per output pixel against 4 (Cin + Cout) bytes; at CompCars 256^2 the conv
// stack to features_28 is 40.1 GFLOP per image, the fp32 matrix instruction's peak is 157 TFLOP/s.
#include "vgg_shared.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct VggConvArgs {
  const float* x; const float* wp; const float* bias; float* out;
  const float* mask_z;             // data gradient: the kept pre-ReLU tensor of the layer below (shape of out) or NULL
  const float* tap_t; float tap_c; // ... its tap target and 2 w^2, or NULL
  const float* gloss;              // ... the loss' incoming gradient (device scalar)
  int B, Cin, Cout, H, W, relu_in;
};

template <int WP>
__global__ void __launch_bounds__(256) vgg_conv3x3_kernel(VggConvArgs a) {
  constexpr int WMV = 4 / WP;                  // waves along the output channels
  constexpr int TH = 4 * WP, TC = 18, TR = TH + 2;
  constexpr int CS = ((TR * TC - 16 + 63) / 64) * 64 + 16;   // channel stride, = 16 mod 64: the four lane quarters of a ds_read_b32
                                                             // (four channels, 16 consecutive columns each) hit disjoint banks
  constexpr int STAGE = 16 * CS;
  constexpr int E = 16 * TR * TC;              // elements of one stage
  constexpr int NU = (E + 255) / 256;          // per thread
  constexpr int FOLD = 1;                      // stages between two folds of the running accumulators
  __shared__ float sT[2 * STAGE];

  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int q = lane >> 4, jn = lane & 15;
  const int wp = wave % WP, wm = wave / WP;
  const int H = a.H, W = a.W, HW = H * W;
  const int tiles_x = (W + 15) / 16, tiles_y = (H + TH - 1) / TH;
  const int tpi = tiles_x * tiles_y;
  const int b = blockIdx.x / tpi, t_img = blockIdx.x % tpi;
  const int oy0 = (t_img / tiles_x) * TH, ox0 = (t_img % tiles_x) * 16;
  const int m0 = (blockIdx.y * WMV + wm) * 64;
  const int K = a.Cin, nstage = K >> 4;
  const float* xb = a.x + (int64_t)b * K * HW;
  const bool active = oy0 + wp * 4 < H;        // wave-uniform: a wave whose rows all lie below the image only helps staging

  // ---- halo staging: per element its LDS offset and its source offset inside a 16-channel stage (-1: outside the image)
  int p_lds[NU], p_src[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int e = tid + 256 * u;
    const int ch = e / (TR * TC), rem = e % (TR * TC);
    const int t = rem / TC, m = rem % TC;
    const int iy = oy0 + t - 1, ix = ox0 + m - 1;
    const bool live = e < E;
    const bool ok = live && iy >= 0 && iy < H && ix >= 0 && ix < W;
    p_lds[u] = live ? ch * CS + t * TC + m : -1;
    p_src[u] = ok ? ch * HW + iy * W + ix : -1;
  }
  float raw[NU];
  auto fill_load = [&](int st) {
    const float* src = xb + (int64_t)st * 16 * HW;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int ps = p_src[u];
      float v = src[ps >= 0 ? ps : 0];
      v = ps >= 0 ? v : 0.f;
      raw[u] = a.relu_in ? fmaxf(v, 0.f) : v;
    }
  };
  auto fill_store = [&](float* dst) {
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (p_lds[u] >= 0) dst[p_lds[u]] = raw[u];
  };

  // ---- A fragments [tap][Cout/16][Cin/16][256]: lane (q, i) holds w[o = 16 ot + i][c = 16 st + 4 j4 + q] in element j4
  f32x4 afr[4], afr_next[4];
  auto a_load = [&](int st, int tap, f32x4 (&dst)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dst[i] = *reinterpret_cast<const f32x4*>(
          a.wp + ((((int64_t)tap * (a.Cout >> 4) + (m0 >> 4) + i) * nstage + st) * 256 + lane * 4));
  };

  f32x4 acc[4][4], tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
      tot[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

  if (active) a_load(0, 0, afr_next);
  fill_load(0);
  fill_store(sT);
  __syncthreads();

#pragma unroll 1
  for (int st = 0; st < nstage; ++st) {
    const float* cur = sT + (st & 1) * STAGE + q * CS + (wp * 4) * TC + jn;
    const bool more = st + 1 < nstage;
    if (more) fill_load(st + 1);
    if (active) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) afr[i] = afr_next[i];
        if (tap < 8) a_load(st, tap + 1, afr_next);
        else if (more) a_load(st + 1, 0, afr_next);
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
          float bv[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) bv[r] = cur[4 * j4 * CS + (r + ky) * TC + kx];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(afr[i][j4], bv[r], acc[i][r], 0, 0, 0);
        }
      }
      if ((st % FOLD) == FOLD - 1 || !more) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            tot[i][r] += acc[i][r];
            acc[i][r] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
      }
    }
    if (more) fill_store(sT + ((st + 1) & 1) * STAGE);       // free since the barrier that ended stage st - 1
    __syncthreads();
  }
  if (!active) return;

  // ---- epilogue.  D layout: tot[i][r][e] = out[o = m0 + 16 i + 4 q + e][oy0 + 4 wp + r][ox0 + jn]
  const int ox = ox0 + jn;
  if (ox >= W) return;
  const float gl = a.tap_t ? a.gloss[0] * a.tap_c : 0.f;
  const int64_t ob = (int64_t)b * a.Cout * HW;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int oy = oy0 + wp * 4 + r;
    if (oy >= H) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int o = m0 + 16 * i + 4 * q + e;
        const int64_t idx = ob + (int64_t)o * HW + oy * W + ox;
        float v = tot[i][r][e];
        if (a.bias) v += a.bias[o];
        if (a.mask_z) {
          const float z = a.mask_z[idx];
          v = z > 0.f ? v : 0.f;
          if (a.tap_t) v += gl * (z - a.tap_t[idx]);
        }
        a.out[idx] = v;
      }
  }
}

// [Cout,Cin,3,3] -> the forward form [tap][Cout/16][Cin/16][lane = 16 q + i][j4] = w[16 ot + i][16 ks + 4 j4 + q][tap] and the
// data-gradient form, the same layout of wT[c][o][tap] = w[o][c][8 - tap] (transposed, rotated 180 degrees)
__global__ void __launch_bounds__(256) vgg_pack_kernel(const float* __restrict__ w, float* __restrict__ fwd,
                                                       float* __restrict__ bwd, int Cout, int Cin) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= 9 * Cout * Cin) return;
  const int j4 = idx & 3, lane = (idx >> 2) & 63, rest = idx >> 8;
  const int i = lane & 15, q = lane >> 4;
  {
    const int ks = rest % (Cin >> 4), ot = (rest / (Cin >> 4)) % (Cout >> 4), tap = rest / ((Cin >> 4) * (Cout >> 4));
    const int o = ot * 16 + i, c = ks * 16 + 4 * j4 + q;
    fwd[idx] = w[((int64_t)o * Cin + c) * 9 + tap];
  }
  {
    const int ks = rest % (Cout >> 4), ot = (rest / (Cout >> 4)) % (Cin >> 4), tap = rest / ((Cin >> 4) * (Cout >> 4));
    const int o = ks * 16 + 4 * j4 + q, c = ot * 16 + i;
    bwd[idx] = w[((int64_t)o * Cin + c) * 9 + (8 - tap)];
  }
}

int launch_conv(const VggConvArgs& a, hipStream_t s) {
  if (a.H < 16 && a.Cout % 256 == 0) {
    dim3 grid(a.B * ceil_div(a.H, 4) * ceil_div(a.W, 16), a.Cout / 256);
    hipLaunchKernelGGL(vgg_conv3x3_kernel<1>, grid, dim3(256), 0, s, a);
  } else {
    dim3 grid(a.B * ceil_div(a.H, 16) * ceil_div(a.W, 16), a.Cout / 64);
    hipLaunchKernelGGL(vgg_conv3x3_kernel<4>, grid, dim3(256), 0, s, a);
  }
  return cips3d_launch_status();
}


int check_ctx_io(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io) {
  if (!ctx || !io || !io->x) return CIPS3D_E_BADARG;
  if (io->n_convs < 1 || io->n_convs > NCONV) return CIPS3D_E_BADARG;
  const int rc = cips3d_vgg_supported(io->B, io->H, io->W);
  if (rc != 0) return rc;
  int pool = 0;
  for (int l = 0; l < io->n_convs; ++l) {
    if (!ctx->w_fwd[l] || !ctx->bias[l] || !io->z[l]) return CIPS3D_E_BADARG;
    if (kPoolBefore[l] && !io->pooled[pool++]) return CIPS3D_E_BADARG;
  }
  return 0;
}

int run_features(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, hipStream_t s) {
  const int B = io->B;
  int H = io->H, W = io->W, pool = 0;
  hipLaunchKernelGGL(vgg_first_fwd_kernel, dim3(blocks_of((int64_t)B * H * W)), dim3(256), 0, s, io->x, ctx->w_fwd[0],
                     ctx->bias[0], io->z[0], B, H, W, io->normalize);
  int rc = cips3d_launch_status();
  for (int l = 1; l < io->n_convs && rc == 0; ++l) {
    const float* in = io->z[l - 1];
    int relu_in = 1;
    if (kPoolBefore[l]) {
      H /= 2; W /= 2;
      const int64_t total = (int64_t)B * kChan[l - 1] * H * W;
      hipLaunchKernelGGL(vgg_pool_fwd_kernel, dim3(blocks_of(total)), dim3(256), 0, s, in, io->pooled[pool], total, H, W);
      if ((rc = cips3d_launch_status()) != 0) break;
      in = io->pooled[pool++];
      relu_in = 0;
    }
    VggConvArgs a = {in, ctx->w_fwd[l], ctx->bias[l], io->z[l], nullptr, nullptr, 0.f, nullptr, B, kChan[l - 1], kChan[l], H, W,
                     relu_in};
    rc = launch_conv(a, s);
  }
  return rc;
}

}  // namespace

extern "C" int cips3d_vgg_supported(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return CIPS3D_E_BADARG;
  if (H % 16 != 0 || W % 16 != 0) return CIPS3D_E_UNSUPP;
  if ((int64_t)H * W > (int64_t)1 << 24) return CIPS3D_E_UNSUPP;        // a sample's 64-channel map is indexed in 32 bits
  if ((int64_t)B * (H / 4) * (W / 16) > 0x7fffffff) return CIPS3D_E_UNSUPP;
  return 0;
}

extern "C" int cips3d_vgg_channels(int conv) { return conv >= 0 && conv < NCONV ? kChan[conv] : CIPS3D_E_BADARG; }

extern "C" int cips3d_vgg_stride(int conv) {
  if (conv < 0 || conv >= NCONV) return CIPS3D_E_BADARG;
  int s = 1;
  for (int l = 0; l <= conv; ++l) s <<= kPoolBefore[l];
  return s;
}

extern "C" int64_t cips3d_vgg_partial_bytes(void) { return (int64_t)NCONV * PARTIALS_PER_TAP * sizeof(double); }

extern "C" int cips3d_vgg_pack(const cips3d_vgg_ctx* ctx, const float* const* weights, int n_convs, void* stream) {
  if (!ctx || !weights || n_convs < 1 || n_convs > NCONV) return CIPS3D_E_BADARG;
  for (int l = 0; l < n_convs; ++l)
    if (!weights[l] || !ctx->w_fwd[l] || (l > 0 && !ctx->w_bwd[l])) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  hipError_t e = hipMemcpyAsync(ctx->w_fwd[0], weights[0], 64 * 27 * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return (int)e;
  for (int l = 1; l < n_convs; ++l) {
    const int n = 9 * kChan[l] * kChan[l - 1];
    hipLaunchKernelGGL(vgg_pack_kernel, dim3(blocks_of(n)), dim3(256), 0, s, weights[l], ctx->w_fwd[l], ctx->w_bwd[l], kChan[l],
                       kChan[l - 1]);
    const int rc = cips3d_launch_status();
    if (rc != 0) return rc;
  }
  return 0;
}

extern "C" int cips3d_vgg_features(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream) {
  const int rc = check_ctx_io(ctx, io);
  if (rc != 0) return rc;
  return run_features(ctx, io, as_stream(stream));
}

extern "C" int cips3d_vgg_loss_forward(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream) {
  int rc = check_ctx_io(ctx, io);
  if (rc != 0) return rc;
  if (!io->partial || !io->loss || !io->target[io->n_convs - 1]) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  if ((rc = run_features(ctx, io, s)) != 0) return rc;
  return launch_tap_loss(io, s);
}

extern "C" int cips3d_vgg_loss_backward(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream) {
  int rc = check_ctx_io(ctx, io);
  if (rc != 0) return rc;
  const int L = io->n_convs - 1;
  if (!io->gloss || !io->dx || !io->target[L] || (L > 0 && (!io->g[0] || !io->g[1]))) return CIPS3D_E_BADARG;
  for (int l = 1; l <= L; ++l)
    if (!ctx->w_bwd[l]) return CIPS3D_E_BADARG;
  hipStream_t s = as_stream(stream);
  const int B = io->B;
  int Hs[NCONV], Ws[NCONV];
  for (int l = 0, H = io->H, W = io->W; l <= L; ++l) {
    if (kPoolBefore[l]) { H /= 2; W /= 2; }
    Hs[l] = H; Ws[l] = W;
  }
  auto tap_c = [&](int l) { return 2.f * io->tap_w[l] * io->tap_w[l]; };
  // the deepest tap starts the chain.  L == 0: the only gradient buffer needed is one of conv 0's output -- g[0] if given
  float* cur = io->g[0];
  float* other = io->g[1];
  if (!cur) return CIPS3D_E_BADARG;
  {
    const int64_t n = (int64_t)B * kChan[L] * Hs[L] * Ws[L];
    hipLaunchKernelGGL(vgg_tap_grad_kernel, dim3(blocks_of(n)), dim3(256), 0, s, io->z[L], io->target[L], tap_c(L), io->gloss, cur,
                       n);
    if ((rc = cips3d_launch_status()) != 0) return rc;
  }
  for (int l = L; l >= 1; --l) {
    // cur = d loss / d z_l  ->  d loss / d z_{l-1}
    const float* t = io->target[l - 1];
    if (!kPoolBefore[l]) {
      VggConvArgs a = {cur, ctx->w_bwd[l], nullptr, other, io->z[l - 1], t, t ? tap_c(l - 1) : 0.f, io->gloss, B, kChan[l],
                       kChan[l - 1], Hs[l], Ws[l], 0};
      if ((rc = launch_conv(a, s)) != 0) return rc;
      float* tmp = cur; cur = other; other = tmp;
    } else {
      VggConvArgs a = {cur, ctx->w_bwd[l], nullptr, other, nullptr, nullptr, 0.f, nullptr, B, kChan[l], kChan[l - 1], Hs[l], Ws[l],
                       0};
      if ((rc = launch_conv(a, s)) != 0) return rc;
      const int64_t total = (int64_t)B * kChan[l - 1] * Hs[l] * Ws[l];
      hipLaunchKernelGGL(vgg_pool_bwd_kernel, dim3(blocks_of(total)), dim3(256), 0, s, other, io->z[l - 1], t,
                         t ? tap_c(l - 1) : 0.f, io->gloss, cur, total, Hs[l], Ws[l]);
      if ((rc = cips3d_launch_status()) != 0) return rc;
    }
  }
  hipLaunchKernelGGL(vgg_first_bwd_kernel, dim3(blocks_of((int64_t)B * io->H * io->W)), dim3(256), 0, s, cur, ctx->w_fwd[0], io->dx,
                     B, io->H, io->W, io->normalize);
  return cips3d_launch_status();
}
