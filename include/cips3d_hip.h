/*
 * cips3d_hip.h -- C ABI of libcips3d_hip.so: the MI355X (gfx950) implementation of the
 * CIPS-3D++ generator-forward hot path.
 *
 * Conventions (every entry point):
 *   - plain pointers + sizes, no framework types; all pointers are DEVICE pointers to
 *     contiguous fp32 (or int32 where stated) unless the name ends in `_host`;
 *   - the caller allocates every output and keeps every buffer alive until the stream
 *     has passed the call; nothing is allocated, freed or synchronised inside;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - returns 0 on success, a hipError_t (> 0) from the launch, or a negative CIPS3D_E_*
 *     code for argument errors (nothing is launched in that case);
 *   - stateless and re-entrant per stream.
 *
 * Reference interfaces replaced (paths relative to /root/reference/exp/):
 *   cips3d_fused_bias_act     op/fused_bias_act.cpp:11-20, op/fused_bias_act_kernel.cu:18-98
 *   cips3d_upfirdn2d          op/upfirdn2d.cpp:12-23, op/upfirdn2d_kernel.cu:49-369
 *   cips3d_linear*            models/model_v3.py:40-65,183-210 (MappingLinear/EqualLinear),
 *                             cips3d/volume_renderer.py:15-35 (LinearLayer gamma/beta heads)
 *   cips3d_camera_params      cips3d/nerf_utils.py:344-436,466-564
 *   cips3d_nerf_*             cips3d/nerf_utils.py:18-338 + cips3d/volume_renderer.py:39-303
 *   cips3d_modconv_* / torgb  models/model_v3.py:218-341,418-482
 *   cips3d_align_volume,      cips3d/utils.py:183-224 (align_volume, extract_mesh_with_marching_cubes;
 *   cips3d_marching_cubes_*   the reference runs skimage.measure.marching_cubes on the host)
 */
#ifndef CIPS3D_HIP_H
#define CIPS3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIPS3D_ABI_VERSION 49 /* bumped with every change of an entry point or of a struct layout below */
/* 49: cips3d_nerf_eikonal_loss, cips3d_nerf_eikonal_supported, cips3d_nerf_eikonal_workspace_bytes added; nothing else changed. */
/* 48: cips3d_nerf_bwd_composite, cips3d_nerf_bwd_camera and cips3d_nerf_bwd_fused CHANGED SIGNATURE (each took the argument list
 * of its former superset, whose name is gone); the per-struct cips3d_sizeof_* functions are gone, cips3d_sizeof_struct covers
 * every struct.  A binding written against 47 must be updated: check cips3d_abi_version() before the first call. */

#define CIPS3D_E_BADARG   (-1)   /* null pointer / non-positive size */
#define CIPS3D_E_UNSUPP   (-2)   /* configuration outside what the kernels implement */

int cips3d_abi_version(void);
/* human-readable text for a return code of any entry point (static storage) */
const char* cips3d_strerror(int code);

/* ------------------------------------------------------------------ op level */

/* out[i] = act(x[i] + bias[(i / step_b) % size_b]) * scale.
 * act: 1 = linear, 3 = leaky-relu(alpha).  grad: 0 = forward; 1 = first derivative w.r.t. x
 * evaluated with `ref` (the saved forward OUTPUT) deciding the branch; 2 = second derivative (0).
 * bias / ref may be NULL (absent).  Same contract as fused.fused_bias_act(input, bias, refer,
 * act, grad, alpha, scale) with step_b = prod(dims[2:]). */
int cips3d_fused_bias_act(const float* x, const float* bias, const float* ref, float* out,
                          int64_t n, int64_t step_b, int64_t size_b,
                          int act, int grad, float alpha, float scale, void* stream);

/* Up-sample by zero insertion, pad / crop, FIR-filter (true convolution with `kernel`),
 * down-sample.  input [major, in_h, in_w, minor] -> out [major, out_h, out_w, minor],
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kernel_h) / down_y + 1 (same for w); the caller
 * sizes `out` accordingly.  kernel [kernel_h, kernel_w] lives in device memory. */
int cips3d_upfirdn2d(const float* input, const float* kernel, float* out,
                     int64_t major, int in_h, int in_w, int minor, int kernel_h, int kernel_w,
                     int up_x, int up_y, int down_x, int down_y,
                     int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* Image post-step of the demo loops (clamp [-1,1] -> [0,255], round to nearest): out[i] = u8((clamp(x)+1)*127.5).
 * Both pointers 16-byte aligned.  Used before the multi-GPU gather (4x fewer bytes over xGMI). */
int cips3d_rgb_to_uint8(const float* rgb, uint8_t* out, int64_t n, void* stream);

/* ------------------------------------------------------------------ small dense layers */

/* One dense layer on a batch of row vectors:
 *   h      = pixelnorm ? x[b] * rsqrt(mean(x[b]^2) + 1e-8) : x[b]
 *   y      = sum_i h[i] * (W[o][i] * w_scale) + bias[o] * b_scale          (bias may be NULL)
 *   y      = lrelu ? leaky_relu(y, 0.2) * act_gain : y
 *   y      = y * out_scale + out_shift
 *   out    = trunc_mean ? trunc_mean[o] + trunc_psi * (y - trunc_mean[o]) : y
 * and the result is written out_repeat (>= 1) times, copy r at out + r * out_repeat_stride (the
 * `w.unsqueeze(1).repeat(1, n_latent, 1)` of the mapping networks, models/model_v3.py:1367,1416).
 * x [B, x_stride] (first in_dim entries used), W [out_dim, in_dim], out [B, out_stride]. */
int cips3d_linear(const float* x, int64_t x_stride, const float* W, const float* bias, float* out,
                  int64_t out_stride, int B, int in_dim, int out_dim,
                  float w_scale, float b_scale, int pixelnorm, int lrelu, float act_gain,
                  float out_scale, float out_shift, const float* trunc_mean, float trunc_psi,
                  int out_repeat, int64_t out_repeat_stride, void* stream);

/* PixelNorm on its own (models/model_v3.py:32-37): y[b] = x[b] * rsqrt(mean(x[b]^2) + 1e-8).  The generator's mapping
 * path folds it into its first cips3d_linear (pixelnorm = 1); this entry serves `G.style_decoder(z)` called as a module. */
int cips3d_pixel_norm(const float* x, float* y, int B, int C, void* stream);

/* A table of independent dense layers evaluated in ONE launch (FiLM gamma/beta heads and the
 * decoder's per-layer style modulations).  The table itself lives in device memory. */
typedef struct cips3d_linear_desc {
  const float* W;        /* [out_dim, in_dim] */
  const float* bias;     /* [out_dim] or NULL */
  const float* x;        /* row b at x + b * x_stride */
  float* out;            /* row b at out + b * out_stride */
  int64_t x_stride;
  int64_t out_stride;
  int32_t in_dim;
  int32_t out_dim;
  float w_scale;
  float b_scale;
  float out_scale;       /* applied after the bias: y * out_scale + out_shift */
  float out_shift;
  int32_t row_begin;     /* exclusive prefix sum of out_dim over the table */
  int32_t pad_;
} cips3d_linear_desc;

int cips3d_linear_table(const cips3d_linear_desc* table_dev, int n_desc, int total_rows, int B,
                        void* stream);

/* Backward of cips3d_linear_table (heads without activation: y = (w_scale W x + b_scale bias) out_scale + out_shift), all
 * heads in two launches.  The table is the forward's; tensors of the backward sit at the same offsets as the forward's:
 *   dy at dy_base + (desc.out - out_base)   [row b at + b * desc.out_stride]
 *   dx at dx_base + (desc.x - x_base)       [row b at + b * desc.x_stride]; ACCUMULATED with atomics (heads share inputs):
 *                                            the caller zeroes dx; NULL = not wanted
 *   dW flat, head i at dW + w_offsets[i] ([out_dim, in_dim]; w_offsets = device array of int64 element offsets); NULL = not wanted
 *   db flat [total_rows] (rows of heads without bias receive their value all the same); NULL = not wanted
 * in_dim: the LARGEST in_dim of the table (it sizes the grid over input columns; every head loops over its own).  The table lives
 * on the device, so what the kernels need of every head is the caller's to check before the call (hip.LinearTable.backward
 * does): in_dim % 4 == 0, x_stride % 4 == 0, x 16-byte aligned -- x is read and dW written in 16-byte pieces; n_desc <= 64. */
int cips3d_linear_table_bwd(const cips3d_linear_desc* table_dev, int n_desc, int total_rows, int in_dim, int B,
                            const float* out_base, const float* dy_base, const float* x_base, float* dx_base,
                            const int64_t* w_offsets_dev, float* dW, float* db, void* stream);

#ifndef CIPS3D_AMAX_SLOTS
#define CIPS3D_AMAX_SLOTS 8       /* see cips3d_range below: slots of one (tensor, sample) */
#endif
#ifndef CIPS3D_AMAX_STRIDE
#define CIPS3D_AMAX_STRIDE 64     /* floats between slots: 256 bytes, the slots of an array sit in different memory channels */
#endif
#define CIPS3D_AMAX_FLOATS (CIPS3D_AMAX_SLOTS * CIPS3D_AMAX_STRIDE)
#define CIPS3D_FEATURES_EXP (-14)
#define CIPS3D_PLANES_EXP_BLOCK 128   /* pixels that share one exponent of a split-fp16 planes tensor */

/* ------------------------------------------------------------------ camera */

/* locations [B,2] = (azim, elev); fov_deg [B] or NULL (then fov_deg_scalar); up [B,3] or NULL
 * (then (0,1,0)).  Writes extrinsics [B,3,4] = [R^T | T], focal/near/far [B]. */
int cips3d_camera_params(const float* locations, const float* fov_deg, float fov_deg_scalar,
                         const float* up, float dist_radius, int img_size, int B,
                         float* extrinsics, float* focal, float* near_, float* far_, void* stream);

/* The free camera of the axis-angle projector (models/projector_axis_angle.py; Camera.get_camera2world,
 * cips3d/nerf_utils.py:439-463): rot [B,3] an axis-angle vector, trans [B,3] a position; fov_deg [B] or NULL (then
 * fov_deg_scalar).  extrinsics [B,3,4] = [exp([rot]x) | trans / max(|trans|, 1e-12)] (pytorch3d's axis_angle_to_matrix and
 * F.normalize), evaluated in fp64 and rounded once; focal / near / far [B] exactly as cips3d_camera_params writes them
 * (focal = 0.5 img_size / tan(fov pi / 180), 1 -+ dist_radius).  At rot = 0, trans = (0,0,1) the pose is that of
 * cips3d_camera_params at azim = elev = 0, bit for bit.  One launch, one thread per view. */
int cips3d_camera_axis_angle(const float* rot, const float* trans, const float* fov_deg, float fov_deg_scalar,
                             float dist_radius, int img_size, int B, float* extrinsics, float* focal, float* near_,
                             float* far_, void* stream);
/* Its backward: dextrinsics [B,3,4] and dfocal [B], either may be NULL (= zero), -> drot [B,3], dtrans [B,3] and dfov [B]
 * (dfov may be NULL: not written; it is d loss / d fov in degrees).  fp64 inside; finite at rot = 0, where d R / d rot_i is
 * the generator [e_i]x; below the clamp of F.normalize dtrans = d column / 1e-12 (the denominator is a constant there), above
 * it dtrans is orthogonal to trans.  One launch. */
int cips3d_camera_axis_angle_bwd(const float* rot, const float* trans, const float* fov_deg, float fov_deg_scalar,
                                 int img_size, const float* dextrinsics, const float* dfocal, int B, float* drot,
                                 float* dtrans, float* dfov, void* stream);

/* ------------------------------------------------------------------ NeRF renderer */

/* Re-pack the FiLM-SIREN weight matrices into the MFMA operand order the render kernel streams
 * (once per weight update).  hidden = H (32, 64, 128 or 256), depth = D >= 1.
 *   w_hidden : D-1 matrices [H,H] (pts_linears.1..D-1.weight), concatenated
 *   w_view   : [H, H+3] (views_linears.weight)
 * packed     : cips3d_nerf_packed_floats(H, D) floats: per layer (hidden layers 1..D-1, then the H x H part of the view
 *              layer) the matrix scaled by a power of two 2^s into fp16's normal range and split into fp16 hi + lo halves
 *              (w 2^s = hi + lo, 22 significant bits) in v_mfma_f32_16x16x32_f16 A-fragment order, 4 bytes per weight;
 *              then (2^s, 2^-s) per layer.  The render kernel accumulates the three exact fp16 products
 *              w_hi x_hi + w_hi x_lo + w_lo x_hi in fp32 (fp32-equivalent results at 16/3 of the fp32 MFMA rate). */
int cips3d_nerf_pack_weights(const float* w_hidden, const float* w_view, float* packed,
                             int hidden, int depth, void* stream);
int64_t cips3d_nerf_packed_floats(int hidden, int depth);

typedef struct cips3d_nerf_params {
  /* geometry, per view */
  const float* cam_poses;   /* [B,3,4] */
  const float* focals;      /* [B] */
  const float* near_;       /* [B] */
  const float* far_;        /* [B] */
  const float* perturb_u;   /* [B, img*img] per-ray uniform in [0,1) or NULL (perturb = False) */
  /* network (all device pointers straight into the module's parameters) */
  const float* w_first;     /* [H,3]    pts_linears.0.weight */
  const float* packed;      /* cips3d_nerf_pack_weights output */
  const float* w_view;      /* [H,H+3]  views_linears.weight (columns H..H+2 = view direction) */
  const float* film;        /* [B, D+1, 2, H]: gamma = 15*g+30, beta = 0.25*b per layer */
  const float* layer_bias;  /* [D+1, H]: pts_linears.i.bias rows, then views_linears.bias */
  const float* w_sigma;     /* [H]      sigma_linear.weight */
  const float* w_rgb;       /* [3,H]    rgb_linear.weight */
  const float* b_sigma;     /* [1] */
  const float* b_rgb;       /* [3] */
  const float* sigmoid_beta;/* [1] */
  int32_t B, img_size, n_samples, hidden, depth;
  int32_t static_viewdirs;
  int32_t n_chunks;         /* sample chunks per ray (partials per ray) */
  int32_t n_rays;           /* 0: R = img_size^2 rays generated from the camera; > 0: explicit-geometry mode with R = n_rays */
  /* outputs */
  float* part;              /* [n_chunks, B, H+8, R] partial composites (see nerf.hip) */
  float* sdf;               /* [B, R, n_samples] or NULL */
  /* explicit-geometry mode = the reference's VolumeFeatureRenderer.forward(pts, rays_d, viewdirs, z_vals, ...)
   * (cips3d/volume_renderer.py:192-303): all four or none; cam_poses / focals / perturb_u are then unused */
  const float* x_pts;       /* [B, R, n_samples, 3] un-normalised sample points */
  const float* x_rays_d;    /* [B, R, 3] */
  const float* x_viewdirs;  /* [B, R, 3] (already normalised) */
  const float* x_z_vals;    /* [B, R, n_samples] */
  /* optional: final maps written by the render kernel itself (all four or none).  When cips3d_nerf_fuses_finish() says
   * yes for this shape, the eight chunk waves of a ray group meet in LDS, combine their partials in sample order (the
   * arithmetic of cips3d_nerf_finish, bit for bit) and write features [B,H,R], thumb_rgb [B,3,R], xyz [B,3,R],
   * mask [B,2,R]; `part` is then not touched and cips3d_nerf_finish must not be called.  Otherwise the pointers are
   * ignored and `part` + cips3d_nerf_finish is the way. */
  float* o_features; float* o_thumb; float* o_xyz; float* o_mask;
  /* != 0 (fused finish only): o_features receives the feature map as split-fp16 planes [B][H/8][hi|lo][R][8] (fp16), the
   * input format of cips3d_modconv1x1_planes, instead of fp32 [B,H,R] (same bytes).  The planes hold features * 2^14: every
   * pixel block has the exponent CIPS3D_FEATURES_EXP (cips3d_range.x_exp_const; a feature is a convex combination of sines,
   * |f| <= 1) */
  int32_t features_planes;
  /* != 0: with_sdf = False (cips3d/nerf_utils.py:288-297, noise-free): the sigma head's output is a raw density,
   * alpha = 1 - exp(-softplus(raw) * delta) (torch's softplus: the identity above 20); sigmoid_beta is then not read.
   * Forward only: the differentiable forward (stash / bwd_*) refuses it */
  int32_t raw_density;
  /* Differentiable forward (camera-driven mode only; all three or none): the render kernel additionally writes what
   * cips3d_nerf_bwd_fused needs, so that the backward does not recompute the forward -- per MFMA layer the fp32 accumulators
   * (`stash`: cips3d_nerf_bwd_fused_stash_floats(B, img_size, n_samples, hidden, depth, n_chunks) floats, the layout of that
   * call, which must then use the same n_chunks) and per point, p = sample * R + ray, the sdf (`bwd_sdf` [B,P]) and the rgb
   * logits (`bwd_crgb` [B,3,P]). */
  float* stash;
  float* bwd_sdf;
  float* bwd_crgb;
  /* != NULL: exact-fp32 arithmetic (the reference's F.linear in IEEE fp32, cips3d/volume_renderer.py:15-35, 74-85): the point
   * MLP's GEMMs run on the fp32 matrix instruction (v_mfma_f32_16x16x4_f32: bit for bit an fmaf chain in k order) over the
   * stream cips3d_nerf_pack_weights32 wrote, instead of three fp16 products per fp32 product over `packed` (which is then not
   * read).  hidden == 256, no stash (CIPS3D_E_UNSUPP otherwise); camera-driven or explicit geometry, fused or separate finish. */
  const float* packed32;
  /* optional (both or neither): n_zero_words floats the launch leaves ZEROED -- scratch that the caller's next launches expect
   * cleared (cips3d_generator_forward: the decoder's measured range rows in a frame of a sequence).  The default kernel's fused
   * finish clears them on its way out, any other form of the launch with one small kernel in front.  Nothing of the render
   * launch itself may live there. */
  float* zero_words;
  int64_t n_zero_words;
  /* != 0 (fused finish only; CIPS3D_E_UNSUPP when the shape does not fuse): o_mask is laid out [2, B, R] -- the background
   * weight of every view, then -|xyz| of every view: the two maps `Generator.forward` returns, each contiguous, without the
   * transposing copy a batch of [B, 2, R] needs */
  int32_t mask_planar;
  int32_t pad3_;
} cips3d_nerf_params;

/* The exact-fp32 weight stream of cips3d_nerf_params.packed32 (cips3d_nerf_packed_floats(hidden, depth) floats, as `packed`):
 * fp32 A fragments of v_mfma_f32_16x16x4_f32 per (layer, 16 output units, 16 input units), unscaled. */
int cips3d_nerf_pack_weights32(const float* w_hidden, const float* w_view, float* packed32, int hidden, int depth, void* stream);

/* 1 when cips3d_nerf_render(p) will write p->o_* itself (o_* set, n_chunks == 8, LDS large enough), else 0 */
int cips3d_nerf_fuses_finish(const cips3d_nerf_params* p);

/* Chunk count the render kernel wants for (B, n_samples): enough workgroups to fill the chip. */
int cips3d_nerf_suggest_chunks(int B, int img_size, int n_samples);
/* floats needed for `part` */
int64_t cips3d_nerf_part_floats(int B, int img_size, int hidden, int n_chunks);

/* rays -> samples -> FiLM-SIREN MLP (fp32 MFMA) -> per-chunk alpha compositing. */
int cips3d_nerf_render(const cips3d_nerf_params* p, void* stream);

/* Gradient of the SDF head with respect to the sample points (the reference's eikonal term, autograd.grad(sdf, pts, ones):
 * cips3d/nerf_utils.py:221-228), forward mode through the FiLM-SIREN trunk in one kernel (csrc/nerf_sdf_grad.hip).
 *   grad [B, R, n_samples, 3] = d sdf / d pts at every sample point, pts the UN-normalised world points (the per-view factor
 *   2 / (far - near) of normalize_points is included); p->sdf [B, R, n_samples] is written too when non-NULL.
 * Reads of `p`: the geometry (camera form: cam_poses, focals, near_, far_, perturb_u, img_size -- the sample positions of
 * cips3d_nerf_render for the same arguments; explicit form: x_pts with n_rays, near_, far_), w_first, film, layer_bias, w_sigma,
 * b_sigma, depth, hidden and packed32 (the exact-fp32 weight stream: the matrix products run on v_mfma_f32_16x16x4_f32 whatever
 * precision the render call uses; may be NULL at depth 1).  The view layer, the rgb head and every compositing field (part, o_*,
 * n_chunks, stash, zero_words, ...) are ignored.  No atomics: bit-reproducible.  Never synchronises.
 * hidden == 256 and depth <= 64, else CIPS3D_E_UNSUPP (cips3d_nerf_sdf_grad_supported: the same answer on the host, no GPU needed). */
int cips3d_nerf_sdf_grad(const cips3d_nerf_params* p, float* grad, void* stream);
int cips3d_nerf_sdf_grad_supported(int hidden, int depth);

/* Eikonal and minimal-surface losses of the SDF head over the sample points of a call, with their gradient to the FiLM table
 * (csrc/nerf_eikonal.hip): the reference's regularisers, exp/stylesdf/losses.py:13-24 on autograd.grad(sdf, pts,
 * create_graph=True), as the forward-mode pass of cips3d_nerf_sdf_grad followed by a reverse sweep over it in one kernel.
 *   loss_out [2] (device, fp64): mean((|g| - 1)^2) and mean(exp(-beta_ms |sdf|)) over the M = B R n_samples points, UNWEIGHTED;
 *   dfilm_out [B, depth + 1, 2, hidden] (device): d (lambda_eikonal loss_out[0] + lambda_minimal_surface loss_out[1]) / d film,
 *   film the table `p->film` as stored (gamma and beta rows after their affine maps); the view layer's row is written as zeros.
 *   |g| = 0 gives the eikonal term no gradient and sdf = 0 the minimal-surface term none (torch's conventions for norm and abs).
 *   values_only != 0: only loss_out is written, the reverse sweep does not run, dfilm_out and packed32_t may be NULL.
 * Reads of `p`: those of cips3d_nerf_sdf_grad (p->sdf is ignored).  packed32_t: cips3d_nerf_pack_weights32's stream of the
 * TRANSPOSED hidden matrices in reverse layer order (w_hidden[i] = W_{depth-1-i}^T, i = 0 .. depth-2; may be NULL at depth 1).
 * workspace: 16-byte aligned device memory of workspace_bytes, private to the call until it has run; it decides the grid: one
 * workgroup per compute unit, at most cips3d_nerf_eikonal_workspace_bytes(.., workgroups, ..)'s `workgroups`, at least B (fewer:
 * CIPS3D_E_BADARG).  A good size is workgroups = compute units + B.  No gradient with respect to the points, the camera or the
 * renderer's own weights.  No floating-point atomics: values and dfilm are bit-identical from run to run for one device and one
 * workspace size.  All products on v_mfma_f32_16x16x4_f32.  Never synchronises.  B >= 1.
 * hidden == 256 and depth <= 64, else CIPS3D_E_UNSUPP (cips3d_nerf_eikonal_supported: host only).
 * cips3d_nerf_eikonal_workspace_bytes: host only; 0 for an unsupported trunk. */
int cips3d_nerf_eikonal_loss(const cips3d_nerf_params* p, const float* packed32_t, float lambda_eikonal,
                             float lambda_minimal_surface, float beta_ms, int values_only, void* workspace, int64_t workspace_bytes,
                             double* loss_out, float* dfilm_out, void* stream);
int cips3d_nerf_eikonal_supported(int hidden, int depth);
int64_t cips3d_nerf_eikonal_workspace_bytes(int hidden, int depth, int workgroups, int values_only);

/* Composited surface normals of a rendered view and its Phong-shaded geometry frame (csrc/nerf_normals.hip): the render's
 * compositing weights applied to the SDF gradient instead of the sample points.
 *   sdf [B,R,N], grad [B,R,N,3]: what cips3d_nerf_sdf_grad wrote; sigmoid_beta [1] (device).
 *   Sample spacing, one of two forms: camera form (x_z_vals NULL): cam_poses [B,3,4], focals, near_, far_ [B], perturb_u [B,R]
 *   or NULL, img_size (R = img_size^2, n_rays = 0) -- z and |d| in cips3d_nerf_render's own expressions; explicit form:
 *   x_z_vals [B,R,N], x_rays_d [B,R,3], n_rays = R.
 *   delta_i = (z_{i+1} - z_i) |d|, delta_{N-1} = 1e10 |d|; sigma_i = sigmoid(-sdf_i / beta) / beta; alpha_i = 1 - exp(-sigma_i
 *   delta_i); T_i = prod_{j<i} (1 - alpha_j + 1e-10); w_i = alpha_i T_i  (cips3d/nerf_utils.py:276-286).
 * Outputs, each may be NULL, at least one set:
 *   normal_raw [B,3,R] = sum_i w_i grad_i (the xyz map's formula and layout); normal [B,3,R] = normal_raw / max(|normal_raw|,
 *   1e-12) (zero, not NaN, where all weights vanish);
 *   shade [B,R] fp32 and shade_u8 [B,3,R] (three equal channels, floor(255 clamp(shade, 0, 1) + 0.5)); both need xyz [B,3,R]
 *   (the render's map), eye [B,3] and light [B,3].  With n the unit normal, p = xyz, l = normalize(light - p), v = normalize(eye
 *   - p), c = n . l:  shade = ka + kd max(c, 0) + ks [c > 0] max(v . (2 c n - l), 0)^shininess  -- pytorch3d's Phong for a white
 *   vertex colour (the reference's create_mesh_renderer: ka, kd, ks = 0.1, 0.65, 0.2, shininess 64).
 * Lanes span samples (coalesced reads); the transmittance is a shifted exclusive prefix product over a wave segment, carried
 * across chunks of 64 samples for N > 64.  No atomics, bit-reproducible, independent of the grid; accurate exp / pow; never
 * synchronises.  CIPS3D_E_BADARG, nothing launched: a null required pointer, n_samples < 1, no output, a shade output without
 * xyz / eye / light.  CIPS3D_E_UNSUPP: B R > INT32_MAX. */
typedef struct cips3d_normals_params {
  const float* sdf; const float* grad; const float* sigmoid_beta;
  const float* cam_poses; const float* focals; const float* near_; const float* far_; const float* perturb_u;   /* camera form */
  const float* x_z_vals; const float* x_rays_d;                                                                   /* explicit form */
  const float* xyz; const float* eye; const float* light;                                                         /* shading */
  float* normal_raw; float* normal; float* shade; uint8_t* shade_u8;
  int32_t B, img_size, n_samples, n_rays;
  float ka, kd, ks, shininess;
} cips3d_normals_params;
int cips3d_nerf_normals(const cips3d_normals_params* p, void* stream);

/* Ordered combination of the chunk partials into the final maps:
 *   features [B,H,R] (channel-major = NCHW), thumb_rgb [B,3,R], xyz [B,3,R], mask [B,2,R]. */
int cips3d_nerf_finish(const float* part, int n_chunks, int B, int img_size, int hidden,
                       float* features, float* thumb_rgb, float* xyz, float* mask, void* stream);
/* the same for an arbitrary ray count per view (explicit-geometry mode): outputs are [B, C, n_rays] */
int cips3d_nerf_finish_rays(const float* part, int n_chunks, int B, int n_rays, int hidden, float* features,
                            float* thumb_rgb, float* xyz, float* mask, void* stream);

/* ------------------------------------------------------------------ decoder */

/* Range tracking of the split-fp16 modes (CIPS3D_GEMM_SPLIT, planes).  An fp32 activation is carried as two fp16 numbers; fp16
 * has 5 exponent bits, the reference's fp32 convolution (models/model_v3.py:296-312) 8.  Every split therefore happens on
 * x * 2^-e with one power of two per (tensor, sample) that puts a rigorous bound of max|x| into [2^14, 2^15); the consumer
 * undoes it exactly on its accumulators.  Two kinds of small per-sample device arrays carry what the kernels need:
 *   amax  [B][CIPS3D_AMAX_FLOATS] fp32: max |x| of a tensor's true values = the maximum over its CIPS3D_AMAX_SLOTS slots
 *         (slot s at float s * CIPS3D_AMAX_STRIDE: one 64-byte line each, so that the atomics of different workgroups do not
 *         queue on one line).  The producing epilogue raises a slot with one atomicMax per workgroup (the caller zeroes the
 *         array before the producer runs); cips3d_absmax fills it for a tensor that exists already.
 *   exp   [B][ceil(HW / CIPS3D_PLANES_EXP_BLOCK)] int32: the exponents a planes tensor was stored with, one per block of 128
 *         consecutive pixels (stored value = x * 2^-e; GEMM columns are independent, so every pixel block may have its own),
 *         written by its producer.
 *   pmax  [B][ceil(HW / 64)][C / 16] fp32: max |x| of every (16 channels x 64 pixels) patch of a planes tensor, written by its
 *         producer with one plain store per wave (no atomics, nothing to zero).  cips3d_modconv1x1_planes takes max|in| of a
 *         128-pixel block from the 2 x Cin/16 entries that cover it, so a planes OUTPUT's exponent needs no word from any
 *         other workgroup of the launch.
 *   lconst[B][4] fp32 {c0, c1, l1, -}: the layer's bound constants, |out| <= max(c1, sqrt(2) l1) * max|in| + c0 with
 *         c0 = sqrt(2) (|noise_w| * noise_bound + max|bias|), c1 = sqrt(2) * (sqrt(Cin) for a demodulated conv; the FIR's
 *         largest polyphase gain for the 2x up-sampler), l1 = the largest row L1 norm of a NON-demodulated weight (measured
 *         by the modulate kernel, else 0).  Written by cips3d_range_consts or by cips3d_modulate_table.
 * A kernel that must scale values it produces itself (planes output, the intermediates of a fused up-sampling stage) uses
 * bound = c1 * max|in| + c0; a kernel that splits an existing fp32 tensor uses bound = amax(in).
 * Passing rg == NULL keeps e = 0 everywhere (legal only for callers that know max|x| of every operand to lie in
 * [2^-3, 6e4]); the Python host always passes it. */
typedef struct cips3d_range {
  const float* x_amax;     /* [B][CIPS3D_AMAX_FLOATS] of an fp32 input activation (split GEMM, fused stage)        */
  const int32_t* x_exp;    /* planes input: its exponents [B][blocks]; NULL: every block has x_exp_const            */
  int32_t x_exp_const;     /* (the NeRF feature map: CIPS3D_FEATURES_EXP)                                           */
  float x_max_const;       /* planes input without x_pmax: a bound of max|x| the caller vouches for (feature map: 1);
                              0: 2^(e + 15), the bound the input's own exponent encodes (looser by ~2^5)             */
  const float* x_pmax;     /* planes input: its patch maxima [B][ceil(HW/64)][Cin/16], or NULL (x_max_const)        */
  const float* lconst;     /* [B][4] of this layer (planes output; conv1 of a fused stage)                         */
  const float* lconst2;    /* [B][4] of conv2 of a fused stage (needed when wm_next != NULL)                       */
  float* out_amax;         /* [B][CIPS3D_AMAX_FLOATS] or NULL: raised to max |out| (GEMM entry points; not the fused stage)      */
  int32_t* out_exp;        /* planes output: receives the exponents this launch chose, [B][blocks]                  */
  float* next_amax;        /* [B][CIPS3D_AMAX_FLOATS] or NULL: raised to max |y_next| (fused stage with wm_next)                 */
  float* out_pmax;         /* planes output: receives its patch maxima [B][ceil(HW/64)][Cout/16]                    */
  float next_gain;         /* fused stage, > 0: next_amax receives the BOUND next_gain * U2 of |y_next| (U2: the stage's bound of
                              |out2|; next_gain = sqrt(C) for a demodulated next up-conv) in slot 0 instead of the measured
                              maximum -- no workgroup reduction, no atomics; for a consumer that is the decoder's last stage */
  int32_t half_chip;       /* cips3d_modconv1x1_planes, != 0: launches of another, independent view are in flight on another stream
                              -- a launch that fills the chip exactly once (256 tiles of 64 x 128) runs as 128 tiles of 128 x 128
                              on half the CUs instead, side by side with the other view's (same results, same ToRGB slots) */
  const struct cips3d_reduce_job* ride;   /* cips3d_modconv1x1_planes only (HOST pointer, may be NULL): a ToRGB fold that rides on
                              this launch -- see cips3d_reduce_job */
} cips3d_range;
/* The job of one cips3d_torgb_reduce (same arithmetic, same fixed order, same bits) carried by a split-planes GEMM launch that
 * does not depend on it and leaves CUs free: one extra row of workgroups of that launch does the fold, so it costs no launch
 * of its own (4.7 us at 64^2 on MI355X).  out[b][r][n] = skip + sum_s part[s] + sum_k bias[k][r] with
 * n4 = B * 3 * HW / 4 float4 positions, HW4 = HW / 4, slot_stride = B * 3 * HW; n_slots <= 48, n_bias <= CIPS3D_TORGB_FOLD_MAX;
 * part / skip / out must not alias the GEMM's operands.  (CIPS3D_TORGB_FOLD_MAX is defined below: 8.) */
typedef struct cips3d_reduce_job {
  const float* part;
  const float* bias[8];
  const float* skip;       /* may be NULL */
  float* out;
  int64_t n4, HW4, slot_stride;
  int32_t n_slots, n_bias;
} cips3d_reduce_job;
/* amax[b][*] = max_i |x[b][i]|, x [B][n] (zeroes the slots, then one pass; HBM-bound) */
int cips3d_absmax(const float* x, int B, int64_t n, float* amax, void* stream);
/* the same pass over slots the caller has zeroed already (or that hold maxima this tensor's are to be merged with): one launch */
int cips3d_absmax_raise(const float* x, int B, int64_t n, float* amax, void* stream);
/* Test hook for the split itself (n even): words[i] = {hi | lo << 16} of x[i] * k -- even i through the fused form (the exact
 * product t k is split), odd i through the plain form on the fp32 product -- and, per pair (x[2j], x[2j+1]),
 * pairs[2j] = [hi_0 | hi_1 << 16], pairs[2j+1] = [lo_0 | lo_1 << 16] of the values themselves. */
int cips3d_split_words(const float* x, float k, uint32_t* words, uint32_t* pairs, int64_t n, void* stream);
/* CIPS3D_AMAX_SLOTS / CIPS3D_AMAX_STRIDE as the library was built (a binding sizes its amax arrays from these) */
int cips3d_amax_layout(int* slots, int* stride);
/* lconst[b] = {c0, c1, 0, 0} from a layer's parameters (device pointers; noise_w / bias / fir may be NULL):
 * c1 = sqrt(2) * (fir ? largest polyphase gain of the 4x4 FIR : w_gain), w_gain = sqrt(Cin) for a demodulated conv.
 * The bound of |noise| is max(noise_bound, the maximum of noise_amax), noise_amax = the slots of ONE sample written by
 * cips3d_absmax over the whole noise tensor (or NULL): no host round trip for a noise map that exists only on the device. */
int cips3d_range_consts(const float* bias, int n_bias, const float* noise_w, float noise_bound, const float* noise_amax,
                        float w_gain, const float* fir, float* lconst, int B, void* stream);

/* Modulated (and optionally demodulated) weights of one conv for every sample:
 *   wm[b][o][i][t] = scale * W[o][i][t] * s[b][i];  wm[b][o] *= rsqrt(sum wm[b][o]^2 + 1e-8)
 * W [Cout, Cin, k*k], s [B, s_stride] (first Cin used), wm [B, Cout, Cin, k*k].
 * flags: bit 0 = demodulate; bit 1 = emit the MFMA A-fragment order cips3d_modconv1x1 consumes
 * (k = 1, Cout % 16 == 0, Cin % 16 == 0; A operand of v_mfma_f32_16x16x4_f32, four k-steps per 16 bytes):
 *   wm[b][o/16][i/16][((i&3)<<4 | (o&15))*4 + ((i>>2)&3)]. */
#define CIPS3D_MOD_DEMODULATE 1
#define CIPS3D_MOD_PACKED     2
/* with CIPS3D_MOD_PACKED: the A-fragment order whose k-steps follow the MFMA *D* layout, so that a GEMM result still in
 * registers is the B operand of the next GEMM (cips3d_fused_up_conv_next):
 *   wm[b][o/16][i/16][(((i>>2)&3)<<4 | (o&15))*4 + (i&3)]. */
#define CIPS3D_MOD_CHAINED    4
/* with CIPS3D_MOD_PACKED and ksq == 9: tap t is stored in slot 8 - t (the 180-degree rotated kernel the up-sampling branch
 * of cips3d_modconv3x3 correlates with).  Packed ksq == 9 layout: wm[b][tap][o/16][i/16][((i&3)<<4 | (o&15))*4 + ((i>>2)&3)]. */
#define CIPS3D_MOD_FLIP       8
/* with CIPS3D_MOD_PACKED and ksq == 1 (Cin % 32 == 0): split-fp16 A fragments for CIPS3D_GEMM_SPLIT -- 2^8 wm as fp16 hi + lo
 * halves in v_mfma_f32_16x16x32_f16 order, wm[b][o/16][i/32][plane][(((i>>3)&3)<<4 | (o&15))][i&7] (fp16), 4 bytes per weight */
#define CIPS3D_MOD_SPLIT      16
/* with CIPS3D_MOD_PACKED [| CIPS3D_MOD_CHAINED] and ksq == 1: split-fp16 fragments for the fused up-sampling stage in
 * CIPS3D_GEMM_SPLIT mode (16-channel k-groups, v_mfma_f32_16x16x16_f16): the element <-> channel map of the fp32 layout, each
 * lane's 16 bytes = {fp16 hi x 4 | fp16 lo x 4} of 2^8 wm */
#define CIPS3D_MOD_SPLIT16    32
/* with CIPS3D_MOD_PACKED and ksq == 1: the packed form of wm^T ([Cin x Cout]: the A operand of the data-gradient GEMM
 * dx = wm^T dy) instead of wm's -- what cips3d_pack_weights(transpose = 1) makes from the plain matrix; fp32 fragments, or
 * with CIPS3D_MOD_SPLIT (Cout % 32 == 0) the split-fp16 ones (cips3d_pack_weights(transpose = 3)) */
#define CIPS3D_MOD_TRANSPOSE  64
/* with CIPS3D_MOD_PACKED and ksq == 1 (Cin % 32 == 0): bf16 A fragments (bf16(wm), round to nearest even, unscaled) for
 * cips3d_modconv1x1_planes16 -- the bf16 decoder mode's form of CIPS3D_MOD_SPLIT */
#define CIPS3D_MOD_BF16       128
/* OR-ed into `epilogue` of cips3d_modconv1x1 / into `skip_up` of cips3d_fused_up_conv: bf16 compute mode of the GEMM
 * (operands rounded to bf16 in registers, v_mfma_f32_16x16x16_bf16, fp32 accumulate; storage stays fp32).  This is the
 * decoder precision of BASELINE config 3; the default (flag absent) is exact fp32. */
#define CIPS3D_GEMM_BF16      0x100
/* OR-ed into `epilogue` of cips3d_modconv1x1[_torgb]: fp32-EQUIVALENT split-fp16 mode.  `wm` must come from
 * cips3d_modulate_weights(..., CIPS3D_MOD_PACKED | CIPS3D_MOD_SPLIT); activations are split x = fp16(x) + fp16(x - fp16(x)) in
 * registers and each product is accumulated in fp32 as three exact fp16 products (w_lo x_hi + w_hi x_lo + w_hi x_hi) on
 * v_mfma_f32_16x16x32_f16: results agree with the fp32 MFMA path to ~1e-6 relative (below fp32's own accumulation
 * rounding) at a fraction of its matrix time.  Storage and epilogues are unchanged fp32. */
#define CIPS3D_GEMM_SPLIT     0x400
/* bf16 STORAGE of the low-resolution GEMM result of an up-sampling stage (the tensor the 2x FIR reads): OR-ed into `epilogue`
 * of cips3d_modconv1x1 (epilogue 0 only) `out` is written as bf16 [B,Cout,HW]; OR-ed into `skip_up` of cips3d_fused_up_conv[_next]
 * (together with CIPS3D_GEMM_BF16) `y_lo` is read and `y_next` is written as bf16.  FIR, epilogues and accumulation stay
 * fp32.  Halves the activation bytes the >= 128^2 stages move through HBM (BASELINE config 3). */
#define CIPS3D_Y_BF16         0x200
/* OR-ed into `skip_up` of cips3d_fused_up_conv[_next]: `rgb` points to a uint8 [B,3,2H,2W] image and receives
 * cips3d_rgb_to_uint8(rgb) -- clamp to [-1, 1], (c + 1) * 127.5, round to nearest even -- instead of the fp32 values (bit-identical
 * to converting the stored fp32 image; the reference's img_tensor_to_pil step, models/render_video_web_v10.py:1825-1826). */
#define CIPS3D_RGB_U8         0x800
/* OR-ed into `skip_up` of cips3d_fused_up_conv[_next]: a FLAT stage -- a decoder block that does not up-sample,
 * [StyledConv, StyledConv, ToRGB] at one resolution (the blocks above the last entry of `upsample_list`: a 256^2 generator still
 * walks the 512 and 1024 blocks, at 256^2; models/model_v3.py:553-590).  `y_lo` is then conv1's GEMM result at the OUTPUT size
 * H x W, `fir` is not read (may be NULL), the outputs are H x W, `skip` (if any) is [B,3,H,W] and is added as it is (bit 0 of
 * skip_up must be clear); rg->x_amax = the maximum of |y_lo| as always, rg->lconst[b][1] (a row gain relative to conv1's INPUT)
 * is not used.  Supported shapes: cips3d_fused_flat_conv_supported. */
#define CIPS3D_STAGE_FLAT     0x1000
int cips3d_modulate_weights(const float* W, const float* s, int64_t s_stride, float* wm,
                            int B, int Cout, int Cin, int ksq, float scale, int flags,
                            void* stream);

/* The same for a table of convs in ONE launch (the whole decoder).  The table lives in device memory;
 * `s` already points at the conv's slice of the style-modulation buffer. */
typedef struct cips3d_modulate_desc {
  const float* W;        /* [Cout, Cin, ksq] */
  const float* s;        /* row b at s + b * s_stride */
  float* out;            /* [B, Cout*Cin*ksq] (plain or packed per flags) */
  int64_t s_stride;
  int32_t Cout, Cin, ksq, flags;
  float scale;
  int32_t row_begin;     /* exclusive prefix sum of Cout over the table */
  /* range constants of the layer this conv belongs to (all optional; lconst NULL = none wanted): the launch writes
   * lconst[b] = {c0, c1, l1, 0} (see cips3d_range) -- c0 / c1 by the wave of row 0, l1 raised by every row of a
   * non-demodulated conv (lconst must then be zero before the launch) */
  float* lconst;         /* [B][4] */
  const float* bias;     /* [n_bias] FusedLeakyReLU bias of the StyledConv */
  const float* noise_w;  /* [1] */
  const float* fir;      /* [16]: the conv up-samples; c1 follows the FIR, not the weight */
  int32_t n_bias, pad_;
} cips3d_modulate_desc;

/* noise_bound: an upper bound of |noise| over every noise map of the call (cips3d_rng_fill draws stay below 5.77) */
int cips3d_modulate_table(const cips3d_modulate_desc* table_dev, int n_desc, int total_rows, int B, float noise_bound,
                          void* stream);

/* 1 when cips3d_modconv1x1 tiles this shape (Cin % 32 == 0, Cout % 32 == 0, HW % 4 == 0). */
int cips3d_modconv1x1_supported(int Cin, int Cout, int64_t HW);

/* 1x1 modulated convolution as a per-sample GEMM with a fused epilogue:
 *   y[b][o][n] = sum_i wm[b][o][i] * x[b][i][n]
 *   epilogue 0: out = y                                              (raw, feeds the FIR up-sampler)
 *   epilogue 1: out = lrelu(y + noise_w * noise[n] + bias[o], 0.2) * sqrt(2)
 * x [B,Cin,HW], wm in the PACKED order above, out [B,Cout,HW], noise [HW] (noise_bstride = 0) or
 * per-sample [B,HW] (noise_bstride = HW). */
int cips3d_modconv1x1(const float* x, const float* wm, float* out, int B, int Cin, int Cout,
                      int64_t HW, int epilogue, const float* noise, int64_t noise_bstride,
                      const float* noise_w, const float* bias, const cips3d_range* rg, void* stream);

/* The same GEMM with the ToRGB that FOLLOWS this conv folded into its epilogue (models/model_v3.py:602-632: ToRGB reads
 * the conv's output): every workgroup also writes the partial sums of its block of output rows,
 *   rgb_part[row_block][b][r][n] = sum_{o in block} rgb_w[b][r][o] * out[b][o][n]      (rgb_w plain [B,3,Cout])
 * and *n_row_blocks receives the number of row blocks (slots) written (the tiling -- 32 to 128 rows per block -- follows the shape
 * and the batch: size rgb_part for Cout / 32 blocks and fold what *n_row_blocks reports).  cips3d_torgb_reduce folds the slots of one or
 * several such layers, their biases and the skip image in a FIXED order (deterministic), replacing cips3d_torgb launches
 * that re-read the activations.  rgb_w == rgb_part == NULL: plain cips3d_modconv1x1. */
#define CIPS3D_TORGB_FOLD_MAX 8
int cips3d_modconv1x1_torgb(const float* x, const float* wm, float* out, int B, int Cin, int Cout, int64_t HW, int epilogue,
                            const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                            const float* rgb_w, float* rgb_part, int* n_row_blocks, const cips3d_range* rg, void* stream);
/* (rg: CIPS3D_GEMM_SPLIT splits x * 2^-e, e from rg->x_amax; every mode raises rg->out_amax to max |out| when given)
 * out[b][r][n] = skip[b][r][n] + sum_{s < n_slots} part[s][b][r][n] + sum_{k < n_bias} biases[k][r]
 * (part = consecutive slots of [B,3,HW]; biases = HOST array of device pointers to [3]; skip may be NULL) */
int cips3d_torgb_reduce(const float* part, int n_slots, const float* const* biases, int n_bias, const float* skip, float* out,
                        int B, int64_t HW, void* stream);

/* 2x FIR up-sampling of a low-resolution conv result fused with the StyledConv epilogue:
 *   u   = upfirdn2d(y_lo, fir, up=2, pad=(2,1))      (fir = outer([1,3,3,1])/64*4, [4,4] device)
 *   out = lrelu(u + noise_w * noise + bias[c], 0.2) * sqrt(2)
 * y_lo [B,C,H,W] -> out [B,C,2H,2W].  out_amax: per-sample amax rows of `out` (cips3d_range; raised, not zeroed) or NULL. */
int cips3d_up2_fir_act(const float* y_lo, const float* fir, float* out, int B, int C, int H, int W,
                       const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                       float* out_amax, void* stream);

/* StyledConv epilogue on its own (used after the k x k path):
 *   out = lrelu(x + noise_w * noise + bias[c], 0.2) * sqrt(2);  x/out [B,C,HW]. */
int cips3d_noise_bias_act(const float* x, const float* noise, int64_t noise_bstride, const float* noise_w,
                          const float* bias, float* out, int B, int C, int64_t HW, void* stream);

/* ToRGB: out[b][c][n] = sum_i wm[b][c][i] * x[b][i][n] + bias[c] + skip_term, where skip_term is
 * absent (skip NULL), skip[b][c][n] (skip_up = 0) or upfirdn2d(skip, fir, up=2, pad=(2,1)) taken
 * from the half-resolution skip [B,3,H/2,W/2] (skip_up = 1).  x [B,Cin,H,W], wm [B,3,Cin]. */
int cips3d_torgb(const float* x, const float* wm, const float* bias, const float* skip, int skip_up,
                 const float* fir, float* out, int B, int Cin, int H, int W, void* stream);


/* One kernel for a whole up-sampling stage after its low-resolution GEMM (models/model_v3.py:618-630 for a
 * stage in `upsample_list`):
 *   act1 = lrelu(upfirdn2d(y_lo, fir, up=2, pad=(2,1)) + nw1*noise1 + bias1) * sqrt(2)     (never stored)
 *   out2 = lrelu(wm2 (1x1) act1 + nw2*noise2 + bias2) * sqrt(2)            -> out2 [B,C,2H,2W] unless NULL
 *   rgb  = wm_rgb (3 x C) out2 + bias_rgb + (skip_up ? upfirdn2d(skip) : skip)   -> rgb [B,3,2H,2W] unless wm_rgb NULL
 * y_lo [B,C,H,W]; wm2 in the PACKED order of cips3d_modulate_weights, wm_rgb plain [B,3,C]; skip [B,3,H,W] when
 * skip_up else [B,3,2H,2W] (or NULL).  C in {32,64,128,256}, W % 32 == 0, H % 2 == 0. */
int cips3d_fused_up_conv_supported(int C, int H, int W);
/* ... and for a FLAT stage (CIPS3D_STAGE_FLAT in `skip_up`; H x W = the one resolution of the block): C in {32,64,128,256},
 * W % 64 == 0, H % 4 == 0.  The same kernel without the FIR: act1 = lrelu(y_lo + nw1*noise1 + bias1) * sqrt(2), skip added as is. */
int cips3d_fused_flat_conv_supported(int C, int H, int W);
/* The stage above plus the low-resolution GEMM of the NEXT up-sampling stage (its `StyledConv(up)` 1x1 conv, C -> C/2,
 * which reads out2): y_next[b] = wm_next[b] (C/2 x C) out2[b], taken from the registers that hold out2, so out2 need not be
 * stored (pass NULL) and the next stage starts at its own cips3d_fused_up_conv with y_lo = y_next.  wm_next in the
 * CIPS3D_MOD_PACKED | CIPS3D_MOD_CHAINED order, y_next [B,C/2,2H,2W].  wm_next == y_next == NULL: plain cips3d_fused_up_conv.
 * cips3d_fused_up_conv_chains(C): 1 for the widths that have the chained form. */
int cips3d_fused_up_conv_chains(int C);
/* What a launch of cips3d_fused_up_conv[_next] hands its kernel instead of having every wave compute it (host only: no GPU call;
 * cips3d_sizeof_struct(21)).  Workgroup `bid` of a sample (after the kernel's permutation of the linear id) owns the tile at row
 * bid / tiles_x, column bid % tiles_x; the kernel takes the quotient as bid >> tx_shift when tiles_x is a power of two
 * (tx_shift >= 0), else as q = (bid * tx_rcp) >> 32 (tx_rcp = 2^32 / tiles_x + 1: the quotient or one more for every
 * bid < 2^32), minus one when q * tiles_x > bid.  *_bs: BYTES from one sample to the next, for the element types `skip_up`
 * selects (CIPS3D_Y_BF16: y_lo / y_next are bf16; CIPS3D_RGB_U8: rgb is uint8; bit 0: the skip image has the input's size).
 * `chained`: the launch has a wm_next / y_next.  Returns CIPS3D_E_UNSUPP for a shape the stage does not take. */
typedef struct cips3d_stage_geom {
  int32_t tile_h, tile_w, threads;   /* output pixels of a workgroup's tile, threads of a workgroup */
  int32_t tiles_x, tiles_y;          /* grid = (tiles_x * tiles_y, 1, B) */
  int32_t tx_shift;                  /* log2(tiles_x), or -1 */
  uint32_t tx_rcp;
  int32_t HWlo, HWo;                 /* elements of one channel plane of y_lo; of the outputs */
  int32_t pad_;
  int64_t ylo_bs, out2_bs, ynext_bs, rgb_bs, skip_bs;
} cips3d_stage_geom;
int cips3d_fused_stage_geometry(int C, int chained, int H, int W, int skip_up, cips3d_stage_geom* geom);
int cips3d_fused_up_conv_next(const float* y_lo, const float* fir, const float* noise1, int64_t noise1_bstride,
                              const float* noise_w1, const float* bias1, const float* wm2, const float* noise2,
                              int64_t noise2_bstride, const float* noise_w2, const float* bias2, float* out2,
                              const float* wm_rgb, const float* bias_rgb, const float* skip, int skip_up, float* rgb,
                              const float* wm_next, float* y_next, int B, int C, int H, int W, const cips3d_range* rg,
                              void* stream);
int cips3d_fused_up_conv(const float* y_lo, const float* fir, const float* noise1, int64_t noise1_bstride,
                         const float* noise_w1, const float* bias1, const float* wm2, const float* noise2,
                         int64_t noise2_bstride, const float* noise_w2, const float* bias2, float* out2,
                         const float* wm_rgb, const float* bias_rgb, const float* skip, int skip_up, float* rgb,
                         int B, int C, int H, int W, const cips3d_range* rg, void* stream);
/* (rg, CIPS3D_GEMM_SPLIT mode: x_amax = amax of y_lo, lconst = conv1's constants, lconst2 = conv2's; next_amax <- max |y_next|.
 * out2 is not tracked -- the register budget of the C = 32 stage; use cips3d_absmax before a split GEMM reads a stored out2) */

/* General k x k modulated convolution (k odd, padding k/2), direct form; used for k = 3 configs.
 * transpose2 = 1 computes conv_transpose2d(stride 2, padding 0): out is (2H-1+k-1)^2. */
int cips3d_modconv_kxk(const float* x, const float* wm, float* out, int B, int Cin, int Cout,
                       int H, int W, int k, int transpose2, void* stream);

/* The same 1x1 modulated conv on activations that are STORED split ("planes": x = fp16 hi + fp16 lo, laid out
 * [B][C/8][plane hi|lo][HW][8] fp16 = the consumer's MFMA B fragments, 4 bytes per value like fp32).  The producer's epilogue
 * splits every output once, so the main loop is LDS reads + MFMA only (csrc/chain.hip); used for the run of equal-resolution
 * StyledConvs at the NeRF resolution.  wm: CIPS3D_MOD_PACKED | CIPS3D_MOD_SPLIT.  out_format: 0 fp32 [B,Cout,HW], 1 planes,
 * 2 bf16 [B,Cout,HW].  epilogue / noise / bias / rgb_w / rgb_part / n_row_blocks as cips3d_modconv1x1_torgb (row blocks of 64).
 * cips3d_planes_supported: Cin % 64 == 0, Cout % 64 == 0. */
int cips3d_planes_supported(int Cin, int Cout, int64_t HW);
/* x_amax [B][CIPS3D_AMAX_FLOATS] (cips3d_absmax) -> planes of x * 2^-e with one e per sample, written to every pixel block's
 * entry of exp_out [B][blocks]; both NULL: e = 0.  pmax_out (optional, C % 16 == 0): the sample's maximum in every entry of the
 * tensor's patch maxima [B][ceil(HW/64)][C/16].  C % 8 == 0 */
int cips3d_to_planes(const float* x, void* planes, int B, int C, int64_t HW, const float* x_amax, int32_t* exp_out,
                     float* pmax_out, void* stream);
int cips3d_from_planes(const void* planes, float* x, int B, int C, int64_t HW, const int32_t* exp, void* stream);
/* rg: x_exp / x_exp_const (input planes); for a planes output x_pmax / x_max_const + lconst (-> its exponents, written to out_exp)
 * and out_pmax; out_amax (fp32 / bf16 output only: raised to max |out| per sample) */
int cips3d_modconv1x1_planes(const void* x_planes, const float* wm, void* out, int out_format, int B, int Cin, int Cout,
                             int64_t HW, int epilogue, const float* noise, int64_t noise_bstride, const float* noise_w,
                             const float* bias, const float* rgb_w, float* rgb_part, int* n_row_blocks, const cips3d_range* rg,
                             void* stream);

/* The bf16 decoder mode's form of the same run (BASELINE config 3: both GEMM operands rounded to bf16, fp32 accumulate --
 * the reference has no bf16 mode; the semantics are oracle/path.py:modulated_conv2d(bf16_gemm=True) over
 * models/model_v3.py:218-314).  "planes16" = [B][C/8][HW][8] bf16: one plane of the layout above, 2 bytes per value.  The stored
 * activation IS the rounded operand of the next layer's GEMM, so results equal the fp32-stored bf16 mode's.
 * wm: CIPS3D_MOD_PACKED | CIPS3D_MOD_BF16.  out_format: 0 fp32 [B,Cout,HW], 2 bf16 [B,Cout,HW], 3 planes16.  The other
 * arguments as cips3d_modconv1x1_planes (rgb_part row blocks of 64). */
int cips3d_to_planes16(const float* x, void* planes16, int B, int C, int64_t HW, void* stream);  /* C % 8 == 0 */
int cips3d_from_planes16(const void* planes16, float* x, int B, int C, int64_t HW, void* stream);
int cips3d_modconv1x1_planes16(const void* x_planes16, const float* wm, void* out, int out_format, int B, int Cin, int Cout,
                               int64_t HW, int epilogue, const float* noise, int64_t noise_bstride, const float* noise_w,
                               const float* bias, const float* rgb_w, float* rgb_part, int* n_row_blocks, const cips3d_range* rg,
                               void* stream);
/* (planes16: bf16 has fp32's exponent range, no scaling; rg->out_amax is still raised when given -- an fp32 / bf16 exit of the
 * run feeds a fused stage that may run split) */

/* 3x3 ModulatedConv2d (models/model_v3.py:264-314, decoder_cfg.kernel_size = 3) as an LDS-tiled implicit GEMM on MFMA.
 *   up = 0: out [B,Cout,H,W] = conv2d(x, wm, padding 1)                                           (:296-311)
 *   up = 1: out [B,Cout,2H,2W] = Blur(conv_transpose2d(x, wm, stride 2)), fir = the Blur's 4x4 taps (:280-291); the FIR is
 *           applied to the input tile in LDS (the two convolutions commute), nothing full-size is materialised
 * wm: cips3d_modulate_weights(..., ksq = 9, CIPS3D_MOD_PACKED [| CIPS3D_MOD_FLIP for up = 1]).
 * epilogue = 1 fuses NoiseInjection + bias + leaky ReLU * sqrt(2) as in cips3d_modconv1x1 (noise at the OUTPUT size).
 * epilogue | CIPS3D_GEMM_SPLIT: fp32-equivalent split-fp16 products (v_mfma_f32_16x16x32_f16, two taps per 32-deep step); wm then
 * additionally CIPS3D_MOD_SPLIT-packed (tap-pair fragments: B * Cout * Cin * 10 floats are written); rg->x_amax = the measured
 * per-sample maximum of x (cips3d_absmax; NULL: x is split unscaled -- for data of O(1)).  rg is not read otherwise.
 * cips3d_modconv3x3_supported: Cin % 16 == 0, Cout % 16 == 0, output width % 4 == 0 (plain: W % 4 == 0); other shapes use
 * cips3d_modconv_kxk. */
int cips3d_modconv3x3_supported(int Cin, int Cout, int H, int W, int up);
int cips3d_modconv3x3(const float* x, const float* wm, float* out, int B, int Cin, int Cout, int H, int W, int up,
                      const float* fir, int epilogue, const float* noise, int64_t noise_bstride, const float* noise_w,
                      const float* bias, const cips3d_range* rg, void* stream);

/* ------------------------------------------------------------------ whole forward, one call */

/* The generator forward (models/model_v3.py:875-1042) as ONE host call that enqueues every kernel of
 * the path on `stream`: mapping networks -> FiLM heads -> fused NeRF render -> finish -> all decoder
 * style modulations + weight modulations (two table launches) -> per layer GEMM / FIR / toRGB.
 * The plan is built once per (module, batch size, N_samples) by the host binding: it holds device
 * pointers into the module's parameters and into a persistent workspace; the per-call tensors travel
 * in cips3d_forward_io.  Only 1x1 convolutions whose shapes cips3d_modconv1x1_supported accepts can be
 * planned (every released v10 config); other configurations use the per-op entry points. */
#define CIPS3D_MAX_MAP_LAYERS 8
#define CIPS3D_MAX_DEC_LAYERS 40

typedef struct cips3d_dec_layer {
  int32_t kind;            /* 0 StyledConv, 1 StyledConv with 2x up-sampling, 2 ToRGB, 3 ToRGB + up-sampled skip */
  int32_t Cin, Cout, H, W; /* H, W = INPUT resolution of the layer (ToRGB: its own resolution) */
  int32_t noise_index;     /* index into cips3d_forward_io.noise (StyledConv) or -1 */
  int32_t flags;           /* CIPS3D_DEC_* bits (below): the route of the layer, written by cips3d_decoder_route_flags */
  int32_t pad_;
  const float* wm;         /* this layer's modulated weights (workspace, written by the modulate table) */
  const float* bias;       /* activate.bias [Cout] or ToRGB.bias [3] */
  const float* noise_w;    /* NoiseInjection.weight [1] (StyledConv) */
  const float* fir;        /* 4x4 FIR (blur.kernel / upsample.kernel) for kinds 1 and 3 */
  /* range workspace rows of this layer (cips3d_range; StyledConvs of a plan whose decoder runs split-fp16, else NULL) */
  float* amax;             /* [B][CIPS3D_AMAX_FLOATS] max |output| (kind 1: of the low-resolution GEMM result y_lo) */
  int32_t* aexp;           /* [B][ceil(H*W / CIPS3D_PLANES_EXP_BLOCK)] exponents of a planes output */
  float* pmax;             /* [B][ceil(H*W / 64)][Cout / 16] patch maxima of a planes output */
  float* lconst;           /* [B][4] written by the modulate table */
} cips3d_dec_layer;

/* cips3d_dec_layer.flags */
#define CIPS3D_DEC_CHAINED    1    /* (kind 1, or kind 0 with FLAT_HEAD): wm is in the CIPS3D_MOD_CHAINED order and this conv's GEMM is
                                      computed by the previous stage's kernel (cips3d_fused_up_conv_next) */
#define CIPS3D_DEC_SPLIT      2    /* wm is CIPS3D_MOD_SPLIT-packed and this layer's stand-alone GEMM runs in CIPS3D_GEMM_SPLIT mode */
#define CIPS3D_DEC_PLANES_IN  4    /* the layer's input is stored as split-fp16 planes (cips3d_modconv1x1_planes) */
#define CIPS3D_DEC_PLANES_OUT 8    /* ... and so is its output */
#define CIPS3D_DEC_SPLIT16    16   /* wm is CIPS3D_MOD_SPLIT16-packed (conv2 / chained up-conv of a fused stage run in CIPS3D_GEMM_SPLIT mode) */
#define CIPS3D_DEC_P16        32   /* (with PLANES_IN / PLANES_OUT): the planes are bf16 planes16 and wm is CIPS3D_MOD_BF16-packed
                                      (cips3d_modconv1x1_planes16) */
#define CIPS3D_DEC_DEMOD      64   /* the conv is demodulated (its rows have unit norm: the sqrt(Cin) gain of the range bounds).  A property
                                      of the layer, not of its route: the caller sets it, cips3d_decoder_route_flags keeps it */
#define CIPS3D_DEC_FLAT_HEAD  128  /* (kind 0): head of a FLAT stage -- this conv, the next StyledConv and the ToRGB behind them (equal
                                      widths, one resolution) run as one launch of the fused stage kernel (CIPS3D_STAGE_FLAT) */

typedef struct cips3d_generator_plan {
  int32_t B, z_dim, n_map_r, n_map_d, style_dim_r, style_dim_d, n_latent, n_dec_layers;
  /* mapping networks: MappingLinear x n_map_r (lrelu gain 1), PixelNorm + EqualLinear x n_map_d (gain sqrt 2) */
  const float* map_r_w[CIPS3D_MAX_MAP_LAYERS]; const float* map_r_b[CIPS3D_MAX_MAP_LAYERS];
  const float* map_d_w[CIPS3D_MAX_MAP_LAYERS]; const float* map_d_b[CIPS3D_MAX_MAP_LAYERS];
  int32_t map_d_in[CIPS3D_MAX_MAP_LAYERS];
  float map_d_lr_mul;
  int32_t decoder_bf16;          /* != 0: every decoder GEMM runs in the bf16 compute mode (CIPS3D_GEMM_BF16); 2: the fused
                                    up-sampling stages also keep y_lo / y_next as bf16 (CIPS3D_Y_BF16) */
  float* lat[4];                 /* ping-pong [B, max(style_dim_r, style_dim_d, z_dim)]: [0,1] renderer chain, [2,3] decoder chain */
  float* styles_r;               /* [B, D+1, style_dim_r] */
  float* styles_d;               /* [B, n_latent, style_dim_d] */
  /* style heads */
  const cips3d_linear_desc* film_table; int32_t film_n, film_rows;     /* -> nerf.film */
  const cips3d_linear_desc* mod_table; int32_t mod_n, mod_rows;        /* -> s_buf */
  const cips3d_modulate_desc* wm_table; int32_t wm_n, wm_rows;         /* s_buf -> wm buffers */
  /* renderer: everything but the per-call camera / perturbation pointers is pre-filled */
  cips3d_nerf_params nerf;
  float* features;               /* [B, H, S, S] NeRF feature map = decoder input */
  /* decoder */
  cips3d_dec_layer layers[CIPS3D_MAX_DEC_LAYERS];
  float* act[2];                 /* activation ping-pong, each >= B * max(C*H*W) floats */
  float* y_lo;                   /* low-resolution GEMM result feeding the FIR up-sampler */
  float* y_lo2;                  /* second one (a chained stage writes the next stage's while reading its own) or NULL */
  float* skip[2];                /* RGB skip ping-pong, each >= B*3*Hout*Wout floats */
  float* rgb_part;               /* ToRGB partial-sum slots, each [B,3,H0*W0] at the input resolution (or NULL: no folding) */
  int64_t rgb_part_slots;        /* capacity in slots */
  /* range workspace (NULL: the decoder does not run split-fp16): zeroed by every forward before its first use */
  float* range_ws;               /* range_ws_words 32-bit words holding every layer's amax / aexp / lconst rows */
  int64_t range_ws_words;
  float* feat_amax;              /* [B][CIPS3D_AMAX_FLOATS] of the NeRF feature map when it takes the fp32 -> planes conversion pass */
  int32_t* feat_exp;             /* [B][blocks] exponents written by that pass */
  float* feat_pmax;              /* [B][ceil(S*S/64)][hidden/16] patch maxima written by that pass */
  float* tmp_amax;               /* [B][CIPS3D_AMAX_FLOATS] scratch for tensors no producer tracked */
  /* workspace of the one-launch style phase (cips3d_style_phase) or NULL (the phase then runs as launches): */
  void* style_xch;               /* 2 * CIPS3D_MAX_MAP_LAYERS * B * style_xch_dim 8-byte {value, tag} granules, zeroed once */
  void* style_sync;              /* 256 bytes, zeroed once: [0] generation of the last launch, [1] waits that gave up (stays 0),
                                    [3..] diagnostics: 10 ns ticks from the start of workgroup 0 to its end / to each stage */
  int32_t style_xch_dim;         /* >= every width of the two mapping networks, % 4 == 0 */
  int32_t range_volatile_words;  /* the first range_volatile_words words of range_ws hold what every forward measures anew (amax /
                                    aexp rows, the feature map's rows); the lconst rows the modulate table writes lie behind them.
                                    A forward with io.styles_resident zeroes only these (0: such forwards are refused on a ranged plan) */
} cips3d_generator_plan;

typedef struct cips3d_forward_io {
  const float* z_r;        /* [B, z_dim] or NULL when styles_r of the plan was filled by the caller */
  const float* z_d;        /* [B, z_dim] or NULL (same for styles_d) */
  const float* mean_r;     /* [style_dim_r] truncation mean or NULL (truncation = 1) */
  const float* mean_d;     /* [style_dim_d] */
  float trunc_psi;
  int32_t pad_;
  const float* cam_poses; const float* focals; const float* near_; const float* far_;   /* [B,...] */
  const float* perturb_u;  /* [B, R] or NULL */
  float* sdf;              /* [B, R, N] or NULL */
  const float* noise[CIPS3D_MAX_DEC_LAYERS];      /* per StyledConv: [1 or B][Hout*Wout] or NULL */
  int64_t noise_bstride[CIPS3D_MAX_DEC_LAYERS];   /* 0 (shared) or Hout*Wout */
  float* rgb;              /* [B, 3, Hout, Wout] final image (written by the last ToRGB); with rgb_is_u8 a uint8 image of that shape */
  float* thumb;            /* [B, 3, S, S] */
  float* xyz;              /* [B, 3, S, S] */
  float* mask;             /* [B, 2, S, S]: background weight, -|xyz| */
  void* ev_nerf_start;     /* optional hipEvent_t recorded on `stream` right before / after the render kernel */
  void* ev_nerf_stop;
  /* optional: the call makes the fresh draws itself -- exactly cips3d_rng_fill(rng_seed, rng_base, rng_normal, rng_n_normal,
   * rng_uniform, rng_n_uniform), its threads spread over the mapping networks' launches (whose few latency-bound work groups
   * leave the chip idle) or, without those, as a launch of its own; the caller points noise[] / perturb_u into the two arrays.
   * Both counts 0: no draw. */
  uint64_t rng_seed, rng_base;
  float* rng_normal; int64_t rng_n_normal;
  float* rng_uniform; int64_t rng_n_uniform;
  float noise_bound;       /* upper bound of |noise[i][...]| over the call (0: the rng draw's own bound, 5.77, is used) */
  int32_t views_in_flight; /* > 1: the caller keeps that many independent forwards in flight on different streams (a hint: the 64^2
                              chain then launches half-chip tiles, cips3d_range.half_chip; results do not depend on it) */
  /* optional timeline of the decoder (measurement only; bench.py's roofline.kernels): ev_marks[0] and ev_marks[1] are
   * recorded back to back right before the first decoder launch (their distance calibrates what a record costs) and
   * ev_marks[k + 1] right after the k-th decoder launch of the call (hipEvent_t handles, at most
   * n_ev_marks of them; further launches are not marked); ev_info[4 k .. 4 k + 3] receives what launch k was:
   * {CIPS3D_MARK_* kind, input channels, output channels, output height}.  *ev_count = marks recorded.  A record between two dependent
   * launches costs ~1-2 us of queue drain: intervals are upper bounds of the kernel times. */
  void** ev_marks; int32_t* ev_info; int32_t* ev_count; int32_t n_ev_marks;
  /* != 0: a frame of a SEQUENCE (multi-view rendering of one latent: models/render_video_web_v10.py:1792-1824 calls G with the same
   * sample_z / truncation / noise_bufs for every frame).  The plan's style tables -- styles_r / styles_d, the FiLM table, the
   * modulation table and all modulated / demodulated decoder matrices with their range constants -- are taken as left by the last
   * full forward of this plan: the mapping networks, the style heads and the modulate table are NOT run (z_r / z_d / mean_* /
   * trunc_psi are ignored); only the measured range rows are zeroed.  The reference offers the same hoist through its
   * style_render= / style_decoder= arguments (models/model_v3.py:875-914).  Results are bit-identical to a full forward with the
   * same inputs.  The caller owns the promise that styles, truncation, weights and the bound of |noise| have not changed. */
  int32_t styles_resident;
  /* != 0: `rgb` points to uint8 [B, 3, Hout, Wout] and receives cips3d_rgb_to_uint8 of the image (CIPS3D_RGB_U8 of the last
   * up-sampling stage).  Only plans whose last layers form a fused up-sampling stage can do it: CIPS3D_E_UNSUPP otherwise (the
   * caller then renders fp32 and converts). */
  int32_t rgb_is_u8;
  /* != 0: `mask` is [2, B, S, S] (cips3d_nerf_params.mask_planar); only for plans whose render launch fuses its finish */
  int32_t mask_planar;
} cips3d_forward_io;

#define CIPS3D_MARK_START 0
#define CIPS3D_MARK_PLANES_GEMM 1   /* a 1x1 StyledConv of the planes run (chain_gemm_kernel), epilogue + folded ToRGB included */
#define CIPS3D_MARK_GEMM 2          /* cips3d_modconv1x1 / _torgb (fp32 activations in HBM) */
#define CIPS3D_MARK_LOWRES_GEMM 3   /* the low-resolution GEMM of an up-sampling StyledConv as a launch of its own */
#define CIPS3D_MARK_FUSED_STAGE 4   /* cips3d_fused_up_conv_next: FIR + act -> conv2 + act -> ToRGB + skip [-> next low-res GEMM] */
#define CIPS3D_MARK_TORGB 5         /* cips3d_torgb / cips3d_torgb_reduce */
#define CIPS3D_MARK_OTHER 6

int cips3d_generator_forward(const cips3d_generator_plan* plan, const cips3d_forward_io* io, void* stream);

/* ---- the decoder's route (csrc/decoder_route.hip): which launch form every layer of the one-call forward takes.  Host-only
 * arithmetic on the layer list: nothing here launches, allocates or makes a HIP call, so both functions run on a machine without a
 * GPU.  Two functions share one set of predicates: the first writes the flags a plan is packed by, the second turns flagged
 * layers into the list of launches; cips3d_generator_forward calls the second before its first enqueue and runs what it says. */
typedef struct cips3d_dec_route_opts {
  int32_t B;
  int32_t nerf_res;        /* resolution of the NeRF feature map = the decoder's input */
  int32_t mode;            /* arithmetic of the decoder: 0 plain fp32 (or fp32_exact), 1 split-fp16, 2 bf16 */
  /* the A/B knobs, != 0 = on: a fused stage also computes the next stage's low-resolution GEMM; blocks above the NeRF resolution
   * that do not up-sample run as flat stages; the run at the NeRF resolution keeps split-fp16 planes (mode 1) / bf16 planes16 (mode 2) */
  int32_t chain_stages, flat_stages, planes_run, planes16_run;
  int32_t pad_;
} cips3d_dec_route_opts;

/* Reads kind, Cin, Cout, H, W (and CIPS3D_DEC_DEMOD of flags) of layers[0 .. n_layers), writes every other bit of their flags and
 * *rgb_part_slots, the number of ToRGB partial-sum slots (cips3d_generator_plan.rgb_part_slots) the plan must allocate.
 * CIPS3D_E_BADARG: a null pointer, n_layers outside [1, CIPS3D_MAX_DEC_LAYERS], a kind outside [0, 3], B or nerf_res < 1,
 * mode outside [0, 2]. */
int cips3d_decoder_route_flags(cips3d_dec_layer* layers, int n_layers, const cips3d_dec_route_opts* opts, int64_t* rgb_part_slots);

#define CIPS3D_STEP_LOWRES_GEMM 0   /* the low-resolution GEMM of a fused stage's head -> y_lo (form: CIPS3D_STEP_PLANES / _P16 or fp32 input) */
#define CIPS3D_STEP_FUSED_STAGE 1   /* cips3d_fused_up_conv_next on layers [layer, layer + 2] (form: CIPS3D_STEP_FLAT, _CHAIN, _LAST) */
#define CIPS3D_STEP_PLANES_GEMM 2   /* a layer of the planes run (form: _P16, _FOLD; out_format as cips3d_modconv1x1_planes / _planes16 take it) */
#define CIPS3D_STEP_GEMM        3   /* cips3d_modconv1x1, with _FOLD cips3d_modconv1x1_torgb */
#define CIPS3D_STEP_GEMM_FIR    4   /* an up-sampling conv outside a fused stage: cips3d_modconv1x1 + cips3d_up2_fir_act */
#define CIPS3D_STEP_TORGB       5   /* a stand-alone cips3d_torgb (form: _LAST) */
#define CIPS3D_STEP_FLUSH       6   /* the pending ToRGB fold becomes the skip image: cips3d_torgb_reduce, or with _RIDE a
                                       cips3d_reduce_job on the CIPS3D_STEP_LOWRES_GEMM that follows */
/* cips3d_dec_step.form */
#define CIPS3D_STEP_PLANES 1        /* the input is split-fp16 planes */
#define CIPS3D_STEP_P16    2        /* the input is bf16 planes16 */
#define CIPS3D_STEP_FLAT   4        /* the stage does not up-sample (CIPS3D_STAGE_FLAT) */
#define CIPS3D_STEP_CHAIN  8        /* the stage also computes the low-resolution GEMM of layer + 3 */
#define CIPS3D_STEP_LAST   16       /* the step writes the final image */
#define CIPS3D_STEP_FOLD   32       /* the GEMM folds the ToRGB at layer + 1 into rgb_part slots [slot, slot + its row blocks) */
#define CIPS3D_STEP_RIDE   64       /* the flush rides on the next step's launch */
#define CIPS3D_MAX_DEC_STEPS (2 * CIPS3D_MAX_DEC_LAYERS)

typedef struct cips3d_dec_step {
  int32_t kind;          /* CIPS3D_STEP_* */
  int32_t layer;         /* the (first) layer the step runs; FLUSH: the layer in front of which the sum is needed */
  int32_t form;
  int32_t out_format;    /* PLANES_GEMM: 0 fp32, 1 split-fp16 planes, 3 planes16 */
  int32_t slot;          /* _FOLD: first slot of rgb_part the launch writes; FLUSH: the number of slots it sums */
  int32_t n_bias;        /* FLUSH: folded ToRGB layers, whose biases join the sum */
  int32_t H, W;          /* FLUSH: resolution of the slots */
  int32_t bias_layer[CIPS3D_TORGB_FOLD_MAX];   /* FLUSH: those layers */
  int32_t mark[4];       /* what the launch records on the timeline (cips3d_forward_io.ev_info): {CIPS3D_MARK_*, Cin, Cout, H};
                            mark[0] < 0: nothing (a riding flush has no launch of its own) */
} cips3d_dec_step;

/* The launches of the decoder, in order, for layers whose flags are set; returns their number (<= max_steps) or a refusal.
 * ranged: the plan tracks ranges (cips3d_generator_plan.range_ws != NULL); rgb_part_slots: the capacity the plan allocated.
 * Flags that do not describe a route these layers can take -- CIPS3D_DEC_CHAINED without a preceding stage that chains,
 * CIPS3D_DEC_PLANES_IN on an up-conv outside a fused stage, CIPS3D_DEC_FLAT_HEAD on a block the flat kernel does not take,
 * CIPS3D_DEC_PLANES_OUT with a ToRGB that cannot be folded, ... -- are CIPS3D_E_BADARG, as are null pointers, n_layers outside
 * [1, CIPS3D_MAX_DEC_LAYERS], a kind outside [0, 3] and max_steps too small (CIPS3D_MAX_DEC_STEPS always suffices).
 * A decoder can leave its image as uint8 (cips3d_forward_io.rgb_is_u8) iff its last step is a CIPS3D_STEP_FUSED_STAGE. */
int cips3d_decoder_steps(const cips3d_dec_layer* layers, int n_layers, int B, int ranged, int64_t rgb_part_slots,
                         cips3d_dec_step* steps, int max_steps);

/* Row blocks (= rgb_part slots) the ToRGB fold of a GEMM launch of this shape writes: cips3d_modconv1x1_torgb's *n_row_blocks /
 * cips3d_modconv1x1_planes' and _planes16's, without the launch. */
int cips3d_modconv1x1_torgb_blocks(int B, int Cin, int Cout, int64_t HW);
int cips3d_planes_torgb_blocks(int Cout);

/* The part of cips3d_generator_forward in front of the modulated weights: Generator.mapping_networks (models/model_v3.py:
 * 1299-1418) -> plan.styles_r / styles_d, the FiLM heads (cips3d/volume_renderer.py:66-67) and every
 * ModulatedConv2d.modulation (models/model_v3.py:254,268) through the plan's tables, the call's fresh draws (io.rng_*) and the
 * zeroing of the range workspace.  mode 0: a chain of dependent launches (two layers or a layer and a table per launch);
 * mode 1: ONE launch of resident workgroups that hand each layer's outputs to each other through plan.style_xch
 * (CIPS3D_E_UNSUPP when the plan has no such workspace, a chain is absent, B > 8 or a width exceeds style_xch_dim);
 * mode -1: what cips3d_generator_forward does -- mode 0, or mode 1 (where supported) when the environment says
 * CIPS3D_STYLE_PHASE=1: the one launch measured slower on MI355X.  Both modes give bit-identical
 * results. */
int cips3d_style_phase(const cips3d_generator_plan* plan, const cips3d_forward_io* io, int mode, void* stream);
/* sizeof() of every struct this header declares (a binding checks its own layout against these at load time):
 * which = 0 cips3d_generator_plan, 1 cips3d_forward_io, 2 cips3d_nerf_params, 3 cips3d_linear_desc,
 * 4 cips3d_modulate_desc, 5 cips3d_dec_layer, 6 cips3d_nerf_bwd_geom, 7 cips3d_nerf_bwd_fused_params, 8 cips3d_range,
 * 9 cips3d_reduce_job, 10 cips3d_normals_params, 11 cips3d_mesh_resolve_params, 12 cips3d_vgg_ctx, 13 cips3d_vgg_io,
 * 14 cips3d_vgg_split_ctx, 15 cips3d_vgg_split_io, 16 cips3d_lpips_io, 17 cips3d_dec_route_opts, 18 cips3d_dec_step,
 * 19 cips3d_mesh_color_params, 20 cips3d_mesh_texture_params, 21 cips3d_stage_geom, 22 cips3d_actbwd, 23 cips3d_slot_job,
 * 24 cips3d_modbwd_desc, 25 cips3d_adam_entry, 26 cips3d_adam_hyper, 27 cips3d_noise_buf, 28 cips3d_grad_layer,
 * 29 cips3d_decoder_grad_plan, 30 cips3d_decoder_grad_io; -1 for an unknown index */
int64_t cips3d_sizeof_struct(int which);

/* ------------------------------------------------------------------ stand-alone renderer steps
 * The fused kernel does these in registers; as separate entry points they give every method of the reference's `Render`
 * class (cips3d/nerf_utils.py:11-338) a callable counterpart with the reference's tensor layouts. */
/* Render.get_rays_in_world (:18-66): rays_o / rays_d / viewdirs [B,S,S,3] */
int cips3d_rays_in_world(const float* cam_poses, const float* focals, int img_size, int static_viewdirs, int B,
                         float* rays_o, float* rays_d, float* viewdirs, void* stream);
/* Render.get_z_vals, offset-sampling branch (:69-121): z [B,R,N]; perturb_u [B,R] per-ray uniform or NULL */
int cips3d_z_vals(const float* near_, const float* far_, const float* perturb_u, int B, int R, int N, float* z, void* stream);
/* the classic stratified branch of Render.get_z_vals (offset_sampling = False, cips3d/nerf_utils.py:98-117; `mlp_init_pass`):
 * t = linspace(0, 1, N); perturb_t [B,R,N] (one uniform per SAMPLE, drawn inside the interval between the neighbouring
 * midpoints) or NULL (perturb = False) */
int cips3d_z_vals_stratified(const float* near_, const float* far_, const float* perturb_t, int B, int R, int N, float* z,
                             void* stream);
/* Render.get_points (+ Render.normalize_points when pts_normalized != NULL) (:124-170): [B,R,N,3]; either output may be NULL */
int cips3d_ray_points(const float* rays_o, const float* rays_d, const float* z, const float* near_, const float* far_, int B,
                      int R, int N, float* pts, float* pts_normalized, void* stream);
/* Render.volume_integration (:231-338): rgb [n_rays,N,3], sdf [n_rays,N], features [n_rays,N,C] or NULL,
 * z_vals [n_rays,N], rays_d [n_rays,3], pts [n_rays,N,3] -> rgb_map [n_rays,3], feature_map [n_rays,C], xyz [n_rays,3],
 * mask [n_rays,2] = (last weight, -|xyz|).  N <= 256, C % 4 == 0.
 * flags: 0 = the with_sdf branch (density = sigmoid(-sdf / beta) / beta, :276-286);
 *   CIPS3D_VI_RAW_DENSITY      `sdf` holds the network's raw density output, density = softplus(raw) (:288-297; the caller adds
 *                              raw_noise_std * randn beforehand); sigmoid_beta may be NULL
 *   CIPS3D_VI_FORCE_BACKGROUND the last sample takes the weight the others leave: w[N-1] = 1 - sum_{k<N-1} w[k] (:309-310) */
#define CIPS3D_VI_RAW_DENSITY 1
#define CIPS3D_VI_FORCE_BACKGROUND 2
int cips3d_volume_integration(const float* rgb, const float* sdf, const float* features, const float* z_vals,
                              const float* rays_d, const float* pts, const float* sigmoid_beta, int64_t n_rays, int N, int C,
                              int flags, float* rgb_map, float* feature_map, float* xyz, float* mask, void* stream);

/* Dense layer over a point-major tensor x [n_points, in] -> y [n_points, out] for the per-point module forwards of the
 * reference when they are called directly (LinearLayer / FiLMSiren, cips3d/volume_renderer.py:15-85):
 *   mode 0: y = out_scale * (x W^T + bias) + out_shift
 *   mode 1: y = sin(gamma * (x W^T + bias) + beta), film = [B][2][out] (gamma, beta), batch = point / points_per_batch */
int cips3d_points_linear(const float* x, const float* W, const float* bias, const float* film, int64_t n_points,
                         int64_t points_per_batch, int in_dim, int out_dim, int mode, float out_scale, float out_shift,
                         float* y, void* stream);

/* ------------------------------------------------------------------ backward of the path
 * The flip-inversion loop (reference models/projector_v10.py:211-277,1058-1216) calls loss.backward() through
 * Generator.forward; the reference gets these gradients from PyTorch autograd over cuBLAS/cuDNN and from the backward
 * wiring of its two native ops (op/fused_act.py:20-84, op/upfirdn2d.py:20-143).  Each entry below is the explicit
 * backward of one forward entry point; torch.autograd.Function objects on the host chain them.
 * Gradient outputs are OVERWRITTEN (not accumulated); NULL output pointers skip that gradient. */

/* Backward of cips3d_linear (pixelnorm = 0, no truncation):  y = act(x W^T w_scale + bias b_scale) * out_scale + shift,
 * act = leaky-ReLU(0.2) * act_gain when lrelu (then `out` = the forward output, whose sign selects the slope).
 * dx [B,in], dW [out,in], dbias [out].  (models/model_v3.py:40-65,183-210; cips3d/volume_renderer.py:15-35) */
int cips3d_linear_bwd(const float* x, int64_t x_stride, const float* W, const float* out, int64_t out_stride,
                      const float* dout, int64_t dout_stride, int B, int in_dim, int out_dim, float w_scale,
                      float b_scale, int lrelu, float act_gain, float out_scale, float* dx, int64_t dx_stride,
                      float* dW, float* dbias, void* stream);

/* Backward of cips3d_modulate_weights (models/model_v3.py:267-278).  dwm [B,Cout,Cin*ksq] holds dL/dwm on entry and is
 * used as scratch (it holds dL/du on return, u = the modulated weight before demodulation).
 * dW [Cout,Cin*ksq] (summed over the batch), ds [B,Cin] with row stride ds_stride. */
int cips3d_modulate_bwd(float* dwm, const float* W, const float* s, int64_t s_stride, int B, int Cout, int Cin, int ksq,
                        float scale, int demodulate, float* dW, float* ds, int64_t ds_stride, void* stream);

/* wm [B,M,K] plain -> the MFMA A-fragment order cips3d_modconv1x1 consumes; transpose bit 0 packs wm[b]^T (K x M),
 * which turns cips3d_modconv1x1 into the data-gradient GEMM dx = wm^T dy.  M, K multiples of 16.  transpose bit 1: split-fp16
 * fragments (2^8 w = fp16 hi + lo) for the CIPS3D_GEMM_SPLIT mode; the packed matrix's K a multiple of 32, |w| < 255. */
int cips3d_pack_weights(const float* wm, float* packed, int B, int M, int K, int transpose, void* stream);

/* Weight gradient of the 1x1 convolution: dwm[b][m][k] = sum_p dy[b][m][p] * x[b][k][p]  (dy [B,M,P], x [B,K,P]).
 * M, K multiples of 32, P multiple of 4, 16-byte aligned pointers.  Pixel chunks are summed with fp32 atomics, so the
 * last bits depend on the execution order (as cuDNN's default weight-gradient algorithms do). */
int cips3d_gemm_wgrad(const float* dy, const float* x, float* dwm, int B, int M, int K, int64_t P, void* stream);
/* ---- one-call decoder backward: the data-gradient GEMM with the previous layer's activation backward as its epilogue.
 * The reference gets all of this from autograd over `StyledConv.forward` / `ToRGB.forward` (models/model_v3.py:444-482).
 *
 * g [B,Cin,HW] = gradient w.r.t. the pre-activation of StyledConv l (at the resolution of its GEMM), wm_t = its modulated
 * weights packed TRANSPOSED (cips3d_modulate_table with CIPS3D_MOD_TRANSPOSE, + CIPS3D_MOD_SPLIT16 for flags =
 * CIPS3D_GEMM_SPLIT): the product wm^T g [B,Cout,HW] is the gradient w.r.t. layer l's input = the output y of StyledConv
 * l-1 (Cout here = that layer's channel count).  The epilogue makes it the gradient w.r.t. layer l-1's pre-activation:
 *   dpre = (wm^T g + sum_c rgb_w[b][c][o] drgb[b][c][p]) * (y > 0 ? sqrt2 : 0.2 sqrt2)
 * and adds, with one fp32 atomic per row and workgroup,
 *   d_bias[o]      += sum_{b,p} dpre                     (FusedLeakyReLU bias, fused_act.py:20-84)
 *   d_noise_w[o]   += sum_{b,p} dpre * noise[b][p]       (per-channel partials of NoiseInjection.weight's gradient; the
 *                                                         caller sums the Cout partials)
 *   d_rgb_w[b][c][o] += sum_p drgb[b][c][p] * y[b][o][p] (the modulated ToRGB weights' gradient)
 * The accumulators must be zeroed by the caller.  rg->x_amax scales the split of g (CIPS3D_GEMM_SPLIT), rg->out_amax
 * records max|dpre| per sample (the next GEMM's and the weight-gradient GEMM's operand scale). */
typedef struct cips3d_actbwd {
  const float* y;        /* [B,Cout,HW] stored output of layer l-1 (only its sign is used) */
  const float* rgb_w;    /* [B,3,Cout] plain modulated weights of the ToRGB that read y, or NULL (both or neither with drgb) */
  const float* drgb;     /* [B,3,HW] gradient w.r.t. that ToRGB's output */
  float* d_bias;         /* [Cout] or NULL */
  float* d_noise_w;      /* [Cout] or NULL (needs `noise`) */
  float* d_rgb_w;        /* [B,3,Cout] or NULL */
  /* Slotted accumulators.  The L2 executes atomics per cache line and instruction: at 256^2 a row's accumulator line would
   * take one add from each of ~2000 workgroups, ~50 ns apiece (measured: 108 us for a 40 us GEMM).  With slots = S (a power
   * of two, 0 / 1 = none) workgroup w adds into copy w % S: d_bias / d_noise_w copy s at + s * slot_stride floats, d_rgb_w
   * copy s at + s * rgb_slot_stride floats; the caller sums the copies (cips3d_slot_reduce). */
  int32_t slots, slot_stride, rgb_slot_stride, pad_;
} cips3d_actbwd;
int cips3d_modconv1x1_actbwd(const float* g, const float* wm_t, float* dpre, int B, int Cin, int Cout, int64_t HW, int flags,
                             const cips3d_actbwd* ab, const float* noise, int64_t noise_bstride, const cips3d_range* rg,
                             void* stream);

/* Activation backward without a GEMM in front of it (the LAST StyledConv: its output is read by the last ToRGB only):
 * dpre = (g_in + rgb_w^T drgb) * lrelu'(y), same reductions as cips3d_actbwd; g_in may be NULL.  out_amax: amax row or NULL. */
int cips3d_act_tail_bwd(const float* g_in, const float* y, const float* rgb_w, const float* drgb, const float* noise,
                        int64_t noise_bstride, float* dpre, float* d_bias, float* d_noise_w, float* d_rgb_w, float* out_amax,
                        int B, int C, int64_t HW, int slots, int slot_stride, int rgb_slot_stride, void* stream);
/* dst[i] = sum_{s < S} src[s * stride + i] for a table of jobs in one launch (dst may be src: copy 0 then holds the sum) */
typedef struct cips3d_slot_job {
  const float* src; float* dst;
  int32_t n, slots, stride;
  int32_t row_begin;     /* exclusive prefix sum of ceil(n / 256) (workgroups) over the table */
} cips3d_slot_job;
int cips3d_slot_reduce(const cips3d_slot_job* table_dev, int n_jobs, int total_blocks, void* stream);
/* Transpose of the 2x FIR up-sampler (upfirdn2d up = 2, pad = (2, 1), 4 x 4 taps; op/upfirdn2d.py:20-143 reaches it through
 * upfirdn2d with swapped factors): g_hi [B,C,2H,2W] -> g_lo [B,C,H,W]; out_amax: per-sample amax rows of g_lo or NULL. */
int cips3d_up2_fir_bwd(const float* g_hi, const float* fir, float* g_lo, float* out_amax, int B, int C, int H, int W,
                       void* stream);
/* Modulation backward (models/model_v3.py:267-278, k = 1) of a table of layers in ONE launch: cips3d_modulate_bwd's
 * arithmetic; dW is stored, ds is ADDED to (the caller zeroes it).  Cin <= 512, B <= 4, n_desc <= 64. */
typedef struct cips3d_modbwd_desc {
  const float* d_wm;     /* [B, Cout, Cin] gradient of the modulated weights */
  const float* W;        /* [Cout, Cin] */
  const float* s;        /* row b at s + b * s_stride */
  float* dW;             /* [Cout, Cin] or NULL */
  float* ds;             /* row b at ds + b * ds_stride, or NULL */
  int64_t s_stride, ds_stride;
  int32_t Cout, Cin;
  float scale;
  int32_t demodulate;
  int32_t row_begin;     /* exclusive prefix sum of ceil(Cout / 32) (workgroups) over the table */
  int32_t pad_;
} cips3d_modbwd_desc;
int cips3d_modulate_table_bwd(const cips3d_modbwd_desc* table_dev, int n_desc, int total_blocks, int B, void* stream);

/* Adam step over a list of parameter tensors in one launch per 48 tensors (csrc/optim.hip): the update rule of
 * torch.optim.Adam (amsgrad off, no weight decay) that the reference's inversion loop runs three of per step
 * (models/projector_v10.py:279-390, 1210-1216).  `entries` is a HOST array (copied into the kernel arguments); p / m / v are
 * updated in place; step = the 1-based step count of these tensors (bias corrections). */
typedef struct cips3d_adam_entry {
  float* p; const float* g; float* m; float* v;
  int64_t n;
} cips3d_adam_entry;
int cips3d_adam_step(const cips3d_adam_entry* entries, int n_entries, float lr, float beta1, float beta2, float eps, int step,
                     void* stream);
/* The same update for the tensors of SEVERAL parameter groups / optimisers in shared launches (48 tensors and up to 8 distinct
 * hyper-parameter sets per launch): entry i takes hypers[group_of[i]].  The three optimisers of an inversion step (camera,
 * NeRF W+, decoder W+ + decoder parameters: 125 tensors in 4 groups) are then 3 launches instead of 6. */
typedef struct cips3d_adam_hyper { float lr, beta1, beta2, eps; int32_t step; } cips3d_adam_hyper;
int cips3d_adam_step_groups(const cips3d_adam_entry* entries, const int* group_of, int n_entries, const cips3d_adam_hyper* hypers,
                            int n_hypers, void* stream);

/* The two squared-difference terms of the inversion loss (models/projector_v10.py:1173-1174:
 * `(target - synth).square().sum() * rgb_weight + (target_thumb - synth_thumb).square().sum() * thumb_weight`; with
 * c_k = weight_k / n_k the F.mse_loss form of :1178):  loss[0] = c0 sum (a0 - b0)^2 + c1 sum (a1 - b1)^2, deterministic
 * (per-workgroup partial sums, then their total in a fixed order: two launches).  partial: scratch of
 * 2 * cips3d_sqdiff_pair_partials(n0, n1) floats.  _bwd: d_k = gloss[0] * 2 c_k (a_k - b_k), one launch; gloss = the
 * loss' incoming gradient, a device scalar.  Either tensor may be empty (n = 0). */
int cips3d_sqdiff_pair_partials(int64_t n0, int64_t n1);
int cips3d_sqdiff_pair(const float* a0, const float* b0, int64_t n0, float c0, const float* a1, const float* b1, int64_t n1,
                       float c1, float* partial, float* loss, void* stream);
int cips3d_sqdiff_pair_bwd(const float* a0, const float* b0, int64_t n0, float c0, float* d0, const float* a1, const float* b1,
                           int64_t n1, float c1, float* d1, const float* gloss, void* stream);

/* The noise regulariser of the inversion loss (models/projector_v10.py:1183-1195, StyleGAN2's multi-scale autocorrelation
 * penalty) over a LIST of noise buffers at once (csrc/inversion_loss.hip).  For every buffer v [B,1,S,S] (fp32, contiguous) and
 * every level n_0 = v, n_{l+1} = avg_pool2d(n_l, 2), down to and including the first level with side <= 8:
 *   loss[0] = weight * sum ( mean(n_l * roll(n_l, 1, dim 3))^2 + mean(n_l * roll(n_l, 1, dim 2))^2 )      (circular rolls).
 * `bufs` is a HOST array (copied into the kernel arguments, 32 buffers per launch).  Forward: per 32 buffers at most four
 * launches (pyramid from level 0; pyramid from level 6 when a side exceeds 512; per-workgroup partial sums of every level;
 * their fixed-order totals -> the 2 x levels means and the loss), backward: one, whatever the number of buffers and levels
 * (cips3d_noise_reg_launches states the count for K buffers of largest side max_S).  No float atomics: value and gradient
 * are bit-reproducible.  workspace: cips3d_noise_reg_workspace(bufs, K) bytes (pyramids, partials, means); _bwd reads the
 * workspace the forward of the same `bufs` filled and OVERWRITES bufs[i].d with gloss[0] * d loss / d v_i (gloss: the loss'
 * incoming gradient, a device scalar); the forward ignores `d`.  Supported (cips3d_noise_reg_supported): B >= 1 and every
 * level that is pooled has an even side (S <= 8: any S), S <= 32768.  Unsupported buffers: CIPS3D_E_BADARG, nothing launched. */
typedef struct cips3d_noise_buf {
  const float* v;
  float* d;
  int32_t B, S;
} cips3d_noise_buf;
int cips3d_noise_reg_supported(int B, int S);
int cips3d_noise_reg_launches(int K, int max_S, int backward);
int64_t cips3d_noise_reg_workspace(const cips3d_noise_buf* bufs, int K);
int cips3d_noise_reg(const cips3d_noise_buf* bufs, int K, float weight, void* workspace, float* loss, void* stream);
int cips3d_noise_reg_bwd(const cips3d_noise_buf* bufs, int K, float weight, const void* workspace, const float* gloss,
                         void* stream);

/* The mask blending of the inversion loss (models/projector_v10.py:1164-1167 with the mask of :268-273):
 *   out = x * m + x * (1 - m)   (the reference's `synth * mask + synth.detach() * (1 - mask)`: the image up to rounding),
 *   m = F.interpolate(1 - mask, scale_factor = f, mode = 'bicubic') (align_corners = False, A = -0.75, taps clamped to the
 *   border, result not clamped), evaluated per pixel from mask [B,1,H/f,W/f]: the full-resolution mask is never written.
 * _bwd: dx = g * m.  x / out / g / dx: [B,C,H,W] fp32 contiguous; f >= 1 divides H and W.  One launch each. */
int cips3d_mask_blend(const float* x, const float* mask, float* out, int B, int C, int H, int W, int f, void* stream);
int cips3d_mask_blend_bwd(const float* g, const float* mask, float* dx, int B, int C, int H, int W, int f, void* stream);

/* The decoder as ONE differentiable node (csrc/decoder_grad.hip): Decoder.forward with every StyledConv output kept, and the
 * whole backward -- gradients of the features, the W+ styles and every decoder parameter -- in one call each.
 * models/model_v3.py:592-637 under `loss.backward()` (models/projector_v10.py:1203-1209).  kernel_size 1. */
#define CIPS3D_GRAD_MAX_LAYERS 48
typedef struct cips3d_grad_layer {
  int32_t kind;            /* 0 StyledConv, 1 StyledConv with up-sampling, 2 ToRGB, 3 ToRGB whose skip is up-sampled first */
  int32_t Cin, Cout;
  int32_t H, W;            /* resolution of the layer's input */
  int32_t noise_index;     /* StyledConv: entry of io->noise; -1 otherwise */
  int32_t flags;           /* bit 0: split-fp16 GEMMs (wm / wm_t packed with CIPS3D_MOD_SPLIT16) */
  int32_t pad_;
  const float* bias;       /* FusedLeakyReLU bias [Cout] / ToRGB bias [3] */
  const float* noise_w;    /* [1] (StyledConv) */
  const float* fir;        /* [4,4] (kinds 1, 3) */
  const float* wm;         /* StyledConv: packed modulated weights; ToRGB: plain [B,3,Cin] (both written by mod_table) */
  const float* wm_t;       /* StyledConv: the packed transpose */
  float* y;                /* StyledConv: the stored output [B,Cout,Ho,Wo] */
  float* y_amax;           /* amax rows of y      (inside plan->amax_base .. + amax_bytes) */
  float* g_amax;           /* amax rows of the gradient w.r.t. this layer's pre-activation (same region) */
  float* glo_amax;         /* kind 1: amax rows of that gradient after the FIR transpose (same region) */
  float* d_wm;             /* [B,Cout,Cin] gradient of the modulated weights      (inside plan->zero_base .. + zero_bytes) */
  float* d_bias;           /* [Cout] / [3]                                         (same region) */
  float* d_nw_part;        /* StyledConv: row of plan->nw_parts                    (same region) */
  /* slotted accumulators (cips3d_actbwd): copies of d_bias / d_nw_part at + s * slot_stride, of d_wm (ToRGB: the
   * accumulators of the epilogue that reads this ToRGB's input) at + s * rgb_slot_stride; slots <= 1: none */
  int32_t slots, slot_stride, rgb_slot_stride, pad2_;
} cips3d_grad_layer;

typedef struct cips3d_decoder_grad_plan {
  int32_t B, n_layers, style_dim, pad_;
  const cips3d_linear_desc* style_table;      /* style -> s of every layer (cips3d_linear_table) */
  int32_t style_n, style_rows;
  const cips3d_modulate_desc* mod_table;      /* s -> wm in every form the layers name */
  int32_t mod_n, mod_rows;
  const cips3d_modbwd_desc* modbwd_table;
  int32_t modbwd_n, modbwd_blocks;
  const int64_t* style_w_offsets;             /* cips3d_linear_table_bwd's w_offsets */
  const float* styles;                        /* [B, n_latent, style_dim]: the style table's input (filled by the caller) */
  const float* s_all;                         /* the style table's output base */
  const float* ds_all;                        /* its gradient, same layout (zero region; the modbwd table adds to it) */
  float* d_styles;                            /* [B, n_latent, style_dim] or NULL (zero region) */
  float* d_style_W; float* d_style_b;         /* flat gradients of the style heads or NULL */
  float* amax_base; int64_t amax_bytes;       /* every amax row of the step: zeroed by the forward call */
  float* zero_base; int64_t zero_bytes;       /* every accumulator of the backward: zeroed by the backward call */
  float* feat_amax;                           /* amax rows of the features (amax region) */
  float* y_lo;                                /* low-resolution GEMM result of an up-sampling layer (largest one) */
  float* g[2];                                /* two gradient buffers of the largest activation */
  float* g_lo;                                /* FIR-transposed gradient of an up-sampling layer (largest one) */
  float* drgb_lo[4];                          /* gradient images of the skip chain below the output resolution */
  float* rgb[2];                              /* intermediate rgb images */
  const float* nw_parts; int32_t nw_stride, pad2_;    /* [n StyledConvs][nw_stride] noise-weight partials (all slots of a row) */
  const cips3d_slot_job* slot_table;          /* sums the slot copies of d_bias / ToRGB d_wm before they are used, or NULL */
  int32_t slot_n, slot_blocks;
  float* d_noise_w;                           /* [n StyledConvs] or NULL */
  cips3d_grad_layer layers[CIPS3D_GRAD_MAX_LAYERS];
} cips3d_decoder_grad_plan;

typedef struct cips3d_decoder_grad_io {
  const float* features;     /* [B, Cin0, H0, W0] */
  const float* noise[CIPS3D_GRAD_MAX_LAYERS];
  int64_t noise_bstride[CIPS3D_GRAD_MAX_LAYERS];
  float* rgb;                /* forward: [B,3,Hf,Wf] */
  const float* d_rgb;        /* backward: gradient of rgb */
  float* d_features;         /* backward: [B, Cin0, H0, W0] or NULL */
  /* optional (both or neither): the plan's style table re-pointed at the caller's own contiguous W+ tensor `styles`
   * [B, n_latent, style_dim] -- forward and backward then read the styles where they are instead of from the plan's copy */
  const cips3d_linear_desc* style_table;
  const float* styles;
} cips3d_decoder_grad_io;
int cips3d_decoder_grad_forward(const cips3d_decoder_grad_plan* plan, const cips3d_decoder_grad_io* io, void* stream);
int cips3d_decoder_grad_backward(const cips3d_decoder_grad_plan* plan, const cips3d_decoder_grad_io* io, void* stream);

/* The same contraction on split-fp16 products (three fp16 MFMA products per fp32 product).  dy_amax / x_amax: the measured
 * per-sample maxima of the operands ([B][CIPS3D_AMAX_FLOATS] slot arrays as cips3d_range uses them, or NULL: unscaled split,
 * for tests on O(1) data); each operand is split as v * 2^-e with max|v| 2^-e in [2^14, 2^15) and the sums are scaled back
 * exactly, so gradients of any magnitude keep fp32-level accuracy.  accumulate != 0: dwm is added to (the caller zeroed it).
 * M % 32 == K % 32 == P % 32 == 0, 16-byte aligned operands, else CIPS3D_E_UNSUPP. */
int cips3d_gemm_wgrad_split(const float* dy, const float* x, float* dwm, int B, int M, int K, int64_t P, const float* dy_amax,
                            const float* x_amax, int accumulate, void* stream);

/* Backward of cips3d_noise_bias_act / the epilogue of StyledConv (models/model_v3.py:327-341; op/fused_act.py:20-84):
 * y = lrelu(x + noise_w*noise + bias_c)*sqrt2.  dx [B,C,HW] (may alias dy), dnoise [1 or B][HW] (layout of `noise`),
 * dnoise_w [1], dbias [C]; scratch_c [C] is required with dnoise_w (per-channel partial sums). */
int cips3d_noise_bias_act_bwd(const float* dy, const float* y, const float* noise, int64_t noise_bstride,
                              const float* noise_w, float* dx, float* dnoise, float* dnoise_w, float* dbias,
                              float* scratch_c, int B, int C, int64_t HW, void* stream);

/* Backward of cips3d_torgb without the skip (its gradient is drgb itself; the FIR up-sampling of the skip is
 * cips3d_upfirdn2d): dx [B,C,HW], dwm [B,3,C], dbias [3].  (models/model_v3.py:469-482) */
int cips3d_torgb_bwd(const float* drgb, const float* x, const float* wm, float* dx, float* dwm, float* dbias, int B, int C,
                     int64_t HW, void* stream);

/* ---- NeRF half, materialised backward (csrc/nerf_bwd.hip).  Replaces autograd through Render.prepare_nerf_inputs,
 * SirenGenerator.forward and Render.volume_integration (cips3d/nerf_utils.py:18-338, cips3d/volume_renderer.py:39-160).
 * Activations are recomputed layer by layer in the decoder's layout act[b][c][p], p = sample * R + ray (R = img_size^2,
 * P = R * n_samples), so the hidden-layer GEMMs and their data gradients are cips3d_modconv1x1 (weights packed with
 * cips3d_pack_weights, transposed for the gradient).  Sequence: cips_3dplusplus_amd/autograd.py:NerfRenderFn.backward. */
typedef struct cips3d_nerf_bwd_geom {
  const float* cam_poses;  /* [B,3,4] */
  const float* focals;     /* [B] */
  const float* near_;      /* [B] */
  const float* far_;       /* [B] */
  const float* perturb_u;  /* [B,R] or NULL */
  int32_t B, img_size, n_samples, static_viewdirs;
} cips3d_nerf_bwd_geom;

/* rays -> ptsn [B,3,P] (normalised points), pre0 / h0 [B,H,P] (layer-0 pre-activation incl. bias, and its FiLM sine),
 * viewdirs [B,3,R].  film points at layer 0 of the [B,L,2,H] table, film_bstride = L*2*H floats. */
int cips3d_nerf_bwd_points(const cips3d_nerf_bwd_geom* geom, const float* w_first, const float* bias0, const float* film,
                           int film_bstride, int H, float* ptsn, float* pre0, float* h0, float* viewdirs, void* stream);
/* acc [B,H,P] (GEMM output) -> pre = acc + bias_c (+ wd[c*wd_stride + 0..2] . viewdir[ray]) in place; h = sin(gamma pre + beta) */
int cips3d_nerf_bwd_film(float* acc, float* h, const float* bias, const float* film, int film_bstride, const float* wd,
                         int wd_stride, const float* viewdirs, int B, int H, int R, int64_t P, void* stream);
/* out[b][r][p] = sum_c Wm[r*row_stride + c*col_stride] * x[b][c][p] + bias[r], n_rows <= 4 (bias may be NULL) */
int cips3d_nerf_bwd_heads(const float* x, const float* Wm, int row_stride, int col_stride, const float* bias, int n_rows,
                          int B, int H, int64_t P, float* out, void* stream);
/* g[b][p] = sum_c dF[b][c][ray(p)] * f[b][c][p] */
int cips3d_nerf_bwd_dot(const float* dF, const float* f, int B, int H, int R, int64_t P, float* g, void* stream);
/* volume integration forward + backward per ray: sdf [B,P], crgb [B,3,P] (rgb logits), g [B,P], dthumb [B,3,R]
 * -> w [B,P] (compositing weights), dsdf [B,P], dcrgb [B,3,P], ddnorm [B,R] (d loss / d |rays_d|, which scales the
 * sample spacing); T_scratch [B,P].  sigmoid_beta == NULL: with_sdf = False -- `sdf` is the raw density, sigma = softplus(sdf)
 * (cips3d/nerf_utils.py:288-297); no dbeta_ray then.  dbeta_ray [B,R] or NULL: per-ray d loss / d sigmoid_beta, for
 * `optim_render_params`, models/projector_v10.py:848-872.
 * The upstreams of the geometry maps of Render.volume_integration (cips3d/nerf_utils.py:329-336: xyz = sum_k w_k p_k,
 * mask[0] = w_{N-1}, mask[1] = depth = -|xyz|): d_mask [2,B,R] (planar: d mask[0], then d depth) and d_xyz [B,3,R], each may be
 * NULL; xyz [B,3,R] is the forward's map (needed with d_mask: d depth acts as -d_depth * xyz / |xyz| on xyz, 0 where |xyz| == 0).
 * With xbar the effective adjoint of xyz, d loss / d w_k gains <xbar, p_k> + [k == N-1] d mask[0], p_k = o + z_k d in world
 * units; the per-ray sums wsum = sum_k w_k and wzsum = sum_k w_k z_k [B,R] (needed and written when d_mask or d_xyz is set, else
 * NULL) carry the direct path through the points to cips3d_nerf_bwd_camera.  d_mask and d_xyz both NULL: the compositing
 * backward of the features and the thumbnail alone. */
int cips3d_nerf_bwd_composite(const cips3d_nerf_bwd_geom* geom, const float* sdf, const float* crgb, const float* g,
                              const float* dthumb, const float* sigmoid_beta, float* w, float* T_scratch, float* dsdf,
                              float* dcrgb, float* ddnorm, float* dbeta_ray, const float* d_mask, const float* d_xyz,
                              const float* xyz, float* wsum, float* wzsum, void* stream);
/* out[row][c] += sum_{b,p} a[b][row][p] * x[b][c][p mod Px] (c < nx <= 3), out[row][3] += sum_{b,p} a[b][row][p]; a [B,rows,P],
 * x [B,nx,Px], out [rows,4] zeroed by the caller: the narrow weight gradients and the biases of the point MLP. */
int cips3d_nerf_bwd_row_dots(const float* a, const float* x, int nx, int64_t Px, float* out, int B, int rows, int64_t P,
                             void* stream);
/* FiLM-sine backward, in place on buf [B,H,P]:
 *   mode 0: buf = dh (+ w_sigma[c]*dsdf[p] when w_sigma != NULL)            -> buf = d(pre)
 *   mode 1: upstream = weights[p]*dF[c][ray] + sum_r w_rgb[r][c]*dcrgb[r][p] -> buf = d(pre)   (buf's old content unused)
 * dfilm (same layout / stride as film, pointing at this layer) += sums for d(gamma), d(beta); zero it before the first call. */
int cips3d_nerf_bwd_film_grad(float* buf, const float* pre, const float* film, int film_bstride, int mode,
                              const float* w_sigma, const float* dsdf, const float* weights, const float* dF,
                              const float* w_rgb, const float* dcrgb, float* dfilm, int B, int H, int R, int64_t P,
                              void* stream);
/* dptsn [B,3,P], dvd_pt [B,3,P] (d loss / d viewdir per point), ddnorm [B,R] -> dcam [B,3,4].  accumulate == 0: dcam is
 * cleared by the call; != 0: ADDED to a dcam the caller has zeroed (cips3d_nerf_bwd_fused clears it in its preparation launch).
 * The direct path of the geometry maps: d o += wsum xbar, d d += wzsum xbar per ray (d_mask, d_xyz, xyz, wsum, wzsum as in
 * cips3d_nerf_bwd_composite; d_mask and d_xyz both NULL: none).
 * The gradient of the intrinsics: dfocal [B] (zeroed by the caller; NULL: none, the kernel's instantiation without the focal
 * sum) += d loss / d focals.  The ray's camera-frame direction is (dcx, dcy, -1) with dcx, dcy ~ 1 / focal, so d focal =
 * -sum_rays (g_cam[0] dcx + g_cam[1] dcy) / focal with g_cam = R^T d rays_d, plus -- with static_viewdirs, where the view
 * direction is normalize(d_cam) and does not pass through the pose -- the view direction's own adjoint.  near / far /
 * perturb_u stay constants. */
int cips3d_nerf_bwd_camera(const cips3d_nerf_bwd_geom* geom, const float* dptsn, const float* dvd_pt, const float* ddnorm,
                           const float* d_mask, const float* d_xyz, const float* xyz, const float* wsum, const float* wzsum,
                           int accumulate, float* dcam, float* dfocal, void* stream);
/* ---- NeRF half, fused backward (csrc/nerf_bwd_fused.hip): the same gradients as the sequence above -- d loss / d film
 * [B,L,2,H] and d loss / d cam_poses [B,3,4] from d_features [B,H,R] and d_thumb [B,3,R] -- with the point MLP kept in the
 * register file in both directions (the reference gets them from autograd through cips3d/volume_renderer.py:39-160 and
 * cips3d/nerf_utils.py:264-338).  Two MFMA kernels with the task shape of cips3d_nerf_render (16 rays x a chunk of samples
 * per wave, weights streamed through the LDS ring, split-fp16 products):
 *   recompute: the forward MLP again, writing per MFMA layer the fp32 accumulators (`stash`, in the wave's own register
 *              order: 16 * H * 4 bytes per layer and 16-point tile, fully coalesced) and per point sdf, rgb logits and
 *              <d_features[:, ray], feature>;
 *   (cips3d_nerf_bwd_composite: volume integration forward + backward per ray, as in the materialised sequence)
 *   backward : per 16-point tile the layers in reverse -- upstream * cos(arg) from the stash, the d(gamma) / d(beta) sums
 *              (cross-lane reduce-scatter + LDS accumulation, one global atomic per workgroup and table entry), the data
 *              gradient W^T d(pre) on the matrix cores with the transposed packed stream (the gradient operand is scaled per
 *              point by a power of two into fp16's range before it is split, and the result unscaled exactly), the
 *              view-direction and point gradients on the VALU;
 *   (cips3d_nerf_bwd_camera: d points / d viewdirs -> d cam_poses)
 * HBM traffic per point and MFMA layer: one write + one read of H floats (the materialised sequence moves ~10). */
typedef struct cips3d_nerf_bwd_fused_params {
  cips3d_nerf_bwd_geom geom;
  const float* w_first;      /* [H,3] */
  const float* packed;       /* cips3d_nerf_pack_weights */
  const float* packed_t;     /* cips3d_nerf_pack_weights_t */
  const float* w_view;       /* [H,H+3] */
  const float* film;         /* [B,L,2,H], L = depth + 1 */
  const float* layer_bias;   /* [L,H] */
  const float* w_sigma;      /* [H] */
  const float* b_sigma;      /* [1] */
  const float* w_rgb;        /* [3,H] */
  const float* b_rgb;        /* [3] */
  const float* sigmoid_beta; /* [1] */
  const float* d_features;   /* [B,H,R] */
  const float* d_thumb;      /* [B,3,R] */
  float* stash;              /* cips3d_nerf_bwd_fused_stash_floats() floats */
  float* scratch;            /* cips3d_nerf_bwd_fused_scratch_floats() floats */
  float* dfilm;              /* out [B,L,2,H] */
  float* dcam;               /* out [B,3,4] */
  int32_t hidden, depth, n_chunks, pad_;
  /* NULL: the call recomputes the forward (nerf_stash_kernel fills `stash`).  Both set: `stash` was filled by
   * cips3d_nerf_render (cips3d_nerf_params.stash / bwd_sdf / bwd_crgb, same n_chunks) and these are its per-point outputs;
   * only g = <d_features, feature> is then rebuilt, from the view layer's stash. */
  const float* fwd_sdf;      /* [B,P] */
  const float* fwd_crgb;     /* [B,3,P] */
  /* upstreams of the mask / depth and xyz maps (cips3d_nerf_bwd_composite); each may be NULL, xyz is needed with d_mask */
  const float* d_mask;       /* [2,B,R] */
  const float* d_xyz;        /* [B,3,R] */
  const float* xyz;          /* [B,3,R]: the forward's map */
} cips3d_nerf_bwd_fused_params;

/* 1 when the fused kernels cover the shape (hidden 32/64/128/256, R % 16 == 0, tables within the LDS) */
int cips3d_nerf_bwd_fused_supported(int hidden, int depth, int img_size, int n_samples);
int64_t cips3d_nerf_bwd_fused_stash_floats(int B, int img_size, int n_samples, int hidden, int depth, int n_chunks);
int64_t cips3d_nerf_bwd_fused_scratch_floats(int B, int img_size, int n_samples, int hidden, int depth);
/* the transposed weight stream of the backward kernel, in its consumption order (view layer first, then hidden layers
 * depth-1 .. 1), each matrix W_l^T packed like cips3d_nerf_pack_weights packs W_l and with W_l's power-of-two scale (read from
 * `packed`); packed_t holds cips3d_nerf_packed_floats(hidden, depth) floats */
int cips3d_nerf_pack_weights_t(const float* w_hidden, const float* w_view, const float* packed, float* packed_t, int hidden,
                               int depth, void* stream);
/* The fused backward.  dfocal [B] (out; cleared by the call) = d loss / d focals, from cips3d_nerf_bwd_camera at the end of the
 * call; NULL: none, and no launch or memset on its behalf.  (An argument, not a field: cips3d_nerf_bwd_fused_params is embedded
 * in the kernels' arguments and keeps its layout.) */
int cips3d_nerf_bwd_fused(const cips3d_nerf_bwd_fused_params* p, float* dfocal, void* stream);

/* Backward of cips3d_camera_params w.r.t. locations (azim, elev): dextrinsics [B,3,4] -> dlocations [B,2]
 * (cips3d/nerf_utils.py:344-436,466-564; focal / near / far do not depend on the angles). */
int cips3d_camera_params_bwd(const float* locations, const float* up, const float* dextrinsics, int B, float* dlocations,
                             void* stream);

/* Fresh noise of one forward in one launch: n_normal N(0,1) values (every NoiseInjection map, models/model_v3.py:334-336
 * `image.new_empty(batch, 1, height, width).normal_()`) and n_uniform U[0,1) values (the per-ray jitter, cips3d/nerf_utils.py:110
 * `torch.rand(B, h, w, 1)`).  The reference takes both from torch's global generator and pins no stream; this draws them from
 * Philox4x32-10 with key = seed and counter = (base + thread, 'CIPS', 0) -- csrc/rng.hip, restated in oracle/rng.py.  A call
 * consumes cips3d_rng_fill_threads(n_normal, n_uniform) counter values from `base` on; the caller advances its offset by that
 * (the Python binding keeps it in torch's generator state: seed = initial_seed(), base = get_offset()).  Either count may be 0.
 * cips3d_rng_words: the raw 4 x 32-bit words of threads 0 .. n_threads-1 (tests). */
int cips3d_rng_fill(uint64_t seed, uint64_t base, float* normal, int64_t n_normal, float* uniform, int64_t n_uniform,
                    void* stream);
int64_t cips3d_rng_fill_threads(int64_t n_normal, int64_t n_uniform);
int cips3d_rng_words(uint64_t seed, uint64_t base, uint32_t* out, int64_t n_threads, void* stream);

/* ------------------------------------------------------------------ geometry export (csrc/mesh.hip) */

/* Frustum alignment of a renderer SDF volume (cips3d/utils.py:183-203): volume, out [B,h,w,d].  With y_i, x_j, z_k =
 * linspace(-1, 1) over h, w, d and c_k = linspace(far / near, 1, d)[k] (torch's fp32 values, bit for bit):
 *   X = x_j c_k, Y = y_i c_k;  out[b,i,j,k] = 1 when X or Y lies outside [-1, 1], else volume[b] sampled trilinearly at
 *   row (Y+1)(h-1)/2, column (X+1)(w-1)/2, depth (z_k+1)(d-1)/2, each clamped to [0, n-1]
 *   (grid_sample(align_corners=True, padding_mode="border")).
 * far / near is formed in double and rounded to fp32, as the reference's Python quotient is. */
int cips3d_align_volume(const float* volume, float* out, int B, int h, int w, int d, double near_, double far_, void* stream);

/* Marching cubes on one volume A [h,w,d] (h, w, d >= 2) at `level`, in two calls on one stream:
 *   cips3d_marching_cubes_count writes totals[0] = V (vertices), totals[1] = F (triangles) to a device int32[2] and
 *   fills `workspace` (cips3d_marching_cubes_workspace_bytes(h, w, d) bytes); the caller reads the totals, allocates the
 *   outputs and calls cips3d_marching_cubes_emit with the same volume, level and workspace: verts [V,3] fp32, faces [F,3]
 *   int32 (max_verts / max_faces bound every store).
 * Contract:
 *   axes as the reference's sdf.permute(1, 0, 2): x <-> column j, y <-> row i, z <-> depth k;
 *   a point is inside when A < level (NaN: outside); one vertex per lattice edge whose ends disagree, shared by every cell
 *   on that edge, at a + t e_axis, t = (level - A_a) / (A_b - A_a), a = the edge's lower end; then per axis
 *   X = x * affine_host[0] + affine_host[1], Y = y * affine_host[2] + affine_host[3], Z = z * affine_host[4] + affine_host[5]
 *   (affine_host NULL: index space);
 *   vertices ordered by the lower end of their edge in memory order of A, then +x, +y, +z; triangles by their cell's lower
 *   corner in the same order, then in case-table order (cips3d_mc_case_table); bit-reproducible (prefix sums, no atomics);
 *   winding: in index space (and in any affine of positive determinant) (v1 - v0) x (v2 - v0) points towards larger values;
 *   a face whose corners form a checkerboard separates its inside corners, so neighbouring cells agree and a surface that
 *   stays off the border is a closed, oriented 2-manifold.
 * No crossing: V = F = 0.  CIPS3D_E_BADARG for a dimension below 2 or null pointers, CIPS3D_E_UNSUPP when the counts could
 * exceed int32 (the workspace query returns the same codes). */
int64_t cips3d_marching_cubes_workspace_bytes(int h, int w, int d);
int cips3d_marching_cubes_count(const float* volume, int h, int w, int d, float level, void* workspace, int32_t* totals,
                                void* stream);
int cips3d_marching_cubes_emit(const float* volume, int h, int w, int d, float level, const float* affine_host,
                               const void* workspace, float* verts, int32_t* faces, int max_verts, int max_faces,
                               void* stream);
/* Vertex normals of that mesh: normals [V,3] fp32 in cips3d_marching_cubes_emit's vertex order, after
 * cips3d_marching_cubes_count with the same volume, level and workspace (the emit call is not needed first; max_verts bounds
 * every store).  With G(p) the index-space gradient of A at lattice point p (central difference (A[p+1] - A[p-1]) / 2 in the
 * interior, one-sided at a border: numpy.gradient, edge_order = 1; x <-> column, y <-> row, z <-> depth), the vertex on edge
 * a -> b = a + e_axis with the emit kernel's t gets  g = (1 - t) G(a) + t G(b),  n_k = g_k / scale_k (the affine's scales
 * affine_host[0], [2], [4]; NULL: 1),  n = n / max(|n|, 1e-12).  The normal points towards larger values: for an affine of
 * positive determinant, the side the triangles' winding faces.  These are the grid normals of skimage's marching_cubes. */
int cips3d_marching_cubes_normals(const float* volume, int h, int w, int d, float level, const float* affine_host,
                                  const void* workspace, float* normals, int max_verts, void* stream);
/* The case table (tools/gen_mc_table.py), host only: corner c = x + 2y + 4z of a cell, case bit c = corner c inside; cube
 * edge e of axis e / 4 starts at corner (0, e&1, e>>1) for x-edges, (e&1, 0, e>>1) for y-edges, (e&1, e>>1, 0) for
 * z-edges (e &= 3).  tri_count_host [256]; tri_edges_host [256][3 * cips3d_mc_table_width()], -1 past the count. */
int cips3d_mc_table_width(void);
int cips3d_mc_case_table(int32_t* tri_count_host, int32_t* tri_edges_host);

/* ------------------------------------------------------------------ mesh rasteriser (csrc/mesh_raster.hip) */

/* Hard z-buffer rasterisation of a triangle mesh, verts [V,3] fp32, faces [F,3] int32, from n_views cameras into square
 * S x S frames: the nearest face per pixel, perspective-correct barycentrics, no blending, no culling by winding
 * (what the reference takes from pytorch3d: exp/cips3d/utils.py:260-308, models/model_v3.py:344-415, with
 * faces_per_pixel = 1 and no blur).
 * Camera: cams [n_views,5] fp32 on the device = (azim, elev [radians], fov_deg, dist, znear) per view -- the reference's
 * create_cameras (pytorch3d's look_at_view_transform + FoVPerspectiveCameras):
 *   C = dist (cos el sin az, sin el, cos el cos az);  z_ax = -C / |C|;  x_ax = normalize((0,1,0) x z_ax);  y_ax = z_ax x x_ax;
 *   p_v = ((p - C) . x_ax, (p - C) . y_ax, (p - C) . z_ax);  s = 1 / tan(fov / 2);  x_n = s p_v.x / p_v.z, y_n = s p_v.y / p_v.z
 *   (+x left, +y up); the centre of pixel (row i, column j) lies at x_n = 1 - (2j + 1) / S, y_n = 1 - (2i + 1) / S.
 * Coverage: a face covers a pixel when the three edge functions at the pixel centre are >= 0 after orienting by the sign
 * of the face's screen area (both windings are drawn).  A face of zero screen area is skipped.  A face with ANY vertex at
 * p_v.z < znear (or p_v.z <= 0) is dropped whole -- there is no clipping against the near plane; the product's mesh sits at
 * distance ~1 with znear = 0.01.  A face with a vertex id outside [0, V) is skipped.
 * Depth: view-space z with 1 / z = sum_k b_k / z_k (b: screen-space barycentrics); bary: w_k = (b_k / z_k) z.
 * Ordering: keys [n_views,S,S] uint64 = (fp32 bits of z) << 32 | face id, lowered with a 64-bit unsigned atomicMin; all ones
 * = empty.  z > 0, so the bits order like the depths; the minimum does not depend on arrival order: bit-reproducible,
 * independent of the grid, and equal depths go to the lower face id.
 *
 * cips3d_mesh_rasterize clears `keys` itself (part of the call), fills `workspace` (cips3d_mesh_raster_workspace_bytes: the
 * derived cameras and the projected vertices) and `keys`.  cips3d_mesh_resolve, on the same stream with the same verts,
 * faces, workspace, keys and sizes, decodes the winners; every output may be NULL:
 *   face [n,S,S] int32, zbuf [n,S,S] fp32, bary [n,S,S,3] fp32: -1 where empty;
 *   attr_out [n,n_attr,S,S] = sum_k w_k attr[v_k,:] (attr [V,n_attr]); an empty pixel takes the same pixel of `base`
 *   [n,n_attr,S,S] when given (base may be attr_out itself), else `fill`;
 *   shade [n,S,S] fp32, shade_u8 [n,3,S,S] (three equal channels, floor(255 clamp(shade, 0, 1) + 0.5)): cips3d_nerf_normals'
 *   Phong with n = normalize(sum_k w_k normals[v_k]), p = sum_k w_k verts[v_k], eye = C, light [n,3]; empty pixels are
 *   white (1.0 / 255).
 * Neither call synchronises.  CIPS3D_E_BADARG, nothing launched: a null required pointer, a negative size, S < 1, attr_out
 * without attr or n_attr < 1, a shade output without normals / light.  CIPS3D_E_UNSUPP: V or F > INT32_MAX, S > 16384,
 * n_views > 65536 (the workspace query returns the same codes). */
typedef struct cips3d_mesh_resolve_params {
  const float* verts; const int32_t* faces; const void* workspace; const uint64_t* keys;
  int32_t* face; float* zbuf; float* bary;
  const float* attr; const float* base; float* attr_out;
  const float* normals; const float* light; float* shade; uint8_t* shade_u8;
  int32_t V, F, n_views, S, n_attr;
  float fill, ka, kd, ks, shininess;
} cips3d_mesh_resolve_params;
int64_t cips3d_mesh_raster_workspace_bytes(int64_t V, int64_t F, int n_views, int S);
int cips3d_mesh_rasterize(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* cams, int n_views,
                          int S, void* workspace, uint64_t* keys, void* stream);
int cips3d_mesh_resolve(const cips3d_mesh_resolve_params* p, void* stream);

/* ------------------------------------------------------------------ mesh vertex colours (csrc/mesh_color.hip) */

/* Colours the mesh's vertices from n_views pictures of it: images [n_views,3,R,R] fp32, picture k taken by camera k of the
 * rasterisation (R is independent of S).  Called after cips3d_mesh_rasterize on the same stream with the same verts, workspace,
 * keys, n_views and S: it reads the rasteriser's projected vertices (x_p, y_p, z, 1/z), derived cameras and keys, so that
 * visibility is the z-buffer's own and nothing is projected twice (a rasterisation with F = 0 projects nothing: its
 * workspace must not be handed to this call).  normals [V,3]: unit, outward.  One thread per vertex,
 * views in ascending order, no atomics: the result does not depend on the grid and is bit-reproducible.  Per vertex p and view k:
 *   skipped when 1/z <= 0 (the rasteriser dropped the vertex behind znear);
 *   j = rintf(x_p), i = rintf(y_p); off the S x S frame: not seen;
 *   z* = the depth of keys[k,i,j], +inf for an empty pixel;  visible = z <= z* + depth_tol;
 *   d = (C_k - p) / max(|C_k - p|, 1e-12);  c = (n.x d.x + n.y d.y) + n.z d.z;  faces = visible && c > 0;
 *   w = faces ? c^power : 0, the power by repeated multiplication (w = c; w *= c, power - 1 times);
 *   w > 0: rgb = the bilinear sample of images[k] at u = (x_p + 1/2) R / S - 1/2, v = (y_p + 1/2) R / S - 1/2 (the rasteriser's
 *   pixel-centre convention carried to R), u and v clamped to [0, R - 1]: x0 = floor(u), x1 = min(x0 + 1, R - 1), fx = u - x0,
 *   row = (1 - fx) a + fx b, value = (1 - fy) top + fy bottom;  acc += w rgb, wsum += w;  seen += faces.
 * Outputs (each may be NULL, at least one is required): colors [V,3] = acc / wsum, or `fill` where wsum == 0; weight [V] = wsum;
 * seen [V] int32.  Does not synchronise.  CIPS3D_E_BADARG, nothing launched: a null required pointer, no output, a negative
 * size, S < 1, R < 1, power outside 1..8.  CIPS3D_E_UNSUPP: V > INT32_MAX, S > 16384, n_views > 65536 (the rasteriser's
 * limits), R > 16384. */
typedef struct cips3d_mesh_color_params {
  const float* verts; const float* normals; const float* images; const void* workspace; const uint64_t* keys;
  float* colors; float* weight; int32_t* seen;
  int32_t V, n_views, S, R, power;
  float depth_tol, fill;
  int32_t pad_;
} cips3d_mesh_color_params;
int cips3d_mesh_vertex_colors(const cips3d_mesh_color_params* p, void* stream);

/* The coloured mesh frame from cips3d_mesh_resolve's maps: face [n,S,S] int32, shade [n,S,S], attr [n,3,S,S] (the interpolated
 * vertex colours, in [-1, 1]) -> out [n,3,S,S] uint8 = floor(255 clamp(shade (attr + 1) / 2, 0, 1) + 0.5), 255 where
 * face < 0.  CIPS3D_E_BADARG: a null pointer, n_views < 0, S < 1.  CIPS3D_E_UNSUPP: S > 16384, n_views > 65536. */
int cips3d_mesh_albedo_frame(const int32_t* face, const float* shade, const float* attr, uint8_t* out, int n_views, int S,
                             void* stream);

/* ------------------------------------------------------------------ mesh texture atlas (csrc/mesh_texture.hip) */

/* Atlas layout (csrc/mesh_texture.h; pure arithmetic, no unwrap).  T = texels, 3 <= T <= 64, m = T - 2.  Faces 2c and 2c + 1
 * share cell c, (T + 1) x T texels at cell column c % cols, cell row c / cols; cells = ceil(F / 2); cols defaults to the
 * smallest integer with cols^2 (T + 1) >= cells T (= max(1, ceil(sqrt(cells T / (T + 1))))); rows = ceil(cells / cols);
 * Wt = cols (T + 1), Ht = rows T, both <= 16384.  A texel at local (i, j) of its cell, d = i + j:
 *   d <= m: face 2c, owned, lattice (li, lj) = (i, j);            d == m + 1: face 2c, gutter, (i - 1/2, j - 1/2);
 *   d == m + 2: face 2c + 1, gutter, (i' - 1/2, j' - 1/2);        d >= m + 3: face 2c + 1, owned, (i', j');   i' = T - i, j' = T - 1 - j.
 * A texel whose face is >= F is unowned.  Barycentrics of a texel: b1 = clamp(li / m, 0, 1), b2 = clamp(lj / m, 0, 1),
 * b0 = max(0, (1 - b1) - b2).  Every face has T (T - 1) / 2 owned and T gutter texels.  Corner UVs in continuous texel
 * coordinates (the centre of texel k is k + 1/2; (ox, oy) the cell's origin): face 2c: (ox + 1/2, oy + 1/2), (ox + 1/2 + m, oy + 1/2),
 * (ox + 1/2, oy + 1/2 + m); face 2c + 1: (ox + T + 1/2, oy + T - 1/2), (ox + T + 1/2 - m, oy + T - 1/2), (ox + T + 1/2, oy + T - 1/2 - m).
 * A bilinear fetch at a point inside a face's UV triangle touches, with non-zero weight, only that face's owned and gutter texels.
 * The three calls below run on the host: the layout for F faces (cols_in = 0: the default), uv_host [F,3,2], and the texel
 * maps face_host [Ht,Wt] int32 (-1: unowned), bary_host [Ht,Wt,3], gutter_host [Ht,Wt] (each may be NULL).
 * CIPS3D_E_BADARG: T outside 3..64, a negative size, a null required pointer, cols x rows cells that do not hold F faces;
 * CIPS3D_E_UNSUPP: Wt or Ht > 16384, F > INT32_MAX. */
int cips3d_mesh_atlas_layout(int64_t F, int T, int cols_in, int32_t* cols, int32_t* rows, int32_t* width, int32_t* height);
int cips3d_mesh_atlas_uv(int64_t F, int T, int cols, float* uv_host);
int cips3d_mesh_atlas_texels(int64_t F, int T, int cols, int rows, int32_t* face_host, float* bary_host, uint8_t* gutter_host);

/* Grows colours from the vertices some view saw into those none saw, ring by ring.  colors [V,3], weight [V] (of
 * cips3d_mesh_vertex_colors), faces [F,3] -> colors_out [V,3] (not `colors` itself), filled [V] int32.  Initially
 * filled[v] = weight[v] > 0 ? 0 : -1.  For ring r = 1..iters (0 <= iters <= 4096) and every vertex a unfilled at the start of the
 * ring: S_a = sum of q(col[b]), q(x) = (int64) rintf(x 2^20) per channel, over all (face containing a, other corner b of it) pairs
 * whose b was filled before ring r; n_a = the number of such pairs; n_a > 0: col[a] = (float) ((double) S_a / ((double) n_a 1048576.0)),
 * filled[a] = r.  Seen vertices keep their bits; a vertex no ring reaches keeps its input colour and -1.  The sums are 64-bit
 * integer atomic adds: exact, independent of order and grid.  workspace: cips3d_mesh_fill_workspace_bytes(V) bytes, cleared by
 * the call.  All rings are enqueued at once (2 launches each); after a ring that filled nothing the remaining launches return on
 * a device flag.  Does not synchronise.  A face with a vertex id outside [0, V) is skipped.
 * CIPS3D_E_BADARG, nothing launched: a null pointer, a negative size, iters outside 0..4096, colors_out == colors.
 * CIPS3D_E_UNSUPP: V or F > INT32_MAX.  V == 0 or F == 0: returns 0, launches nothing, writes nothing. */
int64_t cips3d_mesh_fill_workspace_bytes(int64_t V);
int cips3d_mesh_fill_colors(const float* colors, const float* weight, const int32_t* faces, int64_t V, int64_t F, int iters,
                            float* colors_out, int32_t* filled, void* workspace, void* stream);

/* Bakes the atlas from n_views pictures of the mesh.  Called after cips3d_mesh_rasterize on the same stream with the same verts,
 * faces, workspace, keys, n_views and S (images, normals, R, depth_tol, power, fill: as cips3d_mesh_vertex_colors).  One thread
 * per atlas texel, views in ascending order, no atomics: independent of the grid, bit-reproducible.
 *   unowned texel (or a face with a vertex id outside [0, V)): `fill`, weight 0, seen 0;
 *   p = (b0 v0 + b1 v1) + b2 v2 per component; n = the same combination of the corners' normals, divided by max(|n|, 1e-12);
 *   per view: p is projected with the rasteriser's vertex arithmetic (derived camera of the workspace; x_p, y_p, z; dropped when
 *   z < znear or z <= 0), and from there cips3d_mesh_vertex_colors' contract holds word for word (pixel rint, off-frame, z* of
 *   the key, z <= z* + depth_tol, c = n . d > 0, w = c^power, bilinear sample at u = (x_p + 1/2) R / S - 1/2);
 *   texel = acc / wsum; where wsum == 0: (b0 c0 + b1 c1) + b2 c2 of vertex_colors [V,3] when vertex_colors and filled [V]
 *   (cips3d_mesh_fill_colors) are given and the three corners have filled >= 0, else `fill`.
 * Outputs (each may be NULL, at least one is required): texture [3,Ht,Wt] fp32, weight [Ht,Wt] fp32, seen [Ht,Wt] int32.
 * Does not synchronise.  CIPS3D_E_BADARG, nothing launched: a null required pointer, no output, vertex_colors without filled or
 * the reverse, a negative size, S < 1, R < 1, power outside 1..8, T outside 3..64, cols x rows cells that do not hold F faces.
 * CIPS3D_E_UNSUPP: the rasteriser's limits, R > 16384, Wt or Ht > 16384.  V == 0 or F == 0: returns 0, launches nothing. */
typedef struct cips3d_mesh_texture_params {
  const float* verts; const int32_t* faces; const float* normals; const float* images; const void* workspace; const uint64_t* keys;
  const float* vertex_colors; const int32_t* filled;
  float* texture; float* weight; int32_t* seen;
  int32_t V, F, n_views, S, R, power, T, cols, rows;
  float depth_tol, fill;
  int32_t pad_;
} cips3d_mesh_texture_params;
int cips3d_mesh_texture_bake(const cips3d_mesh_texture_params* p, void* stream);

/* The coloured mesh frame at texture resolution, from cips3d_mesh_resolve's maps face [n,S,S] int32, bary [n,S,S,3], shade [n,S,S]
 * and texture [3,Ht,Wt] of an atlas (T, cols, rows) for F faces -> out [n,3,S,S] uint8.  A hit pixel (0 <= face < F):
 * b1 = clamp(w1, 0, 1), b2 = clamp(w2, 0, 1 - b1); the point b0 uv0 + b1 uv1 + b2 uv2 of the face's corner UVs is fetched
 * bilinearly at (x - 1/2, y - 1/2).  In the face's lattice that point is (fx, fy) = (b1 m, min(b2 m, fl(m - fx))), its taps are
 * the lattice texels (floor(fx) + {0,1}, floor(fy) + {0,1}) with weights (1 - frac, frac): all of them inside the face's cell,
 * and those of non-zero weight among the face's own owned and gutter texels.  c = (1 - wy) ((1 - wx) t00 + wx t10) +
 * wy ((1 - wx) t01 + wx t11);  out = floor(255 clamp(shade (c + 1) / 2, 0, 1) + 0.5); every other pixel is 255 (the albedo
 * frame's formula and background).  CIPS3D_E_BADARG: a null pointer, a negative size, S < 1, a bad atlas; CIPS3D_E_UNSUPP:
 * S > 16384, n_views > 65536, Wt or Ht > 16384.  n_views == 0 or F == 0: returns 0, launches nothing. */
int cips3d_mesh_textured_frame(const int32_t* face, const float* bary, const float* shade, const float* texture, uint8_t* out,
                               int n_views, int S, int64_t F, int T, int cols, int rows, void* stream);

/* VGG16 conv perceptual loss of flip inversion (csrc/vgg.hip; reference exp/cips3d/models/vgg_per_loss.py:203-334,
 * models/projector_v10.py:131-151, 1170-1174).  The network is the 13 convolutions of torchvision's vgg16.features
 * (conv l = features.{0,2,5,7,10,12,14,17,19,21,24,26,28}[l]; widths cips3d_vgg_channels(l); a 2x2/2 max-pool in front of
 * convs 2, 4, 7, 10: cips3d_vgg_stride(l) = 1, 1, 2, 2, 4, 4, 4, 8, ...), ReLU between them, frozen weights shared by the
 * batch.  Every tensor is NCHW fp32.  A "tap" is the PRE-ReLU output of a conv.
 *
 *   loss = sum over tap layers l of tap_w[l]^2 * sum (z_l - target[l])^2            (batch and map summed)
 *
 * Size contract (cips3d_vgg_supported: 0, CIPS3D_E_UNSUPP or CIPS3D_E_BADARG, decided on the host, nothing launched):
 * B >= 1; H and W multiples of 16 (>= 16, not necessarily equal); H W <= 2^24.
 *
 * cips3d_vgg_pack       weights[l] = conv l's [Cout,Cin,3,3] device tensor -> ctx->w_fwd[l] (the MFMA fragment order) and
 *                       ctx->w_bwd[l] (transposed and rotated 180 degrees, same order: the data gradient's operand), 9 Cout Cin
 *                       floats each; conv 0 is copied as it is into w_fwd[0] (1728 floats, w_bwd[0] unused).  Once per network.
 * cips3d_vgg_features   convs 0 .. n_convs - 1: io->z[l] [B,C_l,H_l,W_l] (pre-ReLU) and io->pooled[k] (max-pool of relu(z)
 *                       in front of conv {2,4,7,10}[k]).  normalize != 0: x is in [-1, 1] and conv 0 applies
 *                       ((x + 1) / 2 - mean) / std (ImageNet) first; 0: x is already normalised.
 * cips3d_vgg_loss_forward   the same, then loss[0] as above over the layers with target[l] != NULL (conv n_convs - 1 must be
 *                       one).  Deterministic: fp64 partial sums per workgroup, added in a fixed order (partial:
 *                       cips3d_vgg_partial_bytes() of scratch).
 * cips3d_vgg_loss_backward  dx [B,3,H,W] = gloss[0] * d loss / d x from the z of the forward call (the only tensors kept), the
 *                       targets and two gradient buffers g[0], g[1] of B * 64 * H * W floats each.
 * None of the calls synchronises.  CIPS3D_E_BADARG: a null ctx / io / required pointer, n_convs outside [1, 13]. */
#define CIPS3D_VGG_CONVS 13
typedef struct cips3d_vgg_ctx {
  float* w_fwd[CIPS3D_VGG_CONVS];
  float* w_bwd[CIPS3D_VGG_CONVS];
  const float* bias[CIPS3D_VGG_CONVS];
} cips3d_vgg_ctx;
typedef struct cips3d_vgg_io {
  const float* x;                            /* [B,3,H,W] */
  int32_t B, H, W, n_convs;
  int32_t normalize, pad_;
  float* z[CIPS3D_VGG_CONVS];
  float* pooled[4];
  const float* target[CIPS3D_VGG_CONVS];     /* NULL: conv l is not a tap */
  float tap_w[CIPS3D_VGG_CONVS];
  int32_t pad2_;
  void* partial;
  float* loss;                               /* [1] */
  const float* gloss;                        /* [1]: the loss' incoming gradient */
  float* g[2];
  float* dx;
} cips3d_vgg_io;
int cips3d_vgg_supported(int B, int H, int W);
int cips3d_vgg_channels(int conv);
int cips3d_vgg_stride(int conv);
int64_t cips3d_vgg_partial_bytes(void);
int cips3d_vgg_pack(const cips3d_vgg_ctx* ctx, const float* const* weights, int n_convs, void* stream);
int cips3d_vgg_features(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream);
int cips3d_vgg_loss_forward(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream);
int cips3d_vgg_loss_backward(const cips3d_vgg_ctx* ctx, const cips3d_vgg_io* io, void* stream);

/* The same loss with convs 1 .. 12 and their data gradients on split-fp16 products (csrc/vgg_split.hip): w x = w_lo x_hi +
 * w_hi x_lo + w_hi x_hi on v_mfma_f32_16x16x32_f16 with fp32 accumulation -- fp32-accurate, not bit-equal to the exact form
 * above.  Same network, tensors, size contract, return codes and call pattern; conv 0, the pools and the tap loss are the same
 * kernels.
 *
 * cips3d_vgg_split_pack    w_fwd[l] / w_bwd[l] (l >= 1): [M/16][K/32][tap][hi | lo][lane][8 fp16] of w 2^-e_l, 36 Cout Cin bytes
 *                       each (lane 16 q + i, element j: forward form w[16 mt + i][32 ks + 8 q + j][tap]; data-gradient form
 *                       w[32 ks + 8 q + j][16 mt + i][8 - tap]).  e_l puts max|w_l| 2^-e_l in [2^14, 2^15); the maximum is found
 *                       on the device and kept as its bit pattern in w_amax[l] (CIPS3D_VGG_CONVS words).  w_fwd[0]: conv 0 as it
 *                       is (1728 floats).
 * range                 cips3d_vgg_split_range_bytes(B) of scratch, zeroed by the calls themselves: one word per (tensor,
 *                       sample) holding the bit pattern of max|.|, from which each sample's operand gets its own power of two.
 *                       The backward call reads the words the forward call of the same io left.
 * Determinism: no float atomics (the range words are raised with integer maxima); a B = 2 call equals two B = 1 calls. */
typedef struct cips3d_vgg_split_ctx {
  void* w_fwd[CIPS3D_VGG_CONVS];
  void* w_bwd[CIPS3D_VGG_CONVS];
  const float* bias[CIPS3D_VGG_CONVS];
  uint32_t* w_amax;                          /* [CIPS3D_VGG_CONVS] */
} cips3d_vgg_split_ctx;
typedef struct cips3d_vgg_split_io {
  cips3d_vgg_io io;
  void* range;                               /* cips3d_vgg_split_range_bytes(io.B) */
} cips3d_vgg_split_io;
int cips3d_vgg_split_supported(int B, int H, int W);
int64_t cips3d_vgg_split_range_bytes(int B);
int cips3d_vgg_split_pack(const cips3d_vgg_split_ctx* ctx, const float* const* weights, int n_convs, void* stream);
int cips3d_vgg_split_features(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* io, void* stream);
int cips3d_vgg_split_loss_forward(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* io, void* stream);
int cips3d_vgg_split_loss_backward(const cips3d_vgg_split_ctx* ctx, const cips3d_vgg_split_io* io, void* stream);

/* PSNR and SSIM of image pairs on the device (csrc/metrics.hip): scikit-image's peak_signal_noise_ratio and
 * structural_similarity at their defaults on 8-bit images (data range 255; win_size 7, uniform window, K1 = 0.01, K2 = 0.03,
 * sample covariance), which is what the reference's project_wplus logs (models/projector_v10.py:1125-1139, 1266-1279).
 *
 * a, b [B,C,H,W], each either uint8 (x_is_u8 != 0) or fp32 in [-1, 1] (quantised on load with cips3d_rgb_to_uint8's arithmetic:
 * clamp, (c + 1) * 127.5, round to nearest even; no uint8 copy is written).  For image i the call writes two 64-bit words into
 * row `row + i` of `record` (rows of 16 bytes):
 *     int64   SSE   the sum of squared differences over all channels and pixels (PSNR = 10 log10(255^2 C H W / SSE))
 *     float64 SSIM  the mean over the C (H - 6) (W - 6) windows that lie inside the image
 * Two launches on `stream`, no synchronisation, no atomics: the sums run in a fixed order (integers for the squared error and
 * the window moments, fp32 inside a tile, fp64 across tiles), so a result is bit-identical run to run and does not depend on
 * the batch the image sits in.  `workspace`: cips3d_image_metrics_workspace_bytes(B, C, H, W) bytes, 16-byte aligned, free
 * again once the stream has passed the call.  cips3d_image_metrics_tile: the sides of a workgroup's tile of window origins
 * (returns the threads per workgroup; a thread adds tile_h * tile_w / threads windows in sequence).
 * CIPS3D_E_BADARG: a null pointer, B or C < 1, H or W < 7, row < 0; CIPS3D_E_UNSUPP: a misaligned pointer. */
int cips3d_image_metrics(const void* a, int a_is_u8, const void* b, int b_is_u8, int B, int C, int H, int W, void* workspace,
                         void* record, int64_t row, void* stream);
int64_t cips3d_image_metrics_workspace_bytes(int B, int C, int H, int W);
int cips3d_image_metrics_tile(int* tile_h, int* tile_w);

/* LPIPS v0.1, net = 'vgg', spatial = False, on the device (csrc/lpips.hip): the VGG16 trunk above plus a head on the taps
 * BEHIND the ReLUs of convs 1, 3, 6, 9, 12 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; C_k = 64, 128, 256, 512, 512).  For
 * images a, b in [-1, 1] (io.normalize = 1 is LPIPS's own scaling layer: 2 mean - 1 = shift, 2 std = scale), per layer k:
 *     f = relu(z);  n(p) = sqrt(sum_c f[c,p]^2) + 1e-10;  d_k(p) = sum_c lin_k[c] (fa[c,p] / na(p) - fb[c,p] / nb(p))^2
 * layer value = mean_p d_k(p), LPIPS = the sum of the five.  Two passes over the channels (norms, then differences), fp32 per
 * pixel, fp64 across pixels through per-workgroup partial sums added in a fixed order: no atomics, bit-identical run to run,
 * independent of the batch a sample sits in, exactly 0 for identical inputs, symmetric in (a, b) bit for bit.
 *
 * cips3d_lpips_head     one layer on given maps: za, zb [B,C,H,W] PRE-ReLU (the ReLU is applied on load), lin [C], C in {64,
 *                       128, 256, 512}, any H, W >= 1 -> map [B,1,H,W] (optional) and mean [B] (fp64).  Two launches.
 * cips3d_lpips          the whole metric: the trunk of `io->trunk` (a cips3d_vgg_io with n_convs = 13; for cips3d_lpips_split
 *                       a cips3d_vgg_split_io) and then five heads and one finalising launch.  target[k] all NULL: the trunk's
 *                       batch is 2 B, images a (samples 0 .. B - 1) then b.  target[k] all given: the trunk's batch is B and
 *                       target[k] holds b's pre-ReLU maps of conv 1, 3, 6, 9, 12 from an earlier trunk call ([B,C_k,H_k,W_k], or
 *                       [1,C_k,H_k,W_k] for every sample with target_broadcast != 0); both forms give the same bits.  Sample i
 *                       writes row `row + i` of `record`, rows of 6 float64: {LPIPS, layer 0 .. 4}.  map[k]: optional
 *                       [B,1,H_k,W_k] distance maps.  partial: cips3d_lpips_partial_bytes(B) of scratch (the partial sums are
 *                       keyed by sample: 80 KB each).  heads_only != 0: the trunk is not run, its z[1, 3, 6, 9, 12] are read as
 *                       an earlier call left them (timing the head, re-weighting with other lin vectors).
 * Nothing allocates or synchronises.  CIPS3D_E_BADARG, nothing launched: a null required pointer, B < 1, C outside the list, row
 * < 0, a trunk io whose n_convs or batch does not fit, some but not all targets.  CIPS3D_E_UNSUPP: outside
 * cips3d_lpips_supported (the trunk's contract: H, W multiples of 16; B <= 32767), or H W >= 2^31 - 64 / B > 65535 for the head. */
#define CIPS3D_LPIPS_LAYERS 5
typedef struct cips3d_lpips_io {
  const void* trunk;                         /* cips3d_vgg_io (cips3d_lpips) / cips3d_vgg_split_io (cips3d_lpips_split) */
  const float* lin[CIPS3D_LPIPS_LAYERS];     /* [C_k] */
  const float* target[CIPS3D_LPIPS_LAYERS];  /* all NULL: the pair form */
  float* map[CIPS3D_LPIPS_LAYERS];           /* NULL: no map of layer k */
  void* partial;
  void* record;                              /* rows of 6 float64 */
  int64_t row;
  int32_t B, target_broadcast;
  int32_t heads_only, pad_;                  /* heads_only != 0: trunk->z already holds the maps; the six head launches alone */
} cips3d_lpips_io;
int cips3d_lpips_supported(int B, int H, int W);
int64_t cips3d_lpips_partial_bytes(int B);
int cips3d_lpips_head(const float* za, const float* zb, const float* lin, int B, int C, int H, int W, float* map, void* partial,
                      double* mean, void* stream);
int cips3d_lpips(const cips3d_vgg_ctx* ctx, const cips3d_lpips_io* io, void* stream);
int cips3d_lpips_split(const cips3d_vgg_split_ctx* ctx, const cips3d_lpips_io* io, void* stream);

/* Gaussian-window SSIM of fp32 image pairs as a differentiable loss (csrc/ssim_loss.hip): Wang et al. 2004, which is scikit-image's
 * structural_similarity(gaussian_weights = True, sigma = 1.5, use_sample_covariance = False, data_range = R).  a, b [B,C,H,W]
 * fp32, continuous values, nothing quantised or clamped.  The window is g (x) g with 11 taps g[i] ~ exp(-(i - 5)^2 / 4.5), sum
 * g = 1; only the (H - 10) (W - 10) windows per channel that lie wholly inside the image count.  Per window, with E the weighted
 * mean: mux, muy, vx = E[x^2] - mux^2, vy, vxy = E[xy] - mux muy, C1 = (0.01 R)^2, C2 = (0.03 R)^2,
 *     S = (2 mux muy + C1) (2 vxy + C2) / ((mux^2 + muy^2 + C1) (vx + vy + C2)),
 * ssim[i] = the mean of S over image i's C (H - 10) (W - 10) windows, loss = weight * mean_i (1 - ssim[i]).
 *
 * The moments are taken of x - cx, y - cy with cx, cy the first pixel of the workgroup's tile in each image -- pixel (tile_y *
 * tile_h, tile_x * tile_w) of the plane, the tile being the one that holds the window's origin: variances and the covariance
 * are shift-invariant, only the means add the constant back, and E[x^2] - mux^2 no longer cancels on a bright flat region (a
 * flat image has vx = vy = vxy = 0 exactly).  Equal images give S = 1, ssim = 1 and loss = 0 exactly.
 *
 * cips3d_ssim_loss        two launches: one workgroup per (image, channel, tile of tile_h x tile_w window origins) writes one
 *                         fp32 partial (the windows added in a fixed order: tile_h * tile_w / threads in the thread, the wave's
 *                         butterfly, the waves), then one workgroup adds each image's partials in fp64 in a fixed order ->
 *                         ssim [B] (fp64, optional) and loss (fp32 scalar, optional; at least one of the two).  No atomics: the
 *                         results are bit-identical run to run, and ssim[i] does not depend on the batch.  map: optional
 *                         [B,C,H-10,W-10], receives S.  need_grad != 0: the forward also stores the three per-window maps
 *                         the backward reads, [B,C,H-10,W-10] fp32 each, behind the partials in `workspace`:
 *                             D2 = dS/dvx = -S / B2,  D3 = dS/dvxy = 2 A1 / (B1 B2),  D1 = dS/dmux - 2 (mux - kx) D2 - (muy - ky) D3
 *                         (A1, B1, B2: the factors of S in the order written above; dS/dmux = (2 / B1) (muy A2 / B2 - mux S)),
 *                         i.e. dS/dmux with E[x^2], E[xy] held fixed, for the images shifted by kx, ky = the first pixel of
 *                         the plane (image, channel) of a and b -- a(p) - mux cancels the way the variance does.
 * cips3d_ssim_loss_bwd    one launch, one workgroup per (image, channel, tile of tile_h x tile_w pixels):
 *                             da(p) = coef gloss[0] sum_{w holds p} g(x)g(p - w) (D1(w) + 2 (a(p) - kx) D2(w) + (b(p) - ky) D3(w)),
 *                         coef = -weight / (B C (H - 10) (W - 10)): the transposed ("full") convolution of the three maps,
 *                         zero outside the valid origins.  gloss: the upstream gradient, a device scalar (never read on the
 *                         host).  `workspace`, a, b, the shape and weight: as the forward call with need_grad != 0 left / had
 *                         them.  There is no gradient with respect to b.
 * `workspace`: cips3d_ssim_loss_workspace_bytes(B, C, H, W, need_grad) bytes, 16-byte aligned (3 x 4 bytes per window with
 * need_grad: 37 MB per 1024^2 RGB image).  cips3d_ssim_loss_tile: the tile's sides; returns the threads per workgroup.
 * CIPS3D_E_BADARG, nothing launched: a null required pointer, B or C < 1, H or W < 11, data_range <= 0, a grid beyond 2^31 - 1
 * workgroups (workspace_bytes returns it as a negative size).  CIPS3D_E_UNSUPP: a misaligned workspace or ssim pointer. */
int cips3d_ssim_loss_tile(int* tile_h, int* tile_w);
int64_t cips3d_ssim_loss_workspace_bytes(int B, int C, int H, int W, int need_grad);
int cips3d_ssim_loss(const float* a, const float* b, int B, int C, int H, int W, float weight, float data_range, void* workspace,
                     int need_grad, float* map, double* ssim, float* loss, void* stream);
int cips3d_ssim_loss_bwd(const float* a, const float* b, int B, int C, int H, int W, float weight, const void* workspace,
                         const float* gloss, float* da, void* stream);

/* ------------------------------------------------------------------ frame panels: Pillow's 8-bit resampling (csrc/frame_resample.hip)
 * PIL.Image.resize((ow, oh), BOX | BILINEAR | BICUBIC | LANCZOS) (default box, reducing_gap=None) of every channel of planar 8-bit
 * images, bit for bit: what the reference's demo pages do to each frame's thumbnail and geometry picture on the host before they
 * paste the panel (render_video_web_v10.py:1825-1890), and `load_pil_crop_resize` to an inversion's target.
 *
 * The caller makes the tables on the host in float64 (cips_3dplusplus_amd/frames.py: resample_coeffs; Pillow's precompute_coeffs
 * and normalize_coeffs_8bpc) and keeps them on the device.  Per axis of input size I and output size O:
 *     bounds [O][2] int32   (xmin, n) of output index xx: its taps are input indices xmin .. xmin + n - 1, xmin + n <= I, both
 *                           ends non-decreasing in xx
 *     coeffs [O][ksize] int32   k = round(w 2^22) of the n normalised weights, zero behind them; ksize = 2 ceil(support) + 1
 * and the kernels compute  clamp((2^21 + sum_x p[xmin + x] k_x) >> 22, 0, 255)  in 32-bit integers, the horizontal pass first,
 * its uint8 result the input of the vertical pass.  An axis whose size does not change is not filtered: ksize 0 and null
 * tables for it, and only for it (CIPS3D_E_BADARG otherwise).
 *
 * src [n][C][H][W] uint8, or fp32 in [-1, 1] with src_is_f32 != 0 (quantised on load with cips3d_rgb_to_uint8's arithmetic; no
 * uint8 copy is written), with its row, channel and image pitch in ELEMENTS (unit pitch in W); dst [n][C][oh][ow] uint8 with
 * its own three pitches in bytes: a result can land in one cell of a panel block or in a slice of a frame block, and only the
 * oh x ow bytes of each plane are written.  Dword loads / stores are used where the pointer and the three pitches are
 * multiples of 4, byte accesses otherwise and at a row's ragged end.
 *
 * Routes (cips3d_resample_route: decided on the host from the shape alone, nothing launched):
 *     FUSED        both axes change and what an output tile of tile_h x tile_w reaches -- at most max_stage_rows input rows, and
 *                  with their columns, the intermediate rows and the tile's tables at most 160 KB -- is staged in LDS: one
 *                  launch, the intermediate picture never goes to memory
 *     TWO_LAUNCH   the rest (strong down-scaling; an axis that does not change): horizontal into `workspace`, vertical from
 *                  there; the pass of an unchanged axis is skipped, the other one then writes dst itself and no workspace is
 *                  needed (neither changes: the unfiltered path of the horizontal kernel copies / quantises)
 * `route`: CIPS3D_RESAMPLE_AUTO, or the shape's own route, or TWO_LAUNCH for a FUSED shape (the same bytes; CIPS3D_E_UNSUPP
 * for any other request).  `workspace`: cips3d_resample_workspace_bytes(...) bytes (0 unless TWO_LAUNCH), 4-byte aligned,
 * free again once the stream has passed the call.  Grids never exceed 65535 workgroups: the kernels loop.
 * cips3d_resample_tile returns the threads per workgroup.  Nothing synchronises.  n C == 0: returns 0, launches nothing.
 * CIPS3D_E_BADARG, nothing launched: a null required pointer, a size < 1, a row pitch below the row, a negative pitch, a
 * workspace too small; CIPS3D_E_UNSUPP: n C > INT32_MAX, a misaligned fp32 source or workspace. */
#define CIPS3D_RESAMPLE_AUTO       0
#define CIPS3D_RESAMPLE_FUSED      1
#define CIPS3D_RESAMPLE_TWO_LAUNCH 2
int cips3d_resample_tile(int* tile_h, int* tile_w, int* max_stage_rows);
int cips3d_resample_route(int H, int W, int oh, int ow, int ksize_x, int ksize_y);
int64_t cips3d_resample_workspace_bytes(int n, int C, int H, int W, int oh, int ow, int ksize_x, int ksize_y, int route);
int cips3d_resample_u8(const void* src, int n, int C, int H, int W, int64_t src_row_pitch, int64_t src_channel_pitch,
                       int64_t src_image_pitch, uint8_t* dst, int oh, int ow, int64_t dst_row_pitch, int64_t dst_channel_pitch,
                       int64_t dst_image_pitch, const int32_t* bounds_x, const int32_t* coeffs_x, int ksize_x,
                       const int32_t* bounds_y, const int32_t* coeffs_y, int ksize_y, int src_is_f32, void* workspace,
                       int64_t workspace_bytes, int route, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIPS3D_HIP_H */
