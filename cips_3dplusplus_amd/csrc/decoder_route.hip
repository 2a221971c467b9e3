// The decoder's route: which launch form every layer of cips3d_generator_forward takes.  Host-only: no kernel, no launch, no HIP
// call -- arithmetic on the layer list and the shape predicates of the kernels, so a machine without a GPU can run (and test) it.
//
// Two functions share the predicates below.  cips3d_decoder_route_flags decides, when a plan is built, what every layer's
// weights are packed for (cips3d_dec_layer.flags); cips3d_decoder_steps turns flagged layers into the list of launches, per
// forward call, and refuses flags that promise a launch these layers cannot take.  forward.hip only enqueues that list.
#include "decoder_route.h"

namespace {

typedef cips3d_dec_layer Layer;

// [layers[i], StyledConv, ToRGB] of equal widths: the shape of a fused stage
bool same_widths(const Layer* l, int n, int i) {
  if (i + 2 >= n) return false;
  const int C = l[i].Cout;
  return l[i + 1].kind == 0 && l[i + 1].Cin == C && l[i + 1].Cout == C && l[i + 2].Cin == C;
}

// An up-sampling stage [StyledConv(up), StyledConv, ToRGB(up)] that runs as low-res GEMM + one fused kernel (FIR + act -> conv2 +
// act -> ToRGB + FIR-upsampled skip): the full-resolution intermediate never reaches HBM and the last stage stores only the image.
bool up_stage(const Layer* l, int n, int i) {
  return same_widths(l, n, i) && l[i].kind == 1 && l[i + 2].kind == 3 && cips3d_fused_up_conv_supported(l[i].Cout, l[i].H, l[i].W);
}

// A block of the same shape that does NOT up-sample (model_v3.py:553-590 builds every block up to size_end) through the same
// kernel without the FIR (CIPS3D_STAGE_FLAT): conv1's GEMM, then one launch; chained with its neighbours like the others.
bool flat_stage(const Layer* l, int n, int i) {
  return same_widths(l, n, i) && l[i].kind == 0 && l[i + 2].kind == 2 && cips3d_fused_flat_conv_supported(l[i].Cout, l[i].H, l[i].W);
}

// The stage headed by `a`, with output oh x ow, can also compute the low-resolution GEMM of the stage headed by `nx`: the next
// up-conv reads nothing but this stage's output, at half the width.
bool chains_into(const Layer& a, int oh, int ow, const Layer& nx) {
  return cips3d_fused_up_conv_chains(a.Cout) && nx.Cin == a.Cout && nx.Cout * 2 == a.Cout && nx.H == oh && nx.W == ow;
}

bool layers_ok(const Layer* l, int n) {
  if (!l || n < 1 || n > CIPS3D_MAX_DEC_LAYERS) return false;
  for (int i = 0; i < n; ++i)
    if (l[i].kind < 0 || l[i].kind > 3) return false;
  return true;
}

}  // namespace

extern "C" int cips3d_decoder_route_flags(cips3d_dec_layer* l, int n, const cips3d_dec_route_opts* opts, int64_t* rgb_part_slots) {
  if (!layers_ok(l, n) || !opts || !rgb_part_slots) return CIPS3D_E_BADARG;
  const cips3d_dec_route_opts& o = *opts;
  if (o.B < 1 || o.nerf_res < 1 || o.mode < 0 || o.mode > 2) return CIPS3D_E_BADARG;
  const int S = o.nerf_res;
  // 0: none, 1: up-sampling stage, 2: flat stage.  Flat stages live above the NeRF resolution: the blocks AT it belong to the
  // planes run below.  (At the NeRF resolution itself -- a 64^2 generator's 128 .. 1024 blocks -- the four flat launches take what
  // the eight planes launches they replace do: 0.456 against 0.457 ms per view, measured; left with the run.)
  auto stage_kind = [&](int i) { return up_stage(l, n, i) ? 1 : (o.flat_stages && l[i].H > S && flat_stage(l, n, i)) ? 2 : 0; };
  int flags[CIPS3D_MAX_DEC_LAYERS];
  for (int i = 0; i < n; ++i) flags[i] = (l[i].flags & CIPS3D_DEC_DEMOD) | (stage_kind(i) == 2 ? CIPS3D_DEC_FLAT_HEAD : 0);
  // When the NEXT stage is one too and the fused kernel has the chained form for this width, that kernel also computes the next
  // stage's low-res GEMM from its registers: the next head's weights are then packed in the chained order and its own GEMM launch
  // disappears.
  for (int i = 0; i + 3 < n; ++i) {
    const int k = stage_kind(i), up = k == 1 ? 2 : 1;
    if (o.chain_stages && k && stage_kind(i + 3) && chains_into(l[i], up * l[i].H, up * l[i].W, l[i + 3])) flags[i + 3] |= CIPS3D_DEC_CHAINED;
  }
  // Which StyledConvs the stand-alone GEMM consumes (everything but conv2 of a fused stage and chained heads): in the split-fp16
  // mode those are packed as split-fp16 fragments and run in CIPS3D_GEMM_SPLIT mode; the other two are consumed inside
  // cips3d_fused_up_conv_next.
  const bool use_split = o.mode == 1;
  for (int i = 0; i < n; ++i) {
    if (!use_split || l[i].kind > 1) continue;
    const bool in_stage = (l[i].kind == 0 && i >= 1 && stage_kind(i - 1) != 0) || (flags[i] & CIPS3D_DEC_CHAINED);
    flags[i] |= in_stage ? CIPS3D_DEC_SPLIT16 : CIPS3D_DEC_SPLIT;
  }
  // The run of equal-resolution StyledConvs at the NeRF resolution keeps its activations as split-fp16 planes (chain.hip): the
  // render kernel writes the feature map as planes, every layer of the run reads and writes them, the ToRGBs in between are
  // folded from registers, and the first up-sampling conv's low-resolution GEMM reads them.  In the bf16 mode the run keeps ONE
  // bf16 plane ("planes16", cips3d_modconv1x1_planes16): the stored activation is the rounded operand of the next GEMM, so the
  // mode's results do not change while its operand bytes halve.
  const bool use_p16 = o.mode == 2 && o.planes16_run;
  if ((use_split && o.planes_run) || use_p16) {
    const int64_t hw = (int64_t)S * S;
    const int p16 = use_p16 ? CIPS3D_DEC_P16 : 0;
    auto ok_conv = [&](int i) {
      if (i >= n || l[i].kind > 1 || l[i].H != S) return false;
      const bool mine = use_p16 ? !(flags[i] & CIPS3D_DEC_CHAINED) : (flags[i] & CIPS3D_DEC_SPLIT) != 0;
      return mine && cips3d_planes_supported(l[i].Cin, l[i].Cout, hw) != 0;
    };
    int n_fold = 0;
    for (int i = 0; ok_conv(i);) {
      if (l[i].kind == 1) {
        if (up_stage(l, n, i)) flags[i] |= CIPS3D_DEC_PLANES_IN | p16;
        break;
      }
      const bool has_rgb = i + 1 < n && l[i + 1].kind == 2;
      const bool foldable = has_rgb && i + 1 != n - 1 && l[i + 1].Cin == l[i].Cout && hw % 4 == 0 && n_fold < CIPS3D_TORGB_FOLD_MAX;
      const int j = i + (has_rgb ? 2 : 1);
      const bool next_takes = ok_conv(j) && (l[j].kind == 0 || up_stage(l, n, j));
      const bool planes_out = next_takes && (!has_rgb || foldable);
      flags[i] |= CIPS3D_DEC_PLANES_IN | p16 | (planes_out ? CIPS3D_DEC_PLANES_OUT : 0);
      if (has_rgb && foldable) ++n_fold;
      if (!planes_out) break;
      i = j;
    }
  }
  // ToRGB layers at the input resolution fold into the epilogue of the conv that feeds them: one slot of [B, 3, S, S] per row
  // block per layer
  int foldable_rgbs = 0;
  for (int i = 1; i < n; ++i)
    if (l[i].kind == 2 && l[i - 1].kind == 0 && l[i].H == S) ++foldable_rgbs;
  *rgb_part_slots = 16 * foldable_rgbs;
  for (int i = 0; i < n; ++i) l[i].flags = flags[i];
  return 0;
}

extern "C" int cips3d_decoder_steps(const cips3d_dec_layer* l, int n, int B, int ranged, int64_t rgb_part_slots,
                                    cips3d_dec_step* steps, int max_steps) {
  if (!layers_ok(l, n) || !steps || B < 1 || max_steps < 0) return CIPS3D_E_BADARG;
  int n_steps = 0;
  bool full = false;
  cips3d_dec_step spill;                          // (where steps beyond max_steps go: the call then returns CIPS3D_E_BADARG)
  auto emit = [&](int kind, int layer, int form, int mk, int Ci, int Co, int H) -> cips3d_dec_step* {
    if (n_steps >= max_steps) { full = true; return &spill; }
    cips3d_dec_step& s = steps[n_steps++];
    s = cips3d_dec_step{};
    s.kind = kind; s.layer = layer; s.form = form;
    s.mark[0] = mk; s.mark[1] = Ci; s.mark[2] = Co; s.mark[3] = H;
    return &s;
  };
  cips3d_torgb_fold fold;
  // the pending sum becomes the skip image in front of layer li
  auto flush = [&](int li, bool ride) {
    cips3d_dec_step* s = emit(CIPS3D_STEP_FLUSH, li, ride ? CIPS3D_STEP_RIDE : 0, ride ? -1 : CIPS3D_MARK_TORGB, 0, 3, fold.H);
    s->slot = fold.slots; s->n_bias = fold.nb; s->H = fold.H; s->W = fold.W;
    for (int k = 0; k < fold.nb; ++k) s->bias_layer[k] = fold.layer[k];
    fold.clear();
  };
  // can the ToRGB behind conv li be folded into its launch?  (never the last layer: that one writes the image)
  auto folds = [&](int li) {
    return li + 1 < n - 1 && l[li + 1].kind == 2 && l[li + 1].Cin == l[li].Cout && fold.can_join(l[li].H, l[li].W) &&
           fold.slots + 16 <= rgb_part_slots;
  };
  bool ylo_ready = false;                         // the low-resolution GEMM of the next stage was computed by the previous stage's kernel
  for (int li = 0; li < n; ++li) {
    const Layer& L = l[li];
    if (L.kind >= 2) {
      if (fold.pending()) flush(li, false);       // a ToRGB that could not be folded: settle the pending sum first
      emit(CIPS3D_STEP_TORGB, li, li == n - 1 ? CIPS3D_STEP_LAST : 0, CIPS3D_MARK_TORGB, L.Cin, 3, L.kind == 3 ? 2 * L.H : L.H);
      continue;
    }
    const int64_t hw = (int64_t)L.H * L.W;
    const bool planes_in = (L.flags & CIPS3D_DEC_PLANES_IN) != 0, p16 = (L.flags & CIPS3D_DEC_P16) != 0;
    const bool flat = L.kind == 0 && (L.flags & CIPS3D_DEC_FLAT_HEAD);
    const bool up = up_stage(l, n, li);
    if (flat && (planes_in || !flat_stage(l, n, li))) return CIPS3D_E_BADARG;       // the flags promise a block the flat kernel takes
    // resolution changes, or a flat block begins: the folded sum becomes the skip of this stage.  When the stage's low-resolution
    // GEMM is the next launch and runs on split planes, the fold rides on it (cips3d_reduce_job) instead of taking a launch of its own
    if ((L.kind == 1 || flat) && fold.pending()) {
      const int64_t fhw = fold.hw();
      flush(li, ranged && up && !ylo_ready && planes_in && !p16 && fold.slots <= 48 && fhw % 4 == 0 &&
                    (int64_t)B * 3 * fhw / 4 <= (hw + 127) / 128 * B * 128);
    }
    if (flat || up) {
      if ((L.flags & CIPS3D_DEC_CHAINED) && !ylo_ready) return CIPS3D_E_BADARG;     // chained weights without the stage that chains them
      if (!ylo_ready)
        emit(CIPS3D_STEP_LOWRES_GEMM, li, planes_in ? (p16 ? CIPS3D_STEP_P16 : CIPS3D_STEP_PLANES) : 0, CIPS3D_MARK_LOWRES_GEMM, L.Cin,
             L.Cout, L.H);
      const int OH = flat ? L.H : 2 * L.H, OW = flat ? L.W : 2 * L.W;               // the stage's output resolution
      // the next stage's head, when its weights are packed for this kernel
      const Layer* LN = li + 3 < n ? &l[li + 3] : nullptr;
      const bool ln_chained = LN && (LN->kind == 1 || (LN->kind == 0 && (LN->flags & CIPS3D_DEC_FLAT_HEAD))) && (LN->flags & CIPS3D_DEC_CHAINED);
      if (ln_chained && !chains_into(L, OH, OW, *LN)) return CIPS3D_E_BADARG;
      if (ln_chained && ((LN->flags & CIPS3D_DEC_SPLIT16) != (l[li + 1].flags & CIPS3D_DEC_SPLIT16))) return CIPS3D_E_BADARG;
      emit(CIPS3D_STEP_FUSED_STAGE, li,
           (flat ? CIPS3D_STEP_FLAT : 0) | (ln_chained ? CIPS3D_STEP_CHAIN : 0) | (li + 2 == n - 1 ? CIPS3D_STEP_LAST : 0),
           CIPS3D_MARK_FUSED_STAGE, L.Cout, ln_chained ? LN->Cout : 0, OH);
      ylo_ready = ln_chained;
      li += 2;
      continue;
    }
    if (L.kind == 1) {
      // chained packs only exist for stages that take the fused route above, and planes reach an up-conv only there
      if (L.flags & (CIPS3D_DEC_CHAINED | CIPS3D_DEC_PLANES_IN)) return CIPS3D_E_BADARG;
      emit(CIPS3D_STEP_GEMM_FIR, li, 0, CIPS3D_MARK_OTHER, L.Cout, L.Cout, 2 * L.H);
      continue;
    }
    cips3d_dec_step* s;
    int row_blocks;
    if (planes_in) {
      // a layer of the planes run (chain.hip): planes in; planes out (CIPS3D_DEC_PLANES_OUT) with the ToRGB that follows folded from
      // the registers -- nothing else may read this activation
      const bool has_rgb = li + 1 < n && l[li + 1].kind == 2, fold_it = folds(li);
      const int fmt = (L.flags & CIPS3D_DEC_PLANES_OUT) ? (p16 ? 3 : 1) : 0;    // planes for the next layer of the run, or fp32 when the run ends here
      if ((!p16 && !(L.flags & CIPS3D_DEC_SPLIT)) || (fmt != 0 && has_rgb && !fold_it)) return CIPS3D_E_BADARG;
      s = emit(CIPS3D_STEP_PLANES_GEMM, li, (p16 ? CIPS3D_STEP_P16 : CIPS3D_STEP_PLANES) | (fold_it ? CIPS3D_STEP_FOLD : 0),
               CIPS3D_MARK_PLANES_GEMM, L.Cin, L.Cout, L.H);
      s->out_format = fmt;
      row_blocks = cips3d_planes_torgb_blocks(L.Cout);
    } else {
      s = emit(CIPS3D_STEP_GEMM, li, (hw % 4 == 0 && folds(li)) ? CIPS3D_STEP_FOLD : 0, CIPS3D_MARK_GEMM, L.Cin, L.Cout, L.H);
      row_blocks = cips3d_modconv1x1_torgb_blocks(B, L.Cin, L.Cout, hw);
    }
    if (s->form & CIPS3D_STEP_FOLD) {
      s->slot = fold.slots;
      fold.join(li + 1, row_blocks, L.H, L.W);
      ++li;                                       // the ToRGB layer is done (its sum is pending in the slots)
    }
  }
  return full ? CIPS3D_E_BADARG : n_steps;
}
