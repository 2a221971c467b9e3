// The pending ToRGB fold of a decoder walk, shared by the route resolver (decoder_route.hip) and the forward walker of the
// decoder-gradient plan (decoder_grad.hip).
//
// A non-up-sampling ToRGB that follows a StyledConv is computed from that conv's registers (partial sums per row block:
// cips3d_modconv1x1_torgb, cips3d_modconv1x1_planes); the slots of consecutive such layers at one resolution are summed by ONE
// cips3d_torgb_reduce when their sum is first needed (the skip chain at an unchanged resolution is a plain sum).
#pragma once
#include "../../include/cips3d_hip.h"

struct cips3d_torgb_fold {
  int slots = 0, nb = 0;                   // slots written so far; ToRGB layers folded into them
  int H = 0, W = 0;                        // resolution of the slots
  int layer[CIPS3D_TORGB_FOLD_MAX];        // the folded ToRGB layers: their biases are the flush's bias list

  bool pending() const { return slots != 0; }
  // may the ToRGB behind a conv at h x w join?  (room in the bias list; one resolution per sum)
  bool can_join(int h, int w) const { return nb < CIPS3D_TORGB_FOLD_MAX && (slots == 0 || (H == h && W == w)); }
  void join(int torgb_layer, int row_blocks, int h, int w) {
    slots += row_blocks;
    layer[nb++] = torgb_layer;
    H = h; W = w;
  }
  // arguments of the flush (cips3d_torgb_reduce(part, slots, bias, nb, skip, dst, B, hw(), stream)); then clear()
  int64_t hw() const { return (int64_t)H * W; }
  template <class Layer>
  void biases(const Layer* layers, const float** bias) const {
    for (int k = 0; k < nb; ++k) bias[k] = layers[layer[k]].bias;
  }
  void clear() { slots = nb = 0; }
};
