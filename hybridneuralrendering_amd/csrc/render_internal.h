// What the two whole-path calls share (csrc/render_forward.hip, csrc/render_train.hip): the workspace carver, the stage-event marker, the query
// parameter block, and the layer shapes of the aggregator's per-sample MLPs.  Host code only.
#pragma once
#include "hnr_common.h"

namespace hnr {

// Hands out 256-byte aligned pieces of one workspace.  base == NULL: sizes only (every take returns NULL, `off` still advances).
struct Carver {
    char *base; size_t off, cap; bool ok;
    template <class T> T *take(size_t n)
    {
        off = (off + 255) & ~(size_t)255;
        T *p = reinterpret_cast<T *>(base + off);
        off += n * sizeof(T);
        if (base && off > cap) ok = false;
        return base ? p : nullptr;
    }
};

// Optional HIP events at the stage boundaries of a call (hnr_render_outputs::stage_events; bench.py reads them): mark() records the next one.
struct StageMarker {
    const char *error; void *const *events; hipStream_t st; int stage = 0;      // error: the text set when a record fails
    int operator()()
    {
        void *const e = events ? events[stage] : nullptr;
        ++stage;
        if (e && hipEventRecord((hipEvent_t)e, st) != hipSuccess) { set_error("%s", error); return HNR_ERR_HIP; }
        return HNR_OK;
    }
};

// hnr_march_query's parameter block from a render / train parameter block (hnr_render_params, hnr_train_params: the same field names)
template <class Params> hnr_query_params query_params(const Params &p, int pad_outputs)
{
    hnr_query_params q;
    q.R = p.R; q.D = p.D; q.SR = p.SR; q.K = p.K; q.radius2 = p.radius2; q.tmid_stride = p.tmid_stride; q.pad_outputs = pad_outputs; q.knn_order = p.knn_order;
    for (int i = 0; i < 3; ++i) q.kernel_size[i] = p.kernel_size[i];
    return q;
}

// The per-sample MLPs as hnr_mlp3 layer lists.  N = outputs, K = inputs, LD = row stride of the layer's fp32 weight matrix, ACT = LeakyReLU behind it.
//   CF: color_feature_branch 280 -> 128 -> 128 -> 128, and as a fourth layer on its tail the colour-feature columns of aux_merge_weight_block.0
//       (128 -> 64, once per sample; rows of the [64, 176] matrix);
//   MW: aux_merge_weight_block 48 -> 64 -> 64 -> 64 per (view, sample) row (its first layer without the colour-feature columns);
//   MX: color_mixup_block 90 -> 45 -> 45 -> 45.
constexpr int CF_N[4] = {128, 128, 128, 64}, CF_K[4] = {280, 128, 128, 128}, CF_LD[4] = {280, 128, 128, 176}, CF_ACT[4] = {1, 1, 1, 0};
constexpr int MW_N[3] = {64, 64, 64}, MW_K[3] = {48, 64, 64}, MW_LD[3] = {48, 64, 64}, MW_ACT[3] = {1, 1, 1};
constexpr int MX_N[3] = {45, 45, 45}, MX_K[3] = {90, 45, 45}, MX_LD[3] = {90, 45, 45}, MX_ACT[3] = {1, 1, 0};

}  // namespace hnr
