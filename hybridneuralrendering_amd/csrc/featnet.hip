// Point embeddings from the MVS init checkpoint, on the device: the reference's `FeatureNet(intermediate=True)` in eval mode
// (models/mvs/models.py:717-764) and the `premlp` of `MvsPointsModel.query_embedding` (models/mvs/mvs_points_model.py:22-34, :225-259) as called at
// run/train_ft.py:759-760 for `load_points=2`.  Inference only: no backward.
//
//   hnr_featnet_forward  eight 3x3 / 5x5 convolutions, each followed by the activated batch norm in inference form, + the 1x1 `toplayer`:
//                        conv2d_direct_kernel (conv_direct.h) with the norm + LeakyReLU epilogue, the toplayer fused into the last layer's.
//                        Every sum is one chain of explicit fmaf in (input channel, ky, kx) order: two runs give the same bits.
//   hnr_point_embed      one view, one launch, one point per thread: projection, mask, direction and bilinear samples by the device functions of
//                        hnr_point_view_attrs (view_attrs.h), then premlp (63 -> 32 -> 32, LeakyReLU 0.01) with its weights in LDS.
#include "conv_direct.h"
#include "view_attrs.h"

namespace hnr {

// the packed parameters: the eight layers, each w, mean, mul, bias, then the toplayer (w [32][32], bias [32])
constexpr int FN_TOP = conv2d_offset(CONV2D_LAYERS, 3);
static_assert(FN_TOP + 32 * 32 + 32 == HNR_FEATNET_PACKED_ELEMS, "include/hnr.h: HNR_FEATNET_PACKED_ELEMS");

template <int L, int COG, bool TOP = false>
static int fn_launch(const float *in, int V, int Hi, int Wi, int Ho, int Wo, const float *packed, float *out, hipStream_t st)
{
    return conv2d_direct_launch<L, COG, EpiAbnLeaky<TOP>, const float *__restrict__>(in, V, Hi, Wi, Ho, Wo, packed + conv2d_offset(L, 3), out, st, packed + FN_TOP);
}

constexpr int PE_IN = 63, PE_OUT = 32;
constexpr int PE_B0 = PE_IN * PE_OUT, PE_W1 = PE_B0 + PE_OUT, PE_B1 = PE_W1 + PE_OUT * PE_OUT;
static_assert(PE_B1 + PE_OUT == HNR_PREMLP_PACKED_ELEMS, "include/hnr.h: HNR_PREMLP_PACKED_ELEMS");

// h[j] += sum_k v[k] * W0^T[k0 + k][j], k ascending (premlp's first layer, a few inputs at a time); the inputs are also written to the optional row
template <int NK>
__device__ __forceinline__ void pe_fold(const float *v, int k0, const float *wsm, float *h, float *row)
{
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        if (row) row[k0 + k] = v[k];
#pragma unroll
        for (int j = 0; j < PE_OUT; ++j) h[j] = fmaf(v[k], wsm[(k0 + k) * PE_OUT + j], h[j]);
        __builtin_amdgcn_sched_barrier(0);                              // keeps the scheduler from hoisting every later weight read above this point (300+ VGPRs)
    }
}

// one pyramid level, PE_CH channels at a time: sampled and folded into h
constexpr int PE_CH = 4;
__device__ __forceinline__ void pe_level(bool mask, const ViewTaps &t, const float *__restrict__ f, size_t plane, int Wl, int channels, int k0, const float *wsm,
                                         float *h, float *row)
{
#pragma unroll 1
    for (int c0 = 0; c0 < channels; c0 += PE_CH) {
        float v[PE_CH];
#pragma unroll
        for (int ch = 0; ch < PE_CH; ++ch) v[ch] = mask ? view_sample(t, f + (size_t)(c0 + ch) * plane, Wl) : 0.f;
        pe_fold<PE_CH>(v, k0 + c0, wsm, h, row);
    }
}

// one point per thread.  The row [x1 8 | x2 16 | x3 32 | colour 3 | dir 3 | conf] is consumed a few inputs at a time, in its own order, so only the
// 32 sums of premlp's first layer stay in registers; premlp's weights sit in LDS and every lane reads the same word at a time (broadcast).  A point
// outside the frame has zero features and colour: its row still goes through premlp.  conf NULL: the row's last column is 1.  visible (optional):
// where it is 0 the point is treated as outside the frame.
__global__ void __launch_bounds__(256) point_embed_kernel(const float *__restrict__ xyz, long long n, ViewCam vc, int H, int W, const float *__restrict__ img,
                                                          const float *__restrict__ x1, const float *__restrict__ x2, const float *__restrict__ x3, int H2, int W2,
                                                          int H4, int W4, const float *__restrict__ premlp, float *__restrict__ emb, float *__restrict__ color,
                                                          float *__restrict__ dir, float *__restrict__ row_out, const float *__restrict__ conf,
                                                          const uint8_t *__restrict__ visible)
{
    __shared__ float wsm[HNR_PREMLP_PACKED_ELEMS];
    for (int e = threadIdx.x; e < HNR_PREMLP_PACKED_ELEMS; e += 256) wsm[e] = premlp[e];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[3], gx, gy, tail[7], h[PE_OUT], o[PE_OUT];
    bool mask = view_project(vc, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], H, W, c, gx, gy);
    if (visible) mask = mask && visible[i] != 0;                        // an occluded point is a point outside the frame (hnr_point_occlusion)
    view_dir(vc, c, tail + 3);
    float *row = row_out ? row_out + (size_t)i * PE_IN : nullptr;
#pragma unroll
    for (int j = 0; j < PE_OUT; ++j) h[j] = wsm[PE_B0 + j];
    ViewTaps t0, t1, t2;
    if (mask) { t0 = view_taps(gx, gy, H, W, H, W); t1 = view_taps(gx, gy, H, W, H2, W2); t2 = view_taps(gx, gy, H, W, H4, W4); }
    const size_t p0 = (size_t)H * W;
    pe_level(mask, t0, x1, p0, W, 8, 0, wsm, h, row);
    pe_level(mask, t1, x2, (size_t)H2 * W2, W2, 16, 8, wsm, h, row);
    pe_level(mask, t2, x3, (size_t)H4 * W4, W4, 32, 24, wsm, h, row);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) tail[ch] = mask ? view_sample(t0, img + ch * p0, W) : 0.f;
    tail[6] = conf ? conf[i] : 1.f;
    pe_fold<7>(tail, 56, wsm, h, row);
#pragma unroll
    for (int q = 0; q < 3; ++q) { color[3 * i + q] = tail[q]; dir[3 * i + q] = tail[3 + q]; }
#pragma unroll
    for (int j = 0; j < PE_OUT; ++j) { h[j] = h[j] >= 0.f ? h[j] : h[j] * 0.01f; o[j] = wsm[PE_B1 + j]; }
#pragma unroll
    for (int k = 0; k < PE_OUT; ++k) {
#pragma unroll
        for (int j = 0; j < PE_OUT; ++j) o[j] = fmaf(h[k], wsm[PE_W1 + k * PE_OUT + j], o[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < PE_OUT; ++j) emb[(size_t)i * PE_OUT + j] = o[j] >= 0.f ? o[j] : o[j] * 0.01f;
}

static bool fn_shape_ok(int V, int H, int W) { return V >= 1 && V <= 4096 && H >= 4 && W >= 4 && H <= 32768 && W <= 32768; }

}  // namespace hnr

using namespace hnr;

extern "C" int64_t hnr_featnet_scratch_elems(int V, int H, int W)
{
    if (!fn_shape_ok(V, H, W)) return -1;
    const Pyramid p = pyramid_extents(H, W);
    int64_t m = 8 * (int64_t)H * W;
    if (32 * (int64_t)p.H2 * p.W2 > m) m = 32 * (int64_t)p.H2 * p.W2;
    if (64 * (int64_t)p.H4 * p.W4 > m) m = 64 * (int64_t)p.H4 * p.W4;
    return m * V;
}

extern "C" int hnr_featnet_forward(const float *d_images, int V, int H, int W, const float *d_packed, float *d_x1, float *d_x2, float *d_x3, float *d_scratch,
                                   int64_t scratch_elems, void *stream)
{
    if (!d_images || !d_packed || !d_x1 || !d_x2 || !d_x3 || !d_scratch) { set_error("hnr_featnet_forward: NULL argument"); return HNR_ERR_BADARG; }
    if (!fn_shape_ok(V, H, W)) { set_error("hnr_featnet_forward: bad argument (1 <= V <= 4096, 4 <= H, W <= 32768)"); return HNR_ERR_BADARG; }
    if (scratch_elems < hnr_featnet_scratch_elems(V, H, W)) { set_error("hnr_featnet_forward: scratch smaller than hnr_featnet_scratch_elems(V, H, W)"); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const auto [H2, W2, H4, W4] = pyramid_extents(H, W);
    float *a = d_scratch, *b = d_scratch + (size_t)V * 16 * H2 * W2, *c = d_scratch + (size_t)V * 32 * H4 * W4;
    if (int rc = fn_launch<0, 8>(d_images, V, H, W, H, W, d_packed, a, st)) return rc;                    // conv0
    if (int rc = fn_launch<1, 8>(a, V, H, W, H, W, d_packed, d_x1, st)) return rc;
    if (int rc = fn_launch<2, 16>(d_x1, V, H, W, H2, W2, d_packed, a, st)) return rc;                     // conv1
    if (int rc = fn_launch<3, 16>(a, V, H2, W2, H2, W2, d_packed, b, st)) return rc;
    if (int rc = fn_launch<4, 16>(b, V, H2, W2, H2, W2, d_packed, d_x2, st)) return rc;
    if (int rc = fn_launch<5, 16>(d_x2, V, H2, W2, H4, W4, d_packed, a, st)) return rc;                   // conv2
    if (int rc = fn_launch<6, 16>(a, V, H4, W4, H4, W4, d_packed, c, st)) return rc;
    return fn_launch<7, 32, true>(c, V, H4, W4, H4, W4, d_packed, d_x3, st);                              // + toplayer
}

extern "C" int hnr_point_embed(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                               const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, float *d_emb,
                               float *d_color, float *d_dir, float *d_row, void *stream)
{
    return hnr_point_embed_conf(d_xyz, n, w2c, c2w, cam_pos_cam, K, H, W, d_image, d_x1, d_x2, d_x3, d_premlp, nullptr, d_emb, d_color, d_dir, d_row, stream);
}

extern "C" int hnr_point_embed_conf(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                                    const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, const float *d_conf,
                                    float *d_emb, float *d_color, float *d_dir, float *d_row, void *stream)
{
    return hnr_point_embed_vis(d_xyz, n, w2c, c2w, cam_pos_cam, K, H, W, d_image, d_x1, d_x2, d_x3, d_premlp, d_conf, nullptr, d_emb, d_color, d_dir, d_row, stream);
}

extern "C" int hnr_point_embed_vis(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                                   const float *d_image, const float *d_x1, const float *d_x2, const float *d_x3, const float *d_premlp, const float *d_conf,
                                   const uint8_t *d_visible, float *d_emb, float *d_color, float *d_dir, float *d_row, void *stream)
{
    if (!d_xyz || !w2c || !c2w || !cam_pos_cam || !K || !d_image || !d_x1 || !d_x2 || !d_x3 || !d_premlp || !d_emb || !d_color || !d_dir) {
        set_error("hnr_point_embed: NULL argument"); return HNR_ERR_BADARG;
    }
    if (n <= 0 || n > (int64_t)INT32_MAX * 256 || !fn_shape_ok(1, H, W)) {                      // one block of 256 points per grid entry, at most 2^31 - 1 of them
        set_error("hnr_point_embed: bad argument (1 <= n <= (2^31 - 1) * 256, 4 <= H, W <= 32768)"); return HNR_ERR_BADARG;
    }
    ViewCam vc;
    view_cam_fill(vc, w2c, c2w, cam_pos_cam, K);
    const auto [H2, W2, H4, W4] = pyramid_extents(H, W);
    point_embed_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(d_xyz, (long long)n, vc, H, W, d_image, d_x1, d_x2, d_x3, H2, W2, H4, W4, d_premlp, d_emb,
                                                                      d_color, d_dir, d_row, d_conf, d_visible);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
