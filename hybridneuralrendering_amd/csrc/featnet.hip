// Point embeddings from the MVS init checkpoint, on the device: the reference's `FeatureNet(intermediate=True)` in eval mode
// (models/mvs/models.py:717-764) and the `premlp` of `MvsPointsModel.query_embedding` (models/mvs/mvs_points_model.py:22-34, :225-259) as called at
// run/train_ft.py:759-760 for `load_points=2`.  Inference only: no backward.
//
//   hnr_featnet_forward  eight 3x3 / 5x5 convolutions, each followed by the activated batch norm in inference form, + the 1x1 `toplayer`:
//                        direct convolution in fp32, one output pixel per thread, COG output channels of it in registers, the input tile with its halo
//                        staged in LDS eight input channels at a time, the weights read through wave-uniform addresses (scalar loads), the
//                        norm + LeakyReLU epilogue and the toplayer fused.  Every sum is one chain of explicit fmaf in (input channel, ky, kx) order:
//                        two runs give the same bits.
//   hnr_point_embed      one view, one launch, one point per thread: projection, mask, direction and bilinear samples by the device functions of
//                        hnr_point_view_attrs (view_attrs.h), then premlp (63 -> 32 -> 32, LeakyReLU 0.01) with its weights in LDS.
#include "hnr_launch.h"
#include "view_attrs.h"

namespace hnr {

constexpr int FN_TW = 32, FN_TH = 8;            // output tile of one block: one pixel per thread, a wave covers two rows of 32
constexpr int FN_CCH = 8;                       // input channels staged per round
constexpr int FN_LAYERS = 8;

struct FnLayer { int cin, cout, ks, stride; };
constexpr FnLayer FN_LAYER[FN_LAYERS] = {{3, 8, 3, 1}, {8, 8, 3, 1}, {8, 16, 5, 2}, {16, 16, 3, 1}, {16, 16, 3, 1}, {16, 32, 5, 2}, {32, 32, 3, 1}, {32, 32, 3, 1}};

// offset of layer l in the packed parameters (l = FN_LAYERS: the toplayer): per layer w [cin][ks][ks][cout], mean [cout], mul [cout], bias [cout]
constexpr int fn_offset(int l)
{
    int o = 0;
    for (int i = 0; i < l; ++i) o += FN_LAYER[i].cin * FN_LAYER[i].ks * FN_LAYER[i].ks * FN_LAYER[i].cout + 3 * FN_LAYER[i].cout;
    return o;
}
static_assert(fn_offset(FN_LAYERS) + 32 * 32 + 32 == HNR_FEATNET_PACKED_ELEMS, "include/hnr.h: HNR_FEATNET_PACKED_ELEMS");

template <int CIN, int KS, int STRIDE>
constexpr int fn_lds_bytes()
{
    return (CIN < FN_CCH ? CIN : FN_CCH) * ((FN_TH - 1) * STRIDE + KS) * ((FN_TW - 1) * STRIDE + KS) * (int)sizeof(float);
}

// in [V,CIN,Hi,Wi] -> out [V,COUT,Ho,Wo]; blockIdx.z = view * (COUT / COG) + channel group.  TOP: the 1x1 toplayer (top = w [co][ci], bias [co]) is
// applied to the COG = COUT activated channels of the pixel before the store.
template <int CIN, int COUT, int KS, int STRIDE, int COG, bool TOP>
__global__ void __launch_bounds__(256) featnet_conv_kernel(const float *__restrict__ in, int Hi, int Wi, int Ho, int Wo, const float *__restrict__ prm,
                                                           const float *__restrict__ top, float *__restrict__ out)
{
    extern __shared__ float fn_tile[];
    constexpr int PAD = KS / 2, IW = (FN_TW - 1) * STRIDE + KS, IH = (FN_TH - 1) * STRIDE + KS, CCH = CIN < FN_CCH ? CIN : FN_CCH, GROUPS = COUT / COG;
    static_assert(CIN % CCH == 0 && COUT % COG == 0 && (!TOP || COG == COUT), "featnet_conv_kernel: channel split");
    const int tx = threadIdx.x & (FN_TW - 1), ty = threadIdx.x / FN_TW;
    const int g = blockIdx.z % GROUPS, v = blockIdx.z / GROUPS;
    const int ox0 = blockIdx.x * FN_TW, oy0 = blockIdx.y * FN_TH;
    const int ix0 = ox0 * STRIDE - PAD, iy0 = oy0 * STRIDE - PAD;
    const float *inv = in + (size_t)v * CIN * Hi * Wi;
    float acc[COG];
#pragma unroll
    for (int j = 0; j < COG; ++j) acc[j] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CCH) {
        __syncthreads();                                                // the previous round's reads are done
        for (int e = threadIdx.x; e < CCH * IH * IW; e += 256) {
            const int ch = e / (IH * IW), r = e - ch * (IH * IW), yy = r / IW, xx = r - yy * IW;
            const int iy = iy0 + yy, ix = ix0 + xx;
            fn_tile[e] = (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) ? inv[((size_t)(c0 + ch) * Hi + iy) * Wi + ix] : 0.f;          // zero padding
        }
        __syncthreads();
        const float *t0 = fn_tile + (ty * STRIDE) * IW + tx * STRIDE;
#pragma unroll 1
        for (int ch = 0; ch < CCH; ++ch) {
            const float *t = t0 + ch * (IH * IW);
            const float *w = prm + (size_t)((c0 + ch) * KS * KS) * COUT + g * COG;          // the same address in every lane
#pragma unroll
            for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
                for (int kx = 0; kx < KS; ++kx) {
                    const float a = t[ky * IW + kx];
#pragma unroll
                    for (int j = 0; j < COG; ++j) acc[j] = fmaf(a, w[(ky * KS + kx) * COUT + j], acc[j]);
                }
            }
        }
    }
    const float *mean = prm + CIN * KS * KS * COUT + g * COG, *mul = mean + COUT, *bias = mul + COUT;
    float y[COG];
#pragma unroll
    for (int j = 0; j < COG; ++j) {
        const float u = (acc[j] - mean[j]) * mul[j] + bias[j];
        y[j] = u >= 0.f ? u : u * 0.01f;
    }
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;
    const size_t plane = (size_t)Ho * Wo;
    float *o = out + ((size_t)v * COUT + g * COG) * plane + (size_t)oy * Wo + ox;
    if (!TOP) {
#pragma unroll
        for (int j = 0; j < COG; ++j) o[j * plane] = y[j];
    } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int co = 0; co < COUT; ++co) {                             // (one output at a time: the loop vectoriser would pair them into packed fp32)
            float s = 0.f;
#pragma unroll
            for (int ci = 0; ci < COG; ++ci) s = fmaf(y[ci], top[co * COG + ci], s);
            o[co * plane] = s + top[COUT * COUT + co];
        }
    }
}

template <int L, int COG, bool TOP>
static int fn_launch(const float *in, int V, int Hi, int Wi, int Ho, int Wo, const float *packed, float *out, hipStream_t st)
{
    constexpr FnLayer P = FN_LAYER[L];
    const dim3 grid(cdiv(Wo, FN_TW), cdiv(Ho, FN_TH), V * (P.cout / COG));
    return launch_lds<featnet_conv_kernel<P.cin, P.cout, P.ks, P.stride, COG, TOP>>(grid, dim3(256), fn_lds_bytes<P.cin, P.ks, P.stride>(), st, in, Hi, Wi, Ho, Wo,
                                                                                   packed + fn_offset(L), packed + fn_offset(FN_LAYERS), out);
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
    const int64_t H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1, H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
    int64_t m = 8 * (int64_t)H * W;
    if (32 * H2 * W2 > m) m = 32 * H2 * W2;
    if (64 * H4 * W4 > m) m = 64 * H4 * W4;
    return m * V;
}

extern "C" int hnr_featnet_forward(const float *d_images, int V, int H, int W, const float *d_packed, float *d_x1, float *d_x2, float *d_x3, float *d_scratch,
                                   int64_t scratch_elems, void *stream)
{
    if (!d_images || !d_packed || !d_x1 || !d_x2 || !d_x3 || !d_scratch) { set_error("hnr_featnet_forward: NULL argument"); return HNR_ERR_BADARG; }
    if (!fn_shape_ok(V, H, W)) { set_error("hnr_featnet_forward: bad argument (1 <= V <= 4096, 4 <= H, W <= 32768)"); return HNR_ERR_BADARG; }
    if (scratch_elems < hnr_featnet_scratch_elems(V, H, W)) { set_error("hnr_featnet_forward: scratch smaller than hnr_featnet_scratch_elems(V, H, W)"); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1, H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
    float *a = d_scratch, *b = d_scratch + (size_t)V * 16 * H2 * W2, *c = d_scratch + (size_t)V * 32 * H4 * W4;
    if (int rc = fn_launch<0, 8, false>(d_images, V, H, W, H, W, d_packed, a, st)) return rc;             // conv0
    if (int rc = fn_launch<1, 8, false>(a, V, H, W, H, W, d_packed, d_x1, st)) return rc;
    if (int rc = fn_launch<2, 16, false>(d_x1, V, H, W, H2, W2, d_packed, a, st)) return rc;              // conv1
    if (int rc = fn_launch<3, 16, false>(a, V, H2, W2, H2, W2, d_packed, b, st)) return rc;
    if (int rc = fn_launch<4, 16, false>(b, V, H2, W2, H2, W2, d_packed, d_x2, st)) return rc;
    if (int rc = fn_launch<5, 16, false>(d_x2, V, H2, W2, H4, W4, d_packed, a, st)) return rc;            // conv2
    if (int rc = fn_launch<6, 16, false>(a, V, H4, W4, H4, W4, d_packed, c, st)) return rc;
    return fn_launch<7, 32, true>(c, V, H4, W4, H4, W4, d_packed, d_x3, st);                               // + toplayer
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
    const int H2 = (H - 1) / 2 + 1, W2 = (W - 1) / 2 + 1, H4 = (H2 - 1) / 2 + 1, W4 = (W2 - 1) / 2 + 1;
    point_embed_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(d_xyz, (long long)n, vc, H, W, d_image, d_x1, d_x2, d_x3, H2, W2, H4, W4, d_premlp, d_emb,
                                                                      d_color, d_dir, d_row, d_conf, d_visible);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
