// Depth maps from the pretrained MVSNet, on the device: the reference's `MVSNet(refine=False)` in eval mode (models/depth_estimators/mvsnet.py,
// module.py) and the tail of `MvsPointsModel.gen_points` (models/mvs/mvs_points_model.py:300-341) for `manual_depth_view=1`.  Inference only: no backward.
//
//   hnr_mvsnet_feature       seven conv + norm + ReLU and the `feature` conv: conv2d_direct_kernel (conv_direct.h) with plain BatchNorm + ReLU, or bias
//                            alone, as the epilogue.
//   hnr_mvsnet_cost_volume   one thread per (pixel, depth): the V views' 32 channels sampled and folded into 32 sums and 32 sums of squares.
//   hnr_mvsnet_cost_reg      the 3-D network.  Convolutions: that kernel's arrangement in three dimensions (a block of 32 x 4 x 2 threads, ZPT outputs along z
//                            per thread so that a staged value feeds up to ZPT * COG fmaf; both chosen per layer).  Transposed convolutions: a gather, one block per parity
//                            class of the output, so the 1 / 2 / 4 / 8 taps and their weights are the same for every lane.
//   hnr_mvsnet_depth_head    softmax over D, expected depth, expected index, the four-bin confidence: one thread per pixel.
//   hnr_mvsnet_depth_points  nearest upsampling, the near / far mask, the camera-space point of every pixel.
// Every sum is one chain of explicit fmaf in a fixed order: two runs give the same bits.
#include "conv_direct.h"

namespace hnr {

// ---- the 2-D feature net -----------------------------------------------------------------------------------------------------------------------------
// conv_direct.h's eight layers; the last one is `feature`: bias, no norm, no activation
static_assert(conv2d_offset(CONV2D_LAYERS, 1) == HNR_MVSNET_FEATURE_PACKED_ELEMS, "include/hnr.h: HNR_MVSNET_FEATURE_PACKED_ELEMS");

// every output channel of the pixel in one thread (COG = COUT)
template <int L, class Epi = EpiBnRelu>
static int mf_launch(const float *in, int V, int Hi, int Wi, int Ho, int Wo, const float *packed, float *out, hipStream_t st)
{
    return conv2d_direct_launch<L, CONV2D_LAYER[L].cout, Epi>(in, V, Hi, Wi, Ho, Wo, packed + conv2d_offset(L, 1), out, st);
}

static bool mf_shape_ok(int V, int H, int W) { return V >= 1 && V <= 64 && H >= 4 && W >= 4 && H <= 32768 && W <= 32768; }

// ---- the cost volume ---------------------------------------------------------------------------------------------------------------------------------
constexpr int MV_C = 32;                        // feature channels

__global__ void __launch_bounds__(256) mvsnet_cost_volume_kernel(const float *__restrict__ feat, int V, int h, int w, const float *__restrict__ proj,
                                                                 const float *__restrict__ dvals, int D, float *__restrict__ vol)
{
    const size_t plane = (size_t)h * w, n = plane * D, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i / plane), r = (int)(i - (size_t)k * plane), y = r / w, x = r - y * w;
    const float fx = (float)x, fy = (float)y, d = dvals[k], fw = (float)w, fh = (float)h;
    const float half_w = (float)(w - 1) / 2.f, half_h = (float)(h - 1) / 2.f;
    float s[MV_C], q[MV_C];
#pragma unroll
    for (int c = 0; c < MV_C; ++c) { s[c] = 0.f; q[c] = 0.f; }
#pragma unroll 1
    for (int v = 0; v < V; ++v) {
        const float *P = proj + v * 12;
        const float q0 = ((P[0] * fx + P[1] * fy) + P[2]) * d + P[3];
        const float q1 = ((P[4] * fx + P[5] * fy) + P[6]) * d + P[7];
        const float q2 = ((P[8] * fx + P[9] * fy) + P[10]) * d + P[11];
        const float gx = (q0 / q2) / half_w - 1.f, gy = (q1 / q2) / half_h - 1.f;
        const float ix = ((gx + 1.f) * fw - 1.f) * 0.5f, iy = ((gy + 1.f) * fh - 1.f) * 0.5f;
        if (!(ix > -1.f && ix < fw && iy > -1.f && iy < fh)) continue;          // outside every tap's reach, or not finite: nothing is read
        const float x0f = floorf(ix), y0f = floorf(iy);
        const int x0 = (int)x0f, y0 = (int)y0f;                                  // -1 .. w-1, -1 .. h-1
        const float wx1 = ix - x0f, wx0 = (x0f + 1.f) - ix, wy1 = iy - y0f, wy0 = (y0f + 1.f) - iy;
        const float w00 = wx0 * wy0, w01 = wx1 * wy0, w10 = wx0 * wy1, w11 = wx1 * wy1;
        const bool in_x0 = x0 >= 0, in_x1 = x0 + 1 < w, in_y0 = y0 >= 0, in_y1 = y0 + 1 < h;
        const float *f = feat + (size_t)v * MV_C * plane;
        const size_t o00 = (size_t)(in_y0 ? y0 : 0) * w + (in_x0 ? x0 : 0), o01 = (size_t)(in_y0 ? y0 : 0) * w + (in_x1 ? x0 + 1 : 0);
        const size_t o10 = (size_t)(in_y1 ? y0 + 1 : 0) * w + (in_x0 ? x0 : 0), o11 = (size_t)(in_y1 ? y0 + 1 : 0) * w + (in_x1 ? x0 + 1 : 0);
        const bool in00 = in_x0 && in_y0, in01 = in_x1 && in_y0, in10 = in_x0 && in_y1, in11 = in_x1 && in_y1;
#pragma unroll
        for (int c = 0; c < MV_C; ++c) {
            const float *fc = f + (size_t)c * plane;                             // (a tap outside the map is zero; its offset points at row / column 0)
            const float t00 = in00 ? fc[o00] : 0.f, t01 = in01 ? fc[o01] : 0.f, t10 = in10 ? fc[o10] : 0.f, t11 = in11 ? fc[o11] : 0.f;
            const float t = fmaf(t11, w11, fmaf(t10, w10, fmaf(t01, w01, t00 * w00)));
            s[c] += t;
            q[c] = fmaf(t, t, q[c]);
        }
    }
    const float fv = (float)V;
#pragma unroll
    for (int c = 0; c < MV_C; ++c) {
        const float mean = s[c] / fv;
        vol[(size_t)c * n + i] = q[c] / fv - mean * mean;
    }
}

static bool mv_volume_ok(int D, int h, int w)
{
    return D >= 1 && D <= 4096 && h >= 2 && w >= 2 && h <= 8192 && w <= 8192 && (int64_t)D * h * w <= ((int64_t)1 << 26);
}

// ---- the 3-D network ---------------------------------------------------------------------------------------------------------------------------------
constexpr int C3_TX = 32, C3_TY = 4, C3_TZ = 2;            // threads of a block along x, y, z
struct C3Layer { int cin, cout, stride; bool transposed; };
constexpr int C3_LAYERS = 11;                              // conv0 .. conv6, conv7, conv9, conv11, prob
constexpr C3Layer C3_LAYER[C3_LAYERS] = {{32, 8, 1, false}, {8, 16, 2, false}, {16, 16, 1, false}, {16, 32, 2, false}, {32, 32, 1, false}, {32, 64, 2, false},
                                         {64, 64, 1, false}, {64, 32, 2, true}, {32, 16, 2, true}, {16, 8, 2, true}, {8, 1, 1, false}};

constexpr int c3_offset(int l)
{
    int o = 0;
    for (int i = 0; i < l; ++i) o += C3_LAYER[i].cin * 27 * C3_LAYER[i].cout + (i == C3_LAYERS - 1 ? 1 : 3) * C3_LAYER[i].cout;
    return o;
}
static_assert(c3_offset(C3_LAYERS) == HNR_MVSNET_REG_PACKED_ELEMS, "include/hnr.h: HNR_MVSNET_REG_PACKED_ELEMS");

// in [CIN,Di,Hi,Wi] -> out [COUT,Do,Ho,Wo], 3x3x3, pad 1.  blockIdx.z = z tile * (COUT / COG) + channel group; a thread owns ZPT outputs along z.
// CCH input channels are staged per round.  LAST: `prob` (bias, no norm, no activation).
template <int CIN, int COUT, int STRIDE, int COG, int ZPT, int CCH, bool LAST>
__global__ void __launch_bounds__(256) mvsnet_conv3d_kernel(const float *__restrict__ in, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                                            const float *__restrict__ prm, float *__restrict__ out)
{
    extern __shared__ float mv_tile[];
    constexpr int OZ = C3_TZ * ZPT, IW = (C3_TX - 1) * STRIDE + 3, IH = (C3_TY - 1) * STRIDE + 3, ID = (OZ - 1) * STRIDE + 3, GROUPS = COUT / COG;
    constexpr int TDZ = (ZPT - 1) * STRIDE + 3;                         // input planes one thread reads
    static_assert(CIN % CCH == 0 && COUT % COG == 0, "mvsnet_conv3d_kernel: channel split");
    const int tx = threadIdx.x & (C3_TX - 1), ty = (threadIdx.x / C3_TX) & (C3_TY - 1), tz = threadIdx.x / (C3_TX * C3_TY);
    const int g = blockIdx.z % GROUPS, zt = blockIdx.z / GROUPS;
    const int ox0 = blockIdx.x * C3_TX, oy0 = blockIdx.y * C3_TY, oz0 = zt * OZ;
    const int ix0 = ox0 * STRIDE - 1, iy0 = oy0 * STRIDE - 1, iz0 = oz0 * STRIDE - 1;
    float acc[ZPT][COG];
#pragma unroll
    for (int zo = 0; zo < ZPT; ++zo)
#pragma unroll
        for (int j = 0; j < COG; ++j) acc[zo][j] = 0.f;
    for (int c0 = 0; c0 < CIN; c0 += CCH) {
        __syncthreads();                                                // the previous round's reads are done
        for (int e = threadIdx.x; e < CCH * ID * IH * IW; e += 256) {
            const int ch = e / (ID * IH * IW), r = e - ch * (ID * IH * IW), zz = r / (IH * IW), r2 = r - zz * (IH * IW), yy = r2 / IW, xx = r2 - yy * IW;
            const int iz = iz0 + zz, iy = iy0 + yy, ix = ix0 + xx;
            mv_tile[e] = (iz >= 0 && iz < Di && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) ? in[(((size_t)(c0 + ch) * Di + iz) * Hi + iy) * Wi + ix] : 0.f;
        }
        __syncthreads();
        const float *t0 = mv_tile + ((tz * ZPT * STRIDE) * IH + ty * STRIDE) * IW + tx * STRIDE;
#pragma unroll 1
        for (int ch = 0; ch < CCH; ++ch) {
            const float *t = t0 + ch * (ID * IH * IW);
            const float *w = prm + (size_t)((c0 + ch) * 27) * COUT + g * COG;              // the same address in every lane
#pragma unroll
            for (int dz = 0; dz < TDZ; ++dz) {                          // (dz ascending: for each output kz ascends, so its chain runs in (kz, ky, kx) order)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const float a = t[(dz * IH + ky) * IW + kx];
#pragma unroll
                        for (int zo = 0; zo < ZPT; ++zo) {
                            const int kz = dz - zo * STRIDE;
                            if (kz >= 0 && kz < 3) {
#pragma unroll
                                for (int j = 0; j < COG; ++j) acc[zo][j] = fmaf(a, w[((kz * 3 + ky) * 3 + kx) * COUT + j], acc[zo][j]);
                            }
                        }
                    }
                }
            }
        }
    }
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;
    const size_t vol = (size_t)Do * Ho * Wo;
#pragma unroll
    for (int zo = 0; zo < ZPT; ++zo) {
        const int oz = oz0 + tz * ZPT + zo;
        if (oz >= Do) continue;
        float *o = out + (size_t)(g * COG) * vol + ((size_t)oz * Ho + oy) * Wo + ox;
#pragma unroll
        for (int j = 0; j < COG; ++j) o[j * vol] = mv_epilogue<LAST>(acc[zo][j], prm + CIN * 27 * COUT, COUT, g * COG + j);
    }
}

// COG and ZPT are the launch's to choose (neither changes a sum's order): large ones where the volume is large, so that a staged value feeds many
// fmaf; small ones on the deep levels, whose few thousand voxels would otherwise be a few dozen blocks for 256 CUs.
template <int L, int COG, int ZPT>
static int c3_launch(const float *in, int Di, int Hi, int Wi, const float *packed, float *out, hipStream_t st)
{
    constexpr C3Layer P = C3_LAYER[L];
    constexpr int CCH = P.stride == 1 ? 8 : 4, OZ = C3_TZ * ZPT;
    constexpr int lds = CCH * ((OZ - 1) * P.stride + 3) * ((C3_TY - 1) * P.stride + 3) * ((C3_TX - 1) * P.stride + 3) * (int)sizeof(float);
    const int Do = Di / P.stride, Ho = Hi / P.stride, Wo = Wi / P.stride;                   // (even sizes: (n + 2 - 3) / 2 + 1 = n / 2)
    const dim3 grid(cdiv(Wo, C3_TX), cdiv(Ho, C3_TY), cdiv(Do, OZ) * (P.cout / COG));
    return launch_lds<mvsnet_conv3d_kernel<P.cin, P.cout, P.stride, COG, ZPT, CCH, L == C3_LAYERS - 1>>(grid, dim3(256), lds, st, in, Di, Hi, Wi, Do, Ho, Wo,
                                                                                                       packed + c3_offset(L), out);
}

// ConvTranspose3d(3, stride 2, pad 1, output_padding 1) + norm + ReLU, then skip + y: in [CIN,Di,Hi,Wi] -> out [COUT,2Di,2Hi,2Wi].
// Output o gets in[i] * w[k] wherever o = 2i - 1 + k: an even o has the one tap (k = 1, i = o/2), an odd o the two taps (k = 0, i = (o+1)/2) and
// (k = 2, i = (o-1)/2), the first of which falls off the end for the last o.  blockIdx.z = (z tile * 8 + parity class (pz py px)) * groups + channel group: taps and weights are
// the block's; a thread owns the output (2bx + px, 2by + py, 2bz + pz) of input cell (bx, by, bz).  out may be skip (each voxel is read, then written,
// by its one thread).
// One parity class: the taps are compile-time, so a channel's up to eight loads are in flight together.
template <int CIN, int COUT, int COG, int PZ, int PY, int PX>
__device__ __forceinline__ void mv_deconv_class(const float *__restrict__ in, int Di, int Hi, int Wi, const float *__restrict__ w, int bx, int by, int bz,
                                                float *acc)
{
    const size_t ivol = (size_t)Di * Hi * Wi;
#pragma unroll 2
    for (int ci = 0; ci < CIN; ++ci) {
        const float *ic = in + (size_t)ci * ivol;
        const float *wc = w + (size_t)(ci * 27) * COUT;                                     // the same address in every lane
#pragma unroll
        for (int az = 0; az <= PZ; ++az) {                              // (taps in ascending k)
            const int kz = PZ ? 2 * az : 1, iz = PZ ? bz + 1 - az : bz;
#pragma unroll
            for (int ay = 0; ay <= PY; ++ay) {
                const int ky = PY ? 2 * ay : 1, iy = PY ? by + 1 - ay : by;
#pragma unroll
                for (int ax = 0; ax <= PX; ++ax) {
                    const int kx = PX ? 2 * ax : 1, ix = PX ? bx + 1 - ax : bx;
                    const float a = (iz < Di && iy < Hi && ix < Wi) ? ic[((size_t)iz * Hi + iy) * Wi + ix] : 0.f;
                    const float *wk = wc + ((kz * 3 + ky) * 3 + kx) * COUT;
#pragma unroll
                    for (int j = 0; j < COG; ++j) acc[j] = fmaf(a, wk[j], acc[j]);
                }
            }
        }
    }
}

template <int CIN, int COUT, int COG>
__global__ void __launch_bounds__(256) mvsnet_deconv3d_kernel(const float *__restrict__ in, int Di, int Hi, int Wi, const float *__restrict__ prm,
                                                              const float *skip, float *out)
{
    constexpr int GROUPS = COUT / COG;
    static_assert(COUT % COG == 0, "mvsnet_deconv3d_kernel: channel split");
    const int tx = threadIdx.x & (C3_TX - 1), ty = (threadIdx.x / C3_TX) & (C3_TY - 1), tz = threadIdx.x / (C3_TX * C3_TY);
    const int g = blockIdx.z % GROUPS, zc = blockIdx.z / GROUPS, cls = zc & 7, px = cls & 1, py = (cls >> 1) & 1, pz = cls >> 2;
    const int bx = blockIdx.x * C3_TX + tx, by = blockIdx.y * C3_TY + ty, bz = (zc >> 3) * C3_TZ + tz;
    if (bx >= Wi || by >= Hi || bz >= Di) return;
    float acc[COG];
#pragma unroll
    for (int j = 0; j < COG; ++j) acc[j] = 0.f;
    const float *w = prm + g * COG;
    switch (cls) {                                                      // (the same for the whole block)
    case 0: mv_deconv_class<CIN, COUT, COG, 0, 0, 0>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 1: mv_deconv_class<CIN, COUT, COG, 0, 0, 1>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 2: mv_deconv_class<CIN, COUT, COG, 0, 1, 0>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 3: mv_deconv_class<CIN, COUT, COG, 0, 1, 1>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 4: mv_deconv_class<CIN, COUT, COG, 1, 0, 0>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 5: mv_deconv_class<CIN, COUT, COG, 1, 0, 1>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    case 6: mv_deconv_class<CIN, COUT, COG, 1, 1, 0>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    default: mv_deconv_class<CIN, COUT, COG, 1, 1, 1>(in, Di, Hi, Wi, w, bx, by, bz, acc); break;
    }
    const size_t ovol = (size_t)Di * Hi * Wi * 8, o = ((size_t)(2 * bz + pz) * (2 * Hi) + (2 * by + py)) * (2 * Wi) + (2 * bx + px);
#pragma unroll
    for (int j = 0; j < COG; ++j) {
        const size_t e = (size_t)(g * COG + j) * ovol + o;
        out[e] = skip[e] + mv_epilogue<false>(acc[j], prm + CIN * 27 * COUT, COUT, g * COG + j);
    }
}

template <int L, int COG>
static int c3_launch_transposed(const float *in, int Di, int Hi, int Wi, const float *packed, const float *skip, float *out, hipStream_t st)
{
    constexpr C3Layer P = C3_LAYER[L];
    const dim3 grid(cdiv(Wi, C3_TX), cdiv(Hi, C3_TY), cdiv(Di, C3_TZ) * 8 * (P.cout / COG));
    mvsnet_deconv3d_kernel<P.cin, P.cout, COG><<<grid, 256, 0, st>>>(in, Di, Hi, Wi, packed + c3_offset(L), skip, out);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

// ---- the depth head and the points -------------------------------------------------------------------------------------------------------------------
// The logits of a pixel are read twice (the maximum, then the sums): exp(x - max) is what torch's softmax forms, and the second read comes from the L2.
// (The loops are kept from the loop vectoriser: for a one-pixel plane it would pair iterations into packed fp32.)
__global__ void __launch_bounds__(256) mvsnet_depth_head_kernel(const float *__restrict__ logits, const float *__restrict__ dvals, int D, int plane,
                                                                float *__restrict__ depth, float *__restrict__ conf, float *__restrict__ prob)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    const float *l = logits + p;
    float m = l[0];
#pragma clang loop vectorize(disable) interleave(disable)
    for (int k = 1; k < D; ++k) m = fmaxf(m, l[(size_t)k * plane]);
    float S = 0.f, Sd = 0.f, Sk = 0.f;
#pragma clang loop vectorize(disable) interleave(disable)
    for (int k = 0; k < D; ++k) {
        const float e = expf(l[(size_t)k * plane] - m);
        S += e;
        Sd = fmaf(e, dvals[k], Sd);
        Sk = fmaf(e, (float)k, Sk);
    }
    depth[p] = Sd / S;
    const float fi = Sk / S;
    const int idx = fi >= 0.f && fi < (float)D ? (int)fi : 0;          // (a NaN row: index 0, and the NaN shows in depth and confidence)
    float c = 0.f;
    for (int k = idx - 1; k <= idx + 2; ++k)
        if (k >= 0 && k < D) c += expf(l[(size_t)k * plane] - m) / S;
    conf[p] = fi == fi ? c : fi;
    if (prob)
#pragma clang loop vectorize(disable) interleave(disable)
        for (int k = 0; k < D; ++k) prob[(size_t)k * plane + p] = expf(l[(size_t)k * plane] - m) / S;
}

struct Mat3 { float m[9]; };

__global__ void __launch_bounds__(256) mvsnet_depth_points_kernel(const float *__restrict__ depth, const float *__restrict__ conf, int h, int w, int H, int W,
                                                                  float near, float far, Mat3 M, float *__restrict__ cam, float *__restrict__ conf_out,
                                                                  uint8_t *__restrict__ mask)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const int sy = min((int)floorf((float)y * ((float)h / (float)H)), h - 1), sx = min((int)floorf((float)x * ((float)w / (float)W)), w - 1);
    const float d = depth[(size_t)sy * w + sx];
    const float z = fminf(fmaxf((d - near) / (far - near), 0.f), 1.f);
    const float cz = z * (far - near) + near;
    const float cx = (((float)x / (float)(W - 1)) * (float)(W - 1)) * cz, cy = (((float)y / (float)(H - 1)) * (float)(H - 1)) * cz;
    const size_t i = (size_t)y * W + x;
#pragma unroll
    for (int j = 0; j < 3; ++j) cam[3 * i + j] = fmaf(cz, M.m[6 + j], fmaf(cy, M.m[3 + j], cx * M.m[j]));
    conf_out[i] = conf[(size_t)sy * w + sx];
    mask[i] = (d >= near && d <= far) ? 1 : 0;
}

}  // namespace hnr

using namespace hnr;

// two buffers of the largest layer output
extern "C" int64_t hnr_mvsnet_feature_scratch_elems(int V, int H, int W)
{
    if (!mf_shape_ok(V, H, W)) return -1;
    const Pyramid p = pyramid_extents(H, W);
    int64_t m = 8 * (int64_t)H * W;
    if (16 * (int64_t)p.H2 * p.W2 > m) m = 16 * (int64_t)p.H2 * p.W2;
    if (32 * (int64_t)p.H4 * p.W4 > m) m = 32 * (int64_t)p.H4 * p.W4;
    return 2 * m * V;
}

extern "C" int hnr_mvsnet_feature(const float *d_images, int V, int H, int W, const float *d_packed, float *d_feat, float *d_scratch, int64_t scratch_elems,
                                  void *stream)
{
    if (!d_images || !d_packed || !d_feat || !d_scratch) { set_error("hnr_mvsnet_feature: NULL argument"); return HNR_ERR_BADARG; }
    if (!mf_shape_ok(V, H, W)) { set_error("hnr_mvsnet_feature: bad argument (1 <= V <= 64, 4 <= H, W <= 32768)"); return HNR_ERR_BADARG; }
    const int64_t need = hnr_mvsnet_feature_scratch_elems(V, H, W);
    if (scratch_elems < need) { set_error("hnr_mvsnet_feature: scratch smaller than hnr_mvsnet_feature_scratch_elems(V, H, W)"); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const auto [H2, W2, H4, W4] = pyramid_extents(H, W);
    float *a = d_scratch, *b = d_scratch + need / 2;
    if (int rc = mf_launch<0>(d_images, V, H, W, H, W, d_packed, a, st)) return rc;
    if (int rc = mf_launch<1>(a, V, H, W, H, W, d_packed, b, st)) return rc;
    if (int rc = mf_launch<2>(b, V, H, W, H2, W2, d_packed, a, st)) return rc;
    if (int rc = mf_launch<3>(a, V, H2, W2, H2, W2, d_packed, b, st)) return rc;
    if (int rc = mf_launch<4>(b, V, H2, W2, H2, W2, d_packed, a, st)) return rc;
    if (int rc = mf_launch<5>(a, V, H2, W2, H4, W4, d_packed, b, st)) return rc;
    if (int rc = mf_launch<6>(b, V, H4, W4, H4, W4, d_packed, a, st)) return rc;
    return mf_launch<7, EpiBias>(a, V, H4, W4, H4, W4, d_packed, d_feat, st);                     // `feature`
}

extern "C" int hnr_mvsnet_cost_volume(const float *d_feat, int V, int h, int w, const float *d_proj, const float *d_depth_values, int D, float *d_volume,
                                      void *stream)
{
    if (!d_feat || !d_proj || !d_depth_values || !d_volume) { set_error("hnr_mvsnet_cost_volume: NULL argument"); return HNR_ERR_BADARG; }
    if (V < 1 || V > 64 || !mv_volume_ok(D, h, w)) {
        set_error("hnr_mvsnet_cost_volume: bad argument (1 <= V <= 64, 2 <= h, w <= 8192, 1 <= D <= 4096, D*h*w <= 2^26)"); return HNR_ERR_BADARG;
    }
    mvsnet_cost_volume_kernel<<<cdiv((int64_t)D * h * w, 256), 256, 0, (hipStream_t)stream>>>(d_feat, V, h, w, d_proj, d_depth_values, D, d_volume);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

static bool c3_shape_ok(int D, int h, int w) { return mv_volume_ok(D, h, w) && D % 8 == 0 && h % 8 == 0 && w % 8 == 0; }

// conv0 8N | conv1 2N | conv2 2N | conv3 N/2 | conv4 N/2 | conv5 N/8 | conv6 N/8, N = D*h*w; the three transposed layers write over conv3, conv1 and conv0
extern "C" int64_t hnr_mvsnet_cost_reg_scratch_elems(int D, int h, int w)
{
    if (!c3_shape_ok(D, h, w)) return -1;
    const int64_t N = (int64_t)D * h * w;
    return 8 * N + 2 * N + 2 * N + N / 2 + N / 2 + N / 8 + N / 8;
}

extern "C" int hnr_mvsnet_cost_reg(const float *d_volume, int D, int h, int w, const float *d_packed, float *d_logits, float *d_scratch, int64_t scratch_elems,
                                   void *stream)
{
    if (!d_volume || !d_packed || !d_logits || !d_scratch) { set_error("hnr_mvsnet_cost_reg: NULL argument"); return HNR_ERR_BADARG; }
    if (!c3_shape_ok(D, h, w)) {
        set_error("hnr_mvsnet_cost_reg: bad argument (D, h and w multiples of 8 -- the skip connections do not line up otherwise --, D <= 4096, h, w <= 8192, "
                  "D*h*w <= 2^26)");
        return HNR_ERR_BADARG;
    }
    if (scratch_elems < hnr_mvsnet_cost_reg_scratch_elems(D, h, w)) {
        set_error("hnr_mvsnet_cost_reg: scratch smaller than hnr_mvsnet_cost_reg_scratch_elems(D, h, w)"); return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)D * h * w;
    float *c0 = d_scratch, *c1 = c0 + 8 * N, *c2 = c1 + 2 * N, *c3 = c2 + 2 * N, *c4 = c3 + N / 2, *c5 = c4 + N / 2, *c6 = c5 + N / 8;
    if (int rc = c3_launch<0, 8, 2>(d_volume, D, h, w, d_packed, c0, st)) return rc;
    if (int rc = c3_launch<1, 16, 1>(c0, D, h, w, d_packed, c1, st)) return rc;
    if (int rc = c3_launch<2, 16, 2>(c1, D / 2, h / 2, w / 2, d_packed, c2, st)) return rc;
    if (int rc = c3_launch<3, 8, 1>(c2, D / 2, h / 2, w / 2, d_packed, c3, st)) return rc;
    if (int rc = c3_launch<4, 8, 2>(c3, D / 4, h / 4, w / 4, d_packed, c4, st)) return rc;
    if (int rc = c3_launch<5, 8, 1>(c4, D / 4, h / 4, w / 4, d_packed, c5, st)) return rc;
    if (int rc = c3_launch<6, 8, 1>(c5, D / 8, h / 8, w / 8, d_packed, c6, st)) return rc;
    if (int rc = c3_launch_transposed<7, 8>(c6, D / 8, h / 8, w / 8, d_packed, c4, c3, st)) return rc;          // conv4 + conv7(x)
    if (int rc = c3_launch_transposed<8, 16>(c3, D / 4, h / 4, w / 4, d_packed, c2, c1, st)) return rc;          // conv2 + conv9(x)
    if (int rc = c3_launch_transposed<9, 8>(c1, D / 2, h / 2, w / 2, d_packed, c0, c0, st)) return rc;          // conv0 + conv11(x), in place
    return c3_launch<10, 1, 2>(c0, D, h, w, d_packed, d_logits, st);                                            // prob
}

extern "C" int hnr_mvsnet_depth_head(const float *d_logits, const float *d_depth_values, int D, int h, int w, float *d_depth, float *d_conf, float *d_prob,
                                     void *stream)
{
    if (!d_logits || !d_depth_values || !d_depth || !d_conf) { set_error("hnr_mvsnet_depth_head: NULL argument"); return HNR_ERR_BADARG; }
    if (!mv_volume_ok(D, h, w)) {
        set_error("hnr_mvsnet_depth_head: bad argument (2 <= h, w <= 8192, 1 <= D <= 4096, D*h*w <= 2^26)"); return HNR_ERR_BADARG;
    }
    mvsnet_depth_head_kernel<<<cdiv((int64_t)h * w, 256), 256, 0, (hipStream_t)stream>>>(d_logits, d_depth_values, D, h * w, d_depth, d_conf, d_prob);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_mvsnet_depth_points(const float *d_depth, const float *d_conf, int h, int w, int H, int W, float near, float far, const float *Kt_inv,
                                       float *d_cam_xyz, float *d_conf_out, uint8_t *d_mask, void *stream)
{
    if (!d_depth || !d_conf || !Kt_inv || !d_cam_xyz || !d_conf_out || !d_mask) { set_error("hnr_mvsnet_depth_points: NULL argument"); return HNR_ERR_BADARG; }
    if (H < 2 || W < 2 || H > 32768 || W > 32768 || h < 1 || w < 1 || h > H || w > W) {
        set_error("hnr_mvsnet_depth_points: bad argument (2 <= H, W <= 32768, 1 <= h <= H, 1 <= w <= W)"); return HNR_ERR_BADARG;
    }
    Mat3 M;
    for (int i = 0; i < 9; ++i) M.m[i] = Kt_inv[i];
    mvsnet_depth_points_kernel<<<dim3(cdiv(W, 64), cdiv(H, 4)), 256, 0, (hipStream_t)stream>>>(d_depth, d_conf, h, w, H, W, near, far, M, d_cam_xyz, d_conf_out,
                                                                                             d_mask);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
