// The 2-D direct convolution of the two pretrained feature nets (featnet.hip: the init checkpoint's FeatureNet; mvsnet.hip: the depth estimator's), once:
// fp32, one output pixel per thread, COG output channels of it in registers, the input tile with its halo staged in LDS eight input channels at a
// time, the weights read through wave-uniform addresses (scalar loads).  Every sum is one chain of explicit fmaf in (input channel, ky, kx) order:
// two runs give the same bits, and neither COG nor the epilogue changes a sum.  What follows the sums is the epilogue's, a small policy struct.
#pragma once
#include "hnr_launch.h"

namespace hnr {

struct ConvLayer { int cin, cout, ks, stride; };

// the eight 2-D layers both nets share (pad = ks / 2); what differs is behind each layer's weights: mean, mul, bias [cout] -- or bias alone
constexpr int CONV2D_LAYERS = 8;
constexpr ConvLayer CONV2D_LAYER[CONV2D_LAYERS] = {{3, 8, 3, 1}, {8, 8, 3, 1}, {8, 16, 5, 2}, {16, 16, 3, 1}, {16, 16, 3, 1}, {16, 32, 5, 2}, {32, 32, 3, 1}, {32, 32, 3, 1}};

// offset of layer l in the packed parameters (l = CONV2D_LAYERS: what follows them): per layer w [cin][ks][ks][cout], then 3 vectors [cout];
// last_tail: the number of such vectors behind the last layer (3, or 1 for a bias-only one)
constexpr int conv2d_offset(int l, int last_tail)
{
    int o = 0;
    for (int i = 0; i < l; ++i) o += CONV2D_LAYER[i].cin * CONV2D_LAYER[i].ks * CONV2D_LAYER[i].ks * CONV2D_LAYER[i].cout + (i == CONV2D_LAYERS - 1 ? last_tail : 3) * CONV2D_LAYER[i].cout;
    return o;
}

// extents of the half and quarter resolution maps of an H x W image (the two stride-2 layers: (n + 2 * 2 - 5) / 2 + 1)
struct Pyramid { int H2, W2, H4, W4; };
constexpr Pyramid pyramid_extents(int H, int W) { return {(H - 1) / 2 + 1, (W - 1) / 2 + 1, ((H - 1) / 2 + 1 - 1) / 2 + 1, ((W - 1) / 2 + 1 - 1) / 2 + 1}; }

constexpr int CONV_TW = 32, CONV_TH = 8;        // output tile of one block: one pixel per thread, a wave covers two rows of 32
constexpr int CONV_CCH = 8;                     // input channels staged per round

// ---- epilogues.  activate<COUT, COG>(acc, tail, c0, y) runs on the thread's COG sums (output channels c0 ..) before the test for pixels outside the
//      map, store<COUT, COG>(y, tail, c0, o, plane) after it; tail points behind the layer's weights, o at the pixel in channel c0's plane.  Which
//      of the two applies the norm is as each net's kernel had it, so that its generated code stays what it was.
// relu((acc - mean) * mul + bias), or acc + bias for a last layer; prm points behind the layer's weights, j is the output channel
template <bool LAST>
__device__ __forceinline__ float mv_epilogue(float acc, const float *__restrict__ prm, int cout, int j)
{
    if (LAST) return acc + prm[j];
    const float u = (acc - prm[j]) * prm[cout + j] + prm[2 * cout + j];
    return u < 0.f ? 0.f : u;                                           // (a NaN stays a NaN, as in torch's relu)
}

template <bool LAST>
struct EpiBatchNorm {                           // BatchNorm + ReLU: tail = mean, mul, bias; LAST: bias alone.  No kernel argument.
    template <int COUT, int COG>
    __device__ __forceinline__ void activate(const float *acc, const float *, int, float *y) const
    {
#pragma unroll
        for (int j = 0; j < COG; ++j) y[j] = acc[j];
    }
    template <int COUT, int COG>
    __device__ __forceinline__ void store(const float *y, const float *tail, int c0, float *o, size_t plane) const
    {
#pragma unroll
        for (int j = 0; j < COG; ++j) o[j * plane] = mv_epilogue<LAST>(y[j], tail, COUT, c0 + j);
    }
};
using EpiBnRelu = EpiBatchNorm<false>;
using EpiBias = EpiBatchNorm<true>;

// InPlaceABN in inference form + LeakyReLU 0.01: tail = mean, mul, bias.  TOP: followed by a 1x1 toplayer (top = w [co][ci], bias [co]) on the
// COG = COUT activated channels of the pixel.  One kernel argument, `top`, in both forms (the net's launches share one argument list).
template <bool TOP>
struct EpiAbnLeaky {
    const float *__restrict__ top;
    template <int COUT, int COG>
    __device__ __forceinline__ void activate(const float *acc, const float *tail, int c0, float *y) const
    {
        const float *mean = tail + c0, *mul = mean + COUT, *bias = mul + COUT;
#pragma unroll
        for (int j = 0; j < COG; ++j) {
            const float u = (acc[j] - mean[j]) * mul[j] + bias[j];
            y[j] = u >= 0.f ? u : u * 0.01f;
        }
    }
    template <int COUT, int COG>
    __device__ __forceinline__ void store(const float *y, const float *, int, float *o, size_t plane) const
    {
        static_assert(!TOP || COG == COUT, "EpiAbnLeaky: the toplayer needs every channel of the pixel");
        if (!TOP) {
#pragma unroll
            for (int j = 0; j < COG; ++j) o[j * plane] = y[j];
        } else {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
            for (int co = 0; co < COUT; ++co) {                         // (one output at a time: the loop vectoriser would pair them into packed fp32)
                float s = 0.f;
#pragma unroll
                for (int ci = 0; ci < COG; ++ci) s = fmaf(y[ci], top[co * COG + ci], s);
                o[co * plane] = s + top[COUT * COUT + co];
            }
        }
    }
};

// in [V,CIN,Hi,Wi] -> out [V,COUT,Ho,Wo]; blockIdx.z = view * (COUT / COG) + channel group; prm: the layer's w [cin][ks][ks][cout], then its tail.
// EpiArgs: the epilogue's members as kernel arguments of their own (none for a stateless one), so that each is loaded with the others at entry.
template <int CIN, int COUT, int KS, int STRIDE, int COG, class Epi, class... EpiArgs>
__global__ void __launch_bounds__(256) conv2d_direct_kernel(const float *__restrict__ in, int Hi, int Wi, int Ho, int Wo, const float *__restrict__ prm,
                                                            EpiArgs... epi_args, float *__restrict__ out)
{
    const Epi epi{epi_args...};
    extern __shared__ float conv_tile[];
    constexpr int PAD = KS / 2, IW = (CONV_TW - 1) * STRIDE + KS, IH = (CONV_TH - 1) * STRIDE + KS, CCH = CIN < CONV_CCH ? CIN : CONV_CCH, GROUPS = COUT / COG;
    static_assert(CIN % CCH == 0 && COUT % COG == 0, "conv2d_direct_kernel: channel split");
    const int tx = threadIdx.x & (CONV_TW - 1), ty = threadIdx.x / CONV_TW;
    const int g = blockIdx.z % GROUPS, v = blockIdx.z / GROUPS;
    const int ox0 = blockIdx.x * CONV_TW, oy0 = blockIdx.y * CONV_TH;
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
            conv_tile[e] = (iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) ? inv[((size_t)(c0 + ch) * Hi + iy) * Wi + ix] : 0.f;        // zero padding
        }
        __syncthreads();
        const float *t0 = conv_tile + (ty * STRIDE) * IW + tx * STRIDE;
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
    float y[COG];
    epi.template activate<COUT, COG>(acc, prm + CIN * KS * KS * COUT, g * COG, y);
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= Wo || oy >= Ho) return;                                   // (only here: every thread stages and meets the barriers)
    const size_t plane = (size_t)Ho * Wo;
    epi.template store<COUT, COG>(y, prm + CIN * KS * KS * COUT, g * COG, out + ((size_t)v * COUT + g * COG) * plane + (size_t)oy * Wo + ox, plane);
}

// layer L of the table with COG output channels per thread (the caller's choice: it sets register count and occupancy, not a sum's order)
template <int L, int COG, class Epi, class... EpiArgs>
int conv2d_direct_launch(const float *in, int V, int Hi, int Wi, int Ho, int Wo, const float *prm, float *out, hipStream_t st, EpiArgs... epi_args)
{
    constexpr ConvLayer P = CONV2D_LAYER[L];
    constexpr int CCH = P.cin < CONV_CCH ? P.cin : CONV_CCH;
    constexpr int lds = CCH * ((CONV_TH - 1) * P.stride + P.ks) * ((CONV_TW - 1) * P.stride + P.ks) * (int)sizeof(float);
    const dim3 grid(cdiv(Wo, CONV_TW), cdiv(Ho, CONV_TH), V * (P.cout / COG));
    return launch_lds<conv2d_direct_kernel<P.cin, P.cout, P.ks, P.stride, COG, Epi, EpiArgs...>>(grid, dim3(256), lds, st, in, Hi, Wi, Ho, Wo, prm, epi_args..., out);
}

}  // namespace hnr
