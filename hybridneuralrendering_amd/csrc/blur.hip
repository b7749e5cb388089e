// Blur-handling module with pre-defined kernels (the "select the best-matching blur per patch" step of training on blurry
// captures): /root/reference/models/base_rendering_model.py:677-745 (`blur_update_output`, faster_version), called from
// mvs_points_volumetric_model.py:145-146 between the render and the losses.
//
// The rendered batch is a (patch_num*patch_size)^2 grid of rays made of patch_num^2 patches.  Per patch and colour channel the
// reference convolves the patch with each of the N kernels (F.conv2d = cross-correlation, zero padding ks/2, normalised by the
// same convolution of a ones patch so borders are not darkened), appends the un-blurred patch as candidate N, takes the
// candidate with the smallest L1 distance to the ground-truth patch, and puts it back.  Gradients flow through the selected
// convolution only (argmin is piecewise constant).  The reference does this with two F.conv2d calls over [147,1,8,8], a
// 5-D tile/abs/sum, fancy indexing and a Python re-assembly loop; here it is one block per patch.
#include "hnr_common.h"

namespace hnr {

constexpr int BLUR_MAX_PS = 16;      // patch size (8 in every shipped script)
constexpr int BLUR_MAX_N = 31;       // pre-defined kernels (12 or 36 in the scripts)

struct BlurArgs {
    const float *color, *gt;          // [S*S,3] ray layout: ray = row * S + col, S = patch_num * patch_size
    const float *kernels;             // [N, ks, ks]
    int N, ks, pn, ps;
    int n_patches, patch_major;       // patch_major: ray = (patch * ps + y) * ps + x (a rank's whole patches); else the pn x pn grid
    float *out;                       // [S*S,3]
    int32_t *select;                  // [n_patches] chosen candidate (N = un-blurred)
};

__device__ __forceinline__ size_t blur_ray(int p, int y, int x, int pn, int ps, int patch_major)
{
    if (patch_major) return ((size_t)p * ps + y) * ps + x;
    return (size_t)((p / pn) * ps + y) * (pn * ps) + ((p % pn) * ps + x);
}

// One 1024-thread block per patch; the (candidate, position) pairs -- 13 x 192 in the shipped configuration -- are spread over all 16 waves (the first
// form walked the candidates one after the other with 192 of 256 threads busy: 113 us on the critical path of the training step for seven patches).
// Every |candidate - gt| term goes to LDS and each candidate's L1 distance is summed in a FIXED order (positions lane, lane + 64, ... then a butterfly),
// so the selection cannot change from run to run on a near-tie (LDS float atomics across waves could).
constexpr int BLUR_CHUNK = 4096;     // (candidate, position) terms held in LDS at a time
__global__ __launch_bounds__(1024) void blur_select_kernel(BlurArgs a)
{
    __shared__ float s_in[3][BLUR_MAX_PS][BLUR_MAX_PS], s_gt[3][BLUR_MAX_PS][BLUR_MAX_PS];
    __shared__ float s_term[BLUR_CHUNK];
    __shared__ float s_diff[BLUR_MAX_N + 1];
    __shared__ int s_sel;
    const int p = blockIdx.x;
    const int ps = a.ps, half = a.ks / 2;
    const int npos = 3 * ps * ps;
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        s_in[c][y][x] = a.color[3 * ray + c];
        s_gt[c][y][x] = a.gt[3 * ray + c];
    }
    __syncthreads();
    auto blurred = [&](int n, int c, int y, int x) {
        if (n == a.N) return s_in[c][y][x];
        const float *k = a.kernels + (size_t)n * a.ks * a.ks;
        float acc = 0.f, msk = 0.f;
        for (int dy = 0; dy < a.ks; ++dy) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int dx = 0; dx < a.ks; ++dx) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                const float w = k[dy * a.ks + dx];
                acc = fmaf(s_in[c][yy][xx], w, acc);
                msk += w;
            }
        }
        return hnr_div(acc, msk);
    };
    const int per_chunk = BLUR_CHUNK / npos;                   // candidates per LDS chunk (npos <= 768: at least 5)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (int n0 = 0; n0 <= a.N; n0 += per_chunk) {
        const int nc = min(per_chunk, a.N + 1 - n0);
        for (int it = threadIdx.x; it < nc * npos; it += blockDim.x) {
            const int n = n0 + it / npos, t = it % npos;
            const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
            s_term[it] = fabsf(blurred(n, c, y, x) - s_gt[c][y][x]);
        }
        __syncthreads();
        for (int m = wave; m < nc; m += n_waves) {             // one wave per candidate: fixed summation order
            float d = 0.f;
            for (int t = lane; t < npos; t += 64) d += s_term[m * npos + t];
            for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (lane == 0) s_diff[n0 + m] = d;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        int best = 0;
        for (int n = 1; n <= a.N; ++n) if (s_diff[n] < s_diff[best]) best = n;      // first minimum (torch.argmin)
        s_sel = best;
        a.select[p] = best;
    }
    __syncthreads();
    const int sel = s_sel;
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        a.out[3 * ray + c] = blurred(sel, c, y, x);
    }
}

struct BlurBwdArgs {
    const float *g_out;               // [S*S,3]
    const float *kernels;
    const int32_t *select;
    int N, ks, pn, ps;
    int n_patches, patch_major;
    float *g_in;                      // [S*S,3]
};

__global__ __launch_bounds__(256) void blur_select_bwd_kernel(BlurBwdArgs a)
{
    __shared__ float s_g[3][BLUR_MAX_PS][BLUR_MAX_PS];     // g_out / mask_out of the selected kernel
    const int p = blockIdx.x;
    const int ps = a.ps, half = a.ks / 2;
    const int npos = 3 * ps * ps;
    const int sel = a.select[p];
    const float *k = a.kernels + (size_t)(sel < a.N ? sel : 0) * a.ks * a.ks;
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        float g = a.g_out[3 * ray + c];
        if (sel < a.N) {
            float msk = 0.f;
            for (int dy = 0; dy < a.ks; ++dy) {
                const int yy = y + dy - half;
                if (yy < 0 || yy >= ps) continue;
                for (int dx = 0; dx < a.ks; ++dx) {
                    const int xx = x + dx - half;
                    if (xx >= 0 && xx < ps) msk += k[dy * a.ks + dx];
                }
            }
            g = hnr_div(g, msk);
        }
        s_g[c][y][x] = g;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        float acc;
        if (sel >= a.N) {
            acc = s_g[c][y][x];
        } else {
            // out[y0,x0] = sum in[y0+dy-half, x0+dx-half] k[dy,dx]  =>  d in[y,x] = sum_{y0,x0} g[y0,x0] k[y-y0+half, x-x0+half]
            acc = 0.f;
            for (int y0 = 0; y0 < ps; ++y0) {
                const int dy = y - y0 + half;
                if (dy < 0 || dy >= a.ks) continue;
                for (int x0 = 0; x0 < ps; ++x0) {
                    const int dx = x - x0 + half;
                    if (dx < 0 || dx >= a.ks) continue;
                    acc = fmaf(s_g[c][y0][x0], k[dy * a.ks + dx], acc);
                }
            }
        }
        a.g_in[3 * ray + c] = acc;
    }
}


// ------------------------------------------------------------------------------------------------------------------------
// Learnable blur kernels: /root/reference/models/base_rendering_model.py:827-1020 (`learnable_blur_update_output`,
// faster_version).  The training shell turns each patch of the rendered batch and of the ground truth into a grey patch
// (:886-893), a small predictor network (owned by the aggregator, point_aggregators.py:1339-1344) maps the two grey patches
// to one ks x ks kernel per patch, the kernels are normalised / blended with the identity (:897-911, a few hundred floats:
// torch), and every patch is convolved with ITS kernel (grouped F.conv2d = cross-correlation, zero padding ks/2) with one of
// three border rules (:915-923).  Here: one block per patch for the grey patches, for the convolution and for its backward
// (gradients w.r.t. the rendered colours AND the per-patch kernels, so the predictor trains).
// ------------------------------------------------------------------------------------------------------------------------
constexpr int BLUR_MAX_KS = 15;

struct BlurLearnArgs {
    const float *color, *gt;          // [rays,3]
    const float *kernels;             // [n_patches, ks, ks]
    const float *g_out, *g_gray;      // backward inputs
    int ks, pn, ps, n_patches, patch_major, mode;
    float *out;                       // [rays,3]
    float *gray;                      // [n_patches, 2, ps, ps]: channel 0 = ground truth, 1 = render (torch.cat order, :888 / :892)
    float *g_color, *g_kernels;       // backward outputs
};

__global__ __launch_bounds__(256) void blur_gray_kernel(BlurLearnArgs a)
{
    const int p = blockIdx.x, ps = a.ps;
    for (int t = threadIdx.x; t < ps * ps; t += blockDim.x) {
        const int y = t / ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        const float *g = a.gt + 3 * ray, *c = a.color + 3 * ray;
        a.gray[((size_t)p * 2 + 0) * ps * ps + t] = hnr_div((g[0] + g[1]) + g[2], 3.0f);
        a.gray[((size_t)p * 2 + 1) * ps * ps + t] = hnr_div((c[0] + c[1]) + c[2], 3.0f);
    }
}

__global__ __launch_bounds__(256) void blur_gray_bwd_kernel(BlurLearnArgs a)
{
    const int p = blockIdx.x, ps = a.ps;
    for (int t = threadIdx.x; t < ps * ps; t += blockDim.x) {
        const int y = t / ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        const float g = hnr_div(a.g_gray[((size_t)p * 2 + 1) * ps * ps + t], 3.0f);
        a.g_color[3 * ray + 0] = g; a.g_color[3 * ray + 1] = g; a.g_color[3 * ray + 2] = g;
    }
}

// mode 0: out = conv / (mask + 1e-10); mode 1 / 2: out = conv + (1 - mask) * in, mask = the same convolution of a ones patch
// (mode 2 takes no gradient through the mask)
template <int BWD>
__global__ __launch_bounds__(256) void blur_apply_kernel(BlurLearnArgs a)
{
    __shared__ float s_in[3][BLUR_MAX_PS][BLUR_MAX_PS], s_g[3][BLUR_MAX_PS][BLUR_MAX_PS], s_conv[3][BLUR_MAX_PS][BLUR_MAX_PS];
    __shared__ float s_msk[BLUR_MAX_PS][BLUR_MAX_PS], s_dm[BLUR_MAX_PS][BLUR_MAX_PS], s_k[BLUR_MAX_KS * BLUR_MAX_KS];
    const int p = blockIdx.x, ps = a.ps, ks = a.ks, half = ks / 2;
    const int npos = 3 * ps * ps;
    for (int t = threadIdx.x; t < ks * ks; t += blockDim.x) s_k[t] = a.kernels[(size_t)p * ks * ks + t];
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        s_in[c][y][x] = a.color[3 * ray + c];
        if (BWD) s_g[c][y][x] = a.g_out[3 * ray + c];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        float acc = 0.f, msk = 0.f;
        for (int dy = 0; dy < ks; ++dy) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int dx = 0; dx < ks; ++dx) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                const float w = s_k[dy * ks + dx];
                acc = fmaf(s_in[c][yy][xx], w, acc);
                msk += w;
            }
        }
        if (!BWD) {
            const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
            a.out[3 * ray + c] = a.mode == 0 ? hnr_div(acc, msk + 1e-10f) : acc + (1.f - msk) * s_in[c][y][x];
        } else {
            s_conv[c][y][x] = acc;
            if (c == 0) s_msk[y][x] = msk;
        }
    }
    if (!BWD) return;
    __syncthreads();
    // gradient w.r.t. the convolution result (s_g, in place) and w.r.t. the mask value of every output pixel (s_dm)
    for (int t = threadIdx.x; t < ps * ps; t += blockDim.x) {
        const int y = t / ps, x = t % ps;
        const float m = s_msk[y][x];
        float dm = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float g = s_g[c][y][x];
            if (a.mode == 0) {
                const float d = m + 1e-10f;
                dm -= hnr_div(g * s_conv[c][y][x], d * d);
                s_g[c][y][x] = hnr_div(g, d);
            } else {
                dm -= g * s_in[c][y][x];
            }
        }
        s_dm[y][x] = a.mode == 2 ? 0.f : dm;
    }
    __syncthreads();
    // d in[y,x] = sum_{y0,x0} gc[y0,x0] k[y-y0+half, x-x0+half]  (+ (1 - mask[y,x]) g[y,x] for the pass-through term of modes 1 / 2;
    // s_g still holds g itself in those modes)
    for (int t = threadIdx.x; t < npos; t += blockDim.x) {
        const int c = t / (ps * ps), y = (t / ps) % ps, x = t % ps;
        float acc = 0.f;
        for (int y0 = 0; y0 < ps; ++y0) {
            const int dy = y - y0 + half;
            if (dy < 0 || dy >= ks) continue;
            for (int x0 = 0; x0 < ps; ++x0) {
                const int dx = x - x0 + half;
                if (dx < 0 || dx >= ks) continue;
                acc = fmaf(s_g[c][y0][x0], s_k[dy * ks + dx], acc);
            }
        }
        if (a.mode != 0) acc += (1.f - s_msk[y][x]) * s_g[c][y][x];
        const size_t ray = blur_ray(p, y, x, a.pn, ps, a.patch_major);
        a.g_color[3 * ray + c] = acc;
    }
    // d k[dy,dx] = sum over output pixels whose tap (dy,dx) falls inside the patch of (sum_c gc * in[tap] + d mask)
    for (int t = threadIdx.x; t < ks * ks; t += blockDim.x) {
        const int dy = t / ks, dx = t % ks;
        float acc = 0.f;
        for (int y = 0; y < ps; ++y) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int x = 0; x < ps; ++x) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                float v = s_dm[y][x];
                for (int c = 0; c < 3; ++c) v = fmaf(s_g[c][y][x], s_in[c][yy][xx], v);
                acc += v;
            }
        }
        a.g_kernels[(size_t)p * ks * ks + t] = acc;
    }
}


// ------------------------------------------------------------------------------------------------------------------------
// The whole learnable blur module in three launches (hnr_blur_learn_forward / hnr_blur_learn_backward), for the training step
// that builds no autograd graph: grey patches, the predictor's four layers and sigmoid, normalisation, identity blend and the
// per-patch convolution in ONE forward launch; the way back in one per-patch launch plus one weight-gradient launch.
//
// Patch -> workgroup mapping: BL_PB = 4 patches per 256-thread workgroup.  In a layer thread t owns output (t & 127) of the
// patches (t >> 7) and (t >> 7) + 2, so one pass over a weight matrix serves four patches (one patch per workgroup would read
// the 238 KB of weights 49 times from L2, this reads them 13 times) while 49 patches still spread over 13 CUs; four is also
// the number of waves, and the per-patch reductions (kernel sums, softmax) are one wave per patch.  The forward layer streams
// W[o][i] through LDS in [128 x 32] tiles (coalesced along i, transposed so that thread o reads its row conflict-free; the next
// tile's loads are in flight while this one is consumed); the backward layer reads W[o][i] along i directly (coalesced).
// Summation orders (all fixed by the code): y[o] = b[o] then + W[o][i] a[i] for i ascending, one FMA chain; the input gradient
// sum_o delta[o] W[o][i] for o ascending, one FMA chain; sums over a kernel's taps: lane-strided partial sums, then a butterfly.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int BL_H = 128;                                     // hidden width of the predictor
constexpr int BL_PB = 4;                                      // patches per workgroup = waves per workgroup
constexpr int BL_TK = 32;                                     // input columns per staged weight tile
constexpr int BL_PP = BLUR_MAX_PS * BLUR_MAX_PS;              // 256 pixels per patch at most
constexpr int BL_MAX_IN = 2 * BL_PP;                          // 512
constexpr int BL_KK = BLUR_MAX_KS * BLUR_MAX_KS;              // 225 taps at most
constexpr int BL_LDK = BL_KK + 3;                             // row length of the per-patch tap arrays (>= n_out = 226)

struct BlurFusedArgs {
    const float *color, *gt, *g_out;
    const float *w[4], *b[4];
    float *gw[4], *gb[4];
    float *ws;
    float *out, *kernels, *g_color;
    int ks, pn, ps, n_patches, patch_major, bmode, kmode, knorm, n_in, n_out;
    float slope;
};

// Workspace layout in floats (every part a multiple of 4 floats from the base): a0 [N, n_in] grey gt | grey render, a1..a3 [N, 128] the LeakyReLU
// outputs, pred [N, n_out] the sigmoid outputs, kern [N, ks^2] the final kernels, d0..d2 [N, 128] and d3 [N, n_out] the delta rows.
struct BlurWs { size_t a[4], pred, kern, d[4], total; };
__host__ __device__ inline BlurWs blur_ws(int N, int n_in, int n_out, int kk)
{
    auto up = [](size_t v) { return (v + 3) & ~(size_t)3; };
    BlurWs w;
    size_t o = 0;
    w.a[0] = o; o += up((size_t)N * n_in);
    for (int l = 1; l < 4; ++l) { w.a[l] = o; o += (size_t)N * BL_H; }
    w.pred = o; o += up((size_t)N * n_out);
    w.kern = o; o += up((size_t)N * kk);
    for (int l = 0; l < 3; ++l) { w.d[l] = o; o += (size_t)N * BL_H; }
    w.d[3] = o; o += up((size_t)N * n_out);
    w.total = o;
    return w;
}

__device__ __forceinline__ float bl_wave_sum(float v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// y[q][o] = b[o] + sum_i W[o][i] s_a[q][i] for the workgroup's four patches q, all o < n_out; epi(q, o, y) stores.  Starts with a barrier (the
// activations another layer's epilogue wrote are visible); epi must not write what this call reads.
template <class Epi>
__device__ __forceinline__ void bl_linear(const float *W, const float *B, int K, int n_out, const float *s_a, int lda, float (*s_w)[BL_H + 1], Epi epi)
{
    const int tid = threadIdx.x, ol = tid & (BL_H - 1), pg = tid >> 7;
    const int tr = tid >> 5, tc = tid & 31;                   // tile element (row tr + 8 q, column tc) of load q
    for (int o0 = 0; o0 < n_out; o0 += BL_H) {
        const int o = o0 + ol;
        float acc0 = o < n_out ? B[o] : 0.f, acc1 = acc0;
        float r[16];
        auto load = [&](int i0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int oo = o0 + tr + 8 * q, ii = i0 + tc;
                r[q] = (oo < n_out && ii < K) ? W[(size_t)oo * K + ii] : 0.f;
            }
        };
        load(0);
        for (int i0 = 0; i0 < K; i0 += BL_TK) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16; ++q) s_w[tc][tr + 8 * q] = r[q];
            __syncthreads();
            if (i0 + BL_TK < K) load(i0 + BL_TK);
            const int kk = min(BL_TK, K - i0);
            const float *a0 = s_a + (size_t)pg * lda + i0, *a1 = s_a + (size_t)(pg + 2) * lda + i0;
#pragma unroll 8
            for (int ii = 0; ii < kk; ++ii) {
                const float w = s_w[ii][ol];
                acc0 = fmaf(w, a0[ii], acc0);
                acc1 = fmaf(w, a1[ii], acc1);
            }
        }
        if (o < n_out) { epi(pg, o, acc0); epi(pg + 2, o, acc1); }
    }
}

// g[q][i] = sum_o s_d[q][o] W[o][i] (o ascending) for i_lo <= i < i_hi; epi(q, i, g) stores.  No barrier inside.
template <class Epi>
__device__ __forceinline__ void bl_linear_t(const float *W, int K, int i_lo, int i_hi, int n_o, const float *s_d, int ldd, Epi epi)
{
    const int tid = threadIdx.x, pg = tid >> 7;
    const float *d0 = s_d + (size_t)pg * ldd, *d1 = s_d + (size_t)(pg + 2) * ldd;
    for (int i = i_lo + (tid & (BL_H - 1)); i < i_hi; i += BL_H) {
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 8
        for (int o = 0; o < n_o; ++o) {
            const float w = W[(size_t)o * K + i];
            acc0 = fmaf(d0[o], w, acc0);
            acc1 = fmaf(d1[o], w, acc1);
        }
        epi(pg, i, acc0); epi(pg + 2, i, acc1);
    }
}

// One wave, one patch: the final kernel from the prediction (:895-909).  k1 = the normalised kernel before the blend; k (may be NULL) = the final
// one; S, w, S2 = the first normaliser, the blend weight and the second normaliser.  Every lane touches only the taps lane, lane + 64, ...
__device__ __forceinline__ void bl_make_kernel(const float *pred, float *k1, float *k, int kk, int knorm, int kmode, int lane, float &S, float &w, float &S2)
{
    float s = 0.f;
    if (knorm == 0) {
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) s += pred[j];
        S = bl_wave_sum(s);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) k1[j] = hnr_div(pred[j], S);
    } else {
        float m = -3.0e38f;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) m = fmaxf(m, pred[j]);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) { const float e = expf(pred[j] - m); k1[j] = e; s += e; }
        S = bl_wave_sum(s);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) k1[j] = hnr_div(k1[j], S);
    }
    w = 1.f; S2 = 1.f;
    if (kmode == 4) {
        w = pred[kk];
        float s2 = 0.f;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) s2 += w * k1[j] + (1.f - w) * (j == kk / 2 ? 1.f : 0.f);
        S2 = bl_wave_sum(s2);
    }
    if (k)
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) k[j] = kmode == 4 ? hnr_div(w * k1[j] + (1.f - w) * (j == kk / 2 ? 1.f : 0.f), S2) : k1[j];
}

__global__ __launch_bounds__(256) void blur_learn_fwd_kernel(BlurFusedArgs a)
{
    __shared__ float s_w[BL_TK][BL_H + 1];
    __shared__ float s_col[BL_PB][3][BL_PP];
    __shared__ float s_a0[BL_PB][BL_MAX_IN];
    __shared__ float s_h[2][BL_PB][BL_H];
    __shared__ float s_pred[BL_PB][BL_LDK], s_k1[BL_PB][BL_LDK], s_k[BL_PB][BL_LDK];
    const int tid = threadIdx.x, p0 = blockIdx.x * BL_PB, N = a.n_patches;
    const int ps = a.ps, pp = ps * ps, ks = a.ks, kk = ks * ks, half = ks / 2, n_in = a.n_in, n_out = a.n_out;
    const BlurWs ws = blur_ws(N, n_in, n_out, kk);
    // the patches and their grey versions (hnr_blur_gray_patches' arithmetic and order: ground truth first)
    for (int t = tid; t < BL_PB * pp; t += blockDim.x) {
        const int q = t / pp, s = t % pp, p = p0 + q;
        float c0 = 0.f, c1 = 0.f, c2 = 0.f, gg = 0.f, gc = 0.f;
        if (p < N) {
            const size_t ray = blur_ray(p, s / ps, s % ps, a.pn, ps, a.patch_major);
            const float *g = a.gt + 3 * ray, *c = a.color + 3 * ray;
            c0 = c[0]; c1 = c[1]; c2 = c[2];
            gg = hnr_div((g[0] + g[1]) + g[2], 3.0f);
            gc = hnr_div((c0 + c1) + c2, 3.0f);
            a.ws[ws.a[0] + (size_t)p * n_in + s] = gg;
            a.ws[ws.a[0] + (size_t)p * n_in + pp + s] = gc;
        }
        s_col[q][0][s] = c0; s_col[q][1][s] = c1; s_col[q][2][s] = c2;
        s_a0[q][s] = gg; s_a0[q][pp + s] = gc;
    }
    const float slope = a.slope;
    auto hidden = [&](float *dst, size_t off) {
        return [=](int q, int o, float y) {
            y = y > 0.f ? y : y * slope;
            dst[q * BL_H + o] = y;
            if (p0 + q < N) a.ws[off + (size_t)(p0 + q) * BL_H + o] = y;
        };
    };
    bl_linear(a.w[0], a.b[0], n_in, BL_H, &s_a0[0][0], BL_MAX_IN, s_w, hidden(&s_h[0][0][0], ws.a[1]));
    bl_linear(a.w[1], a.b[1], BL_H, BL_H, &s_h[0][0][0], BL_H, s_w, hidden(&s_h[1][0][0], ws.a[2]));
    bl_linear(a.w[2], a.b[2], BL_H, BL_H, &s_h[1][0][0], BL_H, s_w, hidden(&s_h[0][0][0], ws.a[3]));
    bl_linear(a.w[3], a.b[3], BL_H, n_out, &s_h[0][0][0], BL_H, s_w, [&](int q, int o, float y) {
        const float s = hnr_div(1.0f, 1.0f + expf(-y));
        s_pred[q][o] = s;
        if (p0 + q < N) a.ws[ws.pred + (size_t)(p0 + q) * n_out + o] = s;
    });
    __syncthreads();
    {   // wave q: the kernel of patch q
        const int q = tid >> 6, lane = tid & 63;
        float S, w, S2;
        bl_make_kernel(s_pred[q], s_k1[q], s_k[q], kk, a.knorm, a.kmode, lane, S, w, S2);
        if (p0 + q < N)
#pragma clang loop vectorize(disable) interleave(disable)
            for (int j = lane; j < kk; j += 64) {
                a.ws[ws.kern + (size_t)(p0 + q) * kk + j] = s_k[q][j];
                if (a.kernels) a.kernels[(size_t)(p0 + q) * kk + j] = s_k[q][j];
            }
    }
    __syncthreads();
    // every patch convolved with its kernel (blur_apply_kernel<0>'s arithmetic)
    for (int t = tid; t < BL_PB * 3 * pp; t += blockDim.x) {
        const int q = t / (3 * pp), c = (t / pp) % 3, s = t % pp, y = s / ps, x = s % ps;
        if (p0 + q >= N) continue;
        float acc = 0.f, msk = 0.f;
        for (int dy = 0; dy < ks; ++dy) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int dx = 0; dx < ks; ++dx) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                const float w = s_k[q][dy * ks + dx];
                acc = fmaf(s_col[q][c][yy * ps + xx], w, acc);
                msk += w;
            }
        }
        const size_t ray = blur_ray(p0 + q, y, x, a.pn, ps, a.patch_major);
        a.out[3 * ray + c] = a.bmode == 0 ? hnr_div(acc, msk + 1e-10f) : acc + (1.f - msk) * s_col[q][c][s];
    }
}

__global__ __launch_bounds__(256) void blur_learn_bwd_kernel(BlurFusedArgs a)
{
    __shared__ float s_in[BL_PB][3][BL_PP], s_g[BL_PB][3][BL_PP], s_conv[BL_PB][3][BL_PP];
    __shared__ float s_msk[BL_PB][BL_PP], s_dm[BL_PB][BL_PP];
    __shared__ float s_pred[BL_PB][BL_LDK], s_k1[BL_PB][BL_LDK], s_k[BL_PB][BL_LDK], s_gk[BL_PB][BL_LDK];
    __shared__ float s_d[2][BL_PB][BL_H];
    const int tid = threadIdx.x, p0 = blockIdx.x * BL_PB, N = a.n_patches;
    const int ps = a.ps, pp = ps * ps, ks = a.ks, kk = ks * ks, half = ks / 2, n_in = a.n_in, n_out = a.n_out;
    const BlurWs ws = blur_ws(N, n_in, n_out, kk);
    for (int t = tid; t < BL_PB * 3 * pp; t += blockDim.x) {
        const int q = t / (3 * pp), c = (t / pp) % 3, s = t % pp;
        float v = 0.f, g = 0.f;
        if (p0 + q < N) {
            const size_t ray = blur_ray(p0 + q, s / ps, s % ps, a.pn, ps, a.patch_major);
            v = a.color[3 * ray + c]; g = a.g_out[3 * ray + c];
        }
        s_in[q][c][s] = v; s_g[q][c][s] = g;
    }
    for (int t = tid; t < BL_PB * BL_LDK; t += blockDim.x) {
        const int q = t / BL_LDK, j = t % BL_LDK;
        const bool ok = p0 + q < N;
        s_pred[q][j] = ok && j < n_out ? a.ws[ws.pred + (size_t)(p0 + q) * n_out + j] : 0.5f;
        s_k[q][j] = ok && j < kk ? a.ws[ws.kern + (size_t)(p0 + q) * kk + j] : 0.f;
    }
    __syncthreads();
    // the convolution again (its result for boundary_mode 0, the mask value of every pixel)
    for (int t = tid; t < BL_PB * 3 * pp; t += blockDim.x) {
        const int q = t / (3 * pp), c = (t / pp) % 3, s = t % pp, y = s / ps, x = s % ps;
        float acc = 0.f, msk = 0.f;
        for (int dy = 0; dy < ks; ++dy) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int dx = 0; dx < ks; ++dx) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                const float w = s_k[q][dy * ks + dx];
                acc = fmaf(s_in[q][c][yy * ps + xx], w, acc);
                msk += w;
            }
        }
        s_conv[q][c][s] = acc;
        if (c == 0) s_msk[q][s] = msk;
    }
    __syncthreads();
    // gradient w.r.t. the convolution result (s_g, in place) and w.r.t. the mask value of every output pixel (s_dm); blur_apply_kernel<1>'s steps
    for (int t = tid; t < BL_PB * pp; t += blockDim.x) {
        const int q = t / pp, s = t % pp;
        const float m = s_msk[q][s];
        float dm = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float g = s_g[q][c][s];
            if (a.bmode == 0) {
                const float d = m + 1e-10f;
                dm -= hnr_div(g * s_conv[q][c][s], d * d);
                s_g[q][c][s] = p0 + q < N ? hnr_div(g, d) : 0.f;
            } else {
                dm -= g * s_in[q][c][s];
            }
        }
        s_dm[q][s] = (a.bmode == 2 || p0 + q >= N) ? 0.f : dm;
    }
    __syncthreads();
    // convolution path of the colour gradient -> s_conv (its old content is used up)
    for (int t = tid; t < BL_PB * 3 * pp; t += blockDim.x) {
        const int q = t / (3 * pp), c = (t / pp) % 3, s = t % pp, y = s / ps, x = s % ps;
        float acc = 0.f;
        for (int y0 = 0; y0 < ps; ++y0) {
            const int dy = y - y0 + half;
            if (dy < 0 || dy >= ks) continue;
            for (int x0 = 0; x0 < ps; ++x0) {
                const int dx = x - x0 + half;
                if (dx < 0 || dx >= ks) continue;
                acc = fmaf(s_g[q][c][y0 * ps + x0], s_k[q][dy * ks + dx], acc);
            }
        }
        if (a.bmode != 0) acc += (1.f - s_msk[q][s]) * s_g[q][c][s];
        s_conv[q][c][s] = acc;
    }
    // gradient w.r.t. the final kernel's taps
    for (int t = tid; t < BL_PB * kk; t += blockDim.x) {
        const int q = t / kk, j = t % kk, dy = j / ks, dx = j % ks;
        float acc = 0.f;
        for (int y = 0; y < ps; ++y) {
            const int yy = y + dy - half;
            if (yy < 0 || yy >= ps) continue;
            for (int x = 0; x < ps; ++x) {
                const int xx = x + dx - half;
                if (xx < 0 || xx >= ps) continue;
                float v = s_dm[q][y * ps + x];
                for (int c = 0; c < 3; ++c) v = fmaf(s_g[q][c][y * ps + x], s_in[q][c][yy * ps + xx], v);
                acc += v;
            }
        }
        s_gk[q][j] = acc;
    }
    __syncthreads();
    {   // wave q, patch q: renormalisation, blend, normalisation / softmax, sigmoid -> delta of the last layer, in place in s_gk
        const int q = tid >> 6, lane = tid & 63;
        float S, w, S2;
        bl_make_kernel(s_pred[q], s_k1[q], nullptr, kk, a.knorm, a.kmode, lane, S, w, S2);
        float *g = s_gk[q];
        const float *k1 = s_k1[q], *k = s_k[q], *pr = s_pred[q];
        float gw = 0.f;
        if (a.kmode == 4) {
            // k = k2 / S2, k2 = w k1 + (1 - w) ident
            float dot = 0.f;
#pragma clang loop vectorize(disable) interleave(disable)
            for (int j = lane; j < kk; j += 64) dot += g[j] * k[j];
            dot = bl_wave_sum(dot);
#pragma clang loop vectorize(disable) interleave(disable)
            for (int j = lane; j < kk; j += 64) {
                const float g2 = hnr_div(g[j] - dot, S2);
                gw += g2 * (k1[j] - (j == kk / 2 ? 1.f : 0.f));
                g[j] = w * g2;
            }
            gw = bl_wave_sum(gw);
        }
        float dot1 = 0.f;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < kk; j += 64) dot1 += g[j] * k1[j];
        dot1 = bl_wave_sum(dot1);
        const bool ok = p0 + q < N;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int j = lane; j < n_out; j += 64) {
            float gp;
            if (j < kk) gp = a.knorm == 0 ? hnr_div(g[j] - dot1, S) : k1[j] * (g[j] - dot1);
            else gp = gw;
            const float s = pr[j];
            const float d = ok ? gp * ((1.f - s) * s) : 0.f;
            g[j] = d;
            if (ok) a.ws[ws.d[3] + (size_t)(p0 + q) * n_out + j] = d;
        }
    }
    __syncthreads();
    const float slope = a.slope;
    auto hidden = [&](float *dst, int l) {       // delta of layer l - 1 from the gradient of its LeakyReLU output a_l (sign of the stored output)
        return [=](int q, int i, float gacc) {
            float d = 0.f;
            if (p0 + q < N) {
                const float act = a.ws[ws.a[l] + (size_t)(p0 + q) * BL_H + i];
                d = act > 0.f ? gacc : gacc * slope;
                a.ws[ws.d[l - 1] + (size_t)(p0 + q) * BL_H + i] = d;
            }
            dst[q * BL_H + i] = d;
        };
    };
    bl_linear_t(a.w[3], BL_H, 0, BL_H, n_out, &s_gk[0][0], BL_LDK, hidden(&s_d[0][0][0], 3));
    __syncthreads();
    bl_linear_t(a.w[2], BL_H, 0, BL_H, BL_H, &s_d[0][0][0], BL_H, hidden(&s_d[1][0][0], 2));
    __syncthreads();
    bl_linear_t(a.w[1], BL_H, 0, BL_H, BL_H, &s_d[1][0][0], BL_H, hidden(&s_d[0][0][0], 1));
    __syncthreads();
    // the grey rendered patch is the second half of the first layer's input; d grey / d colour = 1/3 per channel (hnr_blur_gray_patches_bwd)
    bl_linear_t(a.w[0], n_in, pp, 2 * pp, BL_H, &s_d[0][0][0], BL_H, [&](int q, int i, float gacc) { s_dm[q][i - pp] = hnr_div(gacc, 3.0f); });
    __syncthreads();
    for (int t = tid; t < BL_PB * 3 * pp; t += blockDim.x) {
        const int q = t / (3 * pp), c = (t / pp) % 3, s = t % pp;
        if (p0 + q >= N) continue;
        const size_t ray = blur_ray(p0 + q, s / ps, s % ps, a.pn, ps, a.patch_major);
        a.g_color[3 * ray + c] = s_conv[q][c][s] + s_dm[q][s];
    }
}

// dW_l[o][i] = sum_p delta_l[p][o] a_(l-1)[p][i], db_l[o] = sum_p delta_l[p][o]: one thread per element (the bias is column in_l), p ascending in one
// chain, nn.Linear's layout.  blockIdx.y = layer.
__global__ __launch_bounds__(256) void blur_learn_wgrad_kernel(BlurFusedArgs a)
{
    const int l = blockIdx.y, N = a.n_patches;
    const int K = l == 0 ? a.n_in : BL_H, O = l == 3 ? a.n_out : BL_H;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= O * (K + 1)) return;
    const int o = e / (K + 1), i = e % (K + 1);
    const BlurWs ws = blur_ws(N, a.n_in, a.n_out, a.ks * a.ks);
    size_t od, oa;                                             // (constant indices: the argument block stays in registers)
    float *gw, *gb;
    switch (l) {
    case 0: od = ws.d[0]; oa = ws.a[0]; gw = a.gw[0]; gb = a.gb[0]; break;
    case 1: od = ws.d[1]; oa = ws.a[1]; gw = a.gw[1]; gb = a.gb[1]; break;
    case 2: od = ws.d[2]; oa = ws.a[2]; gw = a.gw[2]; gb = a.gb[2]; break;
    default: od = ws.d[3]; oa = ws.a[3]; gw = a.gw[3]; gb = a.gb[3]; break;
    }
    const float *d = a.ws + od + o, *act = a.ws + oa + (i < K ? i : 0);
    float acc = 0.f;
    if (i < K) {
        for (int p = 0; p < N; ++p) acc = fmaf(d[(size_t)p * O], act[(size_t)p * K], acc);
        gw[(size_t)o * K + i] = acc;
    } else {
        for (int p = 0; p < N; ++p) acc += d[(size_t)p * O];
        gb[o] = acc;
    }
}

}  // namespace hnr

using namespace hnr;

static int blur_check(int N, int ks, int pn, int ps, const char *who)
{
    if (N < 0 || N > BLUR_MAX_N || ks <= 0 || (ks & 1) == 0 || pn == 0 || ps <= 0 || ps > BLUR_MAX_PS) {
        set_error("%s: unsupported sizes (N <= %d kernels, odd kernel size, patch size <= %d)", who, BLUR_MAX_N, BLUR_MAX_PS);
        return HNR_ERR_BADARG;
    }
    return HNR_OK;
}

extern "C" int hnr_blur_select(const float *d_color, const float *d_gt, const float *d_kernels, int n_kernels, int kernel_size,
                               int patch_num, int patch_size, float *d_out, int32_t *d_select, void *stream)
{
    if (blur_check(n_kernels, kernel_size, patch_num, patch_size, "hnr_blur_select") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_color || !d_gt || (n_kernels > 0 && !d_kernels) || !d_out || !d_select) { set_error("hnr_blur_select: NULL argument"); return HNR_ERR_BADARG; }
    BlurArgs a;
    a.color = d_color; a.gt = d_gt; a.kernels = d_kernels; a.N = n_kernels; a.ks = kernel_size; a.ps = patch_size;
    a.patch_major = patch_num < 0; a.pn = patch_num < 0 ? 1 : patch_num; a.n_patches = patch_num < 0 ? -patch_num : patch_num * patch_num;
    a.out = d_out; a.select = d_select;
    blur_select_kernel<<<a.n_patches, 1024, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_blur_select_bwd(const float *d_g_out, const float *d_kernels, const int32_t *d_select, int n_kernels, int kernel_size,
                                   int patch_num, int patch_size, float *d_g_in, void *stream)
{
    if (blur_check(n_kernels, kernel_size, patch_num, patch_size, "hnr_blur_select_bwd") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_g_out || (n_kernels > 0 && !d_kernels) || !d_select || !d_g_in) { set_error("hnr_blur_select_bwd: NULL argument"); return HNR_ERR_BADARG; }
    BlurBwdArgs a;
    a.g_out = d_g_out; a.kernels = d_kernels; a.select = d_select; a.N = n_kernels; a.ks = kernel_size; a.ps = patch_size;
    a.patch_major = patch_num < 0; a.pn = patch_num < 0 ? 1 : patch_num; a.n_patches = patch_num < 0 ? -patch_num : patch_num * patch_num;
    a.g_in = d_g_in;
    blur_select_bwd_kernel<<<a.n_patches, 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

static int blur_learn_fill(BlurLearnArgs &a, int kernel_size, int patch_num, int patch_size, int mode, const char *who)
{
    if (kernel_size <= 0 || (kernel_size & 1) == 0 || kernel_size > BLUR_MAX_KS || patch_num == 0 || patch_size <= 0 || patch_size > BLUR_MAX_PS ||
        mode < 0 || mode > 2) {
        set_error("%s: unsupported sizes (odd kernel size <= %d, patch size <= %d, boundary_mode 0..2)", who, BLUR_MAX_KS, BLUR_MAX_PS);
        return HNR_ERR_BADARG;
    }
    memset(&a, 0, sizeof(a));
    a.ks = kernel_size; a.ps = patch_size; a.mode = mode;
    a.patch_major = patch_num < 0; a.pn = patch_num < 0 ? 1 : patch_num; a.n_patches = patch_num < 0 ? -patch_num : patch_num * patch_num;
    return HNR_OK;
}

extern "C" int hnr_blur_gray_patches(const float *d_color, const float *d_gt, int patch_num, int patch_size, float *d_gray, void *stream)
{
    BlurLearnArgs a;
    if (blur_learn_fill(a, 1, patch_num, patch_size, 0, "hnr_blur_gray_patches") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_color || !d_gt || !d_gray) { set_error("hnr_blur_gray_patches: NULL argument"); return HNR_ERR_BADARG; }
    a.color = d_color; a.gt = d_gt; a.gray = d_gray;
    blur_gray_kernel<<<a.n_patches, 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_blur_gray_patches_bwd(const float *d_g_gray, int patch_num, int patch_size, float *d_g_color, void *stream)
{
    BlurLearnArgs a;
    if (blur_learn_fill(a, 1, patch_num, patch_size, 0, "hnr_blur_gray_patches_bwd") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_g_gray || !d_g_color) { set_error("hnr_blur_gray_patches_bwd: NULL argument"); return HNR_ERR_BADARG; }
    a.g_gray = d_g_gray; a.g_color = d_g_color;
    blur_gray_bwd_kernel<<<a.n_patches, 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_blur_apply(const float *d_color, const float *d_kernels, int kernel_size, int patch_num, int patch_size,
                              int boundary_mode, float *d_out, void *stream)
{
    BlurLearnArgs a;
    if (blur_learn_fill(a, kernel_size, patch_num, patch_size, boundary_mode, "hnr_blur_apply") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_color || !d_kernels || !d_out) { set_error("hnr_blur_apply: NULL argument"); return HNR_ERR_BADARG; }
    a.color = d_color; a.kernels = d_kernels; a.out = d_out;
    blur_apply_kernel<0><<<a.n_patches, 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_blur_apply_bwd(const float *d_g_out, const float *d_color, const float *d_kernels, int kernel_size, int patch_num,
                                  int patch_size, int boundary_mode, float *d_g_color, float *d_g_kernels, void *stream)
{
    BlurLearnArgs a;
    if (blur_learn_fill(a, kernel_size, patch_num, patch_size, boundary_mode, "hnr_blur_apply_bwd") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_g_out || !d_color || !d_kernels || !d_g_color || !d_g_kernels) { set_error("hnr_blur_apply_bwd: NULL argument"); return HNR_ERR_BADARG; }
    a.g_out = d_g_out; a.color = d_color; a.kernels = d_kernels; a.g_color = d_g_color; a.g_kernels = d_g_kernels;
    blur_apply_kernel<1><<<a.n_patches, 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

static int blur_fused_fill(BlurFusedArgs &a, const hnr_blur_learn_params *prm, const hnr_blur_learn_weights *w, const char *who)
{
    if (!prm || !w) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    const int ks = prm->kernel_size, ps = prm->patch_size;
    if (ks <= 0 || (ks & 1) == 0 || ks > BLUR_MAX_KS || prm->patch_num == 0 || ps <= 0 || ps > BLUR_MAX_PS) {
        set_error("%s: unsupported sizes (odd kernel size <= %d, patch size <= %d, patch_num != 0)", who, BLUR_MAX_KS, BLUR_MAX_PS);
        return HNR_ERR_BADARG;
    }
    if ((prm->kernel_mode != 0 && prm->kernel_mode != 4) || prm->kernel_norm < 0 || prm->kernel_norm > 1 || prm->boundary_mode < 0 || prm->boundary_mode > 2) {
        set_error("%s: kernel_mode must be 0 or 4, kernel_norm 0 or 1, boundary_mode 0..2", who);
        return HNR_ERR_BADARG;
    }
    const int64_t n = prm->patch_num < 0 ? -(int64_t)prm->patch_num : (int64_t)prm->patch_num * prm->patch_num;
    if (n > (1 << 20)) { set_error("%s: too many patches (%lld)", who, (long long)n); return HNR_ERR_BADARG; }
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < 4; ++l) {
        if (!w->w[l] || !w->b[l]) { set_error("%s: NULL weight pointer (layer %d)", who, l); return HNR_ERR_BADARG; }
        a.w[l] = w->w[l]; a.b[l] = w->b[l];
    }
    a.ks = ks; a.ps = ps; a.bmode = prm->boundary_mode; a.kmode = prm->kernel_mode; a.knorm = prm->kernel_norm; a.slope = prm->slope;
    a.patch_major = prm->patch_num < 0; a.pn = prm->patch_num < 0 ? 1 : prm->patch_num; a.n_patches = (int)n;
    a.n_in = 2 * ps * ps; a.n_out = ks * ks + (prm->kernel_mode == 4 ? 1 : 0);
    return HNR_OK;
}

static int blur_fused_ws(BlurFusedArgs &a, void *d_ws, int64_t ws_bytes, const char *who)
{
    const int64_t need = (int64_t)(blur_ws(a.n_patches, a.n_in, a.n_out, a.ks * a.ks).total * sizeof(float));
    if (!d_ws || ws_bytes < need || ((uintptr_t)d_ws & 15) != 0) {
        set_error("%s: the workspace must be 16-byte aligned and hold %lld bytes (hnr_blur_learn_workspace_bytes), got %lld", who, (long long)need,
                  (long long)ws_bytes);
        return HNR_ERR_BADARG;
    }
    a.ws = (float *)d_ws;
    return HNR_OK;
}

extern "C" int64_t hnr_blur_learn_workspace_bytes(int n_patches, int patch_size, int kernel_size, int kernel_mode)
{
    if (n_patches <= 0 || n_patches > (1 << 20) || patch_size <= 0 || patch_size > BLUR_MAX_PS || kernel_size <= 0 || (kernel_size & 1) == 0 ||
        kernel_size > BLUR_MAX_KS || (kernel_mode != 0 && kernel_mode != 4)) {
        set_error("hnr_blur_learn_workspace_bytes: unsupported sizes (patches > 0, patch size <= %d, odd kernel size <= %d, kernel_mode 0 or 4)",
                  BLUR_MAX_PS, BLUR_MAX_KS);
        return HNR_ERR_BADARG;
    }
    return (int64_t)(blur_ws(n_patches, 2 * patch_size * patch_size, kernel_size * kernel_size + (kernel_mode == 4 ? 1 : 0), kernel_size * kernel_size).total *
                     sizeof(float));
}

extern "C" int hnr_blur_learn_forward(const hnr_blur_learn_params *prm, const hnr_blur_learn_weights *weights, const float *d_color, const float *d_gt,
                                      void *d_ws, int64_t ws_bytes, float *d_out, float *d_kernels, void *stream)
{
    BlurFusedArgs a;
    if (blur_fused_fill(a, prm, weights, "hnr_blur_learn_forward") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_color || !d_gt || !d_out) { set_error("hnr_blur_learn_forward: NULL argument"); return HNR_ERR_BADARG; }
    if (blur_fused_ws(a, d_ws, ws_bytes, "hnr_blur_learn_forward") != HNR_OK) return HNR_ERR_BADARG;
    a.color = d_color; a.gt = d_gt; a.out = d_out; a.kernels = d_kernels;
    blur_learn_fwd_kernel<<<cdiv(a.n_patches, BL_PB), 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_blur_learn_backward(const hnr_blur_learn_params *prm, const hnr_blur_learn_weights *weights, const float *d_color, const float *d_g_out,
                                       void *d_ws, int64_t ws_bytes, float *d_g_color, const hnr_blur_learn_weights *grads, void *stream)
{
    BlurFusedArgs a;
    if (blur_fused_fill(a, prm, weights, "hnr_blur_learn_backward") != HNR_OK) return HNR_ERR_BADARG;
    if (!d_color || !d_g_out || !d_g_color || !grads) { set_error("hnr_blur_learn_backward: NULL argument"); return HNR_ERR_BADARG; }
    for (int l = 0; l < 4; ++l) {
        if (!grads->w[l] || !grads->b[l]) { set_error("hnr_blur_learn_backward: NULL gradient pointer (layer %d)", l); return HNR_ERR_BADARG; }
        a.gw[l] = grads->w[l]; a.gb[l] = grads->b[l];
    }
    if (blur_fused_ws(a, d_ws, ws_bytes, "hnr_blur_learn_backward") != HNR_OK) return HNR_ERR_BADARG;
    a.color = d_color; a.g_out = d_g_out; a.g_color = d_g_color;
    blur_learn_bwd_kernel<<<cdiv(a.n_patches, BL_PB), 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    int max_elems = BL_H * (BL_H + 1);                                         // the largest of the four layers' (out x (in + 1)) elements
    if (BL_H * (a.n_in + 1) > max_elems) max_elems = BL_H * (a.n_in + 1);
    if (a.n_out * (BL_H + 1) > max_elems) max_elems = a.n_out * (BL_H + 1);
    blur_learn_wgrad_kernel<<<dim3(cdiv(max_elems, 256), 4), 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
