// RAFT optical flow (basic model, fp32, inference, test_mode) on gfx950: the flow half of the content-aware frame weights.
// Replaces raft/core/raft.py, extractor.py, corr.py, update.py and utils/utils.py of the reference for the configuration
// raft/demo_content_aware_weights.py runs.  Layouts are NCHW throughout, as in the reference.
//
// One convolution kernel serves every layer: an implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a k-ordered fmaf chain, so the
// numerics stay in the fp32 class).  A workgroup of four waves owns one tile of 32 output channels x 32 output pixels; the waves split the input
// channels of every tap between them and their partial tiles are added through LDS in wave order -- a fixed order, no atomics, two runs give the
// same bits.  The A operand (lane l: A[i = l & 31][k = l >> 5]) is the packed weight, the B operand (B[k = l >> 5][j = l & 31]) the input pixel, so
// both operand loads and the result rows (row = channel, 32 consecutive pixels) are contiguous across lanes.
//   K order: k = tap * cinp + channel, cinp = input channels rounded up to even (a pair of consecutive channels of one tap per MFMA).
//   Packed layer: w [kh*kw][cinp][cout] then bias [cout]; a padded channel row is zero.
// The epilogues carry the norms that fold (batch norm, into w and bias by whoever packs), the activations and the GRU gates, so r*h, z and
// (1-z)h + zq never make a pass of their own; h, inp and the motion features are read in place as three sources (no concatenated copy).
#include "conv_mfma.h"
#include "hnr_launch.h"

namespace hnr {
namespace {

enum { EPI_NONE = 0, EPI_RELU = 1, EPI_RELU_ADD_RELU = 2, EPI_ZR = 3, EPI_GRU = 4, EPI_TANH_RELU = 5 };

struct ConvArgs {
    const float *src[3];         // nsrc sources, [N][csrc[s]][Hi][Wi] each (N > 1 only with one source)
    int csrc[3];
    int nsrc;
    const float *w, *bias;       // w [taps][cinp][cout]
    int cinp, cout;
    int N, Hi, Wi, Ho, Wo, kh, kw, stride, pad_y, pad_x;
    float scale;                 // result = sum * scale + bias
    int epi, split;
    const float *e0, *e1;
    float *out, *out2;
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// T x T tiles of 32 channels x 32 pixels per wave.  T = 1 is what runs: at 60 x 80 a 128-channel layer is only 600 tiles for 1024 SIMDs, and T = 2
// (two operand loads per two MFMAs instead of per one, a quarter of the workgroups) measured 21 % slower on the twenty updates
// (profiles/frame_weights_timing.txt); HNR_RAFT_CONV_TILE=2 selects it for such comparisons.  The numbers do not depend on T: every 32 x 32 tile is
// the same k-ordered chains, one per wave, added in wave order.
constexpr int CONV_WAVES = 4;

template <int T>
__global__ __launch_bounds__(64 * CONV_WAVES) void raft_conv_kernel(ConvArgs a)
{
    __shared__ float part[CONV_WAVES][32][33];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int HoWo = a.Ho * a.Wo, M = a.N * HoWo, HiWi = a.Hi * a.Wi;
    int n[T], oy[T], ox[T], co[T];
    bool mvalid[T], covalid[T];
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int m = (blockIdx.x * T + j) * 32 + l31;
        mvalid[j] = m < M;
        n[j] = mvalid[j] ? m / HoWo : 0;
        const int rem = mvalid[j] ? m - n[j] * HoWo : 0;
        oy[j] = rem / a.Wo; ox[j] = rem - oy[j] * a.Wo;
        co[j] = (blockIdx.y * T + j) * 32 + l31;
        covalid[j] = co[j] < a.cout;
    }
    f32x16 acc[T][T];                                              // [channel tile][pixel tile]
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int taps = a.kh * a.kw;
    // the waves split the channel pairs of every tap; a layer with fewer pairs than waves (3 or 2 input channels) splits its taps instead
    const bool by_tap = (a.cinp >> 1) < CONV_WAVES;
    const int tap0 = by_tap ? wave : 0, tap_step = by_tap ? CONV_WAVES : 1, p0 = by_tap ? 0 : wave, p_step = by_tap ? 1 : CONV_WAVES;
    for (int tap = tap0; tap < taps; tap += tap_step) {
        const int ty = tap / a.kw, tx = tap - ty * a.kw;
        bool inb[T];
        int pixoff[T];
#pragma unroll
        for (int j = 0; j < T; ++j) {
            const int iy = oy[j] * a.stride + ty - a.pad_y, ix = ox[j] * a.stride + tx - a.pad_x;
            inb[j] = mvalid[j] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
            pixoff[j] = inb[j] ? iy * a.Wi + ix : 0;
        }
        int cbase = 0;
        for (int s = 0; s < a.nsrc; ++s) {
            const int cs = a.csrc[s], csp = (cs + 1) & ~1;
            const float *sp[T], *wp[T];
#pragma unroll
            for (int j = 0; j < T; ++j) {
                sp[j] = a.src[s] + (size_t)n[j] * cs * HiWi + pixoff[j];
                wp[j] = a.w + ((size_t)tap * a.cinp + cbase) * a.cout + (covalid[j] ? co[j] : 0);
            }
#pragma unroll 4
            for (int p = p0; p < (csp >> 1); p += p_step) {
                // loads without conditions (32-bit offsets, always inside the tensors: a pixel outside reads pixel 0, a channel tile's ragged end
                // channel 0, the padded channel of an odd source the last real one, whose packed weight row is zero), then selects
                const int c = 2 * p + half, cb = c < cs ? c : cs - 1;
                float b[T], w[T];
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const float bv = sp[j][cb * HiWi], wv = wp[j][c * a.cout];
                    b[j] = inb[j] ? bv : 0.f;
                    w[j] = covalid[j] ? wv : 0.f;
                }
#pragma unroll
                for (int i = 0; i < T; ++i)
#pragma unroll
                    for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[i], b[j], acc[i][j], 0, 0, 0);
            }
            cbase += csp;
        }
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
#pragma unroll
        for (int j = 0; j < T; ++j) {
            if (i + j) __syncthreads();
#pragma unroll
            for (int r = 0; r < 16; ++r) part[wave][mfma32_row(r, half)][l31] = acc[i][j][r];
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 16 / CONV_WAVES; ++q) {
                const int e = tid + 64 * CONV_WAVES * q, row = e >> 5, col = e & 31;
                const int oc = (blockIdx.y * T + i) * 32 + row, om = (blockIdx.x * T + j) * 32 + col;
                if (oc >= a.cout || om >= M) continue;
                float v = part[0][row][col];
#pragma unroll
                for (int k = 1; k < CONV_WAVES; ++k) v += part[k][row][col];
                v = v * a.scale + a.bias[oc];
                const int on = om / HoWo, orem = om - on * HoWo;
                const size_t idx = ((size_t)on * a.cout + oc) * HoWo + orem;
                switch (a.epi) {
                case EPI_NONE: a.out[idx] = v; break;
                case EPI_RELU: a.out[idx] = fmaxf(v, 0.f); break;
                case EPI_RELU_ADD_RELU: a.out[idx] = fmaxf(a.e0[idx] + fmaxf(v, 0.f), 0.f); break;
                case EPI_ZR:                                     // channels below split: z; the others: r * h
                    if (oc < a.split) a.out[idx] = sigmoidf_(v);
                    else { const size_t k = (size_t)(oc - a.split) * HoWo + orem; a.out2[k] = sigmoidf_(v) * a.e1[k]; }
                    break;
                case EPI_GRU: { const float z = a.e0[idx], h = a.e1[idx]; a.out[idx] = (1.0f - z) * h + z * tanhf(v); break; }
                default: a.out[idx] = oc < a.split ? tanhf(v) : fmaxf(v, 0.f); break;
                }
            }
        }
    }
}

int conv(ConvArgs &a, hipStream_t st)
{
    a.Ho = (a.Hi + 2 * a.pad_y - a.kh) / a.stride + 1;
    a.Wo = (a.Wi + 2 * a.pad_x - a.kw) / a.stride + 1;
    a.cinp = 0;
    for (int s = 0; s < a.nsrc; ++s) a.cinp += (a.csrc[s] + 1) & ~1;
    const int64_t M = (int64_t)a.N * a.Ho * a.Wo;
    static const int force = knob("HNR_RAFT_CONV_TILE", 0, 0, 2);
    const int T = force ? force : 1;
    dim3 grid(cdiv(M, 32 * T), cdiv(a.cout, 32 * T));
    if (T == 2) raft_conv_kernel<2><<<grid, 64 * CONV_WAVES, 0, st>>>(a);
    else raft_conv_kernel<1><<<grid, 64 * CONV_WAVES, 0, st>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

// one layer of a packed image: advances `pk` past w and bias
int layer(const float *&pk, const float *s0, int c0, const float *s1, int c1, const float *s2, int c2, int N, int Hi, int Wi, int cout, int kh, int kw,
          int stride, int epi, float *out, hipStream_t st, const float *e0 = nullptr, const float *e1 = nullptr, float *out2 = nullptr, int split = 0)
{
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.src[0] = s0; a.src[1] = s1; a.src[2] = s2;
    a.csrc[0] = c0; a.csrc[1] = c1; a.csrc[2] = c2;
    a.nsrc = s2 ? 3 : s1 ? 2 : 1;
    a.N = N; a.Hi = Hi; a.Wi = Wi; a.cout = cout; a.kh = kh; a.kw = kw; a.stride = stride; a.pad_y = kh / 2; a.pad_x = kw / 2;
    a.scale = 1.0f; a.epi = epi; a.split = split; a.e0 = e0; a.e1 = e1; a.out = out; a.out2 = out2;
    int cinp = 0;
    for (int s = 0; s < a.nsrc; ++s) cinp += (a.csrc[s] + 1) & ~1;
    const PackedLayer l = next_layer(pk, kh * kw, cinp, cout);
    a.w = l.w; a.bias = l.bias;
    return conv(a, st);
}

// ---- encoder ---------------------------------------------------------------------------------------------------------------------------------
__global__ void raft_scale_input_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = 2.0f * (in[i] / 255.0f) - 1.0f;
}

// InstanceNorm2d(affine=False, track_running_stats=False), eps 1e-5, biased variance: one workgroup per (image, channel); per-thread strided sums
// and a tree through LDS, both in a fixed order.  mode 0: y = norm(x);  1: relu(norm(x));  2: relu(res + relu(norm(x))).  In place is fine.
constexpr int NORM_THREADS = 1024;      // one workgroup per (image, channel): at most 256 of them, so each is as wide as a workgroup gets
__global__ __launch_bounds__(NORM_THREADS) void raft_instance_norm_kernel(const float *__restrict__ x, const float *__restrict__ res, float *__restrict__ y, int HW,
                                                                 int mode)
{
    __shared__ float red[NORM_THREADS];
    const float *xp = x + (size_t)blockIdx.x * HW;
    const int tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < HW; i += NORM_THREADS) s += xp[i];
    red[tid] = s;
    __syncthreads();
    for (int k = NORM_THREADS / 2; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
    const float mean = red[0] / (float)HW;
    __syncthreads();
    s = 0.f;
    for (int i = tid; i < HW; i += NORM_THREADS) { const float d = xp[i] - mean; s = fmaf(d, d, s); }
    red[tid] = s;
    __syncthreads();
    for (int k = NORM_THREADS / 2; k > 0; k >>= 1) { if (tid < k) red[tid] += red[tid + k]; __syncthreads(); }
    const float inv = 1.0f / sqrtf(red[0] / (float)HW + 1e-5f);
    float *yp = y + (size_t)blockIdx.x * HW;
    const float *rp = res ? res + (size_t)blockIdx.x * HW : nullptr;
    for (int i = tid; i < HW; i += NORM_THREADS) {
        float v = (xp[i] - mean) * inv;
        if (mode >= 1) v = fmaxf(v, 0.f);
        if (mode == 2) v = fmaxf(rp[i] + v, 0.f);
        yp[i] = v;
    }
}

int inorm(const float *x, const float *res, float *y, int NC, int HW, int mode, hipStream_t st)
{
    raft_instance_norm_kernel<<<NC, NORM_THREADS, 0, st>>>(x, res, y, HW, mode);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

const int ENC_BLOCKS[6][3] = {{64, 64, 1}, {64, 64, 1}, {64, 96, 2}, {96, 96, 1}, {96, 128, 2}, {128, 128, 1}};    // (cin, cout, stride)

bool shape_ok(int H, int W) { return H >= 128 && W >= 128 && H % 8 == 0 && W % 8 == 0 && H <= 4096 && W <= 4096 && (int64_t)(H / 8) * (W / 8) <= 16384; }

#define TRY(expr) do { const int _r = (expr); if (_r != HNR_OK) return _r; } while (0)

int encoder(const float *d_images, int N, int H, int W, const float *pk, int norm, int cout, float *d_out, float *scratch, hipStream_t st)
{
    const int H2 = H / 2, W2 = W / 2;
    const int64_t plane = (int64_t)N * 64 * H2 * W2;                // the largest activation
    float *img = scratch, *x = img + (int64_t)N * 3 * H * W, *t1 = x + plane, *t2 = t1 + plane, *t3 = t2 + plane;
    const int64_t nin = (int64_t)N * 3 * H * W;
    raft_scale_input_kernel<<<cdiv(nin, 256), 256, 0, st>>>(d_images, img, nin);
    HNR_LAUNCH_CHECK();
    const bool in_ = norm == 0;
    TRY(layer(pk, img, 3, nullptr, 0, nullptr, 0, N, H, W, 64, 7, 7, 2, in_ ? EPI_NONE : EPI_RELU, x, st));
    if (in_) TRY(inorm(x, nullptr, x, N * 64, H2 * W2, 1, st));
    int h = H2, w = W2;
    for (int b = 0; b < 6; ++b) {
        const int cin = ENC_BLOCKS[b][0], co = ENC_BLOCKS[b][1], s = ENC_BLOCKS[b][2], ho = (h - 1) / s + 1, wo = (w - 1) / s + 1;
        // y = relu(norm1(conv1(x)));  y = relu(norm2(conv2(y)));  x = downsample(x) (stride 2 only);  x = relu(x + y)
        TRY(layer(pk, x, cin, nullptr, 0, nullptr, 0, N, h, w, co, 3, 3, s, in_ ? EPI_NONE : EPI_RELU, t1, st));
        if (in_) TRY(inorm(t1, nullptr, t1, N * co, ho * wo, 1, st));
        const float *pk2 = pk;                                       // conv2 needs the shortcut first: remember where its weights are
        pk += packed_layer_elems(co, co, 3, 3);
        const float *shortcut = x;
        if (s != 1) {
            TRY(layer(pk, x, cin, nullptr, 0, nullptr, 0, N, h, w, co, 1, 1, s, EPI_NONE, t3, st));
            if (in_) TRY(inorm(t3, nullptr, t3, N * co, ho * wo, 0, st));
            shortcut = t3;
        }
        if (in_) {
            TRY(layer(pk2, t1, co, nullptr, 0, nullptr, 0, N, ho, wo, co, 3, 3, 1, EPI_NONE, t2, st));
            TRY(inorm(t2, shortcut, t2, N * co, ho * wo, 2, st));
        } else {
            TRY(layer(pk2, t1, co, nullptr, 0, nullptr, 0, N, ho, wo, co, 3, 3, 1, EPI_RELU_ADD_RELU, t2, st, shortcut));
        }
        float *sw = x; x = t2; t2 = sw;
        h = ho; w = wo;
    }
    return layer(pk, x, 128, nullptr, 0, nullptr, 0, N, h, w, cout, 1, 1, 1, norm == 2 ? EPI_TANH_RELU : EPI_NONE, d_out, st, nullptr, nullptr, nullptr, cout / 2);
}

// ---- correlation pyramid -----------------------------------------------------------------------------------------------------------------------
void pyramid_dims(int h, int w, int hh[4], int ww[4], int64_t off[5])
{
    off[0] = 0;
    for (int l = 0; l < 4; ++l) {
        hh[l] = l ? hh[l - 1] / 2 : h;
        ww[l] = l ? ww[l - 1] / 2 : w;
        off[l + 1] = off[l] + (int64_t)h * w * hh[l] * ww[l];
    }
}

// avg_pool2d(2, 2) of [P][hi][wi] -> [P][hi/2][wi/2] (floor: an odd last row / column is dropped)
__global__ void raft_pool_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t P, int hi, int wi)
{
    const int ho = hi / 2, wo = wi / 2;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * ho * wo) return;
    const int x = (int)(i % wo), y = (int)((i / wo) % ho);
    const float *p = in + ((i / ((int64_t)wo * ho)) * hi + 2 * y) * wi + 2 * x;
    out[i] = (((p[0] + p[1]) + p[wi]) + p[wi + 1]) * 0.25f;
}

__global__ void raft_zero_bias_kernel(float *b, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) b[i] = 0.f;
}

int corr_pyramid(const float *f1, const float *f2, int h, int w, float *pyr, float *zero_bias, hipStream_t st)
{
    int hh[4], ww[4];
    int64_t off[5];
    pyramid_dims(h, w, hh, ww, off);
    const int hw = h * w;
    raft_zero_bias_kernel<<<cdiv(hw, 256), 256, 0, st>>>(zero_bias, hw);
    HNR_LAUNCH_CHECK();
    // corr[p1][p2] = sum_c f1[c][p1] f2[c][p2] / 16: a 1x1 "convolution" of f2 whose weight image [256][hw] is f1 itself
    ConvArgs a;
    memset(&a, 0, sizeof a);
    a.src[0] = f2; a.csrc[0] = 256; a.nsrc = 1;
    a.w = f1; a.bias = zero_bias; a.cout = hw;
    a.N = 1; a.Hi = h; a.Wi = w; a.kh = a.kw = 1; a.stride = 1;
    a.scale = 0.0625f; a.epi = EPI_NONE; a.out = pyr;
    TRY(conv(a, st));
    for (int l = 1; l < 4; ++l) {
        const int64_t n = (int64_t)hw * hh[l] * ww[l];
        raft_pool_kernel<<<cdiv(n, 256), 256, 0, st>>>(pyr + off[l - 1], pyr + off[l], hw, hh[l - 1], ww[l - 1]);
        HNR_LAUNCH_CHECK();
    }
    return HNR_OK;
}

// ---- lookup ------------------------------------------------------------------------------------------------------------------------------------
// corr.py:29-50 with utils.bilinear_sampler: window index (i, j), i, j = 0..8, taps x = cx / 2^l + (i - 4), y = cy / 2^l + (j - 4) (the reference stacks
// meshgrid(dy, dx) onto (x, y): the first window axis moves x), output channel l*81 + i*9 + j.  The coordinate goes through the reference's
// normalisation 2v/(W-1) - 1 and grid_sample's align_corners=True inverse ((g+1)/2)(W-1); bilinear, a tap outside the map is zero.
struct Pyr { const float *p[4]; int h[4], w[4]; };

__global__ void raft_lookup_kernel(Pyr py, const float *__restrict__ coords, int hw, float *__restrict__ out)
{
    const int i0 = blockIdx.x * 256 + threadIdx.x;
    if (i0 >= 324 * hw) return;
    const int p = i0 % hw, ch = i0 / hw, l = ch / 81, wi_ = (ch % 81) / 9, wj = ch % 9;
    const float sc = (float)(1 << l);
    const float x = coords[p] / sc + (float)(wi_ - 4), y = coords[hw + p] / sc + (float)(wj - 4);
    const int H = py.h[l], W = py.w[l];
    const float gx = 2.0f * x / (float)(W - 1) - 1.0f, gy = 2.0f * y / (float)(H - 1) - 1.0f;
    const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    float v = 0.f;
    if (ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H) {
        const float fx0 = floorf(ix), fy0 = floorf(iy);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const float wx1 = ix - fx0, wx0 = (fx0 + 1.0f) - ix, wy1 = iy - fy0, wy0 = (fy0 + 1.0f) - iy;     // grid_sample's own weight expressions
        const float *m = py.p[l] + (size_t)p * H * W;
        auto tap = [&](int yy, int xx) { return (yy >= 0 && yy < H && xx >= 0 && xx < W) ? m[yy * W + xx] : 0.f; };
        v = ((tap(y0, x0) * (wx0 * wy0) + tap(y0, x0 + 1) * (wx1 * wy0)) + tap(y0 + 1, x0) * (wx0 * wy1)) + tap(y0 + 1, x0 + 1) * (wx1 * wy1);
    }
    out[i0] = v;
}

int lookup(const float *pyr, const float *coords, int h, int w, float *out, hipStream_t st)
{
    int hh[4], ww[4];
    int64_t off[5];
    pyramid_dims(h, w, hh, ww, off);
    Pyr py;
    for (int l = 0; l < 4; ++l) { py.p[l] = pyr + off[l]; py.h[l] = hh[l]; py.w[l] = ww[l]; }
    raft_lookup_kernel<<<cdiv((int64_t)324 * h * w, 256), 256, 0, st>>>(py, coords, h * w, out);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

// ---- update block ------------------------------------------------------------------------------------------------------------------------------
// mode 0: coords = grid (x in plane 0, y in plane 1);  1: out = coords - grid (the flow);  2: coords += delta
__global__ void raft_coords_kernel(float *__restrict__ coords, const float *__restrict__ delta, float *__restrict__ out, int h, int w, int mode)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * h * w) return;
    const int p = i % (h * w);
    const float g = i < h * w ? (float)(p % w) : (float)(p / w);
    if (mode == 0) coords[i] = g;
    else if (mode == 1) out[i] = coords[i] - g;
    else coords[i] = coords[i] + delta[i];
}

int coords_op(float *coords, const float *delta, float *out, int h, int w, int mode, hipStream_t st)
{
    raft_coords_kernel<<<cdiv(2 * h * w, 256), 256, 0, st>>>(coords, delta, out, h, w, mode);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

const int64_t UPD_SCRATCH_PLANES = 324 + 256 + 256 + 128 + 128 + 128 + 128 + 128 + 256 + 2;

int update(const float *pk, const float *pyr, float *net, const float *inp, float *coords, int h, int w, float *d_delta, float *d_mask, float *scratch,
           hipStream_t st)
{
    const int64_t hw = (int64_t)h * w;
    float *corr = scratch, *cor1 = corr + 324 * hw, *corflo = cor1 + 256 * hw, *flo1 = corflo + 256 * hw, *motion = flo1 + 128 * hw,
          *z = motion + 128 * hw, *rh = z + 128 * hw, *h1 = rh + 128 * hw, *big = h1 + 128 * hw, *delta = big + 256 * hw;
    float *flow = motion + 126 * hw;
    if (d_delta) delta = d_delta;
    TRY(lookup(pyr, coords, h, w, corr, st));
    TRY(coords_op(coords, nullptr, flow, h, w, 1, st));
    // BasicMotionEncoder
    TRY(layer(pk, corr, 324, nullptr, 0, nullptr, 0, 1, h, w, 256, 1, 1, 1, EPI_RELU, cor1, st));
    TRY(layer(pk, cor1, 256, nullptr, 0, nullptr, 0, 1, h, w, 192, 3, 3, 1, EPI_RELU, corflo, st));
    TRY(layer(pk, flow, 2, nullptr, 0, nullptr, 0, 1, h, w, 128, 7, 7, 1, EPI_RELU, flo1, st));
    TRY(layer(pk, flo1, 128, nullptr, 0, nullptr, 0, 1, h, w, 64, 3, 3, 1, EPI_RELU, corflo + 192 * hw, st));
    TRY(layer(pk, corflo, 256, nullptr, 0, nullptr, 0, 1, h, w, 126, 3, 3, 1, EPI_RELU, motion, st));
    // SepConvGRU: (1,5) then (5,1); z and r share one launch (their weights are stacked by whoever packs), q takes r*h, inp, motion in place
    TRY(layer(pk, net, 128, inp, 128, motion, 128, 1, h, w, 256, 1, 5, 1, EPI_ZR, z, st, nullptr, net, rh, 128));
    TRY(layer(pk, rh, 128, inp, 128, motion, 128, 1, h, w, 128, 1, 5, 1, EPI_GRU, h1, st, z, net));
    TRY(layer(pk, h1, 128, inp, 128, motion, 128, 1, h, w, 256, 5, 1, 1, EPI_ZR, z, st, nullptr, h1, rh, 128));
    TRY(layer(pk, rh, 128, inp, 128, motion, 128, 1, h, w, 128, 5, 1, 1, EPI_GRU, net, st, z, h1));
    // FlowHead
    TRY(layer(pk, net, 128, nullptr, 0, nullptr, 0, 1, h, w, 256, 3, 3, 1, EPI_RELU, big, st));
    TRY(layer(pk, big, 256, nullptr, 0, nullptr, 0, 1, h, w, 2, 3, 3, 1, EPI_NONE, delta, st));
    TRY(coords_op(coords, delta, nullptr, h, w, 2, st));
    if (d_mask) {                                                      // 0.25 * mask(net): the factor is folded into the packed 1x1 layer
        TRY(layer(pk, net, 128, nullptr, 0, nullptr, 0, 1, h, w, 256, 3, 3, 1, EPI_RELU, big, st));
        TRY(layer(pk, big, 256, nullptr, 0, nullptr, 0, 1, h, w, 576, 1, 1, 1, EPI_NONE, d_mask, st));
    }
    return HNR_OK;
}

// ---- convex upsampling (raft.py:72-83) -------------------------------------------------------------------------------------------------------------
// mask [576,h,w] = [9][8][8][h][w]; up[c][8y+a][8x+b] = sum_k softmax_k(mask[k][a][b][y][x]) * 8 flow[c][y + k/3 - 1][x + k%3 - 1] (zero outside)
__global__ void raft_upsample_kernel(const float *__restrict__ flow, const float *__restrict__ mask, int h, int w, float *__restrict__ up)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 64 * h * w) return;
    const int X = i % (8 * w), Y = i / (8 * w), x = X >> 3, b = X & 7, y = Y >> 3, a = Y & 7, hw = h * w;
    float mk[9], mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < 9; ++k) { mk[k] = mask[(size_t)((k * 8 + a) * 8 + b) * hw + y * w + x]; mx = fmaxf(mx, mk[k]); }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) { mk[k] = expf(mk[k] - mx); s += mk[k]; }
    float u0 = 0.f, u1 = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
        const float wk = mk[k] / s;
        u0 += wk * (8.0f * flow[yy * w + xx]);
        u1 += wk * (8.0f * flow[hw + yy * w + xx]);
    }
    up[i] = u0;
    up[(size_t)64 * hw + i] = u1;
}

int upsample(const float *flow, const float *mask, int h, int w, float *up, hipStream_t st)
{
    raft_upsample_kernel<<<cdiv((int64_t)64 * h * w, 256), 256, 0, st>>>(flow, mask, h, w, up);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

int64_t encoder_packed_elems(int cout)
{
    int64_t n = packed_layer_elems(3, 64, 7, 7);
    for (int b = 0; b < 6; ++b) {
        n += packed_layer_elems(ENC_BLOCKS[b][0], ENC_BLOCKS[b][1], 3, 3) + packed_layer_elems(ENC_BLOCKS[b][1], ENC_BLOCKS[b][1], 3, 3);
        if (ENC_BLOCKS[b][2] != 1) n += packed_layer_elems(ENC_BLOCKS[b][0], ENC_BLOCKS[b][1], 1, 1);
    }
    return n + packed_layer_elems(128, cout, 1, 1);
}

int64_t encoder_scratch(int N, int H, int W) { return (int64_t)N * 3 * H * W + 4 * (int64_t)N * 64 * (H / 2) * (W / 2); }

int64_t pyramid_total(int h, int w)
{
    int hh[4], ww[4];
    int64_t off[5];
    pyramid_dims(h, w, hh, ww, off);
    return off[4];
}

}  // namespace
}  // namespace hnr

using namespace hnr;

#define BAD(...) do { set_error(__VA_ARGS__); return HNR_ERR_BADARG; } while (0)

extern "C" {

int64_t hnr_raft_encoder_packed_elems(void) { return encoder_packed_elems(256); }

int64_t hnr_raft_update_packed_elems(void)
{
    constexpr auto n = packed_layer_elems;
    return n(324, 256, 1, 1) + n(256, 192, 3, 3) + n(2, 128, 7, 7) + n(128, 64, 3, 3) + n(256, 126, 3, 3) + 2 * (n(384, 256, 1, 5) + n(384, 128, 1, 5)) +
           n(128, 256, 3, 3) + n(256, 2, 3, 3) + n(128, 256, 3, 3) + n(256, 576, 1, 1);
}

int64_t hnr_raft_encoder_scratch_elems(int N, int H, int W) { return (N >= 1 && N <= 2 && shape_ok(H, W)) ? encoder_scratch(N, H, W) : -1; }

int hnr_raft_encoder(const float *d_images, int N, int H, int W, const float *d_packed, int norm, float *d_out, float *d_scratch, int64_t scratch_elems,
                     void *stream)
{
    if (!d_images || !d_packed || !d_out || !d_scratch) BAD("hnr_raft_encoder: NULL pointer");
    if (N < 1 || N > 2 || !shape_ok(H, W)) BAD("hnr_raft_encoder: N=%d H=%d W=%d (N 1 or 2; H, W multiples of 8, 128 .. 4096, H/8*W/8 <= 16384)", N, H, W);
    if (norm < 0 || norm > 2) BAD("hnr_raft_encoder: norm=%d (0 instance, 1 folded batch norm, 2 folded batch norm + tanh | relu)", norm);
    if (scratch_elems < encoder_scratch(N, H, W)) BAD("hnr_raft_encoder: scratch of %lld floats, %lld needed", (long long)scratch_elems, (long long)encoder_scratch(N, H, W));
    return encoder(d_images, N, H, W, d_packed, norm, 256, d_out, d_scratch, (hipStream_t)stream);
}

int64_t hnr_raft_pyramid_elems(int h, int w) { return shape_ok(8 * h, 8 * w) ? pyramid_total(h, w) : -1; }
int64_t hnr_raft_pyramid_scratch_elems(int h, int w) { return shape_ok(8 * h, 8 * w) ? (int64_t)h * w : -1; }

int hnr_raft_corr_pyramid(const float *d_fmap1, const float *d_fmap2, int h, int w, float *d_pyramid, float *d_scratch, int64_t scratch_elems, void *stream)
{
    if (!d_fmap1 || !d_fmap2 || !d_pyramid || !d_scratch) BAD("hnr_raft_corr_pyramid: NULL pointer");
    if (!shape_ok(8 * h, 8 * w)) BAD("hnr_raft_corr_pyramid: h=%d w=%d (16 <= h, w; h*w <= 16384)", h, w);
    if (scratch_elems < (int64_t)h * w) BAD("hnr_raft_corr_pyramid: scratch of %lld floats, %lld needed", (long long)scratch_elems, (long long)h * w);
    return corr_pyramid(d_fmap1, d_fmap2, h, w, d_pyramid, d_scratch, (hipStream_t)stream);
}

int hnr_raft_lookup(const float *d_pyramid, const float *d_coords, int h, int w, float *d_corr, void *stream)
{
    if (!d_pyramid || !d_coords || !d_corr) BAD("hnr_raft_lookup: NULL pointer");
    if (!shape_ok(8 * h, 8 * w)) BAD("hnr_raft_lookup: h=%d w=%d (16 <= h, w; h*w <= 16384)", h, w);
    return lookup(d_pyramid, d_coords, h, w, d_corr, (hipStream_t)stream);
}

int64_t hnr_raft_update_scratch_elems(int h, int w) { return shape_ok(8 * h, 8 * w) ? UPD_SCRATCH_PLANES * h * w : -1; }

int hnr_raft_update(const float *d_packed, const float *d_pyramid, float *d_net, const float *d_inp, float *d_coords, int h, int w, float *d_delta,
                    float *d_mask, float *d_scratch, int64_t scratch_elems, void *stream)
{
    if (!d_packed || !d_pyramid || !d_net || !d_inp || !d_coords || !d_scratch) BAD("hnr_raft_update: NULL pointer");
    if (!shape_ok(8 * h, 8 * w)) BAD("hnr_raft_update: h=%d w=%d (16 <= h, w; h*w <= 16384)", h, w);
    if (scratch_elems < UPD_SCRATCH_PLANES * h * w) BAD("hnr_raft_update: scratch of %lld floats, %lld needed", (long long)scratch_elems, (long long)(UPD_SCRATCH_PLANES * h * w));
    return update(d_packed, d_pyramid, d_net, d_inp, d_coords, h, w, d_delta, d_mask, d_scratch, (hipStream_t)stream);
}

int hnr_raft_upsample(const float *d_flow, const float *d_mask, int h, int w, float *d_flow_up, void *stream)
{
    if (!d_flow || !d_mask || !d_flow_up) BAD("hnr_raft_upsample: NULL pointer");
    if (h < 1 || w < 1 || (int64_t)h * w > 16384) BAD("hnr_raft_upsample: h=%d w=%d (h*w <= 16384)", h, w);
    return upsample(d_flow, d_mask, h, w, d_flow_up, (hipStream_t)stream);
}

/* scratch of hnr_raft_flow: [fmaps 2*256*hw][cnet 256*hw][coords 2*hw][mask 576*hw][pyramid][max(encoder, update, hw)] */
int64_t hnr_raft_flow_scratch_elems(int H, int W)
{
    if (!shape_ok(H, W)) return -1;
    const int64_t hw = (int64_t)(H / 8) * (W / 8), enc = encoder_scratch(2, H, W), upd = UPD_SCRATCH_PLANES * hw;
    return (512 + 256 + 2 + 576) * hw + pyramid_total(H / 8, W / 8) + (enc > upd ? enc : upd);
}

int hnr_raft_flow(const float *d_image1, const float *d_image2, int H, int W, const float *d_fnet, const float *d_cnet, const float *d_update, int iters,
                  float *d_flow_low, float *d_flow_up, float *d_scratch, int64_t scratch_elems, void *stream)
{
    if (!d_image1 || !d_image2 || !d_fnet || !d_cnet || !d_update || !d_flow_low || !d_flow_up || !d_scratch) BAD("hnr_raft_flow: NULL pointer");
    if (!shape_ok(H, W)) BAD("hnr_raft_flow: H=%d W=%d (multiples of 8, 128 .. 4096, H/8*W/8 <= 16384)", H, W);
    if (iters < 1 || iters > 1024) BAD("hnr_raft_flow: iters=%d (1 .. 1024)", iters);
    if (d_image2 != d_image1 + (int64_t)3 * H * W) BAD("hnr_raft_flow: image 2 must follow image 1 in memory (one [2,3,H,W] buffer)");
    if (scratch_elems < hnr_raft_flow_scratch_elems(H, W)) BAD("hnr_raft_flow: scratch of %lld floats, %lld needed", (long long)scratch_elems, (long long)hnr_raft_flow_scratch_elems(H, W));
    hipStream_t st = (hipStream_t)stream;
    const int h = H / 8, w = W / 8;
    const int64_t hw = (int64_t)h * w;
    float *fmaps = d_scratch, *cn = fmaps + 512 * hw, *coords = cn + 256 * hw, *mask = coords + 2 * hw, *pyr = mask + 576 * hw, *work = pyr + pyramid_total(h, w);
    TRY(encoder(d_image1, 2, H, W, d_fnet, 0, 256, fmaps, work, st));
    TRY(encoder(d_image1, 1, H, W, d_cnet, 2, 256, cn, work, st));
    TRY(corr_pyramid(fmaps, fmaps + 256 * hw, h, w, pyr, work, st));
    TRY(coords_op(coords, nullptr, nullptr, h, w, 0, st));
    for (int it = 0; it < iters; ++it) TRY(update(d_update, pyr, cn, cn + 128 * hw, coords, h, w, nullptr, it == iters - 1 ? mask : nullptr, work, st));
    TRY(coords_op(coords, nullptr, d_flow_low, h, w, 1, st));
    return upsample(d_flow_low, mask, h, w, d_flow_up, st);
}

}  // extern "C"
