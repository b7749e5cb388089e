// LPIPS v0.1 (AlexNet and VGG-16 backbones, fp32, eval, lpips=True, spatial=False) on gfx950: the two perceptual scores of the reference's test pass.
// Replaces `lpips.LPIPS(net)` + torchvision's `features` as run/evaluate.py:41-75 calls them (after a PNG write, a PNG read and a host-to-device copy).
// Layouts are NCHW; the two images of a pair travel as a batch of two.
//
// Convolution + bias + ReLU: an implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: a k-ordered fmaf chain, the fp32 error class).
//   Workgroup (four waves), large tile: 64 output channels x a pixel tile of 8 rows x 32 columns of ONE image.  Wave v owns rows 2v and 2v+1 of the tile and
//   both 32-channel halves: four 32x32 accumulators, so each operand read from LDS feeds two MFMAs (2 + 2 reads per 4 MFMAs).
//   LDS image per chunk of CK input channels: the input tile with its halo [CK][(8-1)s+kh][(32-1)s+kw] (zero outside the map and beyond the last
//   channel), then the weight slab [kh*kw][CK][64] copied with 16-byte loads.  A operand (lane l: A[i = l & 31][k = l >> 5]) = weight of channel
//   pair element k, output channel i: 32 consecutive dwords per lane half;  B operand (B[k = l >> 5][j = l & 31]) = input pixel: consecutive for s = 1.
//   K order: chunk of CK channels, then tap (row-major), then channel pair inside the chunk.  Every chunk is one chain that starts from zero
//   (kh*kw*CK terms: 72, 100 or 242) and the chunk sums are added in chunk order: blocked summation, whose rounding error grows with
//   sqrt(chain) + sqrt(chunks) instead of sqrt(K) (K = 4608 for a 512-channel 3x3 layer; one chain over it measured 2 .. 4 x the error of the
//   fp32 restatement).  K is NOT split across waves: every output element belongs to one wave, no atomics; two runs give the same bits.
//   Packed layer (flow.pack_layer's): w [kh*kw][cinp][cout], cinp = cin rounded up to even (the added row zero), then bias [cout]; cout % 64 == 0.
// Tap score: one thread per pixel, lanes along pixels; the two channel norms first, then sum_c lin[c] (f0/(n0+eps) - f1/(n1+eps))^2 in the
//   package's form (never the expanded one, which cancels for close images), fp32 terms collected in fp64; per-pixel values are summed in fp64:
//   per workgroup (64 pixels) in pixel order, then per tap by strided sums and a tree, both in a fixed order.
#include "conv_mfma.h"
#include "hnr_launch.h"

namespace hnr {
namespace {

enum { NET_ALEX = 0, NET_VGG = 1 };
constexpr int HEADER = 8;                        // shift [3], scale [3], two zeros: keeps every layer's weights 16-byte aligned
constexpr int TILE_C = 32;                      // pixel columns of a tile; rows and channels: ConvShape
constexpr int MAX_HW = 4096;

struct Layer { int cin, cout, k, stride, pad; };
const Layer ALEX[5] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1}, {256, 256, 3, 1, 1}};
const int VGG_CH[13][2] = {{3, 64}, {64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 256}, {256, 512}, {512, 512}, {512, 512},
                           {512, 512}, {512, 512}, {512, 512}};
const int VGG_TAP_AFTER[5] = {1, 3, 6, 9, 12};  // index of the convolution whose ReLU is tap k
const int TAP_CH[2][5] = {{64, 192, 384, 256, 256}, {64, 128, 256, 512, 512}};

int64_t packed_elems(int net)
{
    int64_t n = HEADER;
    if (net == NET_ALEX) for (int i = 0; i < 5; ++i) n += packed_layer_elems(ALEX[i].cin, ALEX[i].cout, ALEX[i].k, ALEX[i].k);
    else for (int i = 0; i < 13; ++i) n += packed_layer_elems(VGG_CH[i][0], VGG_CH[i][1], 3, 3);
    for (int k = 0; k < 5; ++k) n += TAP_CH[net][k];
    return n;
}

// Smallest input: alex -- conv1 gives o1 = (H + 4 - 11) / 4 + 1, the two 3x3/s2 pools o2 = (o1 - 3) / 2 + 1 and o3 = (o2 - 3) / 2 + 1 (the other layers
// keep the extent); o3 >= 1 needs o2 >= 3, o1 >= 7, (H - 7) / 4 >= 6: H >= 31.  vgg -- four 2x2/s2 floor pools: H / 16 >= 1: H >= 16.
int min_size(int net) { return net == NET_ALEX ? 31 : 16; }

bool net_ok(int net) { return net == NET_ALEX || net == NET_VGG; }
bool shape_ok(int net, int h, int w) { return h >= min_size(net) && w >= min_size(net) && h <= MAX_HW && w <= MAX_HW; }

void tap_dims(int net, int h, int w, int th[5], int tw[5])
{
    if (net == NET_ALEX) {
        th[0] = (h - 7) / 4 + 1; tw[0] = (w - 7) / 4 + 1;
        th[1] = (th[0] - 3) / 2 + 1; tw[1] = (tw[0] - 3) / 2 + 1;
        th[2] = th[3] = th[4] = (th[1] - 3) / 2 + 1; tw[2] = tw[3] = tw[4] = (tw[1] - 3) / 2 + 1;
    } else {
        for (int k = 0; k < 5; ++k) { th[k] = k ? th[k - 1] / 2 : h; tw[k] = k ? tw[k - 1] / 2 : w; }
    }
}

// ---- preparation -------------------------------------------------------------------------------------------------------------------------------
// run/evaluate.py: float32(img) / 255.0, then * 2 - 1.0; the package's ScalingLayer: (x - shift) / scale -- four separately rounded fp32 operations
// (the division correctly rounded).  Only 256 values per channel exist: every workgroup builds the table [3][256] in LDS and looks its pixels up.
// bgr: channel c of the network reads channel 2 - c of the RGB bytes (cv2.imread hands evaluate.py BGR and nothing converts it).
__global__ __launch_bounds__(256) void lpips_prepare8_kernel(const uint8_t *__restrict__ a8, const uint8_t *__restrict__ b8, int hw, int bgr,
                                                              const float *__restrict__ pk, float *__restrict__ x)
{
    __shared__ float table[3][256];
    const int tid = threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = ((float)tid / 255.0f) * 2.0f - 1.0f;
        table[c][tid] = (v - pk[c]) / pk[3 + c];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;                        // pixel of the pair: image i / hw
    if (i >= 2 * hw) return;
    const int n = i >= hw, p = i - n * hw;
    const uint8_t *src = (n ? b8 : a8) + (size_t)p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[((size_t)n * 3 + c) * hw + p] = table[c][src[bgr ? 2 - c : c]];
}

// float inputs [3,h,w] in [-1, 1], channels as given: the ScalingLayer alone
__global__ __launch_bounds__(256) void lpips_prepare_f32_kernel(const float *__restrict__ in0, const float *__restrict__ in1, int hw,
                                                                 const float *__restrict__ pk, float *__restrict__ x)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 6 * hw) return;
    const int n = i >= 3 * hw, r = i - n * 3 * hw, c = r / hw;
    x[i] = ((n ? in1 : in0)[r] - pk[c]) / pk[3 + c];
}

// ---- convolution + bias + ReLU -----------------------------------------------------------------------------------------------------------------------
struct ConvArgs {
    const float *in, *w, *bias;          // in [N][cin][Hi][Wi], w [taps][cinp][cout]
    float *out;                          // [N][cout][Ho][Wo]
    int cin, cinp, cout, Hi, Wi, Ho, Wo, pad, tiles_x;
};

// T = 2: the tile above.  T = 1: 32 channels x 4 rows x 32 columns, one accumulator per wave (two operand reads per MFMA) -- for the layers whose map is
// so small that the large tile leaves most of the 1024 SIMDs without a wave (alex from 5x5 on, vgg block 5 at 460 x 620).  The chains are the same:
// the numbers do not depend on T.
template <int K, int S, int CK, int T>
struct ConvShape {
    static constexpr int TR = 4 * T, CO = 32 * T;
    static constexpr int IR = (TR - 1) * S + K, IC = (TILE_C - 1) * S + K, TAPS = K * K;
    static constexpr int IN_ELEMS = (CK * IR * IC + 3) & ~3, W_ELEMS = TAPS * CK * CO;
    static constexpr int LDS_BYTES = (IN_ELEMS + W_ELEMS) * 4;
};

// (three waves per SIMD: the large tile is held to 168 registers and spills three dwords per lane; left at 172 and two waves, VGG at 460 x 620 took
// 6.66 ms instead of 5.92)
template <int K, int S, int CK, int T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) void lpips_conv_kernel(ConvArgs a)
{
    using Sh = ConvShape<K, S, CK, T>;
    constexpr int IR = Sh::IR, IC = Sh::IC, TAPS = Sh::TAPS, CO = Sh::CO, TR = Sh::TR;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *in_s = lds, *w_s = lds + Sh::IN_ELEMS;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const int tyi = blockIdx.x / a.tiles_x, txi = blockIdx.x - tyi * a.tiles_x;
    const int oy0 = tyi * TR, ox0 = txi * TILE_C, co0 = blockIdx.y * CO, n = blockIdx.z;
    const int iy0 = oy0 * S - a.pad, ix0 = ox0 * S - a.pad, HiWi = a.Hi * a.Wi;
    const float *src = a.in + (size_t)n * a.cin * HiWi;
    f32x16 tot[T][T];                                              // [channel tile][row of the wave]
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
    for (int c0 = 0; c0 < a.cinp; c0 += CK) {
        f32x16 acc[T][T];                                          // this chunk's chain starts from zero
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        __syncthreads();                                           // the previous chunk has been read
        for (int e = tid; e < CK * IR * IC; e += 256) {
            const int c = e / (IR * IC), rem = e - c * (IR * IC), r = rem / IC, q = rem - r * IC;
            const int iy = iy0 + r, ix = ix0 + q, ch = c0 + c;
            float v = 0.f;
            if (ch < a.cin && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) v = src[(size_t)ch * HiWi + iy * a.Wi + ix];
            in_s[e] = v;
        }
        for (int e = tid; e < TAPS * CK * (CO / 4); e += 256) {
            const int row = e / (CO / 4), q = e - row * (CO / 4), tap = row / CK, c = row - tap * CK, ch = c0 + c;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (ch < a.cinp) v = *reinterpret_cast<const uint4 *>(a.w + ((size_t)tap * a.cinp + ch) * a.cout + co0 + 4 * q);
            *reinterpret_cast<uint4 *>(w_s + row * CO + 4 * q) = v;
        }
        __syncthreads();
        const float *bp = in_s + (half * IR + T * wave * S) * IC + l31 * S;     // channel `half` of pair 0, first row of the wave, tap (0, 0)
        const float *ap = w_s + half * CO + l31;
#pragma clang loop unroll_count(K <= 5 ? K : 1)
        for (int ty = 0; ty < K; ++ty) {
#pragma unroll
            for (int tx = 0; tx < K; ++tx) {
                const float *b = bp + ty * IC + tx, *w = ap + (ty * K + tx) * CK * CO;
#pragma unroll
                for (int p = 0; p < CK / 2; ++p) {                 // (channels beyond the last are zero in both LDS images)
                    float bv[T], av[T];
#pragma unroll
                    for (int j = 0; j < T; ++j) bv[j] = b[2 * p * IR * IC + j * S * IC];
#pragma unroll
                    for (int i = 0; i < T; ++i) av[i] = w[2 * p * CO + 32 * i];
#pragma unroll
                    for (int i = 0; i < T; ++i)
#pragma unroll
                        for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[i][j][r] += acc[i][j][r];
    }
    // result row (channel) = mfma32_row(r, half), column (pixel) = l31: 32 consecutive floats per lane half and register
    const int ox = ox0 + l31, HoWo = a.Ho * a.Wo;
    if (ox >= a.Wo) return;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const int oy = oy0 + T * wave + j;
        if (oy >= a.Ho) continue;
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int oc = co0 + 32 * i + mfma32_row(r, half);
                a.out[((size_t)n * a.cout + oc) * HoWo + oy * a.Wo + ox] = fmaxf(tot[i][j][r] + a.bias[oc], 0.f);
            }
    }
}

template <int K, int S, int CK>
int launch_conv(const ConvArgs &a, hipStream_t st)
{
    // the large tile where it still gives every SIMD a wave or two; the small one below that
    const int64_t big = (int64_t)a.tiles_x * cdiv(a.Ho, 8) * (a.cout / 64) * 2;
    const int force = knob_now("HNR_LPIPS_CONV_TILE", 0, 0, 2);         // 1 / 2: that tile for every layer (tests, timing); the bits do not change
    if (force ? force == 2 : big >= 2 * device_num_cus()) {
        dim3 grid(a.tiles_x * cdiv(a.Ho, 8), a.cout / 64, 2);
        return launch_lds<lpips_conv_kernel<K, S, CK, 2>>(grid, dim3(256), ConvShape<K, S, CK, 2>::LDS_BYTES, st, a);
    }
    dim3 grid(a.tiles_x * cdiv(a.Ho, 4), a.cout / 32, 2);
    return launch_lds<lpips_conv_kernel<K, S, CK, 1>>(grid, dim3(256), ConvShape<K, S, CK, 1>::LDS_BYTES, st, a);
}

// one layer of the packed image: advances `pk` past w and bias
int conv(const float *&pk, const float *in, int cin, int Hi, int Wi, int cout, int k, int stride, int pad, float *out, hipStream_t st)
{
    ConvArgs a;
    a.in = in; a.out = out; a.cin = cin; a.cinp = (cin + 1) & ~1; a.cout = cout; a.Hi = Hi; a.Wi = Wi; a.pad = pad;
    a.Ho = (Hi + 2 * pad - k) / stride + 1; a.Wo = (Wi + 2 * pad - k) / stride + 1;
    a.tiles_x = cdiv(a.Wo, TILE_C);
    const PackedLayer l = next_layer(pk, k * k, cin, cout);
    a.w = l.w; a.bias = l.bias;
    if (cout % 64) { set_error("lpips conv: cout=%d is no multiple of 64", cout); return HNR_ERR_BADARG; }
    if (k == 3 && stride == 1) return launch_conv<3, 1, 8>(a, st);
    if (k == 5 && stride == 1) return launch_conv<5, 1, 4>(a, st);
    if (k == 11 && stride == 4) return launch_conv<11, 4, 2>(a, st);
    set_error("lpips conv: no instantiation for k=%d stride=%d", k, stride);
    return HNR_ERR_BADARG;
}

// max_pool2d(k, 2), no padding, floor: every window lies inside the map
__global__ __launch_bounds__(256) void lpips_maxpool_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t planes, int Hi, int Wi, int k)
{
    const int Ho = (Hi - k) / 2 + 1, Wo = (Wi - k) / 2 + 1;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= planes * Ho * Wo) return;
    const int x = (int)(i % Wo), y = (int)((i / Wo) % Ho);
    const float *p = in + ((i / ((int64_t)Wo * Ho)) * Hi + 2 * y) * Wi + 2 * x;
    float m = p[0];
    for (int dy = 0; dy < k; ++dy)
        for (int dx = 0; dx < k; ++dx) m = fmaxf(m, p[dy * Wi + dx]);
    out[i] = m;
}

int maxpool(const float *in, float *out, int planes, int Hi, int Wi, int k, hipStream_t st)
{
    const int64_t n = (int64_t)planes * ((Hi - k) / 2 + 1) * ((Wi - k) / 2 + 1);
    lpips_maxpool_kernel<<<cdiv(n, 256), 256, 0, st>>>(in, out, planes, Hi, Wi, k);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

#define TRY(expr) do { const int _r = (expr); if (_r != HNR_OK) return _r; } while (0)

// x [2,3,h,w] -> taps[k] [2,C_k,h_k,w_k]; wa, wb: two work buffers of work_elems() floats each
int features(int net, const float *x, int h, int w, const float *pk, float *const taps[5], float *wa, float *wb, hipStream_t st)
{
    pk += HEADER;
    int th[5], tw[5];
    tap_dims(net, h, w, th, tw);
    if (net == NET_ALEX) {
        TRY(conv(pk, x, 3, h, w, 64, 11, 4, 2, taps[0], st));
        TRY(maxpool(taps[0], wa, 2 * 64, th[0], tw[0], 3, st));
        TRY(conv(pk, wa, 64, th[1], tw[1], 192, 5, 1, 2, taps[1], st));
        TRY(maxpool(taps[1], wa, 2 * 192, th[1], tw[1], 3, st));
        TRY(conv(pk, wa, 192, th[2], tw[2], 384, 3, 1, 1, taps[2], st));
        TRY(conv(pk, taps[2], 384, th[2], tw[2], 256, 3, 1, 1, taps[3], st));
        return conv(pk, taps[3], 256, th[2], tw[2], 256, 3, 1, 1, taps[4], st);
    }
    const float *cur = x;
    int k = 0;
    for (int i = 0; i < 13; ++i) {
        const bool is_tap = i == VGG_TAP_AFTER[k];
        float *dst = is_tap ? taps[k] : (cur == wa ? wb : wa);
        TRY(conv(pk, cur, VGG_CH[i][0], th[k], tw[k], VGG_CH[i][1], 3, 1, 1, dst, st));
        cur = dst;
        if (is_tap && k < 4) {
            TRY(maxpool(taps[k], wa, 2 * VGG_CH[i][1], th[k], tw[k], 2, st));
            cur = wa;
        }
        if (is_tap) ++k;
    }
    return HNR_OK;
}

// ---- tap score -------------------------------------------------------------------------------------------------------------------------------------
// A workgroup is 64 pixels (the lanes) x 16 channel groups (the waves): group g sums its C/16 channels in channel order, the groups are added in
// group order -- a 512-channel tap of a few pixels is not one thread's chain of 512 dependent loads.
constexpr int SC_PIX = 64, SC_GROUPS = 16;
__global__ __launch_bounds__(SC_PIX * SC_GROUPS) void lpips_score_kernel(const float *__restrict__ f, int C, int hw, const float *__restrict__ lin,
                                                                     double *__restrict__ partial)
{
    __shared__ double part[3][SC_GROUPS][SC_PIX];
    __shared__ float den[2][SC_PIX];
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, p = blockIdx.x * SC_PIX + lane;
    const int cpg = (C + SC_GROUPS - 1) / SC_GROUPS, c_lo = g * cpg, c_hi = c_lo + cpg < C ? c_lo + cpg : C;
    const bool ok = p < hw;
    const float *f0 = f + (ok ? p : 0), *f1 = f0 + (size_t)C * hw;
    // every term is the package's fp32 expression (f * f; f / (n + eps); the difference, its square, times lin); the three sums over the channels
    // collect those fp32 terms in fp64, so that a 512-channel sum adds no rounding of its own to a tap of one pixel
    double n0 = 0.0, n1 = 0.0;
#pragma unroll 8
    for (int c = c_lo; c < c_hi; ++c) {
        const float u = f0[(size_t)c * hw], v = f1[(size_t)c * hw];
        n0 += (double)(u * u);
        n1 += (double)(v * v);
    }
    part[0][g][lane] = n0;
    part[1][g][lane] = n1;
    __syncthreads();
    if (g < 2) {
        double n = part[g][0][lane];
        for (int k = 1; k < SC_GROUPS; ++k) n += part[g][k][lane];
        den[g][lane] = sqrtf((float)n) + 1e-10f;
    }
    __syncthreads();
    const float d0 = den[0][lane], d1 = den[1][lane];
    double s = 0.0;
#pragma unroll 8
    for (int c = c_lo; c < c_hi; ++c) {
        const float d = f0[(size_t)c * hw] / d0 - f1[(size_t)c * hw] / d1;
        s += (double)(lin[c] * (d * d));
    }
    part[2][g][lane] = ok ? s : 0.0;
    __syncthreads();
    if (g == 0) {
        double t = part[2][0][lane];
        for (int k = 1; k < SC_GROUPS; ++k) t += part[2][k][lane];
        part[0][0][lane] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = part[0][0][0];
        for (int k = 1; k < SC_PIX; ++k) t += part[0][0][k];
        partial[blockIdx.x] = t;
    }
}

struct Finish { int64_t off[5]; int count[5]; double hw[5]; };

// row = [d, r_0 .. r_4]: r_k = (sum of tap k's partials) / pixels, d = (((r_0 + r_1) + r_2) + r_3) + r_4
__global__ __launch_bounds__(256) void lpips_finish_kernel(const double *__restrict__ partial, Finish fin, double *__restrict__ row)
{
    __shared__ double red[256];
    __shared__ double r[5];
    const int tid = threadIdx.x;
    for (int k = 0; k < 5; ++k) {
        double s = 0.0;
        for (int i = tid; i < fin.count[k]; i += 256) s += partial[fin.off[k] + i];
        red[tid] = s;
        __syncthreads();
        for (int j = 128; j > 0; j >>= 1) { if (tid < j) red[tid] += red[tid + j]; __syncthreads(); }
        if (tid == 0) r[k] = red[0] / fin.hw[k];
        __syncthreads();
    }
    if (tid == 0) {
        double d = r[0];
        for (int k = 1; k < 5; ++k) d += r[k];
        row[0] = d;
        for (int k = 0; k < 5; ++k) row[1 + k] = r[k];
    }
}

int64_t partial_count(int net, int h, int w)
{
    int th[5], tw[5];
    tap_dims(net, h, w, th, tw);
    int64_t n = 0;
    for (int k = 0; k < 5; ++k) n += cdiv((int64_t)th[k] * tw[k], SC_PIX);
    return n;
}

int score(int net, const float *const taps[5], int h, int w, const float *pk, double *row, double *partial, hipStream_t st)
{
    int th[5], tw[5];
    tap_dims(net, h, w, th, tw);
    const float *lin = pk + packed_elems(net);
    for (int k = 0; k < 5; ++k) lin -= TAP_CH[net][k];
    Finish fin;
    int64_t off = 0;
    for (int k = 0; k < 5; ++k) {
        const int hw = th[k] * tw[k], nb = cdiv(hw, SC_PIX);
        fin.off[k] = off; fin.count[k] = nb; fin.hw[k] = (double)hw;
        lpips_score_kernel<<<nb, SC_PIX * SC_GROUPS, 0, st>>>(taps[k], TAP_CH[net][k], hw, lin, partial + off);
        HNR_LAUNCH_CHECK();
        off += nb;
        lin += TAP_CH[net][k];
    }
    lpips_finish_kernel<<<1, 256, 0, st>>>(partial, fin, row);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

// ---- scratch: [x 2*3*h*w][taps 0..4][work a][work b] floats, each part rounded up to 64 floats, then the partial sums (doubles) -----------------------
int64_t up64(int64_t n) { return (n + 63) & ~(int64_t)63; }

struct Scratch { int64_t x, tap[5], wa, wb, partial, bytes; };

Scratch scratch_layout(int net, int h, int w)
{
    int th[5], tw[5];
    tap_dims(net, h, w, th, tw);
    Scratch s;
    int64_t o = 0;
    s.x = o; o += up64((int64_t)6 * h * w);
    for (int k = 0; k < 5; ++k) { s.tap[k] = o; o += up64((int64_t)2 * TAP_CH[net][k] * th[k] * tw[k]); }
    // the largest map that is no tap: vgg conv1_1's [2,64,h,w]; alex: the pool of tap 0 (smaller than tap 0)
    const int64_t work = up64((int64_t)2 * 64 * th[0] * tw[0]);
    s.wa = o; o += work;
    s.wb = o; o += work;
    s.partial = o;
    s.bytes = o * 4 + partial_count(net, h, w) * 8;
    return s;
}

}  // namespace
}  // namespace hnr

using namespace hnr;

#define BAD(...) do { set_error(__VA_ARGS__); return HNR_ERR_BADARG; } while (0)
#define CHECK_NET_SHAPE(fn) do { \
    if (!net_ok(net)) BAD(fn ": net=%d (0 alex, 1 vgg)", net); \
    if (!shape_ok(net, h, w)) BAD(fn ": h=%d w=%d (%d .. %d for this net)", h, w, min_size(net), MAX_HW); } while (0)
#define CHECK_SCRATCH(fn) do { \
    if (!d_scratch || ((uintptr_t)d_scratch & 15)) BAD(fn ": scratch must be a 16-byte aligned device pointer"); \
    if (scratch_bytes < scratch_layout(net, h, w).bytes) BAD(fn ": scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)scratch_layout(net, h, w).bytes); } while (0)
#define CHECK_PACKED(fn) do { if (!d_packed || ((uintptr_t)d_packed & 15)) BAD(fn ": d_packed must be a 16-byte aligned device pointer"); } while (0)

extern "C" {

int64_t hnr_lpips_packed_elems(int net) { return net_ok(net) ? packed_elems(net) : -1; }

int64_t hnr_lpips_scratch_bytes(int net, int h, int w) { return net_ok(net) && shape_ok(net, h, w) ? scratch_layout(net, h, w).bytes : -1; }

int hnr_lpips_tap_dims(int net, int h, int w, int *dims)
{
    if (!dims) BAD("hnr_lpips_tap_dims: NULL pointer");
    CHECK_NET_SHAPE("hnr_lpips_tap_dims");
    int th[5], tw[5];
    tap_dims(net, h, w, th, tw);
    for (int k = 0; k < 5; ++k) { dims[3 * k] = TAP_CH[net][k]; dims[3 * k + 1] = th[k]; dims[3 * k + 2] = tw[k]; }
    return HNR_OK;
}

int hnr_lpips_prepare(const uint8_t *d_img8, const uint8_t *d_gt8, int h, int w, int bgr, const float *d_packed, float *d_x, void *stream)
{
    if (!d_img8 || !d_gt8 || !d_packed || !d_x) BAD("hnr_lpips_prepare: NULL pointer");
    if (h < 1 || w < 1 || h > MAX_HW || w > MAX_HW) BAD("hnr_lpips_prepare: h=%d w=%d (1 .. %d)", h, w, MAX_HW);
    lpips_prepare8_kernel<<<cdiv((int64_t)2 * h * w, 256), 256, 0, (hipStream_t)stream>>>(d_img8, d_gt8, h * w, bgr != 0, d_packed, d_x);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

int hnr_lpips_prepare_f32(const float *d_in0, const float *d_in1, int h, int w, const float *d_packed, float *d_x, void *stream)
{
    if (!d_in0 || !d_in1 || !d_packed || !d_x) BAD("hnr_lpips_prepare_f32: NULL pointer");
    if (h < 1 || w < 1 || h > MAX_HW || w > MAX_HW) BAD("hnr_lpips_prepare_f32: h=%d w=%d (1 .. %d)", h, w, MAX_HW);
    lpips_prepare_f32_kernel<<<cdiv((int64_t)6 * h * w, 256), 256, 0, (hipStream_t)stream>>>(d_in0, d_in1, h * w, d_packed, d_x);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

int hnr_lpips_features(int net, const float *d_x, int h, int w, const float *d_packed, float *const *d_taps, void *d_scratch, int64_t scratch_bytes,
                       void *stream)
{
    CHECK_NET_SHAPE("hnr_lpips_features");
    if (!d_x || !d_taps) BAD("hnr_lpips_features: NULL pointer");
    for (int k = 0; k < 5; ++k) if (!d_taps[k]) BAD("hnr_lpips_features: tap %d is NULL", k);
    CHECK_PACKED("hnr_lpips_features");
    CHECK_SCRATCH("hnr_lpips_features");
    const Scratch s = scratch_layout(net, h, w);
    float *base = (float *)d_scratch;
    return features(net, d_x, h, w, d_packed, d_taps, base + s.wa, base + s.wb, (hipStream_t)stream);
}

int hnr_lpips_score(int net, const float *const *d_taps, int h, int w, const float *d_packed, double *d_row, void *d_scratch, int64_t scratch_bytes,
                    void *stream)
{
    CHECK_NET_SHAPE("hnr_lpips_score");
    if (!d_taps || !d_row) BAD("hnr_lpips_score: NULL pointer");
    for (int k = 0; k < 5; ++k) if (!d_taps[k]) BAD("hnr_lpips_score: tap %d is NULL", k);
    CHECK_PACKED("hnr_lpips_score");
    CHECK_SCRATCH("hnr_lpips_score");
    const Scratch s = scratch_layout(net, h, w);
    return score(net, d_taps, h, w, d_packed, d_row, (double *)((float *)d_scratch + s.partial), (hipStream_t)stream);
}

static int chain(int net, int h, int w, const float *d_packed, double *d_row, void *d_scratch, hipStream_t st)
{
    const Scratch s = scratch_layout(net, h, w);
    float *base = (float *)d_scratch, *taps[5];
    for (int k = 0; k < 5; ++k) taps[k] = base + s.tap[k];
    TRY(features(net, base + s.x, h, w, d_packed, taps, base + s.wa, base + s.wb, st));
    return score(net, taps, h, w, d_packed, d_row, (double *)(base + s.partial), st);
}

int hnr_lpips(int net, const uint8_t *d_img8, const uint8_t *d_gt8, int h, int w, int bgr, const float *d_packed, double *d_row, void *d_scratch,
              int64_t scratch_bytes, void *stream)
{
    CHECK_NET_SHAPE("hnr_lpips");
    if (!d_img8 || !d_gt8 || !d_row) BAD("hnr_lpips: NULL pointer");
    CHECK_PACKED("hnr_lpips");
    CHECK_SCRATCH("hnr_lpips");
    TRY(hnr_lpips_prepare(d_img8, d_gt8, h, w, bgr, d_packed, (float *)d_scratch + scratch_layout(net, h, w).x, stream));
    return chain(net, h, w, d_packed, d_row, d_scratch, (hipStream_t)stream);
}

int hnr_lpips_f32(int net, const float *d_in0, const float *d_in1, int h, int w, const float *d_packed, double *d_row, void *d_scratch,
                  int64_t scratch_bytes, void *stream)
{
    CHECK_NET_SHAPE("hnr_lpips_f32");
    if (!d_in0 || !d_in1 || !d_row) BAD("hnr_lpips_f32: NULL pointer");
    CHECK_PACKED("hnr_lpips_f32");
    CHECK_SCRATCH("hnr_lpips_f32");
    TRY(hnr_lpips_prepare_f32(d_in0, d_in1, h, w, d_packed, (float *)d_scratch + scratch_layout(net, h, w).x, stream));
    return chain(net, h, w, d_packed, d_row, d_scratch, (hipStream_t)stream);
}

}  // extern "C"
