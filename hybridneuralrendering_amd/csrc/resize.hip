// Raw frames to the frame bank's size on the device: Pillow's convolution resize for 8-bit images, bit for bit, and the steps of RGBA mode around it.
//
// Replaces the reference's per-frame `Image.open(...).resize(self.img_wh, Image.LANCZOS)` (data/scannet_ft_dataset.py:742,824,
// data/nerf_synth360_ft_dataset.py:531,762), decoding aside, and the white / black / alpha / mask images of nerf_synth360_ft_dataset.py:532-536.
// Pillow (src/libImaging/Resample.c, 8 bits per channel) computes, per axis, integer coefficient tables in double arithmetic and then two integer
// passes: horizontal into an image ROUNDED TO uint8, vertical on that image; a pass whose size does not change is skipped.  Here:
//
//   hnr_resize_coeffs       host, no GPU call: one axis's bounds [out,2] and coefficients [out,ksize] for Pillow's five convolution filters.  The
//                           kernels see only tables, so they know nothing of filters.
//   resize_fused_kernel     one launch.  A workgroup owns TILE_W x TILE_H output pixels; it stages the input rows and columns the tile's two
//                           supports reach into LDS as bytes, runs the horizontal pass from LDS into an LDS intermediate (uint8, rounded as Pillow
//                           rounds it), runs the vertical pass from that and stores the tile.  The intermediate image never reaches HBM.
//   resize_h_kernel / _v_   the same two passes as two launches through a scratch intermediate, one lane per output element: for tiles whose
//                           footprint exceeds the LDS budget (extreme reductions), and the cross-check of the fused form.
//   rgba_*_kernel           premultiply / un-premultiply (Pillow's RGBA <-> RGBa conversions) and the compose step, one lane per pixel.
//
// LDS layout of the fused kernel (DESIGN.md has the reasoning): [horizontal coefficients: tile column x taps, odd pitch][vertical: tile row x taps]
// [input tile: rows x in_pitch bytes][intermediate: rows x mid_pitch bytes].  An input row keeps the phase of its global address modulo 4, so rows are
// staged with aligned dword loads whatever the source's alignment (the head and tail bytes of a row go one by one) and land with conflict-free
// ds_write_b32.  The horizontal pass gives a wave four input rows and gives lane l the l-th (column, channel) of the tile: the 32 lanes of a group
// read bytes of at most a few dozen consecutive dwords of one row (several lanes per dword, which broadcast), the coefficient of lane l sits
// at column x odd pitch (distinct banks), and one coefficient read serves four rows.  The vertical pass gives a wave an output row and a lane C of its
// bytes, 64 apart: its coefficients are one address per wave, serving C sums, and the bytes of a read are consecutive.
//
// Stream-ordered; nothing is allocated, nothing is read back.  Bounds read from the tables are clamped to the staged ranges, so a table that did not
// come from hnr_resize_coeffs gives wrong pixels, never an access outside the buffers.
#include <math.h>

#include "hnr_launch.h"

namespace hnr {

constexpr int RS_TW = HNR_RESIZE_TILE_W, RS_TH = HNR_RESIZE_TILE_H, RS_ROWS = 4, RS_BITS = 22;
constexpr int RS_STATIC_LDS = 8 * (RS_TW + RS_TH);                      // the fused kernel's two static bounds arrays

// ------------------------------------------------------------------------------------------------ coefficients (host)
static double rs_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double rs_filter(int id, double x)
{
    switch (id) {
    case HNR_RESIZE_BOX: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case HNR_RESIZE_BILINEAR:
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    case HNR_RESIZE_HAMMING:
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * M_PI;
        return sin(x) / x * (0.54 + 0.46 * cos(x));
    case HNR_RESIZE_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
        if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
        return 0.0;
    }
    default: return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3) : 0.0;
    }
}

static const double rs_support[5] = {0.5, 1.0, 1.0, 2.0, 3.0};

// ------------------------------------------------------------------------------------------------ the fused form
struct RsFused {
    const uint8_t *src;
    uint8_t *dst;
    const int2 *bh, *bv;
    const int *ch, *cv;
    int h, w, H, W, kh, kv;
    int span_c, span_r;          // staged input columns / rows at most
    int khs, kvs;                // taps staged per tile column / row (odd pitches of the coefficient blocks)
    int in_pitch, mid_pitch;     // bytes, multiples of 4
    int tiles_x;
};

// what one tile needs, from sizes alone (the tables live on the device): for T consecutive outputs the supports reach from
// xmin(first) >= centre - support - 0.5 to xmin + xmax (last) <= centre + support + 0.5, i.e. at most (T - 1) scale + 2 support + 1
// <= ceil((T - 1) in / out) + ksize elements; one more for the rounding of the table's double arithmetic.
static int rs_span(int n_in, int n_out, int T, int ksize)
{
    const int64_t s = ((int64_t)(T - 1) * n_in + n_out - 1) / n_out + ksize + 1;
    return (int)(s < n_in ? s : n_in);
}

static int64_t rs_fused_layout(int h, int w, int C, int H, int W, int kh, int kv, RsFused *f)
{
    const int tw = W < RS_TW ? W : RS_TW, th = H < RS_TH ? H : RS_TH;
    const bool hp = w != W, vp = h != H;
    const int span_c = hp ? rs_span(w, W, tw, kh) : tw, span_r = vp ? rs_span(h, H, th, kv) : th;
    const int khs = hp ? ((kh < span_c ? kh : span_c) | 1) : 0, kvs = vp ? ((kv < span_r ? kv : span_r) | 1) : 0;
    const int64_t in_pitch = (((int64_t)span_c * C + 6) >> 2) << 2, mid_pitch = ((int64_t)tw * C + 3) & ~(int64_t)3;
    if (f) {
        f->span_c = span_c; f->span_r = span_r; f->khs = khs; f->kvs = kvs;
        f->in_pitch = (int)(in_pitch < (1 << 30) ? in_pitch : (1 << 30)); f->mid_pitch = (int)mid_pitch;
    }
    // (static + dynamic: the budget is the 64 KB of LDS a kernel gets without asking; the launch passes the dynamic part alone)
    return RS_STATIC_LDS + 4 * ((int64_t)tw * khs + (int64_t)th * kvs) + span_r * in_pitch + (hp && vp ? span_r * mid_pitch : 0);
}

__device__ __forceinline__ int rs_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint8_t rs_clip8(int acc)
{
    const int v = acc >> RS_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

template <int C, bool HP, bool VP>
__global__ void __launch_bounds__(256) resize_fused_kernel(RsFused a)
{
    extern __shared__ int rs_lds[];
    __shared__ int2 s_bh[RS_TW], s_bv[RS_TH];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x, n = blockIdx.y;
    const int x0 = tile_x * RS_TW, y0 = tile_y * RS_TH;
    const int tw = a.W - x0 < RS_TW ? a.W - x0 : RS_TW, th = a.H - y0 < RS_TH ? a.H - y0 : RS_TH;
    // the input columns [c0, c1) and rows [r0, r1) the tile reads: from its first and last bounds (both ends grow with the output index)
    int c0 = x0, c1 = x0 + tw, r0 = y0, r1 = y0 + th;
    if (HP) {
        const int2 bl = a.bh[x0 + tw - 1];
        c0 = rs_clampi(a.bh[x0].x, 0, a.w);
        c1 = rs_clampi(bl.x + bl.y, c0, a.w - c0 < a.span_c ? a.w : c0 + a.span_c);
    }
    if (VP) {
        const int2 bl = a.bv[y0 + th - 1];
        r0 = rs_clampi(a.bv[y0].x, 0, a.h);
        r1 = rs_clampi(bl.x + bl.y, r0, a.h - r0 < a.span_r ? a.h : r0 + a.span_r);
    }
    const int ncols = c1 - c0, nr = r1 - r0, ncc = tw * C;
    const int twm = a.W < RS_TW ? a.W : RS_TW, thm = a.H < RS_TH ? a.H : RS_TH;     // a full tile's size: what the layout was sized for
    int *s_ch = rs_lds, *s_cv = s_ch + twm * a.khs;                        // (a.khs = 0 without a horizontal pass)
    uint8_t *s_in = (uint8_t *)(s_cv + thm * a.kvs), *s_mid = s_in + (size_t)a.span_r * a.in_pitch;
    // bounds relative to the staged ranges and clamped to them; coefficients
    if (HP) {
        if (t < tw) {
            const int2 b = a.bh[x0 + t];
            const int xmin = rs_clampi(b.x, c0, c1) - c0;
            const int most = ncols - xmin < a.kh ? ncols - xmin : a.kh;
            s_bh[t] = make_int2(xmin, rs_clampi(b.y, 0, most));
        }
        for (int i = t; i < tw * a.khs; i += 256) {
            const int col = i / a.khs, x = i - col * a.khs;
            s_ch[i] = x < a.kh ? a.ch[(size_t)(x0 + col) * a.kh + x] : 0;
        }
    }
    if (VP) {
        if (t < th) {
            const int2 b = a.bv[y0 + t];
            const int ymin = rs_clampi(b.x, r0, r1) - r0;
            const int most = nr - ymin < a.kv ? nr - ymin : a.kv;
            s_bv[t] = make_int2(ymin, rs_clampi(b.y, 0, most));
        }
        for (int i = t; i < th * a.kvs; i += 256) {
            const int row = i / a.kvs, y = i - row * a.kvs;
            s_cv[i] = y < a.kv ? a.cv[(size_t)(y0 + row) * a.kv + y] : 0;
        }
    }
    // the input tile: row r of the tile starts at global byte g0; it lands at s_in[r * in_pitch + (g0 & 3)], so every whole dword of the
    // row is an aligned dword on both sides; the bytes of a dword that is only partly the row's are moved one by one
    const uint8_t *src_n = a.src + (size_t)n * a.h * a.w * C;
    const size_t row_bytes = (size_t)a.w * C;
    const uint8_t *g00 = src_n + ((size_t)r0 * a.w + c0) * C;
    const int len = ncols * C;
    for (int r = wave; r < nr; r += 4) {
        const uint8_t *g0 = g00 + (size_t)r * row_bytes;
        const int sh = (int)((uintptr_t)g0 & 3);
        const uint8_t *a0 = g0 - sh;
        uint8_t *d0 = s_in + (size_t)r * a.in_pitch;
        const int ndw = (sh + len + 3) >> 2;
        for (int i = lane; i < ndw; i += 64) {
            const int lo = 4 * i, hi = 4 * i + 4;
            if (lo >= sh && hi <= sh + len) {
                *(uint32_t *)(d0 + lo) = *(const uint32_t *)(a0 + lo);
            } else {
                for (int b = lo < sh ? sh : lo; b < (hi < sh + len ? hi : sh + len); ++b) d0[b] = a0[b];
            }
        }
    }
    __syncthreads();
    uint8_t *dst_n = a.dst + ((size_t)n * a.H * a.W) * C;
    const unsigned g00_lo = (unsigned)(uintptr_t)g00, row_lo = (unsigned)row_bytes;
    if (HP) {
        // horizontal: a wave takes RS_ROWS staged rows, lane l the l-th (column, channel); one coefficient read serves the rows
        for (int g = wave; g * RS_ROWS < nr; g += 4) {
            for (int cc = lane; cc < ncc; cc += 64) {
                const int col = cc / C, chn = cc - col * C;
                const int2 b = s_bh[col];
                int base[RS_ROWS], acc[RS_ROWS];
#pragma unroll
                for (int j = 0; j < RS_ROWS; ++j) {
                    const int row = g * RS_ROWS + j < nr ? g * RS_ROWS + j : nr - 1;
                    base[j] = row * a.in_pitch + (int)((g00_lo + (unsigned)row * row_lo) & 3u) + b.x * C + chn;
                    acc[j] = 1 << (RS_BITS - 1);
                }
                const int *k = s_ch + col * a.khs;
                for (int x = 0; x < b.y; ++x) {
                    const int kx = k[x];
#pragma unroll
                    for (int j = 0; j < RS_ROWS; ++j) acc[j] += (int)s_in[base[j] + x * C] * kx;
                }
#pragma unroll
                for (int j = 0; j < RS_ROWS; ++j) {
                    const int row = g * RS_ROWS + j;
                    if (row < nr) {
                        if (VP) s_mid[row * a.mid_pitch + cc] = rs_clip8(acc[j]);
                        else dst_n[((size_t)(y0 + row) * a.W + x0) * C + cc] = rs_clip8(acc[j]);      // (no vertical pass: staged row = output row)
                    }
                }
            }
        }
    }
    if (VP) {
        if (HP) __syncthreads();
        // vertical: a wave takes an output row, lane l its bytes l, l + 64, ... (C of them: a tile row has at most 64 C bytes), so one coefficient
        // read serves C independent sums; without a horizontal pass it reads the staged input itself
        for (int ty = wave; ty < th; ty += 4) {
            const int2 b = s_bv[ty];
            const int *k = s_cv + ty * a.kvs;
            int acc[C], off[C];
#pragma unroll
            for (int q = 0; q < C; ++q) {
                acc[q] = 1 << (RS_BITS - 1);
                off[q] = lane + 64 * q < ncc ? lane + 64 * q : ncc - 1;         // (a lane past the row's end reads its last byte and stores nothing)
            }
            for (int y = 0; y < b.y; ++y) {
                const int row = b.x + y, ky = k[y];
                const int at = HP ? row * a.mid_pitch : row * a.in_pitch + (int)((g00_lo + (unsigned)row * row_lo) & 3u);
#pragma unroll
                for (int q = 0; q < C; ++q) acc[q] += (int)(HP ? s_mid[at + off[q]] : s_in[at + off[q]]) * ky;
            }
#pragma unroll
            for (int q = 0; q < C; ++q)
                if (lane + 64 * q < ncc) dst_n[((size_t)(y0 + ty) * a.W + x0) * C + lane + 64 * q] = rs_clip8(acc[q]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ the two-pass form
// horizontal: src [rows, w, C] -> out [rows, W, C], one lane per output byte
__global__ void __launch_bounds__(256) resize_h_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ out, int64_t rows, int w, int W, int C,
                                                       const int2 *__restrict__ bh, const int *__restrict__ ch, int kh)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t wc = (int64_t)W * C;
    if (idx >= rows * wc) return;
    const int64_t row = idx / wc;
    const int cc = (int)(idx - row * wc), col = cc / C, chn = cc - col * C;
    const int2 b = bh[col];
    const int xmin = rs_clampi(b.x, 0, w), xmax = rs_clampi(b.y, 0, w - xmin < kh ? w - xmin : kh);
    const uint8_t *p = src + ((size_t)row * w + xmin) * C + chn;
    const int *k = ch + (size_t)col * kh;
    int acc = 1 << (RS_BITS - 1);
    for (int x = 0; x < xmax; ++x) acc += (int)p[(size_t)x * C] * k[x];
    out[idx] = rs_clip8(acc);
}

// vertical: in [N, h, wc] -> out [N, H, wc]
__global__ void __launch_bounds__(256) resize_v_kernel(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, int N, int h, int H, int64_t wc,
                                                       const int2 *__restrict__ bv, const int *__restrict__ cv, int kv)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * H * wc) return;
    const int64_t q = idx / wc, cc = idx - q * wc;
    const int n = (int)(q / H), y = (int)(q - (int64_t)n * H);
    const int2 b = bv[y];
    const int ymin = rs_clampi(b.x, 0, h), ymax = rs_clampi(b.y, 0, h - ymin < kv ? h - ymin : kv);
    const uint8_t *p = in + ((size_t)n * h + ymin) * wc + cc;
    const int *k = cv + (size_t)y * kv;
    int acc = 1 << (RS_BITS - 1);
    for (int yy = 0; yy < ymax; ++yy) acc += (int)p[(size_t)yy * wc] * k[yy];
    out[idx] = rs_clip8(acc);
}

// ------------------------------------------------------------------------------------------------ RGBA mode, compose
// Pillow's MULDIV255 / its rgba2rgbA: see include/hnr.h.  Bytes are moved one by one: a frame view may start at any byte.
__global__ void __launch_bounds__(256) rgba_premultiply_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = src + 4 * i;
    uint8_t *d = dst + 4 * i;
    const int al = hnr_opaque((int)s[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int tmp = hnr_opaque((int)s[c]) * al + 128;
        d[c] = (uint8_t)(((tmp >> 8) + tmp) >> 8);
    }
    d[3] = (uint8_t)al;
}

__global__ void __launch_bounds__(256) rgba_unpremultiply_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = src + 4 * i;
    uint8_t *d = dst + 4 * i;
    const int al = hnr_opaque((int)s[3]);
    const bool keep = al == 0 || al == 255;
    const unsigned den = (unsigned)(al > 0 ? al : 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = hnr_opaque((int)s[c]);
        const unsigned q = (255u * (unsigned)v) / den;
        d[c] = (uint8_t)(keep ? (unsigned)v : (q > 255u ? 255u : q));
    }
    d[3] = (uint8_t)al;
}

// c, a = u8 / 255 (a division, as ToTensor); black = c a; white = black + (1 - a); alpha = a; mask = a > 0.1: every operation rounded on its own
__global__ void __launch_bounds__(256) rgba_compose_kernel(const uint8_t *__restrict__ rgba, int64_t n, float *__restrict__ white, float *__restrict__ black,
                                                           float *__restrict__ alpha, float *__restrict__ mask)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = rgba + 4 * i;
    const float al = hnr_div((float)hnr_opaque((int)s[3]), 255.0f);
    const float rest = __fsub_rn(1.0f, al);
    if (alpha) alpha[i] = al;
    if (mask) mask[i] = al > 0.1f ? 1.0f : 0.0f;
    if (white || black) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float b = __fmul_rn(hnr_div((float)hnr_opaque((int)s[c]), 255.0f), al);
            if (black) black[3 * i + c] = b;
            if (white) white[3 * i + c] = __fadd_rn(b, rest);
        }
    }
}

static bool rs_shape_ok(const char *who, int N, int h, int w, int C, int H, int W)
{
    if (N < 1 || N > 65535 || h < 1 || w < 1 || H < 1 || W < 1 || (int64_t)h * w > (1 << 26) || (int64_t)H * W > (1 << 26) ||
        (int64_t)N * (h > H ? h : H) * (w > W ? w : W) > ((int64_t)1 << 36)) {
        set_error("%s: 1 <= N <= 65535, all sizes >= 1, h * w and H * W <= 2^26, N max(h, H) max(w, W) <= 2^36", who); return false;
    }
    if (C != 1 && C != 3 && C != 4) { set_error("%s: C must be 1, 3 or 4, got %d", who, C); return false; }
    return true;
}

template <int C>
static int rs_launch_fused(const RsFused &f, bool hp, bool vp, dim3 grid, int lds, hipStream_t st)
{
    if (hp && vp) resize_fused_kernel<C, true, true><<<grid, 256, lds, st>>>(f);
    else if (hp) resize_fused_kernel<C, true, false><<<grid, 256, lds, st>>>(f);
    else resize_fused_kernel<C, false, true><<<grid, 256, lds, st>>>(f);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_resize_coeffs(int n_in, int n_out, int filter, int32_t *bounds, int32_t *coef, int64_t coef_elems)
{
    const char *who = "hnr_resize_coeffs";
    if (n_in < 1 || n_out < 1 || n_in > (1 << 26) || n_out > (1 << 26)) { set_error("%s: 1 <= n_in, n_out <= 2^26", who); return HNR_ERR_BADARG; }
    if (filter < HNR_RESIZE_BOX || filter > HNR_RESIZE_LANCZOS) { set_error("%s: filter must be 0 (box) .. 4 (lanczos), got %d", who, filter); return HNR_ERR_BADARG; }
    const double scale = (double)n_in / (double)n_out;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = rs_support[filter] * filterscale;
    const double ks = ceil(support) * 2 + 1;
    if (ks > (double)(1 << 28)) { set_error("%s: the filter spans too many taps", who); return HNR_ERR_TOOBIG; }
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!bounds && !coef) return ksize;                             // sizing call
    if (!bounds || !coef || coef_elems < (int64_t)n_out * ksize) {
        set_error("%s: bounds [n_out,2] and coef [n_out,ksize] (%lld elements) are both needed", who, (long long)n_out * ksize); return HNR_ERR_BADARG;
    }
    const double ss = 1.0 / filterscale;
    double *k = (double *)malloc(sizeof(double) * (size_t)ksize);
    if (!k) { set_error("%s: out of host memory", who); return HNR_ERR_NOMEM; }
    for (int xx = 0; xx < n_out; ++xx) {
        const double center = (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > n_in) xmax = n_in;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = rs_filter(filter, (x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        int32_t *kk = coef + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? k[x] / ww : k[x];
            kk[x] = v < 0 ? (int32_t)(-0.5 + v * (1 << RS_BITS)) : (int32_t)(0.5 + v * (1 << RS_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    free(k);
    return ksize;
}

extern "C" int64_t hnr_resize_u8_scratch_bytes(int N, int h, int w, int C, int H, int W)
{
    if (!rs_shape_ok("hnr_resize_u8_scratch_bytes", N, h, w, C, H, W)) return -1;
    return (w != W && h != H) ? (int64_t)N * h * W * C : 0;
}

extern "C" int hnr_resize_u8_form(int h, int w, int C, int H, int W, int ksize_h, int ksize_v)
{
    if (!rs_shape_ok("hnr_resize_u8_form", 1, h, w, C, H, W)) return HNR_ERR_BADARG;
    if ((w != W && ksize_h < 1) || (h != H && ksize_v < 1)) { set_error("hnr_resize_u8_form: ksize >= 1 for a pass that runs"); return HNR_ERR_BADARG; }
    return rs_fused_layout(h, w, C, H, W, ksize_h, ksize_v, nullptr) <= HNR_RESIZE_LDS_BUDGET ? HNR_RESIZE_FUSED : HNR_RESIZE_TWO_PASS;
}

extern "C" int hnr_resize_u8(const uint8_t *d_src, int N, int h, int w, int C, uint8_t *d_dst, int H, int W, const int32_t *d_bounds_h,
                             const int32_t *d_coef_h, int ksize_h, const int32_t *d_bounds_v, const int32_t *d_coef_v, int ksize_v, int form,
                             void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "hnr_resize_u8";
    if (!rs_shape_ok(who, N, h, w, C, H, W)) return HNR_ERR_BADARG;
    if (!d_src || !d_dst) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    const bool hp = w != W, vp = h != H;
    if ((hp && (!d_bounds_h || !d_coef_h || ksize_h < 1)) || (vp && (!d_bounds_v || !d_coef_v || ksize_v < 1))) {
        set_error("%s: a pass that changes a size needs its bounds and coefficient tables and ksize >= 1", who); return HNR_ERR_BADARG;
    }
    if ((((uintptr_t)d_bounds_h | (uintptr_t)d_bounds_v) & 7) || (((uintptr_t)d_coef_h | (uintptr_t)d_coef_v) & 3)) {
        set_error("%s: bounds tables must be 8-byte aligned, coefficient tables 4-byte", who); return HNR_ERR_BADARG;
    }
    if (form < HNR_RESIZE_AUTO || form > HNR_RESIZE_TWO_PASS) { set_error("%s: form must be 0 (auto), 1 (fused) or 2 (two_pass)", who); return HNR_ERR_BADARG; }
    RsFused f;
    memset(&f, 0, sizeof(f));
    const int64_t lds = rs_fused_layout(h, w, C, H, W, ksize_h, ksize_v, &f);
    if (form == HNR_RESIZE_AUTO) form = lds <= HNR_RESIZE_LDS_BUDGET ? HNR_RESIZE_FUSED : HNR_RESIZE_TWO_PASS;
    if (form == HNR_RESIZE_FUSED && lds > HNR_RESIZE_LDS_BUDGET) {
        set_error("%s: a tile of the fused form needs %lld bytes of LDS, the budget is %d: use auto or two_pass", who, (long long)lds, HNR_RESIZE_LDS_BUDGET);
        return HNR_ERR_BADARG;
    }
    const int64_t mid_bytes = (hp && vp) ? (int64_t)N * h * W * C : 0;
    if (form == HNR_RESIZE_TWO_PASS && mid_bytes > 0 && (!d_scratch || scratch_bytes < mid_bytes)) {
        set_error("%s: scratch smaller than hnr_resize_u8_scratch_bytes", who); return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!hp && !vp) {                                               // neither size changes: a copy, as Pillow's
        HNR_HIP_CHECK(hipMemcpyAsync(d_dst, d_src, (size_t)N * h * w * C, hipMemcpyDeviceToDevice, st));
        return HNR_OK;
    }
    const int2 *bh = (const int2 *)d_bounds_h, *bv = (const int2 *)d_bounds_v;
    if (form == HNR_RESIZE_FUSED) {
        f.src = d_src; f.dst = d_dst; f.bh = bh; f.bv = bv; f.ch = d_coef_h; f.cv = d_coef_v;
        f.h = h; f.w = w; f.H = H; f.W = W; f.kh = hp ? ksize_h : 0; f.kv = vp ? ksize_v : 0;
        f.tiles_x = cdiv(W, RS_TW);
        const dim3 grid((unsigned)(f.tiles_x * cdiv(H, RS_TH)), (unsigned)N);
        return C == 1 ? rs_launch_fused<1>(f, hp, vp, grid, (int)lds - RS_STATIC_LDS, st) : C == 3 ? rs_launch_fused<3>(f, hp, vp, grid, (int)lds - RS_STATIC_LDS, st)
                                                                                   : rs_launch_fused<4>(f, hp, vp, grid, (int)lds - RS_STATIC_LDS, st);
    }
    const int64_t wc = (int64_t)W * C;
    const uint8_t *vsrc = d_src;
    if (hp) {
        uint8_t *hout = vp ? (uint8_t *)d_scratch : d_dst;
        const int64_t n_el = (int64_t)N * h * wc;
        resize_h_kernel<<<(unsigned)((n_el + 255) / 256), 256, 0, st>>>(d_src, hout, (int64_t)N * h, w, W, C, bh, d_coef_h, ksize_h);
        HNR_LAUNCH_CHECK();
        vsrc = hout;
    }
    if (vp) {
        const int64_t n_el = (int64_t)N * H * wc;
        resize_v_kernel<<<(unsigned)((n_el + 255) / 256), 256, 0, st>>>(vsrc, d_dst, N, h, H, wc, bv, d_coef_v, ksize_v);
        HNR_LAUNCH_CHECK();
    }
    return HNR_OK;
}

static int rs_pixels_ok(const char *who, const void *a, const void *b, int64_t n)
{
    if (n < 0 || n > ((int64_t)1 << 36)) { set_error("%s: 0 <= n_pixels <= 2^36", who); return HNR_ERR_BADARG; }
    if (n > 0 && (!a || !b)) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    return HNR_OK;
}

extern "C" int hnr_rgba_premultiply(const uint8_t *d_src, uint8_t *d_dst, int64_t n_pixels, void *stream)
{
    if (rs_pixels_ok("hnr_rgba_premultiply", d_src, d_dst, n_pixels)) return HNR_ERR_BADARG;
    if (n_pixels == 0) return HNR_OK;
    rgba_premultiply_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_src, d_dst, n_pixels);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_rgba_unpremultiply(const uint8_t *d_src, uint8_t *d_dst, int64_t n_pixels, void *stream)
{
    if (rs_pixels_ok("hnr_rgba_unpremultiply", d_src, d_dst, n_pixels)) return HNR_ERR_BADARG;
    if (n_pixels == 0) return HNR_OK;
    rgba_unpremultiply_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_src, d_dst, n_pixels);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_rgba_compose(const uint8_t *d_rgba, int64_t n_pixels, float *d_white, float *d_black, float *d_alpha, float *d_mask, void *stream)
{
    const char *who = "hnr_rgba_compose";
    if (!d_white && !d_black && !d_alpha && !d_mask) { set_error("%s: no output", who); return HNR_ERR_BADARG; }
    if (rs_pixels_ok(who, d_rgba, d_rgba, n_pixels)) return HNR_ERR_BADARG;
    if (n_pixels == 0) return HNR_OK;
    rgba_compose_kernel<<<(unsigned)((n_pixels + 255) / 256), 256, 0, (hipStream_t)stream>>>(d_rgba, n_pixels, d_white, d_black, d_alpha, d_mask);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
