// Device code of the dataset item that more than one file launches: the per-ray kernel (pixel, direction, ground truth) and the reference-image
// kernels (uint8 -> float32, float32 copies), with the argument blocks they read.  frames.hip (items of a bank row) and path.hip (items of a free
// camera) each include this once; the arithmetic, and so every bit of an item, is one definition.
//
// A kernel needs one name per file that launches it (the files are linked into one library): HNR_FRAMES_KERNEL(name) is `name` unless the
// including file defines it otherwise (path.hip: path_<name>).  frames.hip's kernels keep their names and their code.
//
// Every fp32 operation is rounded on its own in the order written (-ffp-contract=off, correctly rounded divide and sqrt); tests/frames_ref.py restates it.
#pragma once
#include "hnr_common.h"
#include "hnr_launch.h"

#ifndef HNR_FRAMES_KERNEL
#define HNR_FRAMES_KERNEL(name) name
#endif

namespace hnr {

constexpr int FB_RANDOM = 0, FB_PATCH = 1, FB_DILATED = 2, FB_PIXELS = 3, FB_NO_CROP = 4;       // FB_PIXELS / FB_NO_CROP: hnr_frame_item only
constexpr unsigned PURPOSE_RANDOM = 0u, PURPOSE_PATCH = 1u, PURPOSE_BG = 2u;
constexpr int HDR_WORDS = 4;        // scratch head: {frame row, step low, step high, 0}, then the patch table (d, x0, y0) x pn^2

struct Philox { unsigned w[4]; };

__host__ __device__ static inline size_t fb_min(size_t a, size_t b) { return a < b ? a : b; }

__device__ __forceinline__ Philox philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Philox p;
    p.w[0] = c0; p.w[1] = c1; p.w[2] = c2; p.w[3] = c3;
    return p;
}

// lo + ((uint64) u * (uint32)(hi - lo) >> 32): lo <= result < hi for hi > lo
__device__ __forceinline__ int fb_randint(unsigned u, int lo, int hi) { return lo + (int)__umulhi(u, (unsigned)(hi - lo)); }

struct BankView {
    const void *images;
    const float *c2w, *w2c, *K, *weight, *angle;
    int f32, F, H, W, K_per_frame;
};

struct BatchArgs {
    int mode, S, pn, ps, dlo, dhi, margin, dir_norm, bg_random, downweight, V, R;
    float bg[3];
    unsigned seed_lo, seed_hi;
};

struct BatchOut {
    float *raydir, *pixel_idx, *gt_image, *campos, *camrot, *c2w, *intrinsic, *c2w_nearest, *w2c_nearest, *campos_nearest, *intrinsic_nearest, *images_nearest,
        *frame_weight_nearest, *vid_angle_nearest, *frame_weight, *bg_color;
    int *frame_row, *patch_table;
};

// (float) v / 255.0f, correctly rounded: hnr_div's fast path alone (v <= 255 and the divisor 255 are always inside its operand range), so the
// sixteen conversions of a lane carry no fallback branch and share one refined reciprocal
__device__ __forceinline__ float fb_u8(unsigned v)
{
    const float n = (float)v, d = 255.0f;
    float r = __builtin_amdgcn_rcpf(d);
    r = fmaf(fmaf(-d, r, 1.0f), r, r);
    const float q0 = __fmul_rn(n, r);
    const float q = fmaf(fmaf(-d, q0, n), r, q0);
    return v == 0u ? q0 : fmaf(fmaf(-d, q, n), r, q);
}

// one lane per ray: pixel, direction, ground truth of ray blockIdx.x * 256 + threadIdx.x of frame hdr[0]
__global__ void __launch_bounds__(256) HNR_FRAMES_KERNEL(frame_rays_kernel)(BankView tb, const int *__restrict__ hdr, const float *__restrict__ pixels, BatchArgs a, BatchOut o)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.R) return;
    const int row = hdr[0];
    float px, py;
    bool inside = true;
    if (a.mode == FB_RANDOM) {
        const Philox r = philox4x32_10((unsigned)hdr[1], (unsigned)hdr[2], PURPOSE_RANDOM, (unsigned)i, a.seed_lo, a.seed_hi);
        px = (float)fb_randint(r.w[0], a.margin, tb.W - a.margin);
        py = (float)fb_randint(r.w[1], a.margin, tb.H - a.margin);
    } else if (a.mode == FB_PIXELS) {
        px = pixels[2 * (size_t)i]; py = pixels[2 * (size_t)i + 1];
        inside = px > -1.f && px < (float)tb.W && py > -1.f && py < (float)tb.H;                  // (int) truncates toward zero; NaN compares false
    } else if (a.mode == FB_NO_CROP) {
        const int wn = tb.W - 2 * a.margin, y = i / wn;
        px = (float)(a.margin + (i - y * wn)); py = (float)(a.margin + y);
    } else {
        const int gy = i / a.S, gx = i - gy * a.S;
        const int pi = gy / a.ps, pa = gy - pi * a.ps, pj = gx / a.ps, pb = gx - pj * a.ps;
        const int *tab = hdr + HDR_WORDS + 3 * (pi * a.pn + pj);
        px = (float)(tab[1] + tab[0] * pb); py = (float)(tab[2] + tab[0] * pa);
    }
    if (o.pixel_idx) { o.pixel_idx[2 * (size_t)i] = px; o.pixel_idx[2 * (size_t)i + 1] = py; }
    if (o.raydir) {
        const float *K = tb.K + (tb.K_per_frame ? 9 * (size_t)row : 0), *M = tb.c2w + 16 * (size_t)row;
        const float x = hnr_div((px + 0.5f) - K[2], K[0]), y = hnr_div((py + 0.5f) - K[5], K[4]);
        float d[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (x * M[4 * c] + y * M[4 * c + 1]) + M[4 * c + 2];
        if (a.dir_norm) {
            const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + 1e-5f;
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = hnr_div(d[c], n);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o.raydir[3 * (size_t)i + c] = d[c];
    }
    if (o.gt_image) {
        float g[3] = {0.f, 0.f, 0.f};                                                             // a pixel outside the frame (hnr_frame_item): zeros
        if (inside) {
            const int ix = (int)px, iy = (int)py;
            const size_t e = 3 * (((size_t)row * tb.H + iy) * tb.W + ix);
#pragma unroll
            for (int c = 0; c < 3; ++c) g[c] = tb.f32 ? ((const float *)tb.images)[e + c] : fb_u8(((const uint8_t *)tb.images)[e + c]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) o.gt_image[3 * (size_t)i + c] = g[c];
    }
}

// The ray of ONE pixel outside the ray kernel (the centre-pixel direction of a camera, path.hip): frame_rays_kernel's expressions, operation for
// operation -- x = ((px + 0.5) - K02) / K00, y alike, dir[c] = (x R[c][0] + y R[c][1]) + R[c][2], R = M[:3,:3] of the row-major 4x4 M; normalised:
// dir / (sqrt((dx^2 + dy^2) + dz^2) + 1e-5).  (The kernel keeps its own text: routed through this function its additions come out with their
// operands swapped -- the same bits, but not the same code.)
__device__ __forceinline__ void fb_raydir(float px, float py, const float *K, const float *M, int dir_norm, float d[3])
{
    const float x = hnr_div((px + 0.5f) - K[2], K[0]), y = hnr_div((py + 0.5f) - K[5], K[4]);
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = (x * M[4 * c] + y * M[4 * c + 1]) + M[4 * c + 2];
    if (dir_norm) {
        const float n = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + 1e-5f;
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = hnr_div(d[c], n);
    }
}

// uint8 -> float32 of the V reference frames.  Per view of n = H*W*3 elements: `head` elements bring the DESTINATION onto a float4 boundary, then
// groups of 16 (one 16-byte load, which may be unaligned: frames of a bank whose n is no multiple of 16 start anywhere; four aligned float4 stores),
// then a tail of n - head - 16 groups < 16 elements.  Head and tail elements are converted one per lane by the first lanes of the grid.
__global__ void __launch_bounds__(256) HNR_FRAMES_KERNEL(frame_images_u8_kernel)(const uint8_t *__restrict__ images, size_t n, int V, int F, const int *__restrict__ hdr,
                                                                                 const int *__restrict__ nearest, float *__restrict__ out)
{
    const int row = hdr[0];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    if (gid < (size_t)V * 32) {
        const int v = (int)(gid >> 5), j = (int)(gid & 31);
        const size_t base = (size_t)v * n;
        const size_t head = fb_min((size_t)((4 - (base & 3)) & 3), n), groups = (n - head) >> 4, tail = n - head - (groups << 4);
        size_t e = n;
        if (j < 16) { if ((size_t)j < head) e = (size_t)j; }
        else if ((size_t)(j - 16) < tail) e = head + (groups << 4) + (size_t)(j - 16);
        if (e < n) {
            int nr = nearest[(size_t)row * V + v];
            if (nr < 0 || nr >= F) nr = 0;
            out[base + e] = fb_u8(images[(size_t)nr * n + e]);
        }
    }
    const size_t gmax = n >> 4;                                     // groups per view differ by at most one: stride over the larger count, test per view
    for (size_t w = gid; w < (size_t)V * gmax; w += stride) {
        const int v = (int)(w / gmax);
        const size_t k = w - (size_t)v * gmax, base = (size_t)v * n;
        const size_t head = fb_min((size_t)((4 - (base & 3)) & 3), n), groups = (n - head) >> 4;
        if (k >= groups) continue;
        int nr = nearest[(size_t)row * V + v];
        if (nr < 0 || nr >= F) nr = 0;
        const size_t e = head + (k << 4);
        uint4 q;
        __builtin_memcpy(&q, images + (size_t)nr * n + e, 16);
        const unsigned wd[4] = {q.x, q.y, q.z, q.w};
        float4 *dst = (float4 *)(out + base + e);
#pragma unroll
        for (int p = 0; p < 4; ++p)
            dst[p] = make_float4(fb_u8(wd[p] & 0xffu), fb_u8((wd[p] >> 8) & 0xffu), fb_u8((wd[p] >> 16) & 0xffu), fb_u8(wd[p] >> 24));
    }
}

// float32 banks: copies.  VEC: n % 4 == 0 and both bases 16-byte aligned -> float4
template <bool VEC>
__global__ void __launch_bounds__(256) HNR_FRAMES_KERNEL(frame_images_f32_kernel)(const float *__restrict__ images, size_t n, int V, int F, const int *__restrict__ hdr,
                                                                                  const int *__restrict__ nearest, float *__restrict__ out)
{
    const int row = hdr[0];
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t per = VEC ? n >> 2 : n;
    for (size_t w = gid; w < (size_t)V * per; w += stride) {
        const int v = (int)(w / per);
        const size_t k = w - (size_t)v * per;
        int nr = nearest[(size_t)row * V + v];
        if (nr < 0 || nr >= F) nr = 0;
        if (VEC) ((float4 *)(out + (size_t)v * n))[k] = ((const float4 *)(images + (size_t)nr * n))[k];
        else out[(size_t)v * n + k] = images[(size_t)nr * n + k];
    }
}

// ---- host side, shared by the two files' entry points
static inline BankView bank_view(const hnr_frame_bank *b)
{
    BankView v;
    v.images = b->d_images; v.c2w = b->d_c2w; v.w2c = b->d_w2c; v.K = b->d_intrinsic; v.weight = b->d_weight; v.angle = b->d_angle;
    v.f32 = b->images_f32; v.F = b->F; v.H = b->H; v.W = b->W; v.K_per_frame = b->intrinsic_per_frame;
    return v;
}

static inline BatchOut batch_out(const hnr_frame_batch_out *o)
{
    BatchOut r;
    r.raydir = o->d_raydir; r.pixel_idx = o->d_pixel_idx; r.gt_image = o->d_gt_image; r.campos = o->d_campos; r.camrot = o->d_camrot; r.c2w = o->d_c2w;
    r.intrinsic = o->d_intrinsic; r.c2w_nearest = o->d_c2w_nearest; r.w2c_nearest = o->d_w2c_nearest; r.campos_nearest = o->d_campos_nearest;
    r.intrinsic_nearest = o->d_intrinsic_nearest; r.images_nearest = o->d_images_nearest; r.frame_weight_nearest = o->d_frame_weight_nearest;
    r.vid_angle_nearest = o->d_vid_angle_nearest; r.frame_weight = o->d_frame_weight; r.bg_color = o->d_bg_color; r.frame_row = o->d_frame_row;
    r.patch_table = o->d_patch_table;
    return r;
}

static inline bool bank_ok(const hnr_frame_bank *b, const char *who, const char *what)
{
    if (!b || !b->d_images || !b->d_c2w || !b->d_w2c || !b->d_intrinsic || !b->d_weight || !b->d_angle) { set_error("%s: %s bank: NULL pointer", who, what); return false; }
    if (b->F <= 0 || b->H <= 0 || b->W <= 0 || (int64_t)b->H * b->W > (1ll << 26)) { set_error("%s: %s bank: F, H, W > 0 and H*W <= 2^26", who, what); return false; }
    return true;
}

}  // namespace hnr
