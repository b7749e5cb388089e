// The per-step data path on the device: a frame bank (all training frames resident, 8-bit or float32) and the ray batch drawn from it.
//
// Replaces the reference's dataset item, data/scannet_ft_dataset.py:736-976 (nerf_synth360_ft_dataset.py:643-800): image decode aside, per step it
// draws pixel coordinates with numpy (:892-949), builds raydir with get_dtu_raydir (data_utils.py:57-71), gathers gt_image (:957) and uploads the
// V reference frames as float32 (:821-855).  Here:
//
//   frame_header_kernel   one workgroup: reads the step counter and the schedule, writes the frame row, the camera / reference-view / weight outputs,
//                         the patch table and bg_color, and advances the counter once
//   frame_rays_kernel     one lane per ray: pixel, direction, ground truth
//   frame_images_kernel   the V reference images as float32 -- the only one that moves real bytes: 16 bytes of uint8 per lane per load, four float4
//                         stores, grid-stride; frames need not start on a 16-byte boundary (head / tail elements per view)
//
// Every fp32 operation is rounded on its own in the order written (-ffp-contract=off, correctly rounded divide and sqrt) and the random words are
// Philox4x32-10: tests/frames_ref.py restates all of it in NumPy and the GPU tests compare bits.  Nothing is allocated, nothing is read back; three
// launches on the caller's stream.
#include "hnr_common.h"
#include "hnr_launch.h"

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

// schedule != NULL: row = schedule[step % n_schedule], the counter advances; schedule == NULL: the explicit row, the counter is not touched
__global__ void __launch_bounds__(64) frame_header_kernel(BankView tb, BankView rb, const int *__restrict__ nearest, const int *__restrict__ schedule,
                                                          int n_schedule, int explicit_row, unsigned long long *__restrict__ d_step, BatchArgs a, BatchOut o,
                                                          int *__restrict__ hdr)
{
    __shared__ int s_row;
    __shared__ unsigned s_step[2];
    const int t = threadIdx.x;
    if (t == 0) {
        unsigned long long step = 0ull;
        int row = explicit_row;
        if (schedule) {
            step = d_step[0];
            row = schedule[(int)(step % (unsigned long long)n_schedule)];
            d_step[0] = step + 1ull;
        }
        if (row < 0 || row >= tb.F) row = 0;             // (the host validates schedules and rows: never taken through frames.py)
        s_row = row; s_step[0] = (unsigned)step; s_step[1] = (unsigned)(step >> 32);
        hdr[0] = row; hdr[1] = (int)s_step[0]; hdr[2] = (int)s_step[1]; hdr[3] = 0;
        if (o.frame_row) o.frame_row[0] = row;
        if (o.frame_weight) o.frame_weight[0] = tb.weight[row];
    }
    __syncthreads();
    const int row = s_row;
    const float *M = tb.c2w + 16 * (size_t)row;
    if (t < 16 && o.c2w) o.c2w[t] = M[t];
    if (t < 9) {
        if (o.camrot) o.camrot[t] = M[4 * (t / 3) + t % 3];
        if (o.intrinsic) o.intrinsic[t] = tb.K[(tb.K_per_frame ? 9 * (size_t)row : 0) + t];
    }
    if (t < 3) {
        if (o.campos) o.campos[t] = M[4 * t + 3];
        if (o.bg_color) {
            float v = a.bg[t];
            if (a.bg_random) v = philox4x32_10(s_step[0], s_step[1], PURPOSE_BG, 0u, a.seed_lo, a.seed_hi).w[0] >= 0x80000000u ? 1.f : 0.f;
            o.bg_color[t] = v;
        }
    }
    for (int e = t; e < a.V * 16; e += 64) {
        const int v = e >> 4, q = e & 15;
        int nr = nearest[(size_t)row * a.V + v];
        if (nr < 0 || nr >= rb.F) nr = 0;
        if (o.c2w_nearest) o.c2w_nearest[e] = rb.c2w[16 * (size_t)nr + q];
        if (o.w2c_nearest) o.w2c_nearest[e] = rb.w2c[16 * (size_t)nr + q];
        if (q < 3 && o.campos_nearest) o.campos_nearest[3 * v + q] = rb.c2w[16 * (size_t)nr + 4 * q + 3];
        if (q == 0) {
            if (o.frame_weight_nearest) o.frame_weight_nearest[v] = a.downweight ? rb.weight[nr] : 1.f;
            if (o.vid_angle_nearest) o.vid_angle_nearest[v] = rb.angle[nr];
        }
        if (v == 0 && q < 9 && o.intrinsic_nearest) o.intrinsic_nearest[q] = rb.K[(rb.K_per_frame ? 9 * (size_t)nr : 0) + q];
    }
    if (a.mode == FB_PATCH || a.mode == FB_DILATED) {
        for (int p = t; p < a.pn * a.pn; p += 64) {
            const Philox r = philox4x32_10(s_step[0], s_step[1], PURPOSE_PATCH, (unsigned)p, a.seed_lo, a.seed_hi);
            const int d = fb_randint(r.w[0], a.dlo, a.dhi + 1);
            const int x0 = fb_randint(r.w[1], a.margin, tb.W - a.margin - (a.ps - 1) * d);
            const int y0 = fb_randint(r.w[2], a.margin, tb.H - a.margin - (a.ps - 1) * d);
            int *dst = hdr + HDR_WORDS + 3 * p;
            dst[0] = d; dst[1] = x0; dst[2] = y0;
            if (o.patch_table) { o.patch_table[3 * p] = d; o.patch_table[3 * p + 1] = x0; o.patch_table[3 * p + 2] = y0; }
        }
    }
}

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

__global__ void __launch_bounds__(256) frame_rays_kernel(BankView tb, const int *__restrict__ hdr, const float *__restrict__ pixels, BatchArgs a, BatchOut o)
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

// uint8 -> float32 of the V reference frames.  Per view of n = H*W*3 elements: `head` elements bring the DESTINATION onto a float4 boundary, then
// groups of 16 (one 16-byte load, which may be unaligned: frames of a bank whose n is no multiple of 16 start anywhere; four aligned float4 stores),
// then a tail of n - head - 16 groups < 16 elements.  Head and tail elements are converted one per lane by the first lanes of the grid.
__global__ void __launch_bounds__(256) frame_images_u8_kernel(const uint8_t *__restrict__ images, size_t n, int V, int F, const int *__restrict__ hdr,
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
__global__ void __launch_bounds__(256) frame_images_f32_kernel(const float *__restrict__ images, size_t n, int V, int F, const int *__restrict__ hdr,
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

static BankView bank_view(const hnr_frame_bank *b)
{
    BankView v;
    v.images = b->d_images; v.c2w = b->d_c2w; v.w2c = b->d_w2c; v.K = b->d_intrinsic; v.weight = b->d_weight; v.angle = b->d_angle;
    v.f32 = b->images_f32; v.F = b->F; v.H = b->H; v.W = b->W; v.K_per_frame = b->intrinsic_per_frame;
    return v;
}

static BatchOut batch_out(const hnr_frame_batch_out *o)
{
    BatchOut r;
    r.raydir = o->d_raydir; r.pixel_idx = o->d_pixel_idx; r.gt_image = o->d_gt_image; r.campos = o->d_campos; r.camrot = o->d_camrot; r.c2w = o->d_c2w;
    r.intrinsic = o->d_intrinsic; r.c2w_nearest = o->d_c2w_nearest; r.w2c_nearest = o->d_w2c_nearest; r.campos_nearest = o->d_campos_nearest;
    r.intrinsic_nearest = o->d_intrinsic_nearest; r.images_nearest = o->d_images_nearest; r.frame_weight_nearest = o->d_frame_weight_nearest;
    r.vid_angle_nearest = o->d_vid_angle_nearest; r.frame_weight = o->d_frame_weight; r.bg_color = o->d_bg_color; r.frame_row = o->d_frame_row;
    r.patch_table = o->d_patch_table;
    return r;
}

static bool bank_ok(const hnr_frame_bank *b, const char *who, const char *what)
{
    if (!b || !b->d_images || !b->d_c2w || !b->d_w2c || !b->d_intrinsic || !b->d_weight || !b->d_angle) { set_error("%s: %s bank: NULL pointer", who, what); return false; }
    if (b->F <= 0 || b->H <= 0 || b->W <= 0 || (int64_t)b->H * b->W > (1ll << 26)) { set_error("%s: %s bank: F, H, W > 0 and H*W <= 2^26", who, what); return false; }
    return true;
}

// the three launches; schedule == NULL: explicit row
static int frame_launch(const char *who, const hnr_frame_bank *target, const hnr_frame_bank *ref, const int32_t *d_nearest, const int32_t *d_schedule,
                        int n_schedule, int row, uint64_t *d_step, const float *d_pixels, BatchArgs a, const hnr_frame_batch_out *out, void *d_scratch,
                        int64_t scratch_bytes, void *stream)
{
    if (!bank_ok(target, who, "target")) return HNR_ERR_BADARG;
    if (!out || !d_scratch) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    const bool views = a.V > 0;
    if (a.V < 0 || a.V > 64 || (views && (!d_nearest || !bank_ok(ref, who, "reference") || ref->H != target->H || ref->W != target->W))) {
        set_error("%s: 0 <= V <= 64; with V > 0 a nearest table and a reference bank of the target's frame size", who); return HNR_ERR_BADARG;
    }
    if (!views && (out->d_c2w_nearest || out->d_w2c_nearest || out->d_campos_nearest || out->d_intrinsic_nearest || out->d_images_nearest ||
                   out->d_frame_weight_nearest || out->d_vid_angle_nearest)) {
        set_error("%s: reference-view outputs need V > 0", who); return HNR_ERR_BADARG;
    }
    if (a.R <= 0 || a.R > (1 << 26) || a.margin < 0) { set_error("%s: 1 <= rays <= 2^26, margin >= 0", who); return HNR_ERR_BADARG; }
    if (scratch_bytes < (int64_t)sizeof(int) * (HDR_WORDS + 3 * (int64_t)a.pn * a.pn)) { set_error("%s: scratch smaller than hnr_frame_batch_scratch_bytes", who); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    int *hdr = (int *)d_scratch;
    const BankView tb = bank_view(target), rb = views ? bank_view(ref) : tb;
    const BatchOut o = batch_out(out);
    frame_header_kernel<<<1, 64, 0, st>>>(tb, rb, d_nearest, d_schedule, n_schedule, row, (unsigned long long *)d_step, a, o, hdr);
    HNR_LAUNCH_CHECK();
    if (o.raydir || o.pixel_idx || o.gt_image) {
        frame_rays_kernel<<<cdiv(a.R, 256), 256, 0, st>>>(tb, hdr, d_pixels, a, o);
        HNR_LAUNCH_CHECK();
    }
    if (o.images_nearest) {
        const size_t n = (size_t)rb.H * rb.W * 3;
        if (rb.f32) {
            const bool vec = (n & 3) == 0 && (((uintptr_t)rb.images | (uintptr_t)o.images_nearest) & 15) == 0;
            const int grid = (int)fb_min((size_t)device_num_cus() * 8, (size_t)cdiv((int64_t)a.V * (int64_t)(vec ? n >> 2 : n), 256));
            if (vec) frame_images_f32_kernel<true><<<grid, 256, 0, st>>>((const float *)rb.images, n, a.V, rb.F, hdr, d_nearest, o.images_nearest);
            else frame_images_f32_kernel<false><<<grid, 256, 0, st>>>((const float *)rb.images, n, a.V, rb.F, hdr, d_nearest, o.images_nearest);
        } else {
            if ((uintptr_t)o.images_nearest & 15) { set_error("%s: d_images_nearest must be 16-byte aligned", who); return HNR_ERR_BADARG; }
            const size_t work = (size_t)a.V * ((n >> 4) > 32 ? (n >> 4) : 32);
            const int grid = (int)fb_min((size_t)device_num_cus() * 8, (size_t)cdiv((int64_t)work, 256));
            frame_images_u8_kernel<<<grid, 256, 0, st>>>((const uint8_t *)rb.images, n, a.V, rb.F, hdr, d_nearest, o.images_nearest);
        }
        HNR_LAUNCH_CHECK();
    }
    return HNR_OK;
}

}  // namespace hnr

using namespace hnr;

extern "C" int64_t hnr_frame_batch_scratch_bytes(int mode, int patch_num)
{
    if (mode < FB_RANDOM || mode > FB_DILATED || patch_num < 0 || patch_num > 1024) return -1;
    const int64_t pn = mode == FB_RANDOM ? 0 : (mode == FB_PATCH ? 1 : patch_num);
    return (int64_t)sizeof(int) * (HDR_WORDS + 3 * pn * pn);
}

extern "C" int hnr_frame_batch(const hnr_frame_bank *target, const hnr_frame_bank *reference, const int32_t *d_nearest, int V,
                               const hnr_frame_batch_params *p, const int32_t *d_schedule, int n_schedule, uint64_t *d_step, const hnr_frame_batch_out *out,
                               void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "hnr_frame_batch";
    if (!p || !d_schedule || !d_step || n_schedule <= 0) { set_error("%s: NULL argument or an empty schedule", who); return HNR_ERR_BADARG; }
    if (!bank_ok(target, who, "target")) return HNR_ERR_BADARG;
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    a.mode = p->mode; a.margin = p->margin; a.dir_norm = p->dir_norm ? 1 : 0; a.bg_random = p->bg_random ? 1 : 0; a.downweight = p->downweight_blurry_feats ? 1 : 0;
    a.V = V; a.seed_lo = (unsigned)p->seed; a.seed_hi = (unsigned)(p->seed >> 32);
    memcpy(a.bg, p->bg_color, sizeof(a.bg));
    const int H = target->H, W = target->W, m = p->margin;
    if (m < 0) { set_error("%s: margin >= 0", who); return HNR_ERR_BADARG; }
    if (p->mode == FB_RANDOM) {
        a.S = p->size; a.pn = 0; a.ps = 1; a.dlo = a.dhi = 1;
        if (p->size <= 0 || p->size > 8192 || W - 2 * m <= 0 || H - 2 * m <= 0) {
            set_error("%s: random: 1 <= size <= 8192 and a margin that leaves pixels (W - 2 margin, H - 2 margin > 0)", who); return HNR_ERR_BADARG;
        }
    } else if (p->mode == FB_PATCH || p->mode == FB_DILATED) {
        if (p->mode == FB_PATCH) { a.pn = 1; a.ps = p->size; a.dlo = a.dhi = 1; }
        else { a.pn = p->patch_num; a.ps = p->patch_size; a.dlo = p->dilation_lo; a.dhi = p->dilation_hi; }
        if (a.pn <= 0 || a.pn > 1024 || a.ps <= 0 || a.ps > 8192 || (int64_t)a.pn * a.ps > 8192 || a.dlo < 1 || a.dhi < a.dlo || a.dhi > (1 << 16)) {
            set_error("%s: patch / dilated: patch_num, patch_size >= 1, patch_num * patch_size <= 8192, 1 <= dilation_lo <= dilation_hi", who); return HNR_ERR_BADARG;
        }
        const int64_t reach = (int64_t)(a.ps - 1) * a.dhi;
        if ((int64_t)W - m - reach <= m || (int64_t)H - m - reach <= m) {
            set_error("%s: a %d-pixel patch at dilation %d does not fit a %dx%d frame with margin %d (an empty range)", who, a.ps, a.dhi, H, W, m); return HNR_ERR_BADARG;
        }
        a.S = a.pn * a.ps;
    } else {
        set_error("%s: mode must be 0 (random), 1 (patch) or 2 (dilated)", who); return HNR_ERR_BADARG;
    }
    a.R = a.S * a.S;
    return frame_launch(who, target, reference, d_nearest, d_schedule, n_schedule, 0, d_step, nullptr, a, out, d_scratch, scratch_bytes, stream);
}

extern "C" int hnr_frame_item(const hnr_frame_bank *target, const hnr_frame_bank *reference, const int32_t *d_nearest, int V, int row, const float *d_pixels,
                              int64_t n_rays, int margin, int dir_norm, const float *bg_color, int downweight_blurry_feats, const hnr_frame_batch_out *out,
                              void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "hnr_frame_item";
    if (!bank_ok(target, who, "target")) return HNR_ERR_BADARG;
    if (!bg_color || row < 0 || row >= target->F || margin < 0) { set_error("%s: 0 <= row < F, margin >= 0, bg_color [3]", who); return HNR_ERR_BADARG; }
    BatchArgs a;
    memset(&a, 0, sizeof(a));
    a.margin = margin; a.dir_norm = dir_norm ? 1 : 0; a.downweight = downweight_blurry_feats ? 1 : 0; a.V = V; a.ps = 1;
    memcpy(a.bg, bg_color, sizeof(a.bg));
    if (d_pixels) {
        a.mode = FB_PIXELS;
        if (n_rays <= 0 || n_rays > (1 << 26)) { set_error("%s: 1 <= n_rays <= 2^26", who); return HNR_ERR_BADARG; }
        a.R = (int)n_rays;
    } else {
        a.mode = FB_NO_CROP;
        const int64_t wn = (int64_t)target->W - 2 * margin, hn = (int64_t)target->H - 2 * margin;
        if (wn <= 0 || hn <= 0) { set_error("%s: the margin leaves no pixel", who); return HNR_ERR_BADARG; }
        if (n_rays != wn * hn) { set_error("%s: without d_pixels n_rays must be (W - 2 margin) * (H - 2 margin)", who); return HNR_ERR_BADARG; }
        a.R = (int)n_rays;
    }
    return frame_launch(who, target, reference, d_nearest, nullptr, 0, row, nullptr, d_pixels, a, out, d_scratch, scratch_bytes, stream);
}
