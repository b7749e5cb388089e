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
// launches on the caller's stream.  frame_rays_kernel and the image kernels are in frames_dev.h (path.hip draws the items of free cameras with them).
#include "frames_dev.h"

namespace hnr {

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
