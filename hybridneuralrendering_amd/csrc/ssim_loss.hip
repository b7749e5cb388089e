// Patch SSIM term of the training loss, value and gradient: 1 - SSIM(win 7, sigma 1.5, data_range 1) over the ps x ps patches of a patch-sampled
// batch, for the colours the colour losses see.
//
// The reference carries the term in models/base_rendering_model.py:1120-1143 (pytorch_msssim's SSIM module, :27), parked behind a pdb.set_trace();
// that package is not part of this project, so include/hnr.h DEFINES the term (operation by operation) and tests/ssim_loss_ref.py restates it.
//
//   ssim_patch_kernel<BLOCK, CH>   one workgroup per patch: masked X, Y in LDS, the two 7-tap passes for the five filtered planes, the per-window
//                                  s and the three coefficients of its analytic gradient, the two transposed 7-tap passes, and the patch's share of
//                                  d term / d colour written (or added in place) -- every ray belongs to one patch, so no atomics.  Leaves the
//                                  patch's {sum s, hit rays} (fp64) in a scratch row.
//   ssim_finish_kernel             ONE wave: the scratch rows summed in a fixed order, out4 = {L, SSIM, fw w L, hit rays}, total[0] += fw w L.
//
// The gradient's scale fw w / (N 3 (ps-6)^2) is known before the launch (N is an argument, not a count), so nothing global sits in front of it.
//
// LDS.  All planes of a pass are [rows][ps] with the SAME row stride ps, rows of the CH channels of the pass stacked, and every pass gives lane t
// the element t (then t + BLOCK, ...): each tap of each pass reads `own index + constant` (+i along a row, +i*ps down a column), so the 32 lanes of
// an LDS group always read 32 consecutive dwords -- conflict-free in both filter directions without padding or a transposed copy.  The price is
// idle lanes where x >= ps-6 (9 % at ps = 64).  Eight planes: X, Y, five filtered planes, one more; the window coefficients wait in registers
// across one barrier and then overwrite filtered planes 0..2, the column-transposed planes go to 3..5.  ps = 64: 8 x 16 KB = 128 KB of the 160.
//
// Shapes.  ps <= 9: one wave per patch takes the three channels at once (3 x 81 <= 4 x 64 elements; 49 patches of 8 x 8 are 49 single-wave
// workgroups whose barriers cost nothing); ps <= 32: 256 lanes, a channel per pass; ps <= 64: 1024 lanes, a channel per pass (4096 elements = 4
// per lane: a single 56 x 56 or 64 x 64 patch keeps all sixteen waves busy).
#include "hnr_common.h"
#include "hnr_launch.h"

namespace hnr {

constexpr int SSIM_WIN = 7, SSIM_MIN_PS = 7, SSIM_MAX_PS = 64, SSIM_ITEMS = 4, SSIM_PLANES = 8;
constexpr float SSIM_C1 = 1e-4f, SSIM_C2 = 9e-4f;          // (0.01 * data_range)^2, (0.03 * data_range)^2

struct SsimArgs {
    const float *color, *gt;          // [R,3]
    const int8_t *ray_mask;           // [R]
    int pn, ps, n_patches, patch_major;
    float g[SSIM_WIN];
    float w_ssim, frame_weight;
    const float *d_frame_weight;      // optional: the item's scalar on the device; wins over frame_weight
    double windows, denom;            // n_patches * 3 * (ps-6)^2, norm_patches * 3 * (ps-6)^2
    float *g_color;                   // may be NULL (value only)
    int accumulate;
    double *scratch;                  // [n_patches][2]: sum s, hit rays
    float *total, *out4;
};

extern __shared__ float ssim_lds[];

template <int BLOCK, int CH>
__global__ void __launch_bounds__(BLOCK) ssim_patch_kernel(SsimArgs a)
{
    __shared__ double s_red[2][BLOCK / 64];
    const int ps = a.ps, W = ps - (SSIM_WIN - 1), P = CH * ps * ps;
    float *X = ssim_lds, *Y = X + P, *T = Y + P;                        // T: planes 0..5
    const int tid = threadIdx.x, patch = blockIdx.x;
    const int ray0 = a.patch_major ? patch * ps * ps : ((patch / a.pn) * ps) * (a.pn * ps) + (patch % a.pn) * ps;      // (n ps^2 <= 2^26: ints do)
    const int rstride = a.patch_major ? ps : a.pn * ps;
    const float fw = a.d_frame_weight ? a.d_frame_weight[0] : a.frame_weight;
    const float nsc = -hnr_div(fw * a.w_ssim, (float)a.denom);
    const float inv_ps = hnr_div(1.f, (float)ps);
    float g[SSIM_WIN];
#pragma unroll
    for (int i = 0; i < SSIM_WIN; ++i) g[i] = a.g[i];
    // element idx = (c * ps + y) * ps + x of the stacked planes; lane t owns tid, tid + BLOCK, ... (at most SSIM_ITEMS of them).  The quotients by
    // ps through a rounded reciprocal: idx + 0.5 is at least 1 / 128 away from a multiple of ps and the product is off by less than 1e-4.
    auto split = [&](int idx, int &c, int &y, int &x) {
        const int row = (int)(((float)idx + 0.5f) * inv_ps);
        x = idx - row * ps;
        c = CH == 1 ? 0 : (int)(((float)row + 0.5f) * inv_ps);
        y = row - c * ps;
    };
    unsigned on = 0;                                                    // bit j: the ray of element tid + j * BLOCK has ray_mask > 0
    double acc_s = 0.0, acc_h = 0.0;
    for (int idx = tid, j = 0; idx < P; idx += BLOCK, ++j) {
        int c, y, x;
        split(idx, c, y, x);
        if (a.ray_mask[ray0 + y * rstride + x] > 0) {
            on |= 1u << j;
            if (c == 0) acc_h += 1.0;
        }
    }

    for (int c0 = 0; c0 < 3; c0 += CH) {
        // masked planes
        for (int idx = tid, j = 0; idx < P; idx += BLOCK, ++j) {
            int c, y, x;
            split(idx, c, y, x);
            const bool m = on >> j & 1u;
            const size_t e = 3 * (size_t)(ray0 + y * rstride + x) + c0 + c;
            X[idx] = m ? a.color[e] : 0.f;
            Y[idx] = m ? a.gt[e] : 0.f;
        }
        __syncthreads();
        // along the rows: T_q(y, x) = sum_i g[i] q(y, x + i), x < W, q = X, Y, XX, YY, XY
        for (int idx = tid; idx < P; idx += BLOCK) {
            int c, y, x;
            split(idx, c, y, x);
            if (x >= W) continue;
            float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f, t4 = 0.f;
#pragma unroll
            for (int i = 0; i < SSIM_WIN; ++i) {
                const float xv = X[idx + i], yv = Y[idx + i];
                t0 = t0 + g[i] * xv; t1 = t1 + g[i] * yv; t2 = t2 + g[i] * (xv * xv); t3 = t3 + g[i] * (yv * yv); t4 = t4 + g[i] * (xv * yv);
            }
            T[idx] = t0; T[P + idx] = t1; T[2 * P + idx] = t2; T[3 * P + idx] = t3; T[4 * P + idx] = t4;
        }
        __syncthreads();
        // down the columns, then the window's s and the coefficients a = ds/dmu_x, b = ds/dG[XX], c = ds/dG[XY]: kept in registers over the
        // barrier behind which they may overwrite the filtered planes
        float ra[SSIM_ITEMS], rb[SSIM_ITEMS], rc[SSIM_ITEMS];
#pragma unroll
        for (int j = 0; j < SSIM_ITEMS; ++j) {
            const int idx = tid + j * BLOCK;
            ra[j] = rb[j] = rc[j] = 0.f;
            int c, y, x;
            split(idx, c, y, x);
            if (idx < P && x < W && y < W) {
                float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
#pragma unroll
                for (int i = 0; i < SSIM_WIN; ++i) {
                    const int o = idx + i * ps;
                    mx = mx + g[i] * T[o]; my = my + g[i] * T[P + o]; exx = exx + g[i] * T[2 * P + o]; eyy = eyy + g[i] * T[3 * P + o];
                    exy = exy + g[i] * T[4 * P + o];
                }
                const float mxx = mx * mx, myy = my * my, mxy = mx * my;
                const float sx = exx - mxx, sy = eyy - myy, sxy = exy - mxy;
                const float A1 = 2.f * mxy + SSIM_C1, B1 = (mxx + myy) + SSIM_C1, A2 = 2.f * sxy + SSIM_C2, B2 = (sx + sy) + SSIM_C2;
                const float l = hnr_div(A1, B1), cs = hnr_div(A2, B2), s = l * cs;
                ra[j] = hnr_div(2.f * (my - l * mx), B1) * cs + l * hnr_div(2.f * (mx * cs - my), B2);
                rb[j] = -hnr_div(s, B2);
                rc[j] = hnr_div(2.f * l, B2);
                acc_s += (double)s;
            }
            __builtin_amdgcn_sched_barrier(0);                          // one element at a time: four at once do not fit 128 registers
        }
        __syncthreads();
        // the coefficients as planes (0 outside the windows), then the transposed column pass: U_k(y, x) = sum_{i <= y} g[i] k(y - i, x)
#pragma unroll
        for (int j = 0; j < SSIM_ITEMS; ++j) {
            const int idx = tid + j * BLOCK;
            if (idx < P) { T[idx] = ra[j]; T[P + idx] = rb[j]; T[2 * P + idx] = rc[j]; }
        }
        __syncthreads();
        for (int idx = tid; idx < P; idx += BLOCK) {
            int c, y, x;
            split(idx, c, y, x);
            float u0 = 0.f, u1 = 0.f, u2 = 0.f;
#pragma unroll
            for (int i = 0; i < SSIM_WIN; ++i) {
                if (i > y) break;
                const int o = idx - i * ps;
                u0 = u0 + g[i] * T[o]; u1 = u1 + g[i] * T[P + o]; u2 = u2 + g[i] * T[2 * P + o];
            }
            T[3 * P + idx] = u0; T[4 * P + idx] = u1; T[5 * P + idx] = u2;
        }
        __syncthreads();
        // the transposed row pass and the ray's gradient: d(sum s)/dX = (GA + (2 X) GB) + Y GC
        if (a.g_color) {
            for (int idx = tid, j = 0; idx < P; idx += BLOCK, ++j) {
                int c, y, x;
                split(idx, c, y, x);
                float ga = 0.f, gb = 0.f, gc = 0.f;
#pragma unroll
                for (int i = 0; i < SSIM_WIN; ++i) {
                    if (i > x) break;
                    const int o = idx - i;
                    ga = ga + g[i] * T[3 * P + o]; gb = gb + g[i] * T[4 * P + o]; gc = gc + g[i] * T[5 * P + o];
                }
                const float d = (ga + (2.f * X[idx]) * gb) + Y[idx] * gc;
                const float v = (on >> j & 1u) ? nsc * d : 0.f;
                float *dst = a.g_color + 3 * (size_t)(ray0 + y * rstride + x) + c0 + c;
                *dst = a.accumulate ? *dst + v : v;
            }
        }
        if (CH < 3) __syncthreads();                                    // the next channel overwrites X, Y
    }

    for (int o = 32; o > 0; o >>= 1) { acc_s += __shfl_xor(acc_s, o); acc_h += __shfl_xor(acc_h, o); }
    if ((tid & 63) == 0) { s_red[0][tid >> 6] = acc_s; s_red[1][tid >> 6] = acc_h; }
    __syncthreads();
    if (tid < 2) {
        double t = 0.0;
        for (int w = 0; w < BLOCK / 64; ++w) t += s_red[tid][w];
        a.scratch[2 * (size_t)patch + tid] = t;
    }
}

__global__ void __launch_bounds__(64) ssim_finish_kernel(SsimArgs a)
{
    double s = 0.0, h = 0.0;
    for (int p = threadIdx.x; p < a.n_patches; p += 64) { s += a.scratch[2 * (size_t)p]; h += a.scratch[2 * (size_t)p + 1]; }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); h += __shfl_xor(h, o); }
    if (threadIdx.x != 0) return;
    const float fw = a.d_frame_weight ? a.d_frame_weight[0] : a.frame_weight;
    const float ssim = (float)hnr_div64(s, a.denom);
    const float L = h > 0.0 ? (float)hnr_div64(a.windows - s, a.denom) : 0.f;
    const float term = (fw * a.w_ssim) * L;
    a.out4[0] = L; a.out4[1] = ssim; a.out4[2] = term; a.out4[3] = (float)h;
    if (a.total && h > 0.0) a.total[0] = a.total[0] + term;
}

}  // namespace hnr

using namespace hnr;

extern "C" int64_t hnr_ssim_loss_scratch_bytes(int n_patches) { return n_patches > 0 ? (int64_t)n_patches * 2 * (int64_t)sizeof(double) : 0; }

extern "C" int hnr_ssim_loss(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int patch_num, int patch_size, int norm_patches,
                             const float *win, float w_ssim, float frame_weight, const float *d_frame_weight, float *d_total, float *d_out4,
                             float *d_g_color, int accumulate, void *d_scratch, void *stream)
{
    const char *who = "hnr_ssim_loss";
    if (patch_size < SSIM_MIN_PS || patch_size > SSIM_MAX_PS) { set_error("%s: patch_size %d outside %d..%d (the window is 7 wide)", who, patch_size, SSIM_MIN_PS, SSIM_MAX_PS); return HNR_ERR_BADARG; }
    const int64_t n = patch_num < 0 ? -(int64_t)patch_num : (int64_t)patch_num * patch_num;
    if (n <= 0 || n * patch_size * patch_size > (1ll << 26)) { set_error("%s: patch_num != 0 and at most 2^26 rays", who); return HNR_ERR_BADARG; }
    if (norm_patches < 0 || (norm_patches > 0 && norm_patches < n)) { set_error("%s: norm_patches is 0 (the call's own patches) or the batch-wide count >= %lld", who, (long long)n); return HNR_ERR_BADARG; }
    if (!(w_ssim >= 0.f) || !(w_ssim <= 3.0e38f) || !(frame_weight >= 0.f) || !(frame_weight <= 3.0e38f)) { set_error("%s: w_ssim and frame_weight must be finite and >= 0", who); return HNR_ERR_BADARG; }
    if (!win) { set_error("%s: NULL window", who); return HNR_ERR_BADARG; }
    for (int i = 0; i < SSIM_WIN; ++i)
        if (!(win[i] >= 0.f && win[i] <= 1.f)) { set_error("%s: window value %d outside [0, 1]", who, i); return HNR_ERR_BADARG; }
    if (!d_color || !d_gt || !d_ray_mask || !d_out4 || !d_scratch) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    if (accumulate && !d_g_color) { set_error("%s: accumulate needs the gradient buffer", who); return HNR_ERR_BADARG; }
    SsimArgs a;
    a.color = d_color; a.gt = d_gt; a.ray_mask = d_ray_mask;
    a.patch_major = patch_num < 0; a.pn = patch_num < 0 ? 1 : patch_num; a.ps = patch_size; a.n_patches = (int)n;
    for (int i = 0; i < SSIM_WIN; ++i) a.g[i] = win[i];
    a.w_ssim = w_ssim; a.frame_weight = frame_weight; a.d_frame_weight = d_frame_weight;
    const double per_patch = 3.0 * (double)((patch_size - 6) * (patch_size - 6));
    a.windows = (double)n * per_patch; a.denom = (double)(norm_patches > 0 ? norm_patches : n) * per_patch;
    a.g_color = d_g_color; a.accumulate = accumulate ? 1 : 0; a.scratch = (double *)d_scratch; a.total = d_total; a.out4 = d_out4;
    const hipStream_t st = (hipStream_t)stream;
    const int plane = patch_size * patch_size * (int)sizeof(float);
    if (patch_size <= 9) {
        ssim_patch_kernel<64, 3><<<(int)n, 64, SSIM_PLANES * 3 * plane, st>>>(a);
        HNR_LAUNCH_CHECK();
    } else if (patch_size <= 32) {
        ssim_patch_kernel<256, 1><<<(int)n, 256, SSIM_PLANES * plane, st>>>(a);
        HNR_LAUNCH_CHECK();
    } else {
        const int rc = launch_lds<ssim_patch_kernel<1024, 1>>(dim3((unsigned)n), dim3(1024), SSIM_PLANES * plane, st, a);
        if (rc != HNR_OK) return rc;
    }
    ssim_finish_kernel<<<1, 64, 0, st>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
