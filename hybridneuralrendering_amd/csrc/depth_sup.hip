// Depth supervision from resident sensor depth: the per-ray ground-truth depth of a batch, the depth term of the training loss with its gradient,
// and the depth error of a rendered test frame.
//
// The reference has a `depth_loss_items` branch (models/base_rendering_model.py:1209-1215) but neither of its datasets emits gt_depth, so there is
// no behaviour to match: include/hnr.h defines it and tests/depth_sup_ref.py restates it in NumPy.
//
//   depth_rays_kernel     one lane per ray: the depth frame's texel under the ray's pixel, raw -> metres, range-checked (0 = no measurement)
//   depth_loss_kernel     ONE workgroup: masked mean of (D - d)^2 over the rays with a hit and a measurement, its gradient, total += w L
//   depth_metrics_kernel  ONE workgroup: {n, sum |e|, sum e^2, sum |e| / d, #(delta < 1.25)} in fp64
//
// A training batch is a few thousand rays and a test frame a few hundred thousand: one workgroup of 1024 lanes strides over them, so a launch holds
// the whole reduction and needs no scratch.  Sums have a fixed order (per lane in ray order, xor butterfly over the wave, the sixteen waves in
// order); no atomics.  Every fp32 operation is rounded on its own in the order written (-ffp-contract=off, hnr_div correctly rounded).
#include "hnr_common.h"
#include "hnr_launch.h"

namespace hnr {

constexpr int DS_BLOCK = 1024, DS_WAVES = DS_BLOCK / 64;

struct DepthBankView {
    const void *depth;
    const float *Kd;
    int f32, F, Hd, Wd;
    float div, dmin, dmax;
};

__global__ void __launch_bounds__(256) depth_rays_kernel(DepthBankView b, const int *__restrict__ frame_row, const float *__restrict__ pixel_idx,
                                                         const float *__restrict__ K, int R, float *__restrict__ gt_depth)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    int row = frame_row[0];
    if (row < 0 || row >= b.F) row = 0;
    const float px = pixel_idx[2 * (size_t)i], py = pixel_idx[2 * (size_t)i + 1];
    int u = -1, v = -1;
    if (b.Kd) {
        const float x = hnr_div((px + 0.5f) - K[2], K[0]), y = hnr_div((py + 0.5f) - K[5], K[4]);
        const float fu = floorf((x * b.Kd[0] + b.Kd[2]) + 0.5f), fv = floorf((y * b.Kd[4] + b.Kd[5]) + 0.5f);
        if (fu >= 0.f && fu < (float)b.Wd) u = (int)fu;                                             // (NaN compares false: outside)
        if (fv >= 0.f && fv < (float)b.Hd) v = (int)fv;
    } else {
        if (px > -1.f && px < (float)b.Wd) u = (int)px;                                             // the texel gt_image reads: (int) truncates toward zero
        if (py > -1.f && py < (float)b.Hd) v = (int)py;
    }
    float d = 0.f;
    if (u >= 0 && v >= 0) {
        const size_t e = ((size_t)row * b.Hd + v) * b.Wd + u;
        d = b.f32 ? ((const float *)b.depth)[e] : hnr_div((float)((const uint16_t *)b.depth)[e], b.div);
        if (!(d >= b.dmin && d <= b.dmax)) d = 0.f;                                                 // (a NaN of a float bank reads as no measurement too)
    }
    gt_depth[i] = d;
}

// sum over the workgroup in a fixed order; every lane returns the total
template <int N>
__device__ __forceinline__ void ds_block_sum(double (&acc)[N], double (*s)[DS_WAVES])
{
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) s[k][wave] = acc[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = 0.0;
        for (int w = 0; w < DS_WAVES; ++w) t += s[k][w];
        acc[k] = t;
    }
}

__global__ void __launch_bounds__(DS_BLOCK) depth_loss_kernel(const float *__restrict__ depth, const float *__restrict__ gt, const int8_t *__restrict__ mask,
                                                              int R, float w_depth, float *__restrict__ total, float *__restrict__ out3,
                                                              float *__restrict__ g_depth)
{
    __shared__ double s[2][DS_WAVES];
    double acc[2] = {0.0, 0.0};                                     // squared error (fp32 squares, fp64 sum), rays counted
    for (int r = threadIdx.x; r < R; r += DS_BLOCK) {
        if (mask[r] > 0 && gt[r] > 0.f) {
            const float e = depth[r] - gt[r];
            acc[0] += (double)(e * e);
            acc[1] += 1.0;
        }
    }
    ds_block_sum(acc, s);
    const double n = acc[1];
    const float L = n > 0.0 ? (float)hnr_div64(acc[0], n) : 0.f;
    if (threadIdx.x == 0) {
        const float wl = w_depth * L;
        out3[0] = L; out3[1] = (float)n; out3[2] = wl;
        if (total && n > 0.0) total[0] = total[0] + wl;
    }
    if (!g_depth) return;
    const float sc = n > 0.0 ? hnr_div(2.f * w_depth, (float)n) : 0.f;
    for (int r = threadIdx.x; r < R; r += DS_BLOCK) {
        const bool on = n > 0.0 && mask[r] > 0 && gt[r] > 0.f;
        g_depth[r] = on ? (depth[r] - gt[r]) * sc : 0.f;
    }
}

__global__ void __launch_bounds__(DS_BLOCK) depth_metrics_kernel(const float *__restrict__ depth, const float *__restrict__ gt, const int8_t *__restrict__ mask,
                                                                 int R, double *__restrict__ row)
{
    __shared__ double s[5][DS_WAVES];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < R; r += DS_BLOCK) {
        if (mask[r] > 0 && gt[r] > 0.f) {
            const double D = (double)depth[r], d = (double)gt[r], e = fabs(D - d);
            acc[0] += 1.0;
            acc[1] += e;
            acc[2] += e * e;
            acc[3] += hnr_div64(e, d);
            // max(D / d, d / D) < 1.25 without a quotient: both products are exact in fp64 (24-bit values times 5/4)
            if (D > 0.0 && D < 1.25 * d && d < 1.25 * D) acc[4] += 1.0;
        }
    }
    ds_block_sum(acc, s);
    if (threadIdx.x < 5) row[threadIdx.x] = acc[threadIdx.x];
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_frame_depth_rays(const hnr_depth_bank *bank, const int32_t *d_frame_row, const float *d_pixel_idx, const float *d_intrinsic, int R,
                                    float *d_gt_depth, void *stream)
{
    const char *who = "hnr_frame_depth_rays";
    if (!bank || !bank->d_depth || !d_frame_row || !d_pixel_idx || !d_gt_depth) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    if (bank->d_depth_intrinsic && !d_intrinsic) { set_error("%s: a depth intrinsic needs the item's colour intrinsic (d_intrinsic)", who); return HNR_ERR_BADARG; }
    if (bank->F <= 0 || bank->Hd <= 0 || bank->Wd <= 0 || (int64_t)bank->Hd * bank->Wd > (1ll << 26)) {
        set_error("%s: F, Hd, Wd > 0 and Hd*Wd <= 2^26", who); return HNR_ERR_BADARG;
    }
    if (!(bank->depth_div > 0.f) || !(bank->depth_min <= bank->depth_max)) { set_error("%s: depth_div > 0, depth_min <= depth_max", who); return HNR_ERR_BADARG; }
    if (R <= 0 || R > (1 << 26)) { set_error("%s: 1 <= R <= 2^26", who); return HNR_ERR_BADARG; }
    DepthBankView b;
    b.depth = bank->d_depth; b.Kd = bank->d_depth_intrinsic; b.f32 = bank->depth_f32; b.F = bank->F; b.Hd = bank->Hd; b.Wd = bank->Wd;
    b.div = bank->depth_div; b.dmin = bank->depth_min; b.dmax = bank->depth_max;
    depth_rays_kernel<<<cdiv(R, 256), 256, 0, (hipStream_t)stream>>>(b, d_frame_row, d_pixel_idx, d_intrinsic, R, d_gt_depth);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_depth_loss(const float *d_depth, const float *d_gt_depth, const int8_t *d_ray_mask, int R, float w_depth, float *d_total, float *d_out3,
                              float *d_g_depth, void *d_scratch, void *stream)
{
    (void)d_scratch;
    const char *who = "hnr_depth_loss";
    if (!d_depth || !d_gt_depth || !d_ray_mask || !d_out3) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    if (R <= 0 || R > (1 << 26)) { set_error("%s: 1 <= R <= 2^26", who); return HNR_ERR_BADARG; }
    if (!(w_depth >= 0.f) || !(w_depth <= 3.0e38f)) { set_error("%s: w_depth must be finite and >= 0", who); return HNR_ERR_BADARG; }
    depth_loss_kernel<<<1, DS_BLOCK, 0, (hipStream_t)stream>>>(d_depth, d_gt_depth, d_ray_mask, R, w_depth, d_total, d_out3, d_g_depth);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_depth_metrics(const float *d_depth, const float *d_gt_depth, const int8_t *d_ray_mask, int R, double *d_row, void *stream)
{
    const char *who = "hnr_depth_metrics";
    if (!d_depth || !d_gt_depth || !d_ray_mask || !d_row) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    if (R <= 0 || R > (1 << 26)) { set_error("%s: 1 <= R <= 2^26", who); return HNR_ERR_BADARG; }
    depth_metrics_kernel<<<1, DS_BLOCK, 0, (hipStream_t)stream>>>(d_depth, d_gt_depth, d_ray_mask, R, d_row);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
