// Evaluation of a rendered frame on the device: the numbers the reference's test pass reports per frame.
//
// Replaces, behind driver.render_image's composite,
//   * the two test losses of run/test_ft.py:233-243 (nn.MSELoss over the whole [h,w,3] image / over the rays with ray_mask > 0; mse2psnr is
//     formed from them on the host),
//   * the 8-bit quantisation of utils/visualizer.py:23-24 (`(np.clip(img, 0, 1) * 255).astype(np.uint8)`, the bytes of the two PNGs) and
//   * run/evaluate.py:34-97 on those bytes: compare_psnr, sqrt(mean_squared_error) and structural_similarity(win_size, multichannel=True)
// -- about ten host round trips, a PNG encode and a PNG decode per frame there; here two small launches on the caller's stream and one fp64
// row of results in a device table.
//
// Arithmetic (include/hnr.h states the contract): the quantised difference and the five window sums of SSIM are integers and are formed exactly;
// the per-window formula, the partial sums and the means are fp64 (-ffp-contract=off: no fused multiply-add).  Reductions are deterministic:
// every thread adds in a fixed order, waves by shuffles, blocks write partials, and one thread per quantity adds them in block order -- no float
// atomics, two runs give the same bits.
//
// A block owns FM_TW x FM_TH window origins of all three channels: it quantises the (FM_TW + win - 1) x (FM_TH + win - 1) pixels under them on
// load (both images, one packed word per value: A | B << 8), forms the horizontal window sums of one channel at a time into a second LDS
// array, then the vertical sums and the formula.  Every pixel is also "owned" by exactly one block (the one whose origin range holds it; the
// last block of a row / column also owns the win - 1 pixels beyond its origins) for the squared errors and the optional uint8 images.
#include "hnr_common.h"

namespace hnr {

constexpr int FM_TW = 32, FM_TH = 16;       // window origins per block
constexpr int FM_MAX_WIN = 31;              // LDS: 62 x 46 x 3 words + 46 x 32 x 4 words = 57.8 KB of the 64 KB a block gets without an attribute
constexpr int FM_NPART = 7;                 // partial row: S, squared error fp32 (full), SSIM sum per channel x 3, squared error (masked), masked rays

struct FrameMetricsArgs {
    const float *image, *gt;                // [h,w,3]
    const float *raycolor, *gt_rays;        // [R,3]
    const int8_t *ray_mask;                 // [R]
    int h, w, R, win;
    int nwx, nwy;                           // window origins per row / column = w - win + 1, h - win + 1
    double dn1, dn2;                        // 255 NP, 65025 NP: a window sum over these = a window mean of x = A / 255 (of x^2, xy)
    double cov_norm;                        // NP / (NP - 1)
    double C1, C2;
    double *partial;                        // [blocks][FM_NPART]
    double *row;                            // [HNR_FM_NCOLS]
    uint8_t *img8, *gt8;                    // optional [h,w,3]
};

// (np.clip(x, 0, 1) * 255).astype(np.uint8) on float32: clamp, ONE fp32 product, truncation.  (A NaN clamps to 0: numpy leaves that cast undefined.)
__device__ __forceinline__ int fm_quantise(float x)
{
    return (int)__fmul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.0f);
}

__device__ __forceinline__ double fm_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void frame_metrics_tile_kernel(FrameMetricsArgs a)
{
    extern __shared__ uint32_t fm_lds[];
    __shared__ double s_red[FM_NPART][4];
    const int win = a.win, hw_ = FM_TW + win - 1, hh_ = FM_TH + win - 1;       // halo tile, pixels
    uint32_t *tile = fm_lds;                                                    // [hh_][hw_][3]: A | B << 8
    uint4 *hsum = reinterpret_cast<uint4 *>(fm_lds + ((hh_ * hw_ * 3 + 3) & ~3));   // [hh_][FM_TW]: {sum A | sum B << 16, sum AA, sum BB, sum AB}
    const int tx0 = blockIdx.x * FM_TW, ty0 = blockIdx.y * FM_TH;
    const bool last_x = tx0 + FM_TW >= a.nwx, last_y = ty0 + FM_TH >= a.nwy;
    const int tid = threadIdx.x;

    // ---- load + quantise; squared errors of the pixels this block owns -------------------------------------------------------------
    double sq8 = 0.0, sqf = 0.0;
    const int row_vals = hw_ * 3;
    for (int i = tid; i < hh_ * row_vals; i += 256) {
        const int r = i / row_vals, c3 = i - r * row_vals;
        const int y = ty0 + r, x3 = tx0 * 3 + c3;
        uint32_t packed = 0u;
        if (y < a.h && x3 < a.w * 3) {
            const int g = (y * a.w) * 3 + x3;                                   // (3hw fits an int: checked by the host)
            const float fa = a.image[g], fb = a.gt[g];
            const int qa = fm_quantise(fa), qb = fm_quantise(fb);
            packed = (uint32_t)qa | ((uint32_t)qb << 8);
            const bool owned = (last_x || c3 < FM_TW * 3) && (last_y || r < FM_TH);
            if (owned) {
                const int d8 = hnr_opaque(qa - qb);
                sq8 += (double)(d8 * d8);                                       // <= 65025: exact; the sum stays an exact integer far below 2^53
                const float df = fa - fb;
                sqf += (double)(df * df);                                       // the square in fp32, as torch forms it
                if (a.img8) { a.img8[g] = (uint8_t)qa; a.gt8[g] = (uint8_t)qb; }
            }
        }
        tile[i] = packed;
    }
    __syncthreads();

    // ---- SSIM: separable integer window sums, one channel at a time ---------------------------------------------------------------------
    double ssim[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        for (int i = tid; i < hh_ * FM_TW; i += 256) {
            const int r = i / FM_TW, ox = i - r * FM_TW;
            const uint32_t *p = tile + (r * hw_ + ox) * 3 + c;
            uint32_t sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
            for (int k = 0; k < win; ++k) {
                const uint32_t v = p[3 * k];
                const uint32_t qa = hnr_opaque((int)(v & 0xffu)), qb = hnr_opaque((int)(v >> 8));
                sa += qa; sb += qb; saa += qa * qa; sbb += qb * qb; sab += qa * qb;
            }
            hsum[i] = make_uint4(sa | (sb << 16), saa, sbb, sab);              // sa, sb <= 31 * 255 < 2^16
        }
        __syncthreads();
        for (int i = tid; i < FM_TH * FM_TW; i += 256) {
            const int oy = i / FM_TW, ox = i - oy * FM_TW;
            if (ty0 + oy < a.nwy && tx0 + ox < a.nwx) {
                uint32_t sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;             // <= 961 * 65025 < 2^26
                for (int k = 0; k < win; ++k) {
                    const uint4 v = hsum[(oy + k) * FM_TW + ox];
                    sa += v.x & 0xffffu; sb += v.x >> 16; saa += v.y; sbb += v.z; sab += v.w;
                }
                // structural_similarity's steps on x = A / 255, y = B / 255 (skimage/metrics/_structural_similarity.py): window means, sample covariances
                const double ux = hnr_div64((double)sa, a.dn1), uy = hnr_div64((double)sb, a.dn1);
                const double uxx = hnr_div64((double)saa, a.dn2), uyy = hnr_div64((double)sbb, a.dn2), uxy = hnr_div64((double)sab, a.dn2);
                const double vx = a.cov_norm * (uxx - ux * ux), vy = a.cov_norm * (uyy - uy * uy), vxy = a.cov_norm * (uxy - ux * uy);
                const double A1 = 2.0 * ux * uy + a.C1, A2 = 2.0 * vxy + a.C2;
                const double B1 = ux * ux + uy * uy + a.C1, B2 = vx + vy + a.C2;
                ssim[c] += hnr_div64(A1 * A2, B1 * B2);
            }
        }
        __syncthreads();
    }

    // ---- the masked test loss: the rays, dealt over the whole grid --------------------------------------------------------------------------
    double sqm = 0.0, nm = 0.0;
    {
        const int nthreads = gridDim.x * gridDim.y * 256, t0 = (blockIdx.y * gridDim.x + blockIdx.x) * 256 + tid;
        for (int r = t0; r < a.R; r += nthreads) {
            if (a.ray_mask[r] > 0) {
                for (int c = 0; c < 3; ++c) { const float d = a.raycolor[3 * r + c] - a.gt_rays[3 * r + c]; sqm += (double)(d * d); }
                nm += 1.0;
            }
        }
    }

    // ---- block partial --------------------------------------------------------------------------------------------------------------------
    const double vals[FM_NPART] = {sq8, sqf, ssim[0], ssim[1], ssim[2], sqm, nm};
    const int wave = tid >> 6;
#pragma unroll
    for (int q = 0; q < FM_NPART; ++q) {
        const double v = fm_wave_sum(vals[q]);
        if ((tid & 63) == 0) s_red[q][wave] = v;
    }
    __syncthreads();
    if (tid < FM_NPART)
        a.partial[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * FM_NPART + tid] = (s_red[tid][0] + s_red[tid][1]) + (s_red[tid][2] + s_red[tid][3]);
}

constexpr int FM_FIN_CHUNK = 512;           // block partials staged per pass of the finish kernel (28 KB of LDS)

// One thread per quantity adds the blocks' partials in block order (the same bits every run).  The partials are staged through LDS by the whole
// block first: a single thread walking them in global memory pays one memory latency per block (81 us for the bench frame's 580 blocks, measured).
__global__ __launch_bounds__(256) void frame_metrics_finish_kernel(FrameMetricsArgs a, int n_blocks)
{
    __shared__ double s[FM_NPART];
    __shared__ double stage[FM_FIN_CHUNK * FM_NPART];
    double v = 0.0;
    for (int b0 = 0; b0 < n_blocks; b0 += FM_FIN_CHUNK) {
        const int nb = n_blocks - b0 < FM_FIN_CHUNK ? n_blocks - b0 : FM_FIN_CHUNK;
        for (int i = threadIdx.x; i < nb * FM_NPART; i += 256) stage[i] = a.partial[(size_t)b0 * FM_NPART + i];
        __syncthreads();
        if (threadIdx.x < FM_NPART) {
#pragma unroll 8                            // (eight LDS reads in flight; the adds keep their order)
            for (int b = 0; b < nb; ++b) v += stage[b * FM_NPART + threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x < FM_NPART) s[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = 3.0 * (double)a.h * (double)a.w, nwin = (double)a.nwx * (double)a.nwy;
        a.row[HNR_FM_SQERR8] = s[0];
        a.row[HNR_FM_N8] = n;
        a.row[HNR_FM_SSIM] = hnr_div64((hnr_div64(s[2], nwin) + hnr_div64(s[3], nwin)) + hnr_div64(s[4], nwin), 3.0);
        a.row[HNR_FM_MSE_FULL] = hnr_div64(s[1], n);
        a.row[HNR_FM_MSE_MASKED] = s[6] > 0.0 ? hnr_div64(s[5], 3.0 * s[6]) : __longlong_as_double(0x7ff8000000000000LL);   // nn.MSELoss of an empty selection
        a.row[HNR_FM_N_MASKED] = s[6];
    }
}

}  // namespace hnr

using namespace hnr;

static bool fm_check_shape(int h, int w, int win, const char *who)
{
    if (h <= 0 || w <= 0) { set_error("%s: empty image (h=%d, w=%d)", who, h, w); return false; }
    if (win < 3 || !(win & 1) || win > FM_MAX_WIN || win > (h < w ? h : w)) {
        set_error("%s: win=%d must be odd, 3 <= win <= min(h, w, %d)", who, win, FM_MAX_WIN); return false;
    }
    return true;
}

extern "C" int64_t hnr_frame_metrics_scratch_bytes(int h, int w, int win)
{
    if (!fm_check_shape(h, w, win, "hnr_frame_metrics_scratch_bytes")) return HNR_ERR_BADARG;
    return (int64_t)cdiv(w - win + 1, FM_TW) * cdiv(h - win + 1, FM_TH) * FM_NPART * (int64_t)sizeof(double);
}

extern "C" int hnr_frame_metrics(const float *d_image, const float *d_gt_full, int h, int w, const float *d_raycolor, const float *d_gt_rays,
                                 const int8_t *d_ray_mask, int R, int win, float data_range, double *d_row, uint8_t *d_img8, uint8_t *d_gt8,
                                 void *d_scratch, void *stream)
{
    if (!fm_check_shape(h, w, win, "hnr_frame_metrics")) return HNR_ERR_BADARG;
    if (!(data_range > 0.f) || !(data_range <= 65536.f)) { set_error("hnr_frame_metrics: data_range=%g must be positive (2: as the reference computes it, 1: the textbook value)", (double)data_range); return HNR_ERR_BADARG; }
    if (R < 0) { set_error("hnr_frame_metrics: R=%d", R); return HNR_ERR_BADARG; }
    if (!d_image || !d_gt_full || !d_row || !d_scratch || (R > 0 && (!d_raycolor || !d_gt_rays || !d_ray_mask)) || (!d_img8 != !d_gt8)) {
        set_error("hnr_frame_metrics: NULL argument (the two uint8 images go together)"); return HNR_ERR_BADARG;
    }
    if ((int64_t)h * w * 3 > (int64_t)INT32_MAX) { set_error("hnr_frame_metrics: %d x %d x 3 values overflow 32-bit indices", h, w); return HNR_ERR_TOOBIG; }
    FrameMetricsArgs a;
    a.image = d_image; a.gt = d_gt_full; a.raycolor = d_raycolor; a.gt_rays = d_gt_rays; a.ray_mask = d_ray_mask;
    a.h = h; a.w = w; a.R = R; a.win = win; a.nwx = w - win + 1; a.nwy = h - win + 1;
    const double NP = (double)(win * win), L = (double)data_range;
    a.dn1 = 255.0 * NP; a.dn2 = 65025.0 * NP; a.cov_norm = NP / (NP - 1.0);
    a.C1 = (0.01 * L) * (0.01 * L); a.C2 = (0.03 * L) * (0.03 * L);
    a.partial = (double *)d_scratch; a.row = d_row; a.img8 = d_img8; a.gt8 = d_gt8;
    const dim3 grid(cdiv(a.nwx, FM_TW), cdiv(a.nwy, FM_TH));
    const int hw_ = FM_TW + win - 1, hh_ = FM_TH + win - 1;
    const size_t lds = (size_t)((hh_ * hw_ * 3 + 3) & ~3) * 4 + (size_t)hh_ * FM_TW * 16;
    frame_metrics_tile_kernel<<<grid, 256, lds, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    frame_metrics_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(a, (int)(grid.x * grid.y));
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
