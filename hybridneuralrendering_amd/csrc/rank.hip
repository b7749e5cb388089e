// The growth schedule's per-step bookkeeping on the device: the step's ray-miss loss and the table of the worst frames, one launch.
//
// Replaces, per optimisation step, the `ray_miss` colour item of BaseRenderingModel.compute_losses (models/base_rendering_model.py:1147-1159: two
// torch.masked_select copies of the batch, l2loss * 3, behind an `if masked_output.shape[1] > 0`) and MvsPointsVolumetricModel.rank_ray_miss /
// update_rank_ray_miss (models/mvs_points_volumetric_model.py:154-172: `if torch.sum(mask) > 0`, a Python max() on device scalars, torch.sort) --
// two host synchronisations per step.  Here:
//
//   ray_miss_rank_kernel   ONE workgroup of 256 lanes: the squared error of the rays with ray_mask == 0 (fp64 sums in a fixed order), the loss
//                          L = sum / 3, then the table update in LDS -- the slot that holds the frame takes max(L, old), otherwise the last slot is
//                          overwritten -- and a stable descending sort by counting (rank = entries greater + equal entries in an earlier slot).
//
// The frame number is read from device memory (the batch sampler's frame_row), nothing is allocated, nothing is read back: the launch follows a
// captured training step inside the same hipGraph.  Every fp32 difference and square is rounded on its own (-ffp-contract=off);
// tests/growth_ref.py restates the arithmetic in NumPy.
#include "hnr_common.h"

namespace hnr {

constexpr int RANK_THREADS = 256, RANK_MAX_N = 1024;

__global__ void __launch_bounds__(RANK_THREADS) ray_miss_rank_kernel(const float *__restrict__ color, const float *__restrict__ gt,
                                                                     const int8_t *__restrict__ ray_mask, int R, const int *__restrict__ frame_id,
                                                                     int *__restrict__ ids, float *__restrict__ losses, int n, float *__restrict__ miss_out)
{
    __shared__ double s_se[RANK_THREADS / 64], s_nm[RANK_THREADS / 64];
    __shared__ float s_loss[RANK_MAX_N], s_L;
    __shared__ int s_id[RANK_MAX_N], s_found, s_ok;
    const int t = threadIdx.x;
    // ---- the loss: lane t takes rays t, t + 256, ...; a butterfly within the wave; the waves in order
    double se = 0.0, nm = 0.0;
    for (int r = t; r < R; r += RANK_THREADS) {
        if (ray_mask[r] == 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { const float d = color[3 * (size_t)r + c] - gt[3 * (size_t)r + c]; se += (double)(d * d); }
            nm += 1.0;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { se += __shfl_xor(se, o); nm += __shfl_xor(nm, o); }
    if ((t & 63) == 0) { s_se[t >> 6] = se; s_nm[t >> 6] = nm; }
    if (t == 0) s_found = 0;
    __syncthreads();
    if (t == 0) {
        const double sum = ((s_se[0] + s_se[1]) + s_se[2]) + s_se[3], cnt = ((s_nm[0] + s_nm[1]) + s_nm[2]) + s_nm[3];
        const float L = cnt > 0.0 ? (float)hnr_div64(sum, 3.0) : 0.f;
        if (miss_out) { miss_out[0] = L; miss_out[1] = (float)cnt; }
        s_L = L;
        s_ok = (__float_as_uint(L) & 0x7f800000u) != 0x7f800000u;                    // finite: a NaN / inf loss leaves the table as it was
    }
    __syncthreads();
    if (!s_ok) return;
    const float L = s_L;
    if (n == 1) {                                                                     // prob_num_step == 1 (:158-159): the running maximum, no frame ids
        if (t == 0) { const float old = losses[0]; losses[0] = old > L ? old : L; }
        return;
    }
    // ---- the table (:162-172), in LDS
    const int fid = frame_id[0];
    for (int i = t; i < n; i += RANK_THREADS) {
        const int id = ids[i];
        float l = losses[i];
        if (id == fid) { l = l > L ? l : L; s_found = 1; }                            // python's max(new, old): old when old > new
        s_id[i] = id; s_loss[i] = l;
    }
    __syncthreads();
    if (t == 0 && !s_found) { s_id[n - 1] = fid; s_loss[n - 1] = L; }
    __syncthreads();
    // ---- descending, stable: the new slot of entry i = entries with a greater loss + equal ones in an earlier slot (always < n)
    for (int i = t; i < n; i += RANK_THREADS) {
        const float l = s_loss[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float m = s_loss[j];
            rank += (m > l || (m == l && j < i)) ? 1 : 0;
        }
        ids[rank] = s_id[i];
        losses[rank] = l;
    }
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_ray_miss_rank(const float *d_color, const float *d_gt, const int8_t *d_ray_mask, int R, const int32_t *d_frame_id, int32_t *d_ids,
                                 float *d_losses, int n, float *d_miss_out, void *stream)
{
    if (n < 1 || n > RANK_MAX_N) { set_error("hnr_ray_miss_rank: 1 <= n <= %d, got %d", RANK_MAX_N, n); return HNR_ERR_BADARG; }
    if (R < 0 || R > (1 << 24)) { set_error("hnr_ray_miss_rank: 0 <= R <= 2^24, got %d", R); return HNR_ERR_BADARG; }
    if (!d_color || !d_gt || !d_ray_mask || !d_frame_id || !d_losses || (!d_ids && n > 1)) {
        set_error("hnr_ray_miss_rank: NULL argument (only d_miss_out, and d_ids with n == 1, may be NULL)"); return HNR_ERR_BADARG;
    }
    ray_miss_rank_kernel<<<1, RANK_THREADS, 0, (hipStream_t)stream>>>(d_color, d_gt, d_ray_mask, R, d_frame_id, d_ids, d_losses, n, d_miss_out);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
