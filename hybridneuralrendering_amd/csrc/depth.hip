// Expected depth of a ray: the compute_depth branch of NeuralPointsRayMarching.forward (models/neural_points_volumetric_model.py:381-385),
//   D = sum_s w_s z_s / (sum_s w_s + 1e-6),
// with w = the composite's blend weight (opacity x transmittance before the sample, :382-383) and z = the shading sample's camera-space depth,
// sample_loc[..., 2] of w2pers -- the quantity ray_dist is built from (:331).  The reference names it `ray_ts` without defining it.
// Its gradient is a term of the composite's backward (csrc/backward.hip, hnr_composite_bwd_depth).
#include "hnr_common.h"

namespace hnr {

struct DepthArgs {
    const float *blend_w;                                // [R,SR] (0 for invalid / padded slots)
    const float *loc_w;                                  // [R,SR,3]; slots >= nsamp[r] are not read
    const int32_t *nsamp;                                // [R] or NULL (padded inputs)
    const int8_t *ray_mask;                              // [R]
    const float *campos, *camrot;                        // [3], [3,3] c2w
    int R, SR, seg_log2;
    float *depth;                                        // [R]
};

// SEG = 2^seg_log2 lanes per ray (the power of two >= SR, at most 64: 64 / SEG rays per wave, a ray's samples are contiguous in memory).  Lane j
// adds the samples j, j + SEG, ... in order; the two sums are then added over the segment with an xor butterfly.  A fixed order: the same bits
// run to run.  Every lane of the wave takes part in the butterfly (no early return).
__global__ __launch_bounds__(256) void ray_depth_kernel(DepthArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int seg = 1 << a.seg_log2;
    const int j = (int)(t & (seg - 1));
    const bool live = (t >> a.seg_log2) < a.R;
    const int r = live ? (int)(t >> a.seg_log2) : 0;
    const bool hit = live && a.ray_mask[r] != 0;
    float A = 0.f, W = 0.f;
    if (hit) {
        const int n = a.nsamp ? a.nsamp[r] : a.SR;
        const int ns = n < a.SR ? n : a.SR;
        const float cp0 = a.campos[0], cp1 = a.campos[1], cp2 = a.campos[2];
        const float cr2 = a.camrot[2], cr5 = a.camrot[5], cr8 = a.camrot[8];
        for (int s = j; s < ns; s += seg) {
            const size_t i = (size_t)r * a.SR + s;
            const float w = a.blend_w[i];
            const float *p = a.loc_w + i * 3;
            // the composite's z (aggregate.hip composite_kernel): same operations, same order
            const float s0 = __fsub_rn(p[0], cp0), s1 = __fsub_rn(p[1], cp1), s2 = __fsub_rn(p[2], cp2);
            const float z = __fadd_rn(__fadd_rn(__fmul_rn(cr2, s0), __fmul_rn(cr5, s1)), __fmul_rn(cr8, s2));
            A += w * z;
            W += w;
        }
    }
    for (int o = seg >> 1; o > 0; o >>= 1) {
        A += __shfl_xor(A, o);
        W += __shfl_xor(W, o);
    }
    if (live && j == 0) a.depth[r] = hit ? hnr_div(A, W + 1e-6f) : 0.f;
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_ray_depth(const float *d_blend_weight, const float *d_sample_loc_w, const int32_t *d_ray_nsamp, const int8_t *d_ray_mask,
                             const float *d_campos, const float *d_camrot, int R, int SR, float *d_depth, void *stream)
{
    if (R < 0 || SR <= 0) { set_error("hnr_ray_depth: bad sizes"); return HNR_ERR_BADARG; }
    if (R == 0) return HNR_OK;
    if (!d_blend_weight || !d_sample_loc_w || !d_ray_mask || !d_campos || !d_camrot || !d_depth) {
        set_error("hnr_ray_depth: NULL argument"); return HNR_ERR_BADARG;
    }
    int lg = 0;
    while ((1 << lg) < SR && lg < 6) ++lg;
    DepthArgs a;
    a.blend_w = d_blend_weight; a.loc_w = d_sample_loc_w; a.nsamp = d_ray_nsamp; a.ray_mask = d_ray_mask; a.campos = d_campos; a.camrot = d_camrot;
    a.R = R; a.SR = SR; a.seg_log2 = lg; a.depth = d_depth;
    ray_depth_kernel<<<cdiv((int64_t)R << lg, 256), 256, 0, (hipStream_t)stream>>>(a);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
