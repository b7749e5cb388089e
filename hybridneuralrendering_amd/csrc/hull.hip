// The two stages of the NeRF-synthetic start of a scene (`load_points=0`, `depth_occ=1`, a dataset with `alphas`) that the ScanNet start does not have,
// on the device.
//
//   hnr_alpha_pack          the silhouettes as ONE BIT per pixel, alpha > 0.1f: all the masking kernel needs of an alpha map (100 views of 800 x 800:
//                           8 MB of bits for 256 MB of floats).  One lane per pixel, a wave's 64 verdicts are one ballot, two words stored.
//   hnr_visual_hull_select  mvs_utils.alpha_masking (models/mvs/mvs_utils.py:573-607) + `masking` (run/train_ft.py:152-158) in one pass over the points:
//                           one lane per point, the views in ascending order, left at the first failing view (the reference multiplies the per-view masks:
//                           the order is free).  The camera table is read at a wave-uniform index (scalar loads); per view a lane does 21 multiply-adds, two
//                           divides and one bit gather.  Then the ordered compaction of hnr_geo_filter_select: flags -> inclusive scan -> scatter.
//   hnr_point_occlusion     the z-buffer test of mvs_utils.homo_warp_nongrid_occ (:333-369) for the points of one view: the per-cell minimum of cam z
//                           by a 32-bit integer atomicMin on an order-preserving key of the float (a minimum does not depend on arrival order: two runs,
//                           or any permutation of the points, give the same flags), then visible = in frame && z <= zmin + tolerate.  The projection is
//                           view_project of view_attrs.h: the frame mask is hnr_point_view_attrs' bit for bit.
//
// Every fp32 operation is rounded on its own, in the order include/hnr.h gives (-ffp-contract=off, correctly rounded divide): tests/hull_ref.py restates
// them in NumPy and the GPU tests compare bits.  No float atomics.
#include "voxel_segments.h"
#include "view_attrs.h"

namespace hnr {

constexpr int HULL_CAM = 21;                // floats per view of the camera table: rows 0..2 of w2c [3][4], K [3][3]

// one lane per pixel of row blockIdx.x (of M*H rows), columns blockIdx.y * 256 ..; bit x of a row is bit (x & 31) of word x >> 5, padding bits are 0
__global__ void __launch_bounds__(256) alpha_pack_kernel(const float *__restrict__ alpha, int W, int Wp, unsigned int *__restrict__ bits)
{
    const size_t row = blockIdx.x;
    const int x = blockIdx.y * 256 + threadIdx.x;
    const bool on = x < W && alpha[row * W + x] > 0.1f;
    const unsigned long long b = __ballot(on);
    const int lane = threadIdx.x & 63, word = x >> 5;
    if ((lane == 0 || lane == 32) && word < Wp) bits[row * Wp + word] = (unsigned int)(lane == 0 ? b : b >> 32);
}

struct HullParams {
    int M, H, W, Wp, use_nf, use_range;
    float near_m1, far;
};

// floor'd pixel coordinate -> index inside the frame: the clamp is done in float, before the conversion, so a large finite quotient cannot overflow;
// a quotient that is not finite reads pixel 0
__device__ __forceinline__ int hull_clamp(float f, int top)
{
    if (!(fabsf(f) < INFINITY)) return 0;
    return (int)fminf(fmaxf(f, 0.f), (float)top);
}

__global__ void __launch_bounds__(256) hull_flags_kernel(const float *__restrict__ xyz, int n, const unsigned int *__restrict__ bits,
                                                         const float *__restrict__ cams, HullParams g, int *__restrict__ flags, uint8_t *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    const size_t plane = (size_t)g.H * g.Wp;
    bool keep = true;
    for (int m = 0; m < g.M; ++m) {
        const float *w = cams + (size_t)m * HULL_CAM, *K = w + 12;             // the same address in every lane
        float c[3], p[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] = ((x * w[4 * q] + y * w[4 * q + 1]) + z * w[4 * q + 2]) + w[4 * q + 3];
#pragma unroll
        for (int q = 0; q < 3; ++q) p[q] = (c[0] * K[3 * q] + c[1] * K[3 * q + 1]) + c[2] * K[3 * q + 2];
        const float uf = floorf(hnr_div(p[0], p[2])), vf = floorf(hnr_div(p[1], p[2]));
        bool pass = true;
        if (g.use_nf) pass = c[2] >= g.near_m1 && c[2] <= g.far;
        const bool inside = uf >= 0.f && uf < (float)g.W && vf >= 0.f && vf < (float)g.H;
        if (pass && !(g.use_range && !inside)) {                                // outside the frame with the range mask on: alpha + 1 > 0.1, no read
            const int u = hull_clamp(uf, g.W - 1), v = hull_clamp(vf, g.H - 1);
            pass = (bits[(size_t)m * plane + (size_t)v * g.Wp + (u >> 5)] >> (u & 31)) & 1u;
        }
        if (!pass) { keep = false; break; }
    }
    flags[i] = keep ? 1 : 0;
    if (mask) mask[i] = keep ? 1 : 0;
}

__global__ void __launch_bounds__(256) hull_scatter_kernel(const float *__restrict__ xyz, const float *__restrict__ conf, const int *__restrict__ view, int n,
                                                           const int *__restrict__ flags, const int *__restrict__ incl, float *__restrict__ out_xyz,
                                                           float *__restrict__ out_conf, int *__restrict__ out_view, long long capacity,
                                                           long long *__restrict__ count, int *__restrict__ status)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i == n - 1) {                                                           // the NEEDED count, also past capacity
        count[0] = (long long)incl[i];
        if ((long long)incl[i] > capacity) status[0] |= HNR_CLOUD_OVERFLOW;
    }
    if (!flags[i]) return;
    const long long dst = (long long)incl[i] - 1;
    if (dst >= capacity) return;
    if (out_xyz) { out_xyz[3 * dst + 0] = xyz[3 * (size_t)i + 0]; out_xyz[3 * dst + 1] = xyz[3 * (size_t)i + 1]; out_xyz[3 * dst + 2] = xyz[3 * (size_t)i + 2]; }
    if (out_conf) out_conf[dst] = conf[i];
    if (out_view) out_view[dst] = view[i];
}

// float -> unsigned key with the same order (negative depths are legal: the reference has no z > 0 test); 0xffffffff (a NaN's key) clears the buffer
__device__ __forceinline__ unsigned int occ_key(float f)
{
    const unsigned int b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float occ_unkey(unsigned int k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the reference's column-major cell: ceil(gx) * H + ceil(gy); inside the frame 0 <= ceil(gx) <= W-1 and 0 <= ceil(gy) <= H-1, so the cell is below H*W
__device__ __forceinline__ int occ_cell(float gx, float gy, int H) { return (int)ceilf(gx) * H + (int)ceilf(gy); }

__global__ void __launch_bounds__(256) occ_min_kernel(const float *__restrict__ xyz, long long n, ViewCam vc, int H, int W, unsigned int *__restrict__ zbuf)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[3], gx, gy;
    if (!view_project(vc, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], H, W, c, gx, gy)) return;
    atomicMin(zbuf + occ_cell(gx, gy, H), occ_key(c[2]));
}

__global__ void __launch_bounds__(256) occ_test_kernel(const float *__restrict__ xyz, long long n, ViewCam vc, int H, int W, float tolerate,
                                                       const unsigned int *__restrict__ zbuf, uint8_t *__restrict__ visible)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[3], gx, gy;
    bool vis = view_project(vc, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], H, W, c, gx, gy);
    if (vis) vis = c[2] <= occ_unkey(zbuf[occ_cell(gx, gy, H)]) + tolerate;
    visible[i] = vis ? 1 : 0;
}

static bool hull_shape_ok(int M, int H, int W) { return M >= 1 && M <= 65535 && H >= 1 && H <= 32768 && W >= 1 && W <= 32768 && (int64_t)M * H <= INT32_MAX; }

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_alpha_pack(const float *d_alphas, int M, int H, int W, uint32_t *d_bits, void *stream)
{
    if (!d_alphas || !d_bits) { set_error("hnr_alpha_pack: NULL argument"); return HNR_ERR_BADARG; }
    if (!hull_shape_ok(M, H, W)) { set_error("hnr_alpha_pack: bad argument (1 <= M <= 65535, 1 <= H, W <= 32768, M*H < 2^31)"); return HNR_ERR_BADARG; }
    const dim3 grid(M * H, cdiv(W, 256), 1);
    alpha_pack_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d_alphas, W, (W + 31) / 32, d_bits);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int64_t hnr_visual_hull_select_scratch_bytes(int64_t n)
{
    if (n <= 0 || n > (1ll << 30)) return -1;
    size_t cb = 0, seg = 0;
    if (vox_layout(n, 1, nullptr, &cb, &seg) != 0) return -1;
    return (int64_t)(2 * vox_align(4 * (size_t)n) + vox_align(cb));
}

extern "C" int hnr_visual_hull_select(const float *d_xyz, const float *d_conf, const int32_t *d_view, int64_t n, const uint32_t *d_alpha_bits, const float *d_cams,
                                      int M, int H, int W, const float *near_far, int range_mask, uint8_t *d_mask, float *d_out_xyz, float *d_out_conf,
                                      int32_t *d_out_view, int64_t capacity, int64_t *d_count, int32_t *d_status, void *d_scratch, int64_t scratch_bytes,
                                      void *stream)
{
    if (!d_xyz || !d_alpha_bits || !d_cams || !d_count || !d_status || !d_scratch || (d_out_conf && !d_conf) || (d_out_view && !d_view)) {
        set_error("hnr_visual_hull_select: NULL argument (d_out_conf needs d_conf, d_out_view needs d_view)"); return HNR_ERR_BADARG;
    }
    if (!hull_shape_ok(M, H, W) || capacity < 0) {
        set_error("hnr_visual_hull_select: bad argument (1 <= M <= 65535, 1 <= H, W <= 32768, M*H < 2^31, capacity >= 0)"); return HNR_ERR_BADARG;
    }
    if (near_far && !(near_far[0] <= near_far[1])) { set_error("hnr_visual_hull_select: near_far must be (near - 1, far) with near - 1 <= far"); return HNR_ERR_BADARG; }
    const int64_t need = hnr_visual_hull_select_scratch_bytes(n);
    if (need < 0 || scratch_bytes < need) {
        set_error("hnr_visual_hull_select: 1 <= n <= 2^30 and scratch >= hnr_visual_hull_select_scratch_bytes(n)"); return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n;
    char *p = (char *)d_scratch;
    int *flags = (int *)p; p += vox_align(4 * (size_t)ni);
    int *incl = (int *)p; p += vox_align(4 * (size_t)ni);
    const size_t cb = (size_t)need - 2 * vox_align(4 * (size_t)ni);
    HullParams g;
    g.M = M; g.H = H; g.W = W; g.Wp = (W + 31) / 32; g.use_nf = near_far ? 1 : 0; g.use_range = range_mask ? 1 : 0;
    g.near_m1 = near_far ? near_far[0] : 0.f; g.far = near_far ? near_far[1] : 0.f;
    hull_flags_kernel<<<cdiv(ni, 256), 256, 0, st>>>(d_xyz, ni, d_alpha_bits, d_cams, g, flags, d_mask);
    HNR_LAUNCH_CHECK();
    if (int rc = vox_scan_flags(flags, incl, ni, p, cb, st)) return rc;
    hull_scatter_kernel<<<cdiv(ni, 256), 256, 0, st>>>(d_xyz, d_conf, d_view, ni, flags, incl, d_out_xyz, d_out_conf, d_out_view, (long long)capacity,
                                                       (long long *)d_count, d_status);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

// the reference forms the cell index in fp32 (exact below 2^24), so the frame is limited to H*W <= 2^24 cells
extern "C" int64_t hnr_point_occlusion_scratch_bytes(int H, int W)
{
    if (H < 2 || W < 2 || H > 32768 || W > 32768 || (int64_t)H * W > (1ll << 24)) return -1;
    return (int64_t)vox_align(4 * (size_t)H * W);
}

extern "C" int hnr_point_occlusion(const float *d_xyz, int64_t n, const float *w2c, const float *K, int H, int W, float tolerate, uint8_t *d_visible,
                                   void *d_scratch, int64_t scratch_bytes, void *stream)
{
    if (!d_xyz || !w2c || !K || !d_visible || !d_scratch) { set_error("hnr_point_occlusion: NULL argument"); return HNR_ERR_BADARG; }
    const int64_t need = hnr_point_occlusion_scratch_bytes(H, W);
    if (n <= 0 || n > (1ll << 31) * 255 || need < 0 || scratch_bytes < need || !(tolerate >= 0.f)) {
        set_error("hnr_point_occlusion: bad argument (n > 0, 2 <= H, W <= 32768, H*W <= 2^24, tolerate >= 0, scratch >= hnr_point_occlusion_scratch_bytes(H, W))");
        return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    ViewCam vc;
    memset(&vc, 0, sizeof(vc));
    memcpy(vc.Wm, w2c, sizeof(vc.Wm));
    memcpy(vc.K, K, sizeof(vc.K));
    HNR_HIP_CHECK(hipMemsetAsync(d_scratch, 0xff, 4 * (size_t)H * W, st));
    occ_min_kernel<<<cdiv(n, 256), 256, 0, st>>>(d_xyz, (long long)n, vc, H, W, (unsigned int *)d_scratch);
    HNR_LAUNCH_CHECK();
    occ_test_kernel<<<cdiv(n, 256), 256, 0, st>>>(d_xyz, (long long)n, vc, H, W, tolerate, (const unsigned int *)d_scratch, d_visible);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
