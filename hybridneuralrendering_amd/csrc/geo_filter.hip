// The geometric-consistency filter of MVS depth maps (`load_points=0`, `manual_depth_view=1`; models/mvs/filter_utils.py:157-297 of the reference,
// called from run/train_ft.py:105-114), on the device.
//
//   hnr_geo_consistency    reproject_with_depth_gpu + check_geometric_consistency_gpu + the double loop of filter_by_masks_gpu (:236-259): every depth
//                          map against every other one in ONE launch.  A workgroup owns a 32 x 8 pixel tile of one reference view (a wave: 32 x 2, so
//                          neighbouring lanes gather neighbouring source texels) and walks the source views in ascending order; count and depth sum
//                          stay in registers.  The pair transforms E_s E_r^-1 and E_r E_s^-1 are uniform per workgroup: they are formed GEO_CHUNK source
//                          views at a time by the workgroup's own lanes and read back from LDS as broadcasts, together with K_s and K_s^-1 -- no V^2 table.
//   hnr_geo_filter_select  the final mask (:262-263), xyz_cam / xyz_world (:264-265, :282), range_mask_torch (:146-154), reassign_conf (:294-297) and
//                          the per-view boolean-mask indexing as one ordered compaction over all views: flags -> inclusive scan -> scatter (the
//                          pattern of hnr_range_crop).
//
// Every fp32 operation is rounded on its own, in the order include/hnr.h gives (-ffp-contract=off, correctly rounded divide and sqrt):
// tests/geo_filter_ref.py restates them in NumPy and the GPU tests compare bits.
#include "voxel_segments.h"

namespace hnr {

constexpr int GEO_TX = 32, GEO_TY = 8;      // pixel tile of a workgroup
constexpr int GEO_CHUNK = 32;               // source views staged through LDS per round
constexpr int GEO_REC = 42;                 // floats per staged source view: pair(E_s, Einv_r) [3][4], pair(E_r, Einv_s) [3][4], K_s [9], Kinv_s [9]

__device__ __forceinline__ void geo_mat3(const float *__restrict__ M, float a0, float a1, float a2, float *o)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (M[3 * c] * a0 + M[3 * c + 1] * a1) + M[3 * c + 2] * a2;
}

// T: rows 0..2 of a 4 x 4 (or a [3][4] record), row stride 4
__device__ __forceinline__ void geo_mat34(const float *__restrict__ T, float a0, float a1, float a2, float *o)
{
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = ((T[4 * c] * a0 + T[4 * c + 1] * a1) + T[4 * c + 2] * a2) + T[4 * c + 3];
}

__device__ __forceinline__ float geo_pair(const float *__restrict__ A, const float *__restrict__ B, int i, int j)
{
    return ((A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j]) + A[4 * i + 3] * B[12 + j];
}

__global__ void __launch_bounds__(GEO_TX * GEO_TY) geo_consistency_kernel(const float *__restrict__ depth, int V, int H, int W, const float *__restrict__ K,
                                                                           const float *__restrict__ Kinv, const float *__restrict__ E,
                                                                           const float *__restrict__ Einv, int *__restrict__ out_count,
                                                                           float *__restrict__ out_avg)
{
    __shared__ float rec[GEO_CHUNK][GEO_REC];
    const int t = threadIdx.y * GEO_TX + threadIdx.x;
    const int r = blockIdx.z;
    const int x = blockIdx.x * GEO_TX + threadIdx.x, y = blockIdx.y * GEO_TY + threadIdx.y;
    const bool valid = x < W && y < H;
    const size_t plane = (size_t)H * W;
    const float *Er = E + 16 * (size_t)r, *Eir = Einv + 16 * (size_t)r, *Kr = K + 9 * (size_t)r, *Kir = Kinv + 9 * (size_t)r;
    const float fx = (float)x, fy = (float)y;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    const float d = valid ? depth[(size_t)r * plane + (size_t)y * W + x] : 0.f;
    float p[3];
    geo_mat3(Kir, fx * d, fy * d, d, p);
    int count = 0;
    float sum = 0.f;
    for (int s0 = 0; s0 < V; s0 += GEO_CHUNK) {
        const int sc = V - s0 < GEO_CHUNK ? V - s0 : GEO_CHUNK;
        __syncthreads();
        for (int e = t; e < sc * GEO_REC; e += GEO_TX * GEO_TY) {
            const int m = e / GEO_REC, q = e - m * GEO_REC;
            const size_t s = (size_t)(s0 + m);
            float v;
            if (q < 12) v = geo_pair(E + 16 * s, Eir, q >> 2, q & 3);
            else if (q < 24) v = geo_pair(Er, Einv + 16 * s, (q - 12) >> 2, (q - 12) & 3);
            else if (q < 33) v = K[9 * s + (q - 24)];
            else v = Kinv[9 * s + (q - 33)];
            rec[m][q] = v;
        }
        __syncthreads();
        for (int m = 0; m < sc; ++m) {
            const int s = s0 + m;
            if (s == r) continue;
            const float *R = rec[m];
            float q[3], k[3];
            geo_mat34(R, p[0], p[1], p[2], q);
            geo_mat3(R + 24, q[0], q[1], q[2], k);
            const float xs = hnr_div(k[0], k[2]), ys = hnr_div(k[1], k[2]);
            // border clamp; fmaxf(NaN, 0) = 0, so the texel indices are inside the map whatever xs and ys are (and are clamped once more as integers)
            const float cx = fminf(fmaxf(xs, 0.f), wmax), cy = fminf(fmaxf(ys, 0.f), hmax);
            const float x0f = floorf(cx), y0f = floorf(cy);
            const float wx1 = cx - x0f, wx0 = (x0f + 1.f) - cx, wy1 = cy - y0f, wy0 = (y0f + 1.f) - cy;
            int x0 = (int)x0f, y0 = (int)y0f;
            x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
            y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
            const int x1 = x0 + 1 > W - 1 ? W - 1 : x0 + 1, y1 = y0 + 1 > H - 1 ? H - 1 : y0 + 1;
            const float *D = depth + (size_t)s * plane;
            const float t00 = D[(size_t)y0 * W + x0], t01 = D[(size_t)y0 * W + x1], t10 = D[(size_t)y1 * W + x0], t11 = D[(size_t)y1 * W + x1];
            const float sd = (((wx0 * wy0) * t00 + (wx1 * wy0) * t01) + (wx0 * wy1) * t10) + (wx1 * wy1) * t11;
            float p2[3], q2[3], k2[3];
            geo_mat3(R + 33, xs * sd, ys * sd, sd, p2);
            geo_mat34(R + 12, p2[0], p2[1], p2[2], q2);
            geo_mat3(Kr, q2[0], q2[1], q2[2], k2);
            const float xr = hnr_div(k2[0], k2[2]), yr = hnr_div(k2[1], k2[2]);
            const float ex = xr - fx, ey = yr - fy;
            const float dist = sqrtf(ex * ex + ey * ey);
            const float rel = hnr_div(fabsf(q2[2] - d), d);
            const bool ok = dist < 1.f && rel < 0.01f;
            count += ok ? 1 : 0;
            sum += ok ? q2[2] : 0.f;
        }
    }
    if (valid) {
        const size_t o = (size_t)r * plane + (size_t)y * W + x;
        out_count[o] = count;
        out_avg[o] = hnr_div(sum + d, (float)(count + 1));
    }
}

struct GeoSelect {
    float ranges[6];
    float table[10];
    float conf_thresh;
    int geo_num, use_table, keep_all, V;
};

// keep flag, camera and world point of entry i (view v): the one definition both passes of the compaction use
__device__ __forceinline__ bool geo_select_point(const float *__restrict__ cam_xyz, const float *__restrict__ conf, const uint8_t *__restrict__ pmask,
                                                 const int *__restrict__ count, const float *__restrict__ avg, const float *__restrict__ Einv, int v, size_t i,
                                                 const GeoSelect &g, float *cam, float *w)
{
    bool keep = conf[i] > g.conf_thresh && pmask[i] != 0 && (g.V == 1 || count[i] >= g.geo_num);
    cam[0] = cam_xyz[3 * i + 0]; cam[1] = cam_xyz[3 * i + 1]; cam[2] = avg[i];
    geo_mat34(Einv + 16 * (size_t)v, cam[0], cam[1], cam[2], w);
    if (!g.keep_all) keep = keep && w[0] >= g.ranges[0] && w[1] >= g.ranges[1] && w[2] >= g.ranges[2] && w[0] <= g.ranges[3] && w[1] <= g.ranges[4] && w[2] <= g.ranges[5];
    return keep;
}

__global__ void __launch_bounds__(256) geo_select_flags_kernel(const float *__restrict__ cam_xyz, const float *__restrict__ conf, const uint8_t *__restrict__ pmask,
                                                                const int *__restrict__ count, const float *__restrict__ avg, const float *__restrict__ Einv,
                                                                int plane, GeoSelect g, int *__restrict__ flags)
{
    const int j = blockIdx.x * 256 + threadIdx.x;                // pixel of view blockIdx.y
    if (j >= plane) return;
    const int v = blockIdx.y;
    const size_t i = (size_t)v * plane + j;
    float cam[3], w[3];
    flags[i] = geo_select_point(cam_xyz, conf, pmask, count, avg, Einv, v, i, g, cam, w) ? 1 : 0;
}

__global__ void __launch_bounds__(256) geo_select_scatter_kernel(const float *__restrict__ cam_xyz, const float *__restrict__ conf, const uint8_t *__restrict__ pmask,
                                                                  const int *__restrict__ count, const float *__restrict__ avg, const float *__restrict__ Einv,
                                                                  int plane, GeoSelect g, const int *__restrict__ flags, const int *__restrict__ incl,
                                                                  float *__restrict__ out_world, float *__restrict__ out_cam, float *__restrict__ out_conf,
                                                                  int *__restrict__ out_view, long long capacity, long long *__restrict__ view_counts,
                                                                  long long *__restrict__ total, int *__restrict__ status)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= plane) return;
    const int v = blockIdx.y;
    const size_t i = (size_t)v * plane + j;
    if (j == plane - 1) {                                        // the view's last pixel: its count, and for the last view the total
        const long long upto = incl[i], before = v > 0 ? incl[i - plane] : 0;
        view_counts[v] = upto - before;
        if (v == g.V - 1) {
            total[0] = upto;
            if (upto > capacity) status[0] |= HNR_CLOUD_OVERFLOW;
        }
    }
    if (!flags[i]) return;
    const long long dst = (long long)incl[i] - 1;
    if (dst >= capacity) return;
    float cam[3], w[3];
    geo_select_point(cam_xyz, conf, pmask, count, avg, Einv, v, i, g, cam, w);
    float c = conf[i];
    if (g.use_table) {
        int k = count[i] - g.geo_num + 1;
        k = k < 1 ? 1 : (k > 10 ? 10 : k);
        c = c * g.table[k - 1];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { out_world[3 * dst + a] = w[a]; out_cam[3 * dst + a] = cam[a]; }
    out_conf[dst] = c;
    out_view[dst] = v;
}

static bool geo_shape_ok(int V, int H, int W)
{
    return V >= 1 && V <= 65535 && H >= 2 && H <= 32768 && W >= 2 && W <= 32768 && (int64_t)V * H * W <= (1ll << 30);
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_geo_consistency(const float *d_depth, int V, int H, int W, const float *d_K, const float *d_Kinv, const float *d_E, const float *d_Einv,
                                   int32_t *d_count, float *d_depth_avg, void *stream)
{
    if (!d_depth || !d_K || !d_Kinv || !d_E || !d_Einv || !d_count || !d_depth_avg) { set_error("hnr_geo_consistency: NULL argument"); return HNR_ERR_BADARG; }
    if (!geo_shape_ok(V, H, W)) {
        set_error("hnr_geo_consistency: bad argument (1 <= V <= 65535, 2 <= H, W <= 32768, V*H*W <= 2^30)"); return HNR_ERR_BADARG;
    }
    const dim3 grid(cdiv(W, GEO_TX), cdiv(H, GEO_TY), V), block(GEO_TX, GEO_TY, 1);
    geo_consistency_kernel<<<grid, block, 0, (hipStream_t)stream>>>(d_depth, V, H, W, d_K, d_Kinv, d_E, d_Einv, d_count, d_depth_avg);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int64_t hnr_geo_filter_select_scratch_bytes(int V, int H, int W)
{
    if (!geo_shape_ok(V, H, W)) return -1;
    const int64_t n = (int64_t)V * H * W;
    size_t cb = 0, seg = 0;
    if (vox_layout(n, 1, nullptr, &cb, &seg) != 0) return -1;
    return (int64_t)(2 * vox_align(4 * (size_t)n) + vox_align(cb));
}

extern "C" int hnr_geo_filter_select(const float *d_cam_xyz, const float *d_conf, const uint8_t *d_points_mask, const int32_t *d_count, const float *d_depth_avg,
                                     int V, int H, int W, const float *d_Einv, float conf_thresh, int geo_cnsst_num, const float *ranges,
                                     const float *conf_table, float *d_world, float *d_cam, float *d_conf_out, int32_t *d_view, int64_t capacity,
                                     int64_t *d_view_counts, int64_t *d_total, int32_t *d_status, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    if (!d_cam_xyz || !d_conf || !d_points_mask || !d_count || !d_depth_avg || !d_Einv || !ranges || !d_world || !d_cam || !d_conf_out || !d_view ||
        !d_view_counts || !d_total || !d_status || !d_scratch) {
        set_error("hnr_geo_filter_select: NULL argument"); return HNR_ERR_BADARG;
    }
    if (!geo_shape_ok(V, H, W) || capacity < 0 || geo_cnsst_num < 0) {
        set_error("hnr_geo_filter_select: bad argument (1 <= V <= 65535, 2 <= H, W <= 32768, V*H*W <= 2^30, capacity >= 0, geo_cnsst_num >= 0)");
        return HNR_ERR_BADARG;
    }
    const int64_t need = hnr_geo_filter_select_scratch_bytes(V, H, W);
    if (need < 0 || scratch_bytes < need) { set_error("hnr_geo_filter_select: scratch smaller than hnr_geo_filter_select_scratch_bytes(V, H, W)"); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const int plane = H * W, n = V * plane;
    char *p = (char *)d_scratch;
    int *flags = (int *)p; p += vox_align(4 * (size_t)n);
    int *incl = (int *)p; p += vox_align(4 * (size_t)n);
    const size_t cb = (size_t)need - 2 * vox_align(4 * (size_t)n);
    GeoSelect g;
    memcpy(g.ranges, ranges, sizeof(g.ranges));
    memset(g.table, 0, sizeof(g.table));
    if (conf_table) memcpy(g.table, conf_table, sizeof(g.table));
    g.conf_thresh = conf_thresh; g.geo_num = geo_cnsst_num; g.use_table = conf_table ? 1 : 0; g.keep_all = ranges[0] <= -99.f ? 1 : 0; g.V = V;
    const dim3 grid(cdiv(plane, 256), V, 1);
    geo_select_flags_kernel<<<grid, 256, 0, st>>>(d_cam_xyz, d_conf, d_points_mask, d_count, d_depth_avg, d_Einv, plane, g, flags);
    HNR_LAUNCH_CHECK();
    if (int rc = vox_scan_flags(flags, incl, n, p, cb, st)) return rc;
    geo_select_scatter_kernel<<<grid, 256, 0, st>>>(d_cam_xyz, d_conf, d_points_mask, d_count, d_depth_avg, d_Einv, plane, g, flags, incl, d_world, d_cam,
                                                    d_conf_out, d_view, (long long)capacity, (long long *)d_view_counts, (long long *)d_total, d_status);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
