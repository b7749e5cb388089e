// The initial neural point cloud from posed depth frames (`load_points=2`, run/train_ft.py:687-770 of the reference), on the device.
//
//   hnr_depth_fuse_frame  data/scannet_ft_dataset.py:616-642 -- back-projection of one depth frame + construct_vox_points_xyz (mvs_utils.py:503-517):
//                         per-voxel centroids on the frame's own bounds, appended at a device-side count.  No host read per frame (the reference does
//                         two: the boolean-mask index and torch.unique).
//   hnr_range_crop        train_ft.py:713-716 -- order-preserving compaction by opt.ranges, counts on the device.
//   hnr_nearest_view      train_ft.py:48-57   -- the best training camera of every point in one launch (the reference: N/10000 rounds of torch ops).
//   hnr_point_view_attrs  mvs_utils.py:299-315 (homo_warp_nongrid), :411-420 (extract_from_2d_grid), mvs_points_model.py:239-251 (the `dir` branch,
//                         pointdir_w=True) -- projection into the chosen view, bilinear samples of an image / feature map, viewing direction.
//
// Every fp32 operation below is rounded on its own, in the order written (-ffp-contract=off, correctly rounded divide and sqrt): tests/cloud_init_ref.py
// restates them in NumPy and the GPU tests compare bits.  The fusion's voxel stage is the machinery of voxelize.hip (voxel_segments.h): keys -> stable
// radix sort -> head flags -> scan -> per-voxel walk; the frame's bounds and the derived cell size stay on the device.
#include "voxel_segments.h"
#include "view_attrs.h"

namespace hnr {

constexpr int NV_CHUNK = 64;        // cameras staged through LDS per round of nearest_view_kernel

struct FuseCam {
    float Ki[9];                    // inverse depth intrinsic, row-major
    float M[16];                    // c2w, row-major
    float div, dmin, dmax;
};

// one pixel per thread, row-major: world point + kept flag; per-block bounds of the kept points (min/max are exact in any order)
template <bool U16>
__global__ void __launch_bounds__(256) fuse_backproject_kernel(const void *__restrict__ depth, int n, int W, FuseCam cam, float *__restrict__ pts,
                                                                int *__restrict__ kept, float *__restrict__ part)
{
    __shared__ float red[6][256];
    const int t = threadIdx.x;
    const int i = blockIdx.x * 256 + t;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
        const int py = i / W, px = i - py * W;
        float d;
        if (U16) d = hnr_div((float)((const uint16_t *)depth)[i], cam.div);
        else d = ((const float *)depth)[i];
        if (d > cam.dmax || d < cam.dmin) d = 0.f;
        const float v0 = (float)px * d, v1 = (float)py * d, v2 = d;
        float c[3], w[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) c[q] = (v0 * cam.Ki[3 * q] + v1 * cam.Ki[3 * q + 1]) + v2 * cam.Ki[3 * q + 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) w[q] = ((c[0] * cam.M[4 * q] + c[1] * cam.M[4 * q + 1]) + c[2] * cam.M[4 * q + 2]) + cam.M[4 * q + 3];
        const bool keep = c[2] > 0.f;
        pts[3 * (size_t)i + 0] = w[0]; pts[3 * (size_t)i + 1] = w[1]; pts[3 * (size_t)i + 2] = w[2];
        kept[i] = keep ? 1 : 0;
        if (keep) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { lo[q] = w[q]; hi[q] = w[q]; }
        }
    }
    if (!part) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) { red[q][t] = lo[q]; red[3 + q][t] = hi[q]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                red[q][t] = fminf(red[q][t], red[q][t + s]);
                red[3 + q][t] = fmaxf(red[3 + q][t], red[3 + q][t + s]);
            }
        }
        __syncthreads();
    }
    if (t < 6) part[6 * (size_t)blockIdx.x + t] = red[t][0];
}

// one block: bounds of the frame -> space_min [3], vox_size: the fp32 formulas of mvs_utils.py:507-513 (voxel.space_of)
__global__ void __launch_bounds__(256) fuse_space_kernel(const float *__restrict__ part, int nblk, float vox_res, float *__restrict__ params)
{
    __shared__ float red[6][256];
    const int t = threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = t; b < nblk; b += 256) {
#pragma unroll
        for (int q = 0; q < 3; ++q) { lo[q] = fminf(lo[q], part[6 * (size_t)b + q]); hi[q] = fmaxf(hi[q], part[6 * (size_t)b + 3 + q]); }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { red[q][t] = lo[q]; red[3 + q][t] = hi[q]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                red[q][t] = fminf(red[q][t], red[q][t + s]);
                red[3 + q][t] = fmaxf(red[3 + q][t], red[3 + q][t + s]);
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        const float ex = red[3][0] - red[0][0], ey = red[4][0] - red[1][0], ez = red[5][0] - red[2][0];
        const float edge = fmaxf(fmaxf(ex, ey), ez) * 1.05f;
        const float half = hnr_div(edge, 2.f);
#pragma unroll
        for (int q = 0; q < 3; ++q) params[q] = hnr_div(red[3 + q][0] + red[q][0], 2.f) - half;
        params[3] = hnr_div(edge, vox_res);
    }
}

// cell key of every pixel; dropped pixels get the key `invalid` (above every cell key: they sort behind all voxels).  The bounding cube is 1.05 x the
// extent, so cells lie in [0, vox_res]; a degenerate frame (one point: 0 / 0) puts everything in cell 0, one voxel, as the reference's NaN cells do.
__global__ void fuse_keys_kernel(const float *__restrict__ pts, const int *__restrict__ kept, int n, const float *__restrict__ params, int bits,
                                 unsigned long long *__restrict__ keys)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!kept[i]) { keys[i] = 1ull << (3 * bits); return; }
    const float sz = params[3], top = (float)((1 << bits) - 1);
    float q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = vox_cell(pts[3 * (size_t)i + a], params[a], sz);
        if (!(q[a] >= 0.f)) q[a] = 0.f;
        if (q[a] > top) q[a] = top;
    }
    keys[i] = vox_pack_key(q[0], q[1], q[2], bits);
}

__global__ void fuse_emit_kernel(const float *__restrict__ pts, const unsigned long long *__restrict__ keys_sorted, const int *__restrict__ perm,
                                 const int *__restrict__ head, const int *__restrict__ vid1, int n, unsigned long long invalid, float *__restrict__ cloud,
                                 long long capacity, const long long *__restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !head[i]) return;
    const unsigned long long key = keys_sorted[i];
    if (key == invalid) return;
    float cx, cy, cz;
    vox_run_centroid(pts, keys_sorted, perm, i, n, key, cx, cy, cz);
    const long long dst = count[0] + (long long)(vid1[i] - 1);
    if (dst >= capacity) return;
    cloud[3 * dst + 0] = cx; cloud[3 * dst + 1] = cy; cloud[3 * dst + 2] = cz;
}

// frame_vox_res <= 0: the kept points themselves, pixel order (incl = inclusive scan of the kept flags)
__global__ void fuse_emit_raw_kernel(const float *__restrict__ pts, const int *__restrict__ kept, const int *__restrict__ incl, int n, float *__restrict__ cloud,
                                     long long capacity, const long long *__restrict__ count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !kept[i]) return;
    const long long dst = count[0] + (long long)(incl[i] - 1);
    if (dst >= capacity) return;
    cloud[3 * dst + 0] = pts[3 * (size_t)i + 0]; cloud[3 * dst + 1] = pts[3 * (size_t)i + 1]; cloud[3 * dst + 2] = pts[3 * (size_t)i + 2];
}

// after the emit kernel has read the count: count += appended (the NEEDED total: it keeps growing past capacity), overflow bit
__global__ void fuse_commit_kernel(const unsigned long long *__restrict__ keys_sorted, const int *__restrict__ incl, int n, unsigned long long invalid,
                                   long long capacity, long long *__restrict__ count, int *__restrict__ status)
{
    long long v = incl[n - 1];
    if (keys_sorted && keys_sorted[n - 1] == invalid) v -= 1;
    const long long need = count[0] + v;
    if (need > capacity) status[0] |= HNR_CLOUD_OVERFLOW;
    count[0] = need;
}

__global__ void crop_flags_kernel(const float *__restrict__ xyz, const long long *__restrict__ n_in, int n_max, float r0, float r1, float r2, float r3, float r4,
                                  float r5, int keep_all, int *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_max) return;
    int f = 0;
    if ((long long)i < n_in[0]) {
        const float x = xyz[3 * (size_t)i + 0], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        f = keep_all || (x >= r0 && y >= r1 && z >= r2 && x <= r3 && y <= r4 && z <= r5);
    }
    flags[i] = f;
}

__global__ void crop_scatter_kernel(const float *__restrict__ xyz, const int *__restrict__ flags, const int *__restrict__ incl, int n_max, float *__restrict__ out,
                                    long long *__restrict__ n_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_max) return;
    if (i == n_max - 1) n_out[0] = (long long)incl[i];
    if (!flags[i]) return;
    const size_t dst = (size_t)(incl[i] - 1);
    out[3 * dst + 0] = xyz[3 * (size_t)i + 0]; out[3 * dst + 1] = xyz[3 * (size_t)i + 1]; out[3 * dst + 2] = xyz[3 * (size_t)i + 2];
}

// one point per lane; cameras staged through LDS NV_CHUNK at a time (every lane of the block reads the same camera: LDS broadcast)
__global__ void __launch_bounds__(256) nearest_view_kernel(const float *__restrict__ xyz, long long N, const float *__restrict__ campos,
                                                           const float *__restrict__ camdir, int M, int *__restrict__ out)
{
    __shared__ float cam[NV_CHUNK][6];
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < N;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (valid) { px = xyz[3 * i + 0]; py = xyz[3 * i + 1]; pz = xyz[3 * i + 2]; }
    float best = INFINITY;
    int arg = 0;
    for (int m0 = 0; m0 < M; m0 += NV_CHUNK) {
        const int mc = M - m0 < NV_CHUNK ? M - m0 : NV_CHUNK;
        __syncthreads();
        for (int e = threadIdx.x; e < mc * 3; e += 256) {
            const int m = e / 3, a = e - 3 * m;
            cam[m][a] = campos[3 * (size_t)(m0 + m) + a];
            cam[m][3 + a] = camdir[3 * (size_t)(m0 + m) + a];
        }
        __syncthreads();
        for (int m = 0; m < mc; ++m) {
            const float dx = px - cam[m][0], dy = py - cam[m][1], dz = pz - cam[m][2];
            const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz);
            const float den = nrm + 1e-6f;
            const float ux = hnr_div(dx, den), uy = hnr_div(dy, den), uz = hnr_div(dz, den);
            const float score = hnr_div(nrm, 200.f) + (1.1f - ((ux * cam[m][3] + uy * cam[m][4]) + uz * cam[m][5]));
            if (score < best) { best = score; arg = m0 + m; }          // first strict minimum (torch.argmin)
        }
    }
    if (valid) out[i] = arg;
}

__global__ void __launch_bounds__(256) view_attrs_kernel(const float *__restrict__ xyz, long long n, ViewCam vc, int H, int W, const float *__restrict__ feat, int C,
                                                         int Hl, int Wl, float *__restrict__ out_feat, float *__restrict__ out_dir, uint8_t *__restrict__ out_mask,
                                                         const uint8_t *__restrict__ visible)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float c[3], gx, gy;
    bool mask = view_project(vc, xyz[3 * i + 0], xyz[3 * i + 1], xyz[3 * i + 2], H, W, c, gx, gy);
    if (visible) mask = mask && visible[i] != 0;                     // an occluded point is a point outside the frame (hnr_point_occlusion)
    if (out_mask) out_mask[i] = mask ? 1 : 0;
    if (out_dir) {
        float d[3];
        view_dir(vc, c, d);
#pragma unroll
        for (int q = 0; q < 3; ++q) out_dir[3 * i + q] = d[q];
    }
    if (!out_feat) return;
    float *o = out_feat + (size_t)i * C;
    if (!mask) {
        for (int ch = 0; ch < C; ++ch) o[ch] = 0.f;
        return;
    }
    const ViewTaps t = view_taps(gx, gy, H, W, Hl, Wl);
    const size_t plane = (size_t)Hl * Wl;
    for (int ch = 0; ch < C; ++ch) o[ch] = view_sample(t, feat + ch * plane, Wl);
}

static int fuse_bits(int vox_res)
{
    int b = 1;
    while (b <= VOX_BITS && (1ll << b) < (long long)vox_res + 2) ++b;
    return b;
}

// scratch of one frame: the voxel_segments layout for n = H*W entries + world points [n,3] + kept flags [n] + per-block bounds + the space record
static int fuse_layout(int64_t n, int end_bit, size_t *sb, size_t *cb, size_t *seg_total, size_t *total)
{
    size_t seg = 0;
    if (vox_layout(n, end_bit, sb, cb, &seg) != 0) return -1;
    if (seg_total) *seg_total = seg;
    *total = seg + vox_align(12 * (size_t)n) + vox_align(4 * (size_t)n) + vox_align(24 * (size_t)cdiv(n, 256)) + 256;
    return 0;
}

}  // namespace hnr

using namespace hnr;

extern "C" int64_t hnr_depth_fuse_scratch_bytes(int H, int W)
{
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1ll << 26)) return -1;
    size_t total = 0;
    if (fuse_layout((int64_t)H * W, 3 * VOX_BITS + 1, nullptr, nullptr, nullptr, &total) != 0) return -1;
    return (int64_t)total;
}

extern "C" int hnr_depth_fuse_frame(const void *d_depth, int depth_is_u16, int H, int W, const float *Ki, const float *c2w, float depth_div, float depth_min,
                                    float depth_max, int frame_vox_res, float *d_cloud, int64_t capacity, int64_t *d_count, int32_t *d_status, void *d_scratch,
                                    int64_t scratch_bytes, void *stream)
{
    if (!d_depth || !Ki || !c2w || !d_cloud || !d_count || !d_status || !d_scratch) { set_error("hnr_depth_fuse_frame: NULL argument"); return HNR_ERR_BADARG; }
    if (H <= 0 || W <= 0 || (int64_t)H * W > (1ll << 26) || capacity < 1 || !(depth_div > 0.f) || frame_vox_res > (1 << VOX_BITS) - 2) {
        set_error("hnr_depth_fuse_frame: bad argument (H, W > 0, H*W <= 2^26, capacity >= 1, depth_div > 0, frame_vox_res <= 2^21 - 2)");
        return HNR_ERR_BADARG;
    }
    const int n = H * W, nblk = cdiv(n, 256);
    const bool thin = frame_vox_res > 0;
    const int bits = thin ? fuse_bits(frame_vox_res) : 1;
    size_t sb = 0, cb = 0, seg = 0, total = 0, full = 0;
    if (fuse_layout(n, 3 * bits + 1, &sb, &cb, &seg, &total) != 0 || fuse_layout(n, 3 * VOX_BITS + 1, nullptr, nullptr, nullptr, &full) != 0 ||
        (size_t)scratch_bytes < full || total > full) {
        set_error("hnr_depth_fuse_frame: scratch smaller than hnr_depth_fuse_scratch_bytes(H, W)"); return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    char *p = (char *)d_scratch;
    unsigned long long *keys = (unsigned long long *)p; p += vox_align(8 * (size_t)n);
    unsigned long long *keys_sorted = (unsigned long long *)p; p += vox_align(8 * (size_t)n);
    int *perm = (int *)p; p += vox_align(4 * (size_t)n);
    int *head = (int *)p; p += vox_align(4 * (size_t)n);
    int *vid = (int *)p; p += vox_align(4 * (size_t)n);
    p += 256;
    void *tmp = p; p = (char *)d_scratch + seg;
    float *pts = (float *)p; p += vox_align(12 * (size_t)n);
    int *kept = (int *)p; p += vox_align(4 * (size_t)n);
    float *part = (float *)p; p += vox_align(24 * (size_t)nblk);
    float *params = (float *)p;
    FuseCam cam;
    memcpy(cam.Ki, Ki, sizeof(cam.Ki));
    memcpy(cam.M, c2w, sizeof(cam.M));
    cam.div = depth_div; cam.dmin = depth_min; cam.dmax = depth_max;
    if (depth_is_u16) fuse_backproject_kernel<true><<<nblk, 256, 0, st>>>(d_depth, n, W, cam, pts, kept, thin ? part : nullptr);
    else fuse_backproject_kernel<false><<<nblk, 256, 0, st>>>(d_depth, n, W, cam, pts, kept, thin ? part : nullptr);
    HNR_LAUNCH_CHECK();
    if (!thin) {
        if (int rc = vox_scan_flags(kept, vid, n, tmp, cb, st)) return rc;
        fuse_emit_raw_kernel<<<nblk, 256, 0, st>>>(pts, kept, vid, n, d_cloud, (long long)capacity, (const long long *)d_count);
        HNR_LAUNCH_CHECK();
        fuse_commit_kernel<<<1, 1, 0, st>>>(nullptr, vid, n, 0ull, (long long)capacity, (long long *)d_count, d_status);
        HNR_LAUNCH_CHECK();
        return HNR_OK;
    }
    const unsigned long long invalid = 1ull << (3 * bits);
    fuse_space_kernel<<<1, 256, 0, st>>>(part, nblk, (float)frame_vox_res, params);
    HNR_LAUNCH_CHECK();
    fuse_keys_kernel<<<nblk, 256, 0, st>>>(pts, kept, n, params, bits, keys);
    HNR_LAUNCH_CHECK();
    if (int rc = vox_sort_segments(keys, n, 3 * bits + 1, keys_sorted, perm, head, vid, tmp, sb, cb, st)) return rc;
    fuse_emit_kernel<<<nblk, 256, 0, st>>>(pts, keys_sorted, perm, head, vid, n, invalid, d_cloud, (long long)capacity, (const long long *)d_count);
    HNR_LAUNCH_CHECK();
    fuse_commit_kernel<<<1, 1, 0, st>>>(keys_sorted, vid, n, invalid, (long long)capacity, (long long *)d_count, d_status);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int64_t hnr_range_crop_scratch_bytes(int64_t n_max)
{
    if (n_max <= 0 || n_max > (1ll << 30)) return -1;
    size_t cb = 0, seg = 0;
    if (vox_layout(n_max, 1, nullptr, &cb, &seg) != 0) return -1;
    return (int64_t)(2 * vox_align(4 * (size_t)n_max) + vox_align(cb));
}

extern "C" int hnr_range_crop(const float *d_xyz, const int64_t *d_n_in, int64_t n_max, const float *ranges, float *d_out, int64_t *d_n_out, void *d_scratch,
                              int64_t scratch_bytes, void *stream)
{
    if (!d_xyz || !d_n_in || !ranges || !d_out || !d_n_out || !d_scratch || d_out == d_xyz) {
        set_error("hnr_range_crop: NULL argument (or d_out == d_xyz)"); return HNR_ERR_BADARG;
    }
    const int64_t need = hnr_range_crop_scratch_bytes(n_max);
    if (need < 0 || scratch_bytes < need) { set_error("hnr_range_crop: 1 <= n_max <= 2^30 and scratch >= hnr_range_crop_scratch_bytes(n_max)"); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const int n = (int)n_max;
    char *p = (char *)d_scratch;
    int *flags = (int *)p; p += vox_align(4 * (size_t)n);
    int *incl = (int *)p; p += vox_align(4 * (size_t)n);
    const size_t cb = (size_t)need - 2 * vox_align(4 * (size_t)n);
    crop_flags_kernel<<<cdiv(n, 256), 256, 0, st>>>(d_xyz, (const long long *)d_n_in, n, ranges[0], ranges[1], ranges[2], ranges[3], ranges[4], ranges[5],
                                                    ranges[0] <= -99.f ? 1 : 0, flags);
    HNR_LAUNCH_CHECK();
    if (int rc = vox_scan_flags(flags, incl, n, p, cb, st)) return rc;
    crop_scatter_kernel<<<cdiv(n, 256), 256, 0, st>>>(d_xyz, flags, incl, n, d_out, (long long *)d_n_out);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_nearest_view(const float *d_xyz, int64_t N, const float *d_campos, const float *d_camdir, int M, int32_t *d_view, void *stream)
{
    if (!d_xyz || !d_campos || !d_camdir || !d_view) { set_error("hnr_nearest_view: NULL argument"); return HNR_ERR_BADARG; }
    if (N <= 0 || M <= 0 || N > (1ll << 31) * 255) { set_error("hnr_nearest_view: bad argument (N > 0, M > 0)"); return HNR_ERR_BADARG; }
    nearest_view_kernel<<<cdiv(N, 256), 256, 0, (hipStream_t)stream>>>(d_xyz, (long long)N, d_campos, d_camdir, M, d_view);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

extern "C" int hnr_point_view_attrs(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                                    const float *d_feat, int C, int Hl, int Wl, float *d_out_feat, float *d_out_dir, uint8_t *d_out_mask, void *stream)
{
    return hnr_point_view_attrs_vis(d_xyz, n, w2c, c2w, cam_pos_cam, K, H, W, d_feat, C, Hl, Wl, nullptr, d_out_feat, d_out_dir, d_out_mask, stream);
}

extern "C" int hnr_point_view_attrs_vis(const float *d_xyz, int64_t n, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K, int H, int W,
                                        const float *d_feat, int C, int Hl, int Wl, const uint8_t *d_visible, float *d_out_feat, float *d_out_dir,
                                        uint8_t *d_out_mask, void *stream)
{
    if (!d_xyz || !w2c || !c2w || !cam_pos_cam || !K || (!d_out_feat && !d_out_dir && !d_out_mask) || (d_out_feat && !d_feat)) {
        set_error("hnr_point_view_attrs: NULL argument"); return HNR_ERR_BADARG;
    }
    if (n <= 0 || H < 2 || W < 2 || (d_out_feat && (C <= 0 || Hl <= 0 || Wl <= 0)) || n > (1ll << 31) * 255) {
        set_error("hnr_point_view_attrs: bad argument (n > 0, H, W >= 2, C, Hl, Wl > 0)"); return HNR_ERR_BADARG;
    }
    ViewCam vc;
    view_cam_fill(vc, w2c, c2w, cam_pos_cam, K);
    view_attrs_kernel<<<cdiv(n, 256), 256, 0, (hipStream_t)stream>>>(d_xyz, (long long)n, vc, H, W, d_feat, C, Hl, Wl, d_out_feat, d_out_dir, d_out_mask, d_visible);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
