// Frames of a camera path: the front and the back of a frame whose camera is not a row of a frame bank (a fly-through, an orbit, a viewer's pose).
//
// The reference's run/render_vid.py is no usable definition (its get_dummyrot_item carries no reference views, it builds rays with the Blender ray
// builder from a pose already in OpenCV convention, and the ScanNet dataset has no render_poses), so the behaviour is DEFINED in include/hnr.h and
// restated in tests/path_ref.py.  Here:
//
//   pose_views_kernel     one workgroup per query camera: the reference views of a free pose, get_nearest_cam_id
//                         (data/nerf_synth360_ft_dataset.py:49-74) with every tie decided.  Scores and distances become 64-bit keys
//                         (order-preserving bits of the float << 32 | index: all different, so ANY correct sort gives the stable order) and are
//                         sorted in LDS by a bitonic network: T = 8192 cameras are 91 passes over 64 KB, not 67 M comparisons.
//                         In path mode (one workgroup) it also reads the step counter, picks the pose, writes the item's camera / reference-view
//                         outputs and advances the counter once: what frame_header_kernel does for a bank row.
//   path_frame_rays_kernel      frames_dev.h's frame_rays_kernel over the pose table standing in for a bank's c2w: the bits of hnr_frame_item
//   path_frame_images_*_kernel  its image kernels over the V rows just chosen
//   frame_store_kernel    the back: colour (and depth) rays -> one frame of a clip, 8-bit by the rule of hnr_frame_metrics, float32, depth
//
// Nothing is allocated, nothing is read back, no atomics; stream-ordered and capturable on one stream.
#define HNR_FRAMES_KERNEL(name) path_##name       // this file's copies of the ray and image kernels
#include "frames_dev.h"

namespace hnr {

constexpr int PV_MAX_T = 8192, PV_MAX_V = 64, PV_MAX_THREADS = 1024;
constexpr int PI_VIEWS = 2 * HDR_WORDS;      // scratch words: {frame i, 0, 0, 0} for the rays, {0, 0, 0, 0} = "row 0" of the V-row table that follows

struct PoseViewArgs {
    BankView rb;                             // the reference bank: T = rb.F cameras
    const float *poses, *K;                  // [Q,4,4]; [3,3] or [Q,3,3]
    const int *exclude;                      // [Q] or NULL
    int *nearest;                            // [Q,V] (not in path mode)
    int Q, K_per_pose, V, n1, npow, n2pow;
    // path mode
    unsigned long long *d_step;
    int explicit_i, downweight;
    float bg[3];
    int *hdr;
    BatchOut o;
};

// bits of a float whose unsigned order is the float order (ascending); -0 = +0; NaN = the largest word
__device__ __forceinline__ unsigned pv_ascending(float x)
{
    if (x != x) return 0xFFFFFFFFu;
    const unsigned b = x == 0.f ? 0u : __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// ... descending; NaN again the largest word (finite and infinite values map into 0x007FFFFF .. 0xFF800000, so nothing else reaches it)
__device__ __forceinline__ unsigned pv_descending(float x) { return x != x ? 0xFFFFFFFFu : ~pv_ascending(x); }

// ascending bitonic sort of n = 2^k >= 2 keys in LDS by the whole workgroup
__device__ __forceinline__ void pv_sort(unsigned long long *k, int n)
{
    const int t = threadIdx.x, nt = blockDim.x;
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int p = t; p < (n >> 1); p += nt) {
                const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long a = k[lo], b = k[hi];
                if ((a > b) == up) { k[lo] = b; k[hi] = a; }
            }
        }
    }
    __syncthreads();
}

template <bool PATH>
__global__ void __launch_bounds__(PV_MAX_THREADS) pose_views_kernel(PoseViewArgs a)
{
    extern __shared__ unsigned long long pv_keys[];                 // [npow] step 1, then [n2pow] step 2
    __shared__ int s_q, s_sel[PV_MAX_V];
    const int t = threadIdx.x, nt = blockDim.x, T = a.rb.F;
    int q = blockIdx.x;
    if (PATH) {
        if (t == 0) {
            int i = a.explicit_i;
            if (a.d_step) {
                const unsigned long long step = a.d_step[0];
                i = (int)(step % (unsigned long long)a.Q);
                a.d_step[0] = step + 1ull;
            }
            if (i < 0 || i >= a.Q) i = 0;                           // (the host validates an explicit frame: never taken through frames.py)
            s_q = i;
            a.hdr[0] = i; a.hdr[1] = 0; a.hdr[2] = 0; a.hdr[3] = 0;
            for (int e = HDR_WORDS; e < PI_VIEWS; ++e) a.hdr[e] = 0;
            if (a.o.frame_row) a.o.frame_row[0] = i;
        }
        __syncthreads();
        q = s_q;
    }
    const float *M = a.poses + 16 * (size_t)q, *K = a.K + (a.K_per_pose ? 9 * (size_t)q : 0);
    const float cx = (float)(a.rb.W / 2), cy = (float)(a.rb.H / 2);
    float d[3];
    fb_raydir(cx, cy, K, M, 1, d);
    const float cp[3] = {M[3], M[7], M[11]};

    // step 1: the n1 cameras whose centre direction is closest to the query's (largest dot product first, lower row first among equals)
    for (int e = t; e < a.npow; e += nt) {
        unsigned long long key = 0xFFFFFFFF00000000ull | (unsigned)e;
        if (e < T) {
            float td[3];
            fb_raydir(cx, cy, a.rb.K + (a.rb.K_per_frame ? 9 * (size_t)e : 0), a.rb.c2w + 16 * (size_t)e, 1, td);
            const float s = (td[0] * d[0] + td[1] * d[1]) + td[2] * d[2];
            key = ((unsigned long long)pv_descending(s) << 32) | (unsigned)e;
        }
        pv_keys[e] = key;
    }
    pv_sort(pv_keys, a.npow);

    // step 2: those n1 by distance to the query's position (ascending, step-1 order among equals)
    unsigned long long *k2 = pv_keys + a.npow;
    for (int j = t; j < a.n2pow; j += nt) {
        unsigned long long key = 0xFFFFFFFF00000000ull | (unsigned)j;
        if (j < a.n1) {
            int row = (int)(unsigned)(pv_keys[j] & 0xFFFFFFFFull);
            if (row >= T) row = 0;                                   // (n1 <= T: the first n1 keys are cameras, never padding)
            const float *P = a.rb.c2w + 16 * (size_t)row;
            const float ax = P[3] - cp[0], ay = P[7] - cp[1], az = P[11] - cp[2];
            const float dist = sqrtf((ax * ax + ay * ay) + az * az);
            key = ((unsigned long long)pv_ascending(dist) << 32) | (unsigned)j;
        }
        k2[j] = key;
    }
    pv_sort(k2, a.n2pow);

    if (t < a.V) {
        const int first = (int)(unsigned)(pv_keys[(unsigned)(k2[0] & 0xFFFFFFFFull)] & 0xFFFFFFFFull);
        const int ex = (!PATH && a.exclude) ? a.exclude[q] : -1;
        int j = t + ((ex >= 0 && first == ex) ? 1 : 0);
        if (j > a.n1 - 1) j = a.n1 - 1;                              // (n1 >= V + 1 with an exclude table: never taken)
        int row = (int)(unsigned)(pv_keys[(unsigned)(k2[j] & 0xFFFFFFFFull)] & 0xFFFFFFFFull);
        if (row >= T) row = 0;
        if (PATH) { s_sel[t] = row; a.hdr[PI_VIEWS + t] = row; }
        else a.nearest[(size_t)q * a.V + t] = row;
    }
    if (!PATH) return;

    // the item's small outputs, as frame_header_kernel writes them for a bank row
    __syncthreads();
    const BatchOut &o = a.o;
    if (t < 16 && o.c2w) o.c2w[t] = M[t];
    if (t < 9) {
        if (o.camrot) o.camrot[t] = M[4 * (t / 3) + t % 3];
        if (o.intrinsic) o.intrinsic[t] = K[t];
    }
    if (t < 3) {
        if (o.campos) o.campos[t] = M[4 * t + 3];
        if (o.bg_color) o.bg_color[t] = a.bg[t];
    }
    const BankView &rb = a.rb;
    for (int e = t; e < a.V * 16; e += nt) {
        const int v = e >> 4, c = e & 15, nr = s_sel[v];
        if (o.c2w_nearest) o.c2w_nearest[e] = rb.c2w[16 * (size_t)nr + c];
        if (o.w2c_nearest) o.w2c_nearest[e] = rb.w2c[16 * (size_t)nr + c];
        if (c < 3 && o.campos_nearest) o.campos_nearest[3 * v + c] = rb.c2w[16 * (size_t)nr + 4 * c + 3];
        if (c == 0) {
            if (o.frame_weight_nearest) o.frame_weight_nearest[v] = a.downweight ? rb.weight[nr] : 1.f;
            if (o.vid_angle_nearest) o.vid_angle_nearest[v] = rb.angle[nr];
        }
        if (v == 0 && c < 9 && o.intrinsic_nearest) o.intrinsic_nearest[c] = rb.K[(rb.K_per_frame ? 9 * (size_t)nr : 0) + c];
    }
}

// (np.clip(x, 0, 1) * 255).astype(np.uint8) as hnr_frame_metrics quantises: clamp, ONE fp32 product, truncation (a NaN clamps to 0)
__device__ __forceinline__ uint8_t fs_quantise(float x) { return (uint8_t)(int)__fmul_rn(fminf(fmaxf(x, 0.f), 1.f), 255.0f); }

// one lane per ray; the frame was cleared before.  A pixel index outside the frame (or NaN) is dropped.
__global__ void __launch_bounds__(256) frame_store_kernel(const float *__restrict__ color, const float *__restrict__ pix, const float *__restrict__ depth, int R,
                                                          int h, int w, uint8_t *__restrict__ img8, float *__restrict__ image, float *__restrict__ dimg)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R) return;
    const float px = pix[2 * (size_t)i], py = pix[2 * (size_t)i + 1];
    if (!(px >= 0.f && px < (float)w && py >= 0.f && py < (float)h)) return;
    const size_t p = (size_t)(int)py * w + (int)px;
    if (img8 || image) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = color[3 * (size_t)i + c];
            if (image) image[3 * p + c] = v;
            if (img8) img8[3 * p + c] = fs_quantise(v);
        }
    }
    if (dimg) dimg[p] = depth[i];
}

static int pow2_at_least(int n) { int p = 2; while (p < n) p <<= 1; return p; }

// the checks the two selecting entries share; fills the launch shape
static int pose_views_args(const char *who, const hnr_frame_bank *ref, const float *d_poses, int Q, const float *d_intrinsic, int V, int n1, bool exclude,
                           PoseViewArgs &a, int &threads, int &lds)
{
    if (!ref || !ref->d_c2w || !ref->d_intrinsic || !d_poses || !d_intrinsic) { set_error("%s: NULL pointer", who); return HNR_ERR_BADARG; }
    if (ref->F < 1 || ref->F > PV_MAX_T || ref->H < 1 || ref->W < 1 || Q < 1 || Q > (1 << 24)) {
        set_error("%s: 1 <= T <= %d reference cameras, H, W >= 1, 1 <= Q <= 2^24", who, PV_MAX_T); return HNR_ERR_BADARG;
    }
    if (V < 1 || V > PV_MAX_V) { set_error("%s: 1 <= V <= %d", who, PV_MAX_V); return HNR_ERR_BADARG; }
    if (n1 < V + (exclude ? 1 : 0) || n1 > ref->F) {
        set_error("%s: n1 = %d candidates cannot give %d views%s out of %d cameras", who, n1, V, exclude ? " plus an excluded row" : "", ref->F); return HNR_ERR_BADARG;
    }
    memset(&a, 0, sizeof(a));
    a.rb = bank_view(ref);
    a.poses = d_poses; a.K = d_intrinsic; a.Q = Q; a.V = V; a.n1 = n1;
    a.npow = pow2_at_least(ref->F); a.n2pow = pow2_at_least(n1);
    threads = a.npow / 2 < 64 ? 64 : (a.npow / 2 > PV_MAX_THREADS ? PV_MAX_THREADS : a.npow / 2);
    lds = (int)sizeof(unsigned long long) * (a.npow + a.n2pow);
    return HNR_OK;
}

}  // namespace hnr

using namespace hnr;

extern "C" int hnr_pose_views(const hnr_frame_bank *reference, const float *d_poses, int Q, const float *d_intrinsic, int intrinsic_per_pose,
                              const int32_t *d_exclude_row, int V, int n1, int32_t *d_nearest, void *stream)
{
    const char *who = "hnr_pose_views";
    PoseViewArgs a;
    int threads = 0, lds = 0;
    const int rc = pose_views_args(who, reference, d_poses, Q, d_intrinsic, V, n1, d_exclude_row != nullptr, a, threads, lds);
    if (rc != HNR_OK) return rc;
    if (!d_nearest) { set_error("%s: NULL pointer", who); return HNR_ERR_BADARG; }
    a.K_per_pose = intrinsic_per_pose ? 1 : 0; a.exclude = d_exclude_row; a.nearest = d_nearest;
    return launch_lds<pose_views_kernel<false>>(dim3(Q), dim3(threads), lds, (hipStream_t)stream, a);
}

extern "C" int hnr_path_item(const hnr_frame_bank *reference, const float *d_poses, int P, const float *d_intrinsic, int intrinsic_per_pose, int V, int n1,
                             uint64_t *d_step, int i, int margin, int dir_norm, const float *bg_color, int downweight_blurry_feats,
                             const hnr_frame_batch_out *out, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    const char *who = "hnr_path_item";
    if (!bank_ok(reference, who, "reference")) return HNR_ERR_BADARG;
    PoseViewArgs a;
    int threads = 0, lds = 0;
    const int rc = pose_views_args(who, reference, d_poses, P, d_intrinsic, V, n1, false, a, threads, lds);
    if (rc != HNR_OK) return rc;
    if (!out || !d_scratch || !bg_color) { set_error("%s: NULL argument", who); return HNR_ERR_BADARG; }
    if (scratch_bytes < HNR_PATH_SCRATCH_BYTES) { set_error("%s: scratch smaller than HNR_PATH_SCRATCH_BYTES", who); return HNR_ERR_BADARG; }
    if (out->d_gt_image || out->d_frame_weight || out->d_patch_table) {
        set_error("%s: a path frame has no ground truth, frame weight or patch table (gt_image, frame_weight, patch_table must be NULL)", who); return HNR_ERR_BADARG;
    }
    if (!d_step && (i < 0 || i >= P)) { set_error("%s: 0 <= i < P without a step counter", who); return HNR_ERR_BADARG; }
    const int64_t wn = (int64_t)reference->W - 2 * (int64_t)margin, hn = (int64_t)reference->H - 2 * (int64_t)margin;
    if (margin < 0 || wn <= 0 || hn <= 0) { set_error("%s: margin >= 0 and a margin that leaves pixels", who); return HNR_ERR_BADARG; }
    if (out->d_images_nearest && !reference->images_f32 && ((uintptr_t)out->d_images_nearest & 15)) {
        set_error("%s: d_images_nearest must be 16-byte aligned", who); return HNR_ERR_BADARG;
    }
    hipStream_t st = (hipStream_t)stream;
    int *hdr = (int *)d_scratch;
    a.K_per_pose = intrinsic_per_pose ? 1 : 0; a.d_step = (unsigned long long *)d_step; a.explicit_i = d_step ? 0 : i;
    a.downweight = downweight_blurry_feats ? 1 : 0; a.hdr = hdr; a.o = batch_out(out);
    memcpy(a.bg, bg_color, sizeof(a.bg));
    const int lrc = launch_lds<pose_views_kernel<true>>(dim3(1), dim3(threads), lds, st, a);
    if (lrc != HNR_OK) return lrc;
    const BatchOut &o = a.o;
    if (o.raydir || o.pixel_idx) {
        BankView tb = a.rb;                                          // the pose table in place of a bank's cameras: frame hdr[0] = pose i
        tb.images = nullptr; tb.c2w = d_poses; tb.w2c = nullptr; tb.K = d_intrinsic; tb.K_per_frame = a.K_per_pose; tb.F = P;
        BatchArgs b;
        memset(&b, 0, sizeof(b));
        b.mode = FB_NO_CROP; b.margin = margin; b.dir_norm = dir_norm ? 1 : 0; b.V = V; b.ps = 1; b.R = (int)(wn * hn);
        path_frame_rays_kernel<<<cdiv(b.R, 256), 256, 0, st>>>(tb, hdr, nullptr, b, o);
        HNR_LAUNCH_CHECK();
    }
    if (o.images_nearest) {
        const BankView &rb = a.rb;
        const int *hdr0 = hdr + HDR_WORDS, *sel = hdr + PI_VIEWS;    // "row 0" of the one-row table of the V rows chosen
        const size_t n = (size_t)rb.H * rb.W * 3;
        if (rb.f32) {
            const bool vec = (n & 3) == 0 && (((uintptr_t)rb.images | (uintptr_t)o.images_nearest) & 15) == 0;
            const int grid = (int)fb_min((size_t)device_num_cus() * 8, (size_t)cdiv((int64_t)V * (int64_t)(vec ? n >> 2 : n), 256));
            if (vec) path_frame_images_f32_kernel<true><<<grid, 256, 0, st>>>((const float *)rb.images, n, V, rb.F, hdr0, sel, o.images_nearest);
            else path_frame_images_f32_kernel<false><<<grid, 256, 0, st>>>((const float *)rb.images, n, V, rb.F, hdr0, sel, o.images_nearest);
        } else {
            const size_t work = (size_t)V * ((n >> 4) > 32 ? (n >> 4) : 32);
            const int grid = (int)fb_min((size_t)device_num_cus() * 8, (size_t)cdiv((int64_t)work, 256));
            path_frame_images_u8_kernel<<<grid, 256, 0, st>>>((const uint8_t *)rb.images, n, V, rb.F, hdr0, sel, o.images_nearest);
        }
        HNR_LAUNCH_CHECK();
    }
    return HNR_OK;
}

extern "C" int hnr_frame_store(const float *d_color, const float *d_pixel_idx, const float *d_depth, int64_t R, int h, int w, uint8_t *d_img8,
                               float *d_image, float *d_depth_image, void *stream)
{
    const char *who = "hnr_frame_store";
    if (h < 1 || w < 1 || (int64_t)h * w > (1ll << 26) || R < 0 || R > (1ll << 26)) { set_error("%s: h, w >= 1, h * w <= 2^26, 0 <= R <= 2^26", who); return HNR_ERR_BADARG; }
    if (!d_img8 && !d_image && !d_depth_image) { set_error("%s: no output", who); return HNR_ERR_BADARG; }
    if (R > 0 && (!d_pixel_idx || ((d_img8 || d_image) && !d_color))) { set_error("%s: NULL d_pixel_idx / d_color", who); return HNR_ERR_BADARG; }
    if (d_depth_image && R > 0 && !d_depth) { set_error("%s: d_depth_image without d_depth", who); return HNR_ERR_BADARG; }
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)h * w;
    if (d_img8) HNR_HIP_CHECK(hipMemsetAsync(d_img8, 0, 3 * n, st));
    if (d_image) HNR_HIP_CHECK(hipMemsetAsync(d_image, 0, 3 * n * sizeof(float), st));
    if (d_depth_image) HNR_HIP_CHECK(hipMemsetAsync(d_depth_image, 0, n * sizeof(float), st));
    if (R > 0) {
        frame_store_kernel<<<cdiv(R, 256), 256, 0, st>>>(d_color, d_pixel_idx, d_depth, (int)R, h, w, d_img8, d_image, d_depth_image);
        HNR_LAUNCH_CHECK();
    }
    return HNR_OK;
}
