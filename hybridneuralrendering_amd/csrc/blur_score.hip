// Blur scores of the content-aware frame weights (raft/demo_content_aware_weights.py:78-92, 141-184 of the reference): Laplacian edge maps in fp64 and the
// variance of two frames' edges over their flow-aligned overlap.  Every sum has a fixed order (per-thread strided sums, LDS trees, per-workgroup
// partials added in index order): no float atomics, two runs give the same bits.
#include "hnr_launch.h"

namespace hnr {
namespace {

constexpr int SCORE_BLOCKS = 64;

__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : i >= n ? 2 * n - 2 - i : i; }

// cv2.blur(gray, (5, 5)) of a float64 plane: the 25 taps (exact as an integer) times 1/25, BORDER_REFLECT_101
__device__ __forceinline__ double box5(const uint8_t *g, int y, int x, int H, int W)
{
    int s = 0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const uint8_t *row = g + (size_t)reflect101(y + dy, H) * W;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) s += row[reflect101(x + dx, W)];
    }
    return (double)s * (1.0 / 25.0);
}

// cv2.Laplacian(., CV_64F), ksize 1: aperture [[0,1,0],[1,-4,1],[0,1,0]] on the blurred plane, BORDER_REFLECT_101 again (on the blurred plane)
__global__ void blur_edges_kernel(const uint8_t *__restrict__ gray, int P, int H, int W, double *__restrict__ edges)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)P * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const uint8_t *g = gray + (i / ((int64_t)W * H)) * H * W;
    const double up = box5(g, reflect101(y - 1, H), x, H, W), dn = box5(g, reflect101(y + 1, H), x, H, W);
    const double lf = box5(g, y, reflect101(x - 1, W), H, W), rt = box5(g, y, reflect101(x + 1, W), H, W);
    edges[i] = (((up + lf) + rt) + dn) - 4.0 * box5(g, y, x, H, W);
}

// warp(., flow, mode='nearest') of the reference as torch evaluates it: (x + fx, y + fy) -> 2 v / max(W-1, 1) - 1 -> grid_sample WITHOUT align_corners,
// ((g + 1) W - 1) / 2 -> round half to even; every operation a separately rounded fp32 one (the library is built with -ffp-contract=off).
// Returns the picked pixel's index or -1 (outside: the sample is 0).
__device__ __forceinline__ int warp_pick(const float *flow, int x, int y, int H, int W)
{
    const size_t hw = (size_t)H * W, i = (size_t)y * W + x;
    const float vx = (float)x + flow[i], vy = (float)y + flow[hw + i];
    const float gx = 2.0f * vx / (float)(W - 1 > 1 ? W - 1 : 1) - 1.0f, gy = 2.0f * vy / (float)(H - 1 > 1 ? H - 1 : 1) - 1.0f;
    const float ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f, iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    const float rx = rintf(ix), ry = rintf(iy);
    if (!(rx >= 0.f && rx < (float)W && ry >= 0.f && ry < (float)H)) return -1;
    return (int)ry * W + (int)rx;
}

// pixel used: inside the border frame, and its pick inside the frame and inside the border frame of image 2
__device__ __forceinline__ int used_pick(const float *flow, int i, int H, int W, int border)
{
    const int x = i % W, y = i / W;
    if (x < border || x >= W - border || y < border || y >= H - border) return -1;
    const int pk = warp_pick(flow, x, y, H, W);
    if (pk < 0) return -1;
    const int px = pk % W, py = pk / W;
    return (px < border || px >= W - border || py < border || py >= H - border) ? -1 : pk;
}

template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*red)[256], double *out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if (tid < k) {
#pragma unroll
            for (int q = 0; q < NV; ++q) red[q][tid] += red[q][tid + k];
        }
        __syncthreads();
    }
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) out[q] = red[q][0];
    }
}

// pass 1: per-workgroup (count, sum e1, sum warped e2); optionally the pick and used maps
__global__ __launch_bounds__(256) void blur_score_sums_kernel(const double *__restrict__ e1, const double *__restrict__ e2, const float *__restrict__ flow,
                                                              int H, int W, int border, double *__restrict__ part, int32_t *__restrict__ d_pick,
                                                              uint8_t *__restrict__ d_used)
{
    __shared__ double red[3][256];
    double v[3] = {0.0, 0.0, 0.0};
    const int n = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += SCORE_BLOCKS * 256) {
        const int pk = used_pick(flow, i, H, W, border);
        if (d_pick) d_pick[i] = warp_pick(flow, i % W, i / W, H, W);
        if (d_used) d_used[i] = pk >= 0;
        if (pk < 0) continue;
        v[0] += 1.0; v[1] += e1[i]; v[2] += (double)(float)e2[pk];
    }
    block_sum<3>(v, red, part + 3 * blockIdx.x);
}

// pass 2: the means from pass 1's partials (every workgroup adds them in the same order), then per-workgroup sums of squared deviations
__global__ __launch_bounds__(256) void blur_score_dev_kernel(const double *__restrict__ e1, const double *__restrict__ e2, const float *__restrict__ flow,
                                                             int H, int W, int border, const double *__restrict__ part, double *__restrict__ part2)
{
    __shared__ double red[2][256];
    __shared__ double mean[2];
    if (threadIdx.x == 0) {
        double c = 0.0, s1 = 0.0, s2 = 0.0;
        for (int b = 0; b < SCORE_BLOCKS; ++b) { c += part[3 * b]; s1 += part[3 * b + 1]; s2 += part[3 * b + 2]; }
        mean[0] = c > 0.0 ? s1 / c : 0.0;
        mean[1] = c > 0.0 ? s2 / c : 0.0;
    }
    __syncthreads();
    const double m1 = mean[0], m2 = mean[1];
    double v[2] = {0.0, 0.0};
    const int n = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += SCORE_BLOCKS * 256) {
        const int pk = used_pick(flow, i, H, W, border);
        if (pk < 0) continue;
        const double a = e1[i] - m1, b = (double)(float)e2[pk] - m2;
        v[0] += a * a; v[1] += b * b;
    }
    block_sum<2>(v, red, part2 + 2 * blockIdx.x);
}

// pass 3: row = (population variance of e1, of warped e2, used-pixel count); count 0 leaves (0, 0, 0)
__global__ void blur_score_final_kernel(const double *__restrict__ part, const double *__restrict__ part2, double *__restrict__ row)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double c = 0.0, q1 = 0.0, q2 = 0.0;
    for (int b = 0; b < SCORE_BLOCKS; ++b) { c += part[3 * b]; q1 += part2[2 * b]; q2 += part2[2 * b + 1]; }
    row[0] = c > 0.0 ? q1 / c : 0.0;
    row[1] = c > 0.0 ? q2 / c : 0.0;
    row[2] = c;
}

bool frame_ok(int H, int W) { return H >= 8 && W >= 8 && H <= 16384 && W <= 16384 && (int64_t)H * W <= (1 << 28); }

}  // namespace
}  // namespace hnr

using namespace hnr;

#define BAD(...) do { set_error(__VA_ARGS__); return HNR_ERR_BADARG; } while (0)

extern "C" {

int hnr_blur_edges(const uint8_t *d_gray, int P, int H, int W, double *d_edges, void *stream)
{
    if (!d_gray || !d_edges) BAD("hnr_blur_edges: NULL pointer");
    if (P < 1 || P > 65536 || !frame_ok(H, W) || (int64_t)P * H * W > ((int64_t)1 << 34)) BAD("hnr_blur_edges: P=%d H=%d W=%d (8 <= H, W <= 16384, H*W <= 2^28)", P, H, W);
    blur_edges_kernel<<<cdiv((int64_t)P * H * W, 256), 256, 0, (hipStream_t)stream>>>(d_gray, P, H, W, d_edges);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

int64_t hnr_blur_score_pair_scratch_bytes(int H, int W) { return frame_ok(H, W) ? (int64_t)SCORE_BLOCKS * 5 * sizeof(double) : -1; }

int hnr_blur_score_pair(const double *d_edge1, const double *d_edge2, const float *d_flow, int H, int W, int border, double *d_row, int32_t *d_pick,
                        uint8_t *d_used, void *d_scratch, int64_t scratch_bytes, void *stream)
{
    if (!d_edge1 || !d_edge2 || !d_flow || !d_row || !d_scratch) BAD("hnr_blur_score_pair: NULL pointer");
    if (!frame_ok(H, W)) BAD("hnr_blur_score_pair: H=%d W=%d (8 <= H, W <= 16384, H*W <= 2^28)", H, W);
    if (border < 0 || 2 * border >= H || 2 * border >= W) BAD("hnr_blur_score_pair: border=%d leaves nothing of a %dx%d frame", border, H, W);
    if (((uintptr_t)d_scratch & 7) || scratch_bytes < (int64_t)SCORE_BLOCKS * 5 * (int64_t)sizeof(double)) BAD("hnr_blur_score_pair: scratch too short or not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    double *part = (double *)d_scratch, *part2 = part + 3 * SCORE_BLOCKS;
    blur_score_sums_kernel<<<SCORE_BLOCKS, 256, 0, st>>>(d_edge1, d_edge2, d_flow, H, W, border, part, d_pick, d_used);
    HNR_LAUNCH_CHECK();
    blur_score_dev_kernel<<<SCORE_BLOCKS, 256, 0, st>>>(d_edge1, d_edge2, d_flow, H, W, border, part, part2);
    HNR_LAUNCH_CHECK();
    blur_score_final_kernel<<<1, 64, 0, st>>>(part, part2, d_row);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}

}  // extern "C"
