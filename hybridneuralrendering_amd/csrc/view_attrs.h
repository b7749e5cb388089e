// The per-point view arithmetic shared by hnr_point_view_attrs (cloud_init.hip) and hnr_point_embed (featnet.hip): projection into a view, the frame
// mask, the viewing direction and the bilinear sample of a channels-first map.  ONE text for both kernels: a point within an ulp of the frame border
// or of a texel must get the same mask, the same taps and the same bits from either.  Every fp32 operation is rounded on its own, in the order
// written (-ffp-contract=off); tests/cloud_init_ref.py restates them.
#pragma once
#include "hnr_common.h"

namespace hnr {

struct ViewCam {
    float Wm[16];                   // w2c
    float R[9];                     // c2w[:3,:3]
    float cpc[3];                   // cam_pos_cam
    float K[9];
};

inline void view_cam_fill(ViewCam &vc, const float *w2c, const float *c2w, const float *cam_pos_cam, const float *K)
{
    memcpy(vc.Wm, w2c, sizeof(vc.Wm));
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) vc.R[3 * r + c] = c2w[4 * r + c];
    memcpy(vc.cpc, cam_pos_cam, sizeof(vc.cpc));
    memcpy(vc.K, K, sizeof(vc.K));
}

// cam = w2c x (x, y, z, 1); (gx, gy) = K x (cam / cam.z); returns the frame mask 0 <= gx <= W-1 && 0 <= gy <= H-1 (NaN compares false)
__device__ __forceinline__ bool view_project(const ViewCam &vc, float x, float y, float z, int H, int W, float c[3], float &gx, float &gy)
{
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = ((x * vc.Wm[4 * q] + y * vc.Wm[4 * q + 1]) + z * vc.Wm[4 * q + 2]) + vc.Wm[4 * q + 3];
    const float q0 = hnr_div(c[0], c[2]), q1 = hnr_div(c[1], c[2]);
    gx = (q0 * vc.K[0] + q1 * vc.K[1]) + vc.K[2];
    gy = (q0 * vc.K[3] + q1 * vc.K[4]) + vc.K[5];
    return gx >= 0.f && gx <= (float)(W - 1) && gy >= 0.f && gy <= (float)(H - 1);
}

// e = cam - cam_pos_cam, u = e / (|e| + 1e-6), dir = R u
__device__ __forceinline__ void view_dir(const ViewCam &vc, const float c[3], float d[3])
{
    const float e0 = c[0] - vc.cpc[0], e1 = c[1] - vc.cpc[1], e2 = c[2] - vc.cpc[2];
    const float den = sqrtf((e0 * e0 + e1 * e1) + e2 * e2) + 1e-6f;
    const float u0 = hnr_div(e0, den), u1 = hnr_div(e1, den), u2 = hnr_div(e2, den);
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q] = (u0 * vc.R[3 * q] + u1 * vc.R[3 * q + 1]) + u2 * vc.R[3 * q + 2];
}

// bilinear, zero padding, align_corners=True on a [C,Hl,Wl] map of an H x W frame: the weights as F.grid_sample forms them (ix_se - ix, ix - ix_nw, ...)
struct ViewTaps {
    float w00, w01, w10, w11;
    int x0, y0, x1, y1;
    bool bx0, bx1, by0, by1;
};

__device__ __forceinline__ ViewTaps view_taps(float gx, float gy, int H, int W, int Hl, int Wl)
{
    ViewTaps t;
    const float sx = hnr_div(gx * (float)(Wl - 1), (float)(W - 1)), sy = hnr_div(gy * (float)(Hl - 1), (float)(H - 1));
    const float x0f = floorf(sx), y0f = floorf(sy), x1f = x0f + 1.f, y1f = y0f + 1.f;
    const float wx0 = x1f - sx, wx1 = sx - x0f, wy0 = y1f - sy, wy1 = sy - y0f;
    t.w00 = wx0 * wy0; t.w01 = wx1 * wy0; t.w10 = wx0 * wy1; t.w11 = wx1 * wy1;
    t.x0 = (int)x0f; t.y0 = (int)y0f; t.x1 = t.x0 + 1; t.y1 = t.y0 + 1;
    t.bx0 = t.x0 >= 0 && t.x0 < Wl; t.bx1 = t.x1 >= 0 && t.x1 < Wl; t.by0 = t.y0 >= 0 && t.y0 < Hl; t.by1 = t.y1 >= 0 && t.y1 < Hl;
    return t;
}

// one channel plane f [Hl,Wl]
__device__ __forceinline__ float view_sample(const ViewTaps &t, const float *__restrict__ f, int Wl)
{
    const float v00 = (t.bx0 && t.by0) ? f[(size_t)t.y0 * Wl + t.x0] : 0.f, v01 = (t.bx1 && t.by0) ? f[(size_t)t.y0 * Wl + t.x1] : 0.f;
    const float v10 = (t.bx0 && t.by1) ? f[(size_t)t.y1 * Wl + t.x0] : 0.f, v11 = (t.bx1 && t.by1) ? f[(size_t)t.y1 * Wl + t.x1] : 0.f;
    return ((t.w00 * v00 + t.w01 * v01) + t.w10 * v10) + t.w11 * v11;
}

}  // namespace hnr
