// The sort / segment machinery shared by voxelize.hip (hnr_voxel_downsample) and cloud_init.hip (per-frame depth fusion):
//   cell keys -> stable radix sort of (key, entry id) -> head flags -> inclusive scan (= 1 + voxel of every sorted entry) -> per-voxel walk.
// The host side (vox_layout, vox_sort_segments) is compiled once, in voxelize.hip; the per-voxel walk is a device function both callers inline.
#pragma once
#include "hnr_common.h"

namespace hnr {

constexpr int VOX_BITS = 21;        // cells per axis < 2^21 (hnr_voxel_downsample); the fusion path picks the bits from frame_vox_res

static inline size_t vox_align(size_t v) { return (v + 255) & ~(size_t)255; }

// floor((p - space_min) / vox_size): fp32 subtract, correctly rounded fp32 divide (mvs_utils.py:552-553)
__device__ __forceinline__ float vox_cell(float p, float mn, float sz) { return floorf(hnr_div(__fsub_rn(p, mn), sz)); }

__device__ __forceinline__ unsigned long long vox_pack_key(float qx, float qy, float qz, int bits)
{
    return ((unsigned long long)(unsigned)qx << (2 * bits)) | ((unsigned long long)(unsigned)qy << bits) | (unsigned long long)(unsigned)qz;
}

// Centroid of the run of sorted entries that starts at i (all entries with keys_sorted == key): sequential fp32 sum in entry-id order (the sort is
// stable), divided by the count.  Returns the end of the run.
__device__ __forceinline__ int vox_run_centroid(const float *__restrict__ xyz, const unsigned long long *__restrict__ keys_sorted, const int *__restrict__ perm,
                                                int i, int n, unsigned long long key, float &cx, float &cy, float &cz)
{
    int e = i;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (; e < n && keys_sorted[e] == key; ++e) {
        const int p = perm[e];
        sx += xyz[3 * p + 0]; sy += xyz[3 * p + 1]; sz += xyz[3 * p + 2];
    }
    const float cnt = (float)(e - i);
    cx = hnr_div(sx, cnt); cy = hnr_div(sy, cnt); cz = hnr_div(sz, cnt);
    return e;
}

// rocprim temporary sizes for n entries with keys of end_bit significant bits; *total = keys, keys_sorted (u64), perm, head, vid (i32), 256 B of
// flags, rocprim temp (max of sort and scan)
int vox_layout(int64_t n, int end_bit, size_t *sort_bytes, size_t *scan_bytes, size_t *total);

// keys [n] -> keys_sorted, perm (stable), head (1 where a new key starts), vid1 (inclusive scan of head).  Stream-ordered; returns an HNR status.
int vox_sort_segments(const unsigned long long *keys, int n, int end_bit, unsigned long long *keys_sorted, int *perm, int *head, int *vid1, void *tmp,
                      size_t sort_bytes, size_t scan_bytes, hipStream_t st);

// inclusive scan of n int flags (order-preserving compaction); tmp: scan_bytes of vox_layout(n, ...)
int vox_scan_flags(const int *flags, int *incl, int n, void *tmp, size_t scan_bytes, hipStream_t st);

}  // namespace hnr
