// What the two MFMA convolutions (raft.hip, lpips.hip) have in common: the packed layer `w [taps][cinp][cout] | bias [cout]`, cinp = input channels
// rounded up to even (a pair of consecutive channels of one tap per v_mfma_f32_32x32x2_f32; the added row is zero), and the 32 x 32 result layout.
// The kernels themselves differ on purpose (K split across waves against blocked chunks: other summation orders, other bits) and stay where they are.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hnr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int64_t packed_layer_elems(int cin, int cout, int kh, int kw) { return (int64_t)kh * kw * ((cin + 1) & ~1) * cout + cout; }

struct PackedLayer { const float *w, *bias; };

// the layer at `pk` (cin: its input channels, each source of several already rounded up to even); advances `pk` past w and bias
inline PackedLayer next_layer(const float *&pk, int taps, int cin, int cout)
{
    const PackedLayer l = {pk, pk + (size_t)taps * ((cin + 1) & ~1) * cout};
    pk = l.bias + cout;
    return l;
}

// row of the 32 x 32 result that accumulator register r of a lane in half `half` (lane >> 5) holds; the column is lane & 31
__host__ __device__ constexpr int mfma32_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

}  // namespace hnr
