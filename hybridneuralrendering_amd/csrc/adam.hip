// The optimiser step on the device: ONE multi-tensor Adam launch over every tensor of every parameter group, behind ONE single-thread "tick"
// launch that advances the counters and evaluates the learning-rate schedule.
//
// Replaces the two torch.optim.Adam steps of MvsPointsVolumetricModel.backward (models/mvs_points_volumetric_model.py:111-131: self.optimizer.step(),
// self.neural_point_optimizer.step(), built at :94-104 with betas (0.9, 0.999), no weight decay, no amsgrad) and `scheduler.step()` of
// BaseModel.update_learning_rate (models/base_model.py:148-150) under lr_policy 'iter_exponential_decay' (models/helpers/networks.py:56-61:
// LambdaLR with lambda_rule(it) = pow(lr_decay_exp, it / lr_decay_iters)).
//
//   adam_tick_kernel    one thread.  counters = {adam_step, sched_it} (int64, device).  Reads the groups' hyper-parameters (device fp64 rows of
//                       HNR_ADAM_GROUP_DOUBLES), increments both counters and writes one row of HNR_ADAM_ROW_DOUBLES fp64 scalars per group:
//                         lr_t = lr0 * decay_exp^(sched_it_before / decay_iters),  bc1 = 1 - beta1^step,  bc2 = 1 - beta2^step,
//                         lr_t / bc1,  sqrt(bc2),  1 - beta1,  1 - beta2,  beta2,  eps,  step
//                       (step = adam_step after the increment: torch's `state['step']`).
//   adam_update_kernel  one workgroup per HNR_ADAM_CHUNK elements of one tensor (the chunk table says which).  Reads ONLY the tensor table, the chunk
//                       table and its group's row; the six scalars it uses are rounded to fp32 once.  Per element, every operation rounded on its
//                       own (-ffp-contract=off, correctly rounded divide and sqrt):
//                         m' = m + w1 * (g - m)                    exp_avg.lerp_(grad, 1 - beta1)
//                         v' = (v * b2) + ((w2 * g) * g)           exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
//                         den = (sqrt(v') / bs) + e                (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
//                         p' = p - ss * (m' / den)                 param.addcdiv_(exp_avg, denom, value=-step_size)
//                       the element order of torch's _single_tensor_adam.  16 bytes per lane where p, g, m, v are all 16-byte aligned, one element per
//                       lane otherwise (a bias that is a slice of a larger buffer) and in a chunk's last 1..3 elements.  Component arithmetic is
//                       scalar: no packed fp32 instruction.
//
// No host value enters a step (both launches read device memory only), nothing is allocated, nothing is read back, no atomics: the two launches
// sit inside a captured training step and one graph serves every step; results are bit-identical between runs.  A row with m = v = g = 0 stays
// bit-unchanged (m' = 0, v' = 0, p - ss * (0 / e) = p).  Not special-cased: subnormal intermediates are kept (fp32 denormals are on), NaN / inf
// gradients propagate into m, v and p as they do in torch.  tests/adam_ref.py restates the arithmetic in NumPy.
#include "hnr_common.h"

#include <math.h>

namespace hnr {

constexpr int ADAM_THREADS = 256;
static_assert(HNR_ADAM_CHUNK % (4 * ADAM_THREADS) == 0, "a chunk is a whole number of 16-byte passes of the workgroup");

__global__ void adam_tick_kernel(int64_t *__restrict__ counters, const double *__restrict__ groups, int n_groups, double *__restrict__ rows)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t step = counters[0] + 1, it = counters[1];
    counters[0] = step;
    counters[1] = it + 1;
    for (int g = 0; g < n_groups; ++g) {
        const double *h = groups + (size_t)g * HNR_ADAM_GROUP_DOUBLES;
        const double lr0 = h[0], beta1 = h[1], beta2 = h[2], eps = h[3], decay_exp = h[4], decay_iters = h[5];
        const double lr_t = lr0 * pow(decay_exp, (double)it / decay_iters);
        const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
        double *r = rows + (size_t)g * HNR_ADAM_ROW_DOUBLES;
        r[0] = lr_t; r[1] = bc1; r[2] = bc2; r[3] = lr_t / bc1; r[4] = sqrt(bc2);
        r[5] = 1.0 - beta1; r[6] = 1.0 - beta2; r[7] = beta2; r[8] = eps; r[9] = (double)step;
    }
}

struct AdamScalars { float w1, w2, b2, e, ss, bs; };

__device__ __forceinline__ void adam_element(const AdamScalars &s, float g, float &p, float &m, float &v)
{
    m = m + s.w1 * (g - m);
    v = (v * s.b2) + ((s.w2 * g) * g);
    const float den = (sqrtf(v) / s.bs) + s.e;
    p = p - s.ss * (m / den);
}

// The tensor table hands out generic pointers; the buffers are global memory, and saying so gives global_ (not flat_) loads and stores.
// (v4f: 16 bytes per lane; only its components are ever used in arithmetic.)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) v4f gv4f;

__device__ __forceinline__ void adam_quad(const AdamScalars &s, const v4f G, v4f &P, v4f &M, v4f &V)
{
    float p[4] = {P.x, P.y, P.z, P.w}, m[4] = {M.x, M.y, M.z, M.w}, v[4] = {V.x, V.y, V.z, V.w};
    const float g[4] = {G.x, G.y, G.z, G.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) adam_element(s, g[c], p[c], m[c], v[c]);
    P.x = p[0]; P.y = p[1]; P.z = p[2]; P.w = p[3];
    M.x = m[0]; M.y = m[1]; M.z = m[2]; M.w = m[3];
    V.x = v[0]; V.y = v[1]; V.z = v[2]; V.w = v[3];
}

__global__ void __launch_bounds__(ADAM_THREADS) adam_update_kernel(const hnr_adam_tensor *__restrict__ tensors, const int32_t *__restrict__ chunks,
                                                                   const double *__restrict__ rows, int n_tensors, int n_groups)
{
    const int ti = chunks[2 * (size_t)blockIdx.x], ci = chunks[2 * (size_t)blockIdx.x + 1];
    if ((unsigned)ti >= (unsigned)n_tensors || ci < 0) return;                       // (a table hnr_adam_plan did not write)
    const hnr_adam_tensor T = tensors[ti];
    if ((unsigned)T.group >= (unsigned)n_groups) return;
    const double *r = rows + (size_t)T.group * HNR_ADAM_ROW_DOUBLES;
    AdamScalars s;
    s.w1 = (float)r[5]; s.w2 = (float)r[6]; s.b2 = (float)r[7]; s.e = (float)r[8]; s.ss = (float)r[3]; s.bs = (float)r[4];
    const int64_t start = (int64_t)ci * HNR_ADAM_CHUNK;
    const int64_t left = T.n - start;
    if (left <= 0) return;
    const int n = left < HNR_ADAM_CHUNK ? (int)left : HNR_ADAM_CHUNK;
    gf32 *p = (gf32 *)T.p + start, *m = (gf32 *)T.m + start, *v = (gf32 *)T.v + start;
    const gf32 *g = (const gf32 *)T.g + start;
    const int t = threadIdx.x;
    // (a chunk starts a multiple of 16 KB behind its tensor: the chunk's alignment is the tensor's)
    const bool wide = ((((uintptr_t)T.p) | ((uintptr_t)T.g) | ((uintptr_t)T.m) | ((uintptr_t)T.v)) & 15u) == 0;
    int done = 0;
    if (wide) {
        const int n4 = n >> 2;
        gv4f *p4 = (gv4f *)p, *m4 = (gv4f *)m, *v4 = (gv4f *)v;
        const gv4f *g4 = (const gv4f *)g;
        if (n == HNR_ADAM_CHUNK) {
            // whole chunk: all loads of the lane's passes first, then the arithmetic
            constexpr int PASSES = HNR_ADAM_CHUNK / (4 * ADAM_THREADS);
            v4f P[PASSES], G[PASSES], M[PASSES], V[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int i = t + k * ADAM_THREADS;
                P[k] = p4[i]; G[k] = g4[i]; M[k] = m4[i]; V[k] = v4[i];
            }
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int i = t + k * ADAM_THREADS;
                adam_quad(s, G[k], P[k], M[k], V[k]);
                p4[i] = P[k]; m4[i] = M[k]; v4[i] = V[k];
            }
            return;
        }
        for (int i = t; i < n4; i += ADAM_THREADS) {
            v4f P = p4[i], M = m4[i], V = v4[i];
            const v4f G = g4[i];
            adam_quad(s, G, P, M, V);
            p4[i] = P; m4[i] = M; v4[i] = V;
        }
        done = n4 << 2;
    }
    for (int i = done + t; i < n; i += ADAM_THREADS) {
        float P = p[i], M = m[i], V = v[i];
        adam_element(s, g[i], P, M, V);
        p[i] = P; m[i] = M; v[i] = V;
    }
}

static int check_table(const char *who, int n_tensors, int n_groups)
{
    if (n_tensors < 1 || n_tensors > HNR_ADAM_MAX_TENSORS) { set_error("%s: 1 <= n_tensors <= %d, got %d", who, HNR_ADAM_MAX_TENSORS, n_tensors); return HNR_ERR_BADARG; }
    if (n_groups < 1 || n_groups > HNR_ADAM_MAX_GROUPS) { set_error("%s: 1 <= n_groups <= %d, got %d", who, HNR_ADAM_MAX_GROUPS, n_groups); return HNR_ERR_BADARG; }
    return HNR_OK;
}

}  // namespace hnr

using namespace hnr;

extern "C" int64_t hnr_adam_plan(const hnr_adam_tensor *tensors, int n_tensors, int n_groups, int32_t *chunks, int64_t chunk_cap)
{
    if (check_table("hnr_adam_plan", n_tensors, n_groups) != HNR_OK) return HNR_ERR_BADARG;
    if (!tensors) { set_error("hnr_adam_plan: NULL tensor table"); return HNR_ERR_BADARG; }
    if (chunks && chunk_cap < 0) { set_error("hnr_adam_plan: negative chunk capacity %lld", (long long)chunk_cap); return HNR_ERR_BADARG; }
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const hnr_adam_tensor &T = tensors[i];
        if (!T.p || !T.g || !T.m || !T.v) { set_error("hnr_adam_plan: tensor %d has a NULL p / g / m / v pointer", i); return HNR_ERR_BADARG; }
        if (((((uintptr_t)T.p) | ((uintptr_t)T.g) | ((uintptr_t)T.m) | ((uintptr_t)T.v)) & 3u) != 0) {
            set_error("hnr_adam_plan: tensor %d: p / g / m / v must be 4-byte aligned", i); return HNR_ERR_BADARG;
        }
        if (T.n < 0) { set_error("hnr_adam_plan: tensor %d has a negative element count %lld", i, (long long)T.n); return HNR_ERR_BADARG; }
        if (T.group < 0 || T.group >= n_groups) { set_error("hnr_adam_plan: tensor %d names group %d of %d", i, T.group, n_groups); return HNR_ERR_BADARG; }
        const int64_t nc = (T.n + HNR_ADAM_CHUNK - 1) / HNR_ADAM_CHUNK;
        if (total + nc > INT32_MAX) { set_error("hnr_adam_plan: more than 2^31 - 1 chunks"); return HNR_ERR_TOOBIG; }
        if (chunks) {
            if (total + nc > chunk_cap) { set_error("hnr_adam_plan: the chunk table holds %lld entries, the tensors need more", (long long)chunk_cap); return HNR_ERR_BADARG; }
            for (int64_t c = 0; c < nc; ++c) { chunks[2 * (total + c)] = i; chunks[2 * (total + c) + 1] = (int32_t)c; }
        }
        total += nc;
    }
    return total;
}

extern "C" int hnr_adam_step(int64_t *d_counters, const double *d_groups, int n_groups, double *d_rows, const hnr_adam_tensor *d_tensors, int n_tensors,
                             const int32_t *d_chunks, int64_t n_chunks, void *stream)
{
    // every argument is checked before the first launch: a refused step leaves the counters where they were
    if (check_table("hnr_adam_step", n_tensors, n_groups) != HNR_OK) return HNR_ERR_BADARG;
    if (n_chunks < 0 || n_chunks > INT32_MAX) { set_error("hnr_adam_step: 0 <= n_chunks < 2^31, got %lld", (long long)n_chunks); return HNR_ERR_BADARG; }
    if (!d_counters || !d_groups || !d_rows || !d_tensors || (!d_chunks && n_chunks > 0)) {
        set_error("hnr_adam_step: NULL counters / groups / rows / tensor table / chunk table"); return HNR_ERR_BADARG;
    }
    if ((((uintptr_t)d_counters) | ((uintptr_t)d_groups) | ((uintptr_t)d_rows) | ((uintptr_t)d_tensors)) & 7u) {
        set_error("hnr_adam_step: the counters, groups, rows and the tensor table must be 8-byte aligned"); return HNR_ERR_BADARG;
    }
    if (((uintptr_t)d_chunks) & 3u) { set_error("hnr_adam_step: the chunk table must be 4-byte aligned"); return HNR_ERR_BADARG; }
    const hipStream_t st = (hipStream_t)stream;
    adam_tick_kernel<<<1, 64, 0, st>>>(d_counters, d_groups, n_groups, d_rows);
    HNR_LAUNCH_CHECK();
    if (n_chunks == 0) return HNR_OK;
    adam_update_kernel<<<(unsigned)n_chunks, ADAM_THREADS, 0, st>>>(d_tensors, d_chunks, d_rows, n_tensors, n_groups);
    HNR_LAUNCH_CHECK();
    return HNR_OK;
}
