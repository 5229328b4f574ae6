// ema.hip -- an exponential moving average of the weights, kept and exchanged on the device (mdx/optim.py: WeightEMA), gfx950.
//
// The training step is a replayed hipGraph, so the average cannot be a host-launched torch._foreach_lerp_ with a Python decay: the
// decay's warm-up depends on the number of updates so far, and a step the guard skipped (adam.hip) must not move the average.  Both
// are decided here from two device records.  The work split is adam.hip's: a device table, a {tensor, chunk} block map, 4096
// elements per block of 256 threads, float4 where every pointer of the tensor is 16-byte aligned, a scalar tail otherwise.
//
//   ema_update_kernel   shadow <- lerp(shadow, live, w), w = (float)(1 - d_t), ATen's lerp rule in float32; 12 B per element
//   ema_tick_kernel     one thread, after the last update launch of one update: the counters (every launch saw the same t)
//   ema_swap_kernel     live <-> shadow, bit for bit, in place: the weights' storage then holds the average
#include "mdx_multi_tensor.hpp"

namespace mdx {

struct EmaTensor {
    float *p;                 // the live tensor
    float *e;                 // its shadow: same numel, same dense storage order
    long long n;
};
struct EmaRecord {            // mdx_ema_record_bytes(); zeroed once by the caller
    long long updates;        // updates applied so far: t of the next one
    long long held;           // updates withheld because the guard skipped the step
};

// ATen's lerp (ATen/native/Lerp.h) with self = e, end = p: the form that is exact at the nearer end.
__device__ __forceinline__ float ema_one(float e, float p, float w)
{
    const float diff = p - e;
    return w < 0.5f ? e + w * diff : p - diff * (1.0f - w);
}

__global__ __launch_bounds__(256) void ema_update_kernel(const EmaTensor *__restrict__ tab, int first,
                                                         const int2 *__restrict__ blockmap, double decay, int warmup,
                                                         const EmaRecord *__restrict__ rec, const GuardRecord *__restrict__ guard)
{
    if (guard && guard->skipped) return;
    const long long updates = rec->updates;               // ema_tick_kernel advances it behind the last launch of this update
    double d = decay;
    if (warmup) {
        const double ramp = (1.0 + (double)updates) / (10.0 + (double)updates);
        d = ramp < d ? ramp : d;
    }
    const float w = (float)(1.0 - d);
    const int2 bm = blockmap[blockIdx.x];                 // (tensor of this launch, chunk)
    const EmaTensor t = tab[first + bm.x];
    const long long base = (long long)bm.y * MT_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.e) & 15) == 0);
    constexpr int K = MT_CHUNK / (256 * 4);
    if (vec && base + MT_CHUNK <= t.n) {                 // a whole chunk: every load in flight before the first store
        float4 P[K], E[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            P[k] = *reinterpret_cast<const float4 *>(t.p + i);
            E[k] = *reinterpret_cast<const float4 *>(t.e + i);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            E[k].x = ema_one(E[k].x, P[k].x, w);
            E[k].y = ema_one(E[k].y, P[k].y, w);
            E[k].z = ema_one(E[k].z, P[k].z, w);
            E[k].w = ema_one(E[k].w, P[k].w, w);
            *reinterpret_cast<float4 *>(t.e + i) = E[k];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
        if (i >= t.n) break;
        if (vec && i + 3 < t.n) {
            const float4 P = *reinterpret_cast<const float4 *>(t.p + i);
            float4 E = *reinterpret_cast<const float4 *>(t.e + i);
            E.x = ema_one(E.x, P.x, w);
            E.y = ema_one(E.y, P.y, w);
            E.z = ema_one(E.z, P.z, w);
            E.w = ema_one(E.w, P.w, w);
            *reinterpret_cast<float4 *>(t.e + i) = E;
        } else {
            for (long long j = i; j < i + 4 && j < t.n; ++j) t.e[j] = ema_one(t.e[j], t.p[j], w);
        }
    }
}

__global__ __launch_bounds__(1) void ema_tick_kernel(EmaRecord *__restrict__ rec, const GuardRecord *__restrict__ guard)
{
    if (guard && guard->skipped) rec->held += 1;
    else rec->updates += 1;
}

// Words, not floats: a NaN's payload travels unchanged.
__global__ __launch_bounds__(256) void ema_swap_kernel(const EmaTensor *__restrict__ tab, int first, const int2 *__restrict__ blockmap)
{
    const int2 bm = blockmap[blockIdx.x];
    const EmaTensor t = tab[first + bm.x];
    unsigned int *p = reinterpret_cast<unsigned int *>(t.p), *e = reinterpret_cast<unsigned int *>(t.e);
    const long long base = (long long)bm.y * MT_CHUNK;
    const bool vec = ((((uintptr_t)p | (uintptr_t)e) & 15) == 0);
#pragma unroll
    for (int k = 0; k < MT_CHUNK / (256 * 4); ++k) {
        const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
        if (i >= t.n) break;
        if (vec && i + 3 < t.n) {
            const uint4 P = *reinterpret_cast<const uint4 *>(p + i), E = *reinterpret_cast<const uint4 *>(e + i);
            *reinterpret_cast<uint4 *>(p + i) = E;
            *reinterpret_cast<uint4 *>(e + i) = P;
        } else {
            for (long long j = i; j < i + 4 && j < t.n; ++j) {
                const unsigned int P = p[j], E = e[j];
                p[j] = E;
                e[j] = P;
            }
        }
    }
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_ema_table_entry_bytes(void) { return sizeof(EmaTensor); }
MDX_EXPORT size_t mdx_ema_record_bytes(void) { return sizeof(EmaRecord); }

MDX_EXPORT int mdx_ema_update(const void *table, int first, int count, const void *blockmap, int nblocks, double decay, int warmup,
                              const void *record, const void *guard_record, void *stream)
{
    if (!record) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    if (!(decay >= 0.0 && decay < 1.0)) return MDX_ERR_BAD_SHAPE;                    // a NaN fails both comparisons
    if (!aligned(record, sizeof(long long)) || (guard_record && !aligned(guard_record, sizeof(long long)))) return MDX_ERR_MISALIGNED;
    hipLaunchKernelGGL(ema_update_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const EmaTensor *)table, first,
                       (const int2 *)blockmap, decay, warmup ? 1 : 0, (const EmaRecord *)record, (const GuardRecord *)guard_record);
    return check_launch();
}

MDX_EXPORT int mdx_ema_tick(void *record, const void *guard_record, void *stream)
{
    if (!record) return MDX_ERR_NULL_POINTER;
    if (!aligned(record, sizeof(long long)) || (guard_record && !aligned(guard_record, sizeof(long long)))) return MDX_ERR_MISALIGNED;
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (EmaRecord *)record,
                       (const GuardRecord *)guard_record);
    return check_launch();
}

MDX_EXPORT int mdx_ema_swap(const void *table, int first, int count, const void *blockmap, int nblocks, void *stream)
{
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    hipLaunchKernelGGL(ema_swap_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const EmaTensor *)table, first,
                       (const int2 *)blockmap);
    return check_launch();
}
