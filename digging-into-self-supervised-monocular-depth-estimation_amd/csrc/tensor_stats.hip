// tensor_stats.hip -- per-tensor gradient and weight statistics, computed on the device (mdx/optim.py: GradStats), gfx950.
//
// The step guard knows ONE norm; when it goes to infinity, or clips every step, nothing says which layer did it.  One read-only pass
// over every trained parameter and its gradient gives each tensor a record -- the two sums of squares, the two largest magnitudes,
// counts of non-finite and of zero elements -- and a history entry that stays on the device, so that a run checked at every step
// still reads the host once per epoch.  The work split is adam.hip's: a device table, gradient pointers as kernel arguments (they
// change from step to step), a {tensor, chunk} block map, 4096 elements per block of 256 threads, float4 where the pointers are
// 16-byte aligned and the chunk is whole, a scalar path otherwise and for a tensor's tail.
//
// Two launches, ordered by the stream alone: every block's partial record into the block's own slot, then one block per tensor adds
// that tensor's slots in a fixed order.  No atomics and nothing to clear -- every slot, record and history entry the pass owns is
// overwritten (or advanced) by exactly one thread -- so the same inputs give the same bits at every launch and a replayed graph has
// no state of its own (LABNOTES, "hipMemsetAsync inside a captured graph").
#include "mdx_multi_tensor.hpp"

namespace mdx {

struct StatsTensor {
    const float *w;           // the parameter's dense storage
    long long n;
};
static_assert(sizeof(StatsTensor) == 16, "the statistics' table entry is 16 bytes (include/mdx.h)");

// One record: a tensor's (mdx_tensor_stats) and, with the same fields over one chunk, a block's partial.
struct StatsRecord {
    double grad_sumsq, weight_sumsq;          // over finite elements
    float grad_absmax, weight_absmax;         // over finite elements; 0 when there is none
    uint32_t grad_nonfinite, weight_nonfinite, grad_zeros;
    uint32_t grad_present;
};
static_assert(sizeof(StatsRecord) == sizeof(mdx_tensor_stats) && sizeof(StatsRecord) == 40, "include/mdx.h: mdx_tensor_stats");
static_assert(sizeof(mdx_tensor_stats_history) == 56, "include/mdx.h: mdx_tensor_stats_history");

// What a thread carries.  The magnitudes as the bits of |x|: among finite floats the order of the bits is the order of the values,
// denormals included, whatever the denormal mode.  The counts of one block fit 16 bits (<= 4096 each), the counts of a tensor are
// taken modulo 2^32 (include/mdx.h).
struct StatsAcc {
    double gsum = 0.0, wsum = 0.0;
    uint32_t gmax = 0, wmax = 0;
    uint32_t gnf = 0, wnf = 0, gz = 0;
};

__device__ __forceinline__ void stats_grad(StatsAcc &a, float x)
{
    const uint32_t mag = __float_as_uint(x) & 0x7FFFFFFFu;
    const bool finite = (mag & 0x7F800000u) != 0x7F800000u;        // from the exponent bits: Inf and every NaN payload
    a.gsum += finite ? (double)x * (double)x : 0.0;                 // the product of two floats is exact in double
    a.gmax = finite && mag > a.gmax ? mag : a.gmax;
    a.gnf += finite ? 0u : 1u;
    a.gz += mag == 0u ? 1u : 0u;                                   // +0 and -0
}

__device__ __forceinline__ void stats_weight(StatsAcc &a, float x)
{
    const uint32_t mag = __float_as_uint(x) & 0x7FFFFFFFu;
    const bool finite = (mag & 0x7F800000u) != 0x7F800000u;
    a.wsum += finite ? (double)x * (double)x : 0.0;
    a.wmax = finite && mag > a.wmax ? mag : a.wmax;
    a.wnf += finite ? 0u : 1u;
}

// 256 threads: wave shuffles, four LDS slots, a fixed order.  The result is valid in thread 0.
struct StatsLds { double gsum[4], wsum[4]; uint32_t gmax[4], wmax[4], gnf[4], wnf[4], gz[4]; };

__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ void stats_block_reduce(StatsAcc &a, StatsLds &lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.gsum += __shfl_down(a.gsum, off, 64);
        a.wsum += __shfl_down(a.wsum, off, 64);
        a.gmax = umax(a.gmax, __shfl_down(a.gmax, off, 64));
        a.wmax = umax(a.wmax, __shfl_down(a.wmax, off, 64));
        a.gnf += __shfl_down(a.gnf, off, 64);
        a.wnf += __shfl_down(a.wnf, off, 64);
        a.gz += __shfl_down(a.gz, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        lds.gsum[wv] = a.gsum; lds.wsum[wv] = a.wsum;
        lds.gmax[wv] = a.gmax; lds.wmax[wv] = a.wmax;
        lds.gnf[wv] = a.gnf; lds.wnf[wv] = a.wnf; lds.gz[wv] = a.gz;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.gsum = ((lds.gsum[0] + lds.gsum[1]) + lds.gsum[2]) + lds.gsum[3];
        a.wsum = ((lds.wsum[0] + lds.wsum[1]) + lds.wsum[2]) + lds.wsum[3];
        a.gmax = umax(umax(lds.gmax[0], lds.gmax[1]), umax(lds.gmax[2], lds.gmax[3]));
        a.wmax = umax(umax(lds.wmax[0], lds.wmax[1]), umax(lds.wmax[2], lds.wmax[3]));
        a.gnf = ((lds.gnf[0] + lds.gnf[1]) + lds.gnf[2]) + lds.gnf[3];
        a.wnf = ((lds.wnf[0] + lds.wnf[1]) + lds.wnf[2]) + lds.wnf[3];
        a.gz = ((lds.gz[0] + lds.gz[1]) + lds.gz[2]) + lds.gz[3];
    }
}

__device__ __forceinline__ void stats_store(StatsRecord *__restrict__ out, const StatsAcc &a, uint32_t present)
{
    StatsRecord r;
    r.grad_sumsq = a.gsum; r.weight_sumsq = a.wsum;
    r.grad_absmax = __uint_as_float(a.gmax); r.weight_absmax = __uint_as_float(a.wmax);
    r.grad_nonfinite = a.gnf; r.weight_nonfinite = a.wnf; r.grad_zeros = a.gz;
    r.grad_present = present;
    *out = r;
}

// Pass 1.  Block b of the launch: chunk bm.y of tensor first + bm.x -> partials[b].  A NULL gradient pointer (a parameter that
// received no gradient this step): the weight half alone, and the partial says "gradient absent".
__global__ __launch_bounds__(256) void tensor_stats_partials_kernel(const StatsTensor *__restrict__ tab, GradPointers grads, int first,
                                                                    const int2 *__restrict__ blockmap, StatsRecord *__restrict__ partials)
{
    __shared__ StatsLds lds;
    const int2 bm = blockmap[blockIdx.x];                 // (tensor of this launch, chunk)
    const StatsTensor t = tab[first + bm.x];
    const float *__restrict__ g = grads.g[bm.x];
    const long long base = (long long)bm.y * MT_CHUNK;
    constexpr int K = MT_CHUNK / (256 * 4);
    StatsAcc a;
    if (((((uintptr_t)t.w) | ((uintptr_t)g)) & 15) == 0 && base + MT_CHUNK <= t.n) {     // whole and aligned: every load in flight first
        float4 W[K], G[K];
#pragma unroll
        for (int k = 0; k < K; ++k) W[k] = *reinterpret_cast<const float4 *>(t.w + base + ((long long)k * 256 + threadIdx.x) * 4);
        if (g) {
#pragma unroll
            for (int k = 0; k < K; ++k) G[k] = *reinterpret_cast<const float4 *>(g + base + ((long long)k * 256 + threadIdx.x) * 4);
#pragma unroll
            for (int k = 0; k < K; ++k) { stats_grad(a, G[k].x); stats_grad(a, G[k].y); stats_grad(a, G[k].z); stats_grad(a, G[k].w); }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) { stats_weight(a, W[k].x); stats_weight(a, W[k].y); stats_weight(a, W[k].z); stats_weight(a, W[k].w); }
    } else {
        for (int k = 0; k < K; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            for (long long j = i; j < i + 4 && j < t.n; ++j) {
                if (g) stats_grad(a, g[j]);
                stats_weight(a, t.w[j]);
            }
        }
    }
    stats_block_reduce(a, lds);
    if (threadIdx.x == 0) stats_store(partials + blockIdx.x, a, g ? 1u : 0u);
}

// Pass 2.  Block b: tensor first + b, whose partials are slots offsets[first + b] .. offsets[first + b + 1] - 1 of the WHOLE partials
// buffer.  Thread t takes slots lo + t, lo + t + 256, ...; then the fixed tree of stats_block_reduce.  Thread 0 writes the record and
// advances the tensor's history entry.
__global__ __launch_bounds__(256) void tensor_stats_finish_kernel(int first, const int *__restrict__ offsets,
                                                                  const StatsRecord *__restrict__ partials,
                                                                  StatsRecord *__restrict__ records,
                                                                  mdx_tensor_stats_history *__restrict__ history)
{
    __shared__ StatsLds lds;
    const int t = first + blockIdx.x;
    const int lo = offsets[t], hi = offsets[t + 1];
    StatsAcc a;
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        const StatsRecord p = partials[i];
        a.gsum += p.grad_sumsq; a.wsum += p.weight_sumsq;
        a.gmax = umax(a.gmax, __float_as_uint(p.grad_absmax)); a.wmax = umax(a.wmax, __float_as_uint(p.weight_absmax));
        a.gnf += p.grad_nonfinite; a.wnf += p.weight_nonfinite; a.gz += p.grad_zeros;
    }
    stats_block_reduce(a, lds);
    if (threadIdx.x != 0) return;
    const uint32_t present = lo < hi ? partials[lo].grad_present : 0u;      // one pointer per tensor: every slot says the same
    stats_store(records + t, a, present);
    if (!history) return;
    mdx_tensor_stats_history h = history[t];
    h.passes += 1;
    if (a.gnf > 0) {
        h.bad_passes += 1;
        if (h.first_bad_pass == 0) h.first_bad_pass = h.passes;
        h.last_bad_pass = h.passes;
    }
    if (a.wnf > 0 && h.first_bad_weight_pass == 0) h.first_bad_weight_pass = h.passes;
    if (present && a.gsum > h.max_grad_sumsq) {
        h.max_grad_sumsq = a.gsum;
        h.max_grad_pass = h.passes;
    }
    history[t] = h;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_tensor_stats_table_entry_bytes(void) { return sizeof(StatsTensor); }
MDX_EXPORT size_t mdx_tensor_stats_partial_bytes(void) { return sizeof(StatsRecord); }
MDX_EXPORT size_t mdx_tensor_stats_record_bytes(void) { return sizeof(mdx_tensor_stats); }
MDX_EXPORT size_t mdx_tensor_stats_history_bytes(void) { return sizeof(mdx_tensor_stats_history); }

MDX_EXPORT int mdx_tensor_stats_partials(const void *table, int first, int count, const float *const *grads, const void *blockmap,
                                         int nblocks, void *partials, void *stream)
{
    if (!grads || !partials) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    if (!aligned(partials, sizeof(double))) return MDX_ERR_MISALIGNED;
    GradPointers G;
    fill_grads(G, grads, count, true);                                  // NULL: no gradient for this tensor in this pass
    hipLaunchKernelGGL(tensor_stats_partials_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const StatsTensor *)table, G,
                       first, (const int2 *)blockmap, (StatsRecord *)partials);
    return check_launch();
}

MDX_EXPORT int mdx_tensor_stats_finish(int first, int count, const int *offsets, const void *partials, void *records, void *history,
                                       void *stream)
{
    if (!offsets || !partials || !records) return MDX_ERR_NULL_POINTER;
    if (first < 0 || count < 1 || count > MT_MAX_TENSORS) return MDX_ERR_BAD_SHAPE;
    if (!aligned(partials, sizeof(double)) || !aligned(records, sizeof(double)) || !aligned(history, sizeof(double)))
        return MDX_ERR_MISALIGNED;
    hipLaunchKernelGGL(tensor_stats_finish_kernel, dim3(count), dim3(256), 0, (hipStream_t)stream, first, offsets,
                       (const StatsRecord *)partials, (StatsRecord *)records, (mdx_tensor_stats_history *)history);
    return check_launch();
}
