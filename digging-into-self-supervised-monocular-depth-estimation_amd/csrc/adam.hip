// adam.hip -- the optimiser step of the training loop (reference model_tool/loader.py:93-97: torch.optim.Adam), gfx950.
//
// torch.optim.Adam(fused=True) walks its tensor lists with multi_tensor_apply: at most 320 blocks of 512 threads per launch, each
// looping over a 65536-element chunk -- five launches of 54 us for the 27.8 M parameters of the two ResNet-18 networks, 3 TB/s, at
// the one point of a step where nothing else can run.  Here the step is ONE launch: a block owns 4096 elements of one tensor
// (7000 blocks), reads parameter, gradient and both moments once and writes the three that change.  The arithmetic is
// fused_adam_utils.cuh's expression by expression, including where it is carried out in double (beta * moment, lr / bias
// correction, + eps): the results agree with torch's kernel to the last bit wherever its compiler did not contract a
// multiply-add, and to an ulp otherwise.
#include "mdx_multi_tensor.hpp"

namespace mdx {

struct AdamTensor {
    float *p, *m, *v;
    const float *step;        // this tensor's step count (float32, already incremented for this step)
    long long n;
};

__device__ __forceinline__ void adam_one(float &param, float grad, float &exp_avg, float &exp_avg_sq, double beta1, double beta2,
                                         double eps, float step_size, float bias_correction2_sqrt)
{
    exp_avg = (float)(beta1 * exp_avg + (1 - beta1) * grad);
    exp_avg_sq = (float)(beta2 * exp_avg_sq + (1 - beta2) * grad * grad);
    const float denom = (float)((sqrtf(exp_avg_sq) / bias_correction2_sqrt) + eps);
    param -= step_size * exp_avg / denom;
}

// One block's work of the step.  GUARDED: the launch returns at once when the record says "skipped", and Adam consumes
// grad * coef (one float32 multiply, rounded before Adam's own arithmetic); coef == 1.0f leaves every gradient its bits.
template <bool GUARDED>
__device__ __forceinline__ void adam_step_block(const AdamTensor *__restrict__ tab, const GradPointers &grads, int first,
                                                const int2 *__restrict__ blockmap, const float *__restrict__ lr_ptr, double lr,
                                                double beta1, double beta2, double eps, const GuardRecord *__restrict__ rec)
{
    float coef = 1.0f;
    if (GUARDED) {
        if (rec->skipped) return;
        coef = rec->coef;
    }
    const int2 bm = blockmap[blockIdx.x];                 // (tensor of this launch, chunk)
    const AdamTensor t = tab[first + bm.x];
    const float *__restrict__ g = grads.g[bm.x];
    const float step_count = *t.step;
    const double bc1 = 1 - pow(beta1, (double)step_count);
    const double bc2 = 1 - pow(beta2, (double)step_count);
    const float bias_correction1 = (float)bc1, bias_correction2_sqrt = (float)sqrt(bc2);
    const double lr_double = lr_ptr ? (double)*lr_ptr : lr;
    const float step_size = (float)(lr_double / bias_correction1);
    const long long base = (long long)bm.y * MT_CHUNK;
    const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.m | (uintptr_t)t.v | (uintptr_t)g) & 15) == 0);
#pragma unroll
    for (int k = 0; k < MT_CHUNK / (256 * 4); ++k) {
        const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
        if (i >= t.n) break;
        if (vec && i + 3 < t.n) {
            float4 P = *reinterpret_cast<const float4 *>(t.p + i), G = *reinterpret_cast<const float4 *>(g + i);
            float4 M = *reinterpret_cast<const float4 *>(t.m + i), V = *reinterpret_cast<const float4 *>(t.v + i);
            if (GUARDED) { G.x *= coef; G.y *= coef; G.z *= coef; G.w *= coef; }
            adam_one(P.x, G.x, M.x, V.x, beta1, beta2, eps, step_size, bias_correction2_sqrt);
            adam_one(P.y, G.y, M.y, V.y, beta1, beta2, eps, step_size, bias_correction2_sqrt);
            adam_one(P.z, G.z, M.z, V.z, beta1, beta2, eps, step_size, bias_correction2_sqrt);
            adam_one(P.w, G.w, M.w, V.w, beta1, beta2, eps, step_size, bias_correction2_sqrt);
            *reinterpret_cast<float4 *>(t.p + i) = P;
            *reinterpret_cast<float4 *>(t.m + i) = M;
            *reinterpret_cast<float4 *>(t.v + i) = V;
        } else {
            for (long long j = i; j < i + 4 && j < t.n; ++j) {
                float P = t.p[j], M = t.m[j], V = t.v[j];
                adam_one(P, GUARDED ? g[j] * coef : g[j], M, V, beta1, beta2, eps, step_size, bias_correction2_sqrt);
                t.p[j] = P; t.m[j] = M; t.v[j] = V;
            }
        }
    }
}

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamTensor *__restrict__ tab, GradPointers grads, int first,
                                                        const int2 *__restrict__ blockmap, const float *__restrict__ lr_ptr, double lr,
                                                        double beta1, double beta2, double eps)
{
    adam_step_block<false>(tab, grads, first, blockmap, lr_ptr, lr, beta1, beta2, eps, nullptr);
}

// ---- the step guard: global-norm clip, skip of a non-finite step -------------------------------------------------------------
// Three launches, ordered by the stream alone (no block waits for another, no atomics): every block's sum of squares into its own
// slot; one block adds the slots in a fixed order, writes the record and advances the step counters; the guarded Adam reads it.

__device__ __forceinline__ double block_sum(double acc, double *lds)      // 256 threads; the result is valid in thread 0
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

// Same table, block map and gradient pointers as adam_step_kernel; partials[blockIdx.x] = the sum of g^2 over this block's chunk.
// Squares and sums in double: 1e30 squared overflows float32 and must not read as non-finite.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamTensor *__restrict__ tab, GradPointers grads, int first,
                                                         const int2 *__restrict__ blockmap, double *__restrict__ partials)
{
    __shared__ double lds[4];
    const int2 bm = blockmap[blockIdx.x];
    const long long n = tab[first + bm.x].n;
    const float *__restrict__ g = grads.g[bm.x];
    const long long base = (long long)bm.y * MT_CHUNK;
    constexpr int K = MT_CHUNK / (256 * 4);
    double acc = 0.0;
    if ((((uintptr_t)g) & 15) == 0 && base + MT_CHUNK <= n) {
        float4 G[K];
#pragma unroll
        for (int k = 0; k < K; ++k) G[k] = *reinterpret_cast<const float4 *>(g + base + ((long long)k * 256 + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < K; ++k) acc += ((sq(G[k].x) + sq(G[k].y)) + sq(G[k].z)) + sq(G[k].w);
    } else {
        for (int k = 0; k < K; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            for (long long j = i; j < i + 4 && j < n; ++j) acc += sq(g[j]);
        }
    }
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// One block.  Adds the partials (thread t takes t, t + 256, ...; then the fixed tree of block_sum), writes the record and, unless the
// step is skipped, advances every tensor's step count -- what torch._foreach_add_(steps, 1) does in front of the unguarded step.
__global__ __launch_bounds__(256) void guard_finish_kernel(const AdamTensor *__restrict__ tab, int ntensors,
                                                           const double *__restrict__ partials, int npartials, float max_grad_norm,
                                                           int skip_nonfinite, GuardRecord *__restrict__ rec)
{
    __shared__ double lds[4];
    __shared__ int skip;
    double acc = 0.0;
    for (int i = threadIdx.x; i < npartials; i += 256) acc += partials[i];
    acc = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(acc);
        float coef = 1.0f;
        if (max_grad_norm > 0.0f) {
            const float c = max_grad_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;                       // a NaN stays a NaN, as under torch.clamp(max=1)
        }
        const int skipped = (skip_nonfinite && !isfinite(norm)) ? 1 : 0;
        rec->total_norm = norm;
        rec->coef = coef;
        rec->skipped = skipped;
        rec->reserved = 0;
        rec->steps += 1;
        rec->skipped_steps += skipped;
        skip = skipped;
    }
    __syncthreads();
    if (skip) return;
    for (int i = threadIdx.x; i < ntensors; i += 256) *const_cast<float *>(tab[i].step) += 1.0f;
}

__global__ __launch_bounds__(256) void adam_step_guarded_kernel(const AdamTensor *__restrict__ tab, GradPointers grads, int first,
                                                                const int2 *__restrict__ blockmap, const float *__restrict__ lr_ptr,
                                                                double lr, double beta1, double beta2, double eps,
                                                                const GuardRecord *__restrict__ rec)
{
    adam_step_block<true>(tab, grads, first, blockmap, lr_ptr, lr, beta1, beta2, eps, rec);
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT int mdx_adam_max_tensors(void) { return MT_MAX_TENSORS; }
MDX_EXPORT int mdx_adam_chunk(void) { return MT_CHUNK; }
MDX_EXPORT size_t mdx_adam_table_entry_bytes(void) { return sizeof(AdamTensor); }

// table: DEVICE array of {float *param, *exp_avg, *exp_avg_sq; const float *step; int64 numel} (mdx_adam_table_entry_bytes() each);
// this launch takes entries first .. first + count - 1 (count <= mdx_adam_max_tensors()); grads: HOST array of count device
// pointers; blockmap: DEVICE array of nblocks {int32 tensor (0-based within the launch), int32 chunk} covering every tensor in
// chunks of mdx_adam_chunk() elements; lr_ptr: device float32 (a captured step's learning rate) or NULL (then lr).
// Adam without weight decay, amsgrad or maximize -- what the reference configures (loader.py:93-95).
MDX_EXPORT int mdx_adam_step(const void *table, int first, int count, const float *const *grads, const void *blockmap, int nblocks,
                             const float *lr_ptr, double lr, double beta1, double beta2, double eps, void *stream)
{
    if (!grads) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    GradPointers G;
    if (int rc = fill_grads(G, grads, count, false)) return rc;
    hipLaunchKernelGGL(adam_step_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const AdamTensor *)table, G, first,
                       (const int2 *)blockmap, lr_ptr, lr, beta1, beta2, eps);
    return check_launch();
}

// ---- the guarded step (include/mdx.h) ----
MDX_EXPORT size_t mdx_adam_guard_record_bytes(void) { return sizeof(GuardRecord); }
MDX_EXPORT size_t mdx_adam_guard_partials_bytes(int nblocks) { return nblocks < 1 ? 0 : (size_t)nblocks * sizeof(double); }

MDX_EXPORT int mdx_adam_grad_sumsq(const void *table, int first, int count, const float *const *grads, const void *blockmap,
                                   int nblocks, double *partials, void *stream)
{
    if (!grads || !partials) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    if (!aligned(partials, sizeof(double))) return MDX_ERR_MISALIGNED;
    GradPointers G;
    if (int rc = fill_grads(G, grads, count, false)) return rc;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const AdamTensor *)table, G, first,
                       (const int2 *)blockmap, partials);
    return check_launch();
}

MDX_EXPORT int mdx_adam_guard_finish(const void *table, int ntensors, const double *partials, int npartials, double max_grad_norm,
                                     int skip_nonfinite, void *record, void *stream)
{
    if (!table || !partials || !record) return MDX_ERR_NULL_POINTER;
    if (ntensors < 1 || npartials < 1 || max_grad_norm != max_grad_norm) return MDX_ERR_BAD_SHAPE;
    if (!aligned(partials, sizeof(double)) || !aligned(record, sizeof(long long))) return MDX_ERR_MISALIGNED;
    hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const AdamTensor *)table, ntensors, partials,
                       npartials, (float)max_grad_norm, skip_nonfinite ? 1 : 0, (GuardRecord *)record);
    return check_launch();
}

MDX_EXPORT int mdx_adam_step_guarded(const void *table, int first, int count, const float *const *grads, const void *blockmap,
                                     int nblocks, const float *lr_ptr, double lr, double beta1, double beta2, double eps,
                                     const void *record, void *stream)
{
    if (!grads || !record) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    if (!aligned(record, sizeof(long long))) return MDX_ERR_MISALIGNED;
    GradPointers G;
    if (int rc = fill_grads(G, grads, count, false)) return rc;
    hipLaunchKernelGGL(adam_step_guarded_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const AdamTensor *)table, G, first,
                       (const int2 *)blockmap, lr_ptr, lr, beta1, beta2, eps, (const GuardRecord *)record);
    return check_launch();
}
