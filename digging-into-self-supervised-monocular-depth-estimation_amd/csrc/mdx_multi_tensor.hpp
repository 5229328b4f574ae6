// mdx_multi_tensor.hpp -- what the multi-tensor passes share: adam.hip, ema.hip, digest.hip, tensor_stats.hip (mdx/optim.py).
//
// A PLAN is a device table of {pointers..., numel} entries (each file's own struct) and, per launch, the entries first .. first +
// count - 1 of it with a device block map of nblocks {int32 tensor (0-based within the launch), int32 chunk} pairs: one block of
// 256 threads per MT_CHUNK elements of one tensor, at most MT_MAX_TENSORS tensors per launch.
#pragma once
#include <stddef.h>
#include "mdx_common.hpp"

namespace mdx {

constexpr int MT_MAX_TENSORS = 384;          // mdx_adam_max_tensors()
constexpr int MT_CHUNK = 4096;               // mdx_adam_chunk(): 256 threads x 4 float4

// Gradient pointers travel as kernel arguments (they change from step to step); entries past the launch's count are NULL.
struct GradPointers { const float *g[MT_MAX_TENSORS]; };

// The step guard's device record (mdx_adam_guard_record_bytes()): written by adam.hip's guard_finish_kernel, read by its guarded
// step, by ema.hip (`skipped` alone) and, on request, by the host (mdx.optim.Adam.guard_stats).
struct GuardRecord {
    float total_norm;         // L2 norm of every gradient of the step: sum of squares in double, rounded once
    float coef;               // min(1, max_grad_norm / (total_norm + 1e-6)) in float32; exactly 1 without a limit
    int skipped;              // 1: total_norm was not finite and the step wrote nothing
    int reserved;
    long long steps;          // guarded steps so far, skipped ones included
    long long skipped_steps;
};
static_assert(sizeof(GuardRecord) == 32 && offsetof(GuardRecord, skipped) == 8, "the step guard's record (include/mdx.h)");

// The refusal every entry point that takes a plan shares: null, then shape.
static inline int check_plan(const void *table, int first, int count, const void *blockmap, int nblocks)
{
    if (!table || !blockmap) return MDX_ERR_NULL_POINTER;
    if (first < 0 || count < 1 || count > MT_MAX_TENSORS || nblocks < 1) return MDX_ERR_BAD_SHAPE;
    return MDX_OK;
}

// allow_null: a NULL entry is "no gradient for this tensor in this pass" (tensor_stats.hip); Adam refuses it.
static inline int fill_grads(GradPointers &G, const float *const *grads, int count, bool allow_null)
{
    for (int i = 0; i < count; ++i) {
        if (!grads[i] && !allow_null) return MDX_ERR_NULL_POINTER;
        G.g[i] = grads[i];
    }
    for (int i = count; i < MT_MAX_TENSORS; ++i) G.g[i] = nullptr;
    return MDX_OK;
}

}  // namespace mdx
