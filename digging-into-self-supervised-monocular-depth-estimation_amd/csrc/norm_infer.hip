// norm_infer.hip -- EVAL-mode BatchNorm2d + residual add + ReLU, gfx950.
//
// The operator of norm.hip / norm_nhwc.hip with the running statistics in place of the batch's (model_layer/depth_encoder.py
// BatchNorm2d.act when the module is not training: validation, model_test.inference, any encoder.eval()):
//     y = act(x * s + t [+ res]),   s = gamma / sqrt(running_var + eps),   t = beta - running_mean * s   (per channel)
// One launch, no workspace, no atomics: every thread folds s and t for its own channels from the four float32 vectors
// (1 / sqrt in float64, as the training finalize pass forms invstd) and then streams its rows with the training apply pass's
// one-FMA expression.  Traffic: x [+ res] read once, y written once.
//     channels-last [B][H][W][C]: a thread owns one 16-byte channel vector (nhwc_common.hpp) and walks every PL-th row of
//                                 its block's range, four row loads (per input) in flight
//     planar [B][C][H][W]       : a block owns a span of one (b, c) plane, 16-byte loads, a scalar head / tail where the
//                                 plane does not start or end on a 16-byte boundary; any C, any H * W
#include "nhwc_common.hpp"

namespace mdx {
namespace infer {

using nhwc::bf16;
using nhwc::from_float;
using nhwc::load_vec;
using nhwc::store_vec;
using nhwc::to_float;
using nhwc::Vec;
using nhwc::VecN;

constexpr int NB = nhwc::NB;
constexpr int MAX_BLOCKS = 4096, ITERS = 4;     // channels-last: the training apply pass's grid (norm_nhwc.hip)
constexpr int SPAN = 8192;                      // planar: elements of one plane a block owns

__device__ __forceinline__ void fold(const float *__restrict__ gamma, const float *__restrict__ beta,
                                     const float *__restrict__ mean, const float *__restrict__ var, float eps, int c,
                                     float &scale, float &shift)
{
    const float invstd = (float)(1.0 / sqrt((double)var[c] + (double)eps));
    scale = gamma[c] * invstd;
    shift = beta[c] - mean[c] * scale;
}

__device__ __forceinline__ float act(float v, float scale, float shift, float r, bool has_res, int relu)
{
    float f = __builtin_fmaf(v, scale, shift);
    if (has_res) f += r;
    return (relu && f < 0.f) ? 0.f : f;
}

// ---- channels-last ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NB) void bn_infer_nhwc_kernel(const T *__restrict__ x, const T *__restrict__ res,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ mean, const float *__restrict__ var,
                                                           float eps, int M, int C, int CVB, int PL, int RB, int relu,
                                                           T *__restrict__ y)
{
    constexpr int N = VecN<T>::N;
    const nhwc::Pos p = nhwc::position<N>(M, C, CVB, PL, RB);
    if (!p.active) return;
    float scale[N], shift[N];
#pragma unroll
    for (int j = 0; j < N; ++j) fold(gamma, beta, mean, var, eps, p.cv * N + j, scale[j], shift[j]);
    const size_t base = (size_t)p.cv * N;
    const T *px = x + base;
    const T *pr = res ? res + base : nullptr;
    T *py = y + base;
    auto apply = [&](const Vec<T, N> &v, const Vec<T, N> &rv, size_t off) {
        Vec<T, N> w;
#pragma unroll
        for (int j = 0; j < N; ++j) w.v[j] = from_float<T>(act(to_float(v.v[j]), scale[j], shift[j], to_float(rv.v[j]), pr, relu));
        store_vec<T, N>(py + off, w);
    };
    int r = p.r0 + p.pl;
    for (; r + 3 * PL < p.r1; r += 4 * PL) {
        const size_t o0 = (size_t)r * C, o1 = (size_t)(r + PL) * C, o2 = (size_t)(r + 2 * PL) * C, o3 = (size_t)(r + 3 * PL) * C;
        const Vec<T, N> v0 = load_vec<T, N>(px + o0), v1 = load_vec<T, N>(px + o1), v2 = load_vec<T, N>(px + o2), v3 = load_vec<T, N>(px + o3);
        Vec<T, N> r0 = {}, r1 = {}, r2 = {}, r3 = {};
        if (pr) { r0 = load_vec<T, N>(pr + o0); r1 = load_vec<T, N>(pr + o1); r2 = load_vec<T, N>(pr + o2); r3 = load_vec<T, N>(pr + o3); }
        apply(v0, r0, o0); apply(v1, r1, o1); apply(v2, r2, o2); apply(v3, r3, o3);
    }
    for (; r < p.r1; r += PL) {
        const size_t o = (size_t)r * C;
        Vec<T, N> rv = {};
        if (pr) rv = load_vec<T, N>(pr + o);
        apply(load_vec<T, N>(px + o), rv, o);
    }
}

// ---- planar -----------------------------------------------------------------------------------------------------------
// grid (B * C planes, spans of SPAN elements).  vec: x, res and y lie at the same offset modulo 16 bytes (the host checks), so one
// head length brings all three onto a 16-byte boundary; otherwise every element goes the scalar way.
template <typename T>
__global__ __launch_bounds__(NB) void bn_infer_planar_kernel(const T *__restrict__ x, const T *__restrict__ res,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             const float *__restrict__ mean, const float *__restrict__ var,
                                                             float eps, int C, int HW, int relu, int vec, T *__restrict__ y)
{
    constexpr int N = VecN<T>::N;
    const size_t plane = blockIdx.x;
    float scale, shift;
    fold(gamma, beta, mean, var, eps, (int)(plane % C), scale, shift);
    const size_t base = plane * HW;
    const T *px = x + base;
    const T *pr = res ? res + base : nullptr;
    T *py = y + base;
    const int s0 = blockIdx.y * SPAN, s1 = min(HW, s0 + SPAN);
    auto one = [&](int i) {
        py[i] = from_float<T>(act(to_float(px[i]), scale, shift, pr ? to_float(pr[i]) : 0.f, pr, relu));
    };
    int a = s1, b = s1;                     // [a, b): the 16-byte vectors of the span
    if (vec) {
        const int head = (int)((16 - ((uintptr_t)(px + s0) & 15)) & 15) / (int)sizeof(T);
        a = min(s1, s0 + head);
        b = a + (s1 - a) / N * N;
    }
    for (int i = s0 + (int)threadIdx.x; i < a; i += NB) one(i);
    for (int i = b + (int)threadIdx.x; i < s1; i += NB) one(i);
    const int nv = (b - a) / N;
    auto apply = [&](const Vec<T, N> &v, const Vec<T, N> &rv, int off) {
        Vec<T, N> w;
#pragma unroll
        for (int j = 0; j < N; ++j) w.v[j] = from_float<T>(act(to_float(v.v[j]), scale, shift, to_float(rv.v[j]), pr, relu));
        store_vec<T, N>(py + off, w);
    };
    int k = threadIdx.x;
    for (; k + 3 * NB < nv; k += 4 * NB) {
        const int o0 = a + k * N, o1 = o0 + NB * N, o2 = o1 + NB * N, o3 = o2 + NB * N;
        const Vec<T, N> v0 = load_vec<T, N>(px + o0), v1 = load_vec<T, N>(px + o1), v2 = load_vec<T, N>(px + o2), v3 = load_vec<T, N>(px + o3);
        Vec<T, N> r0 = {}, r1 = {}, r2 = {}, r3 = {};
        if (pr) { r0 = load_vec<T, N>(pr + o0); r1 = load_vec<T, N>(pr + o1); r2 = load_vec<T, N>(pr + o2); r3 = load_vec<T, N>(pr + o3); }
        apply(v0, r0, o0); apply(v1, r1, o1); apply(v2, r2, o2); apply(v3, r3, o3);
    }
    for (; k < nv; k += NB) {
        const int o = a + k * N;
        Vec<T, N> rv = {};
        if (pr) rv = load_vec<T, N>(pr + o);
        apply(load_vec<T, N>(px + o), rv, o);
    }
}

}  // namespace infer
}  // namespace mdx

// ---- mdx_bn_act_*infer_abi ----------------------------------------------------------------------------------------------
using namespace mdx;
using namespace mdx::infer;

MDX_EXPORT int mdx_bn_act_infer(const void *x, const void *res, const float *gamma, const float *beta, const float *run_mean,
                                const float *run_var, void *y, int B, int C, int H, int W, float eps, int relu, int dtype,
                                void *stream)
{
    if (!x || !gamma || !beta || !run_mean || !run_var || !y) return MDX_ERR_NULL_POINTER;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return MDX_ERR_BAD_SHAPE;
    if ((long long)H * W >= (1ll << 31) || (long long)B * C >= (1ll << 31)) return MDX_ERR_BAD_SHAPE;
    const int HW = H * W, spans = (HW + SPAN - 1) / SPAN;
    if (spans > 65535) return MDX_ERR_BAD_SHAPE;
    const size_t es = elem_bytes(dtype);
    if (!aligned(x, es) || !aligned(y, es) || (res && !aligned(res, es))) return MDX_ERR_MISALIGNED;
    const uintptr_t mx = (uintptr_t)x & 15;
    const int vec = ((uintptr_t)y & 15) == mx && (!res || ((uintptr_t)res & 15) == mx);
    const dim3 grid((unsigned)(B * C), spans), block(NB);
    hipStream_t st = (hipStream_t)stream;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((bn_infer_planar_kernel<T>), grid, block, 0, st, (const T *)x, (const T *)res, gamma, beta, run_mean,
                           run_var, eps, C, HW, relu, vec, (T *)y);
    });
    return check_launch();
}

MDX_EXPORT int mdx_bn_act_nhwc_infer(const void *x, const void *res, const float *gamma, const float *beta, const float *run_mean,
                                     const float *run_var, void *y, int B, int C, int H, int W, float eps, int relu, int dtype,
                                     void *stream)
{
    if (!x || !gamma || !beta || !run_mean || !run_var || !y) return MDX_ERR_NULL_POINTER;
    const int bad = nhwc_map_ok(B, C, H, W, dtype);
    if (bad) return bad;
    if (!aligned(x, 16) || !aligned(y, 16) || (res && !aligned(res, 16))) return MDX_ERR_MISALIGNED;
    const int M = B * H * W, N = vec_elems(dtype);
    const nhwc::Rows g = nhwc::make_rows(M, C, N, MAX_BLOCKS, ITERS);
    const dim3 grid(g.nblk, g.t.ny), block(NB);
    hipStream_t st = (hipStream_t)stream;
    dispatch_dtype(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((bn_infer_nhwc_kernel<T>), grid, block, 0, st, (const T *)x, (const T *)res, gamma, beta, run_mean,
                           run_var, eps, M, C, g.t.CVB, g.t.PL, g.RB, relu, (T *)y);
    });
    return check_launch();
}
