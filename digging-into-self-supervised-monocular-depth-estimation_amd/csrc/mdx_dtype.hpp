// mdx_dtype.hpp -- the storage types of the network kernels (norm*.hip, glue*.hip, *_head_nhwc.hip) and the host-side dispatch on
// their dtype codes: one place for the codes, the bfloat16 type with its conversions, and the "which instantiation" decision
// every entry point makes on `void *` arguments.
#pragma once
#include "mdx_common.hpp"
#include <stdint.h>
#include <type_traits>

namespace mdx {

enum { MDX_F32 = 0, MDX_BF16 = 1 };            // the dtype codes include/mdx.h documents

struct bf16 { uint16_t v; };                   // storage only: arithmetic is float32

__device__ __forceinline__ float to_float(float x) { return x; }
__device__ __forceinline__ float to_float(bf16 x) { return __uint_as_float((uint32_t)x.v << 16); }

// float -> T, round to nearest even, NaN stays NaN (torch's float -> bfloat16).  Two forms of the same rounding:
template <typename T> __device__ __forceinline__ T from_float_cvt(float x);
template <typename T> __device__ __forceinline__ T from_float_int(float x);
template <> __device__ __forceinline__ float from_float_cvt<float>(float x) { return x; }
template <> __device__ __forceinline__ float from_float_int<float>(float x) { return x; }
// the channels-last kernels and norm_infer.hip: gfx950's v_cvt_pk_bf16_f32, one instruction (the integer form made their bfloat16 apply passes VALU-bound)
template <> __device__ __forceinline__ bf16 from_float_cvt<bf16>(float x)
{
    bf16 r;
    r.v = __builtin_bit_cast(uint16_t, (__bf16)x);
    return r;
}
// the planar kernels (norm.hip, glue.hip): six integer instructions, a NaN quieted with its payload kept -- as measured and as their tests pin the bits
template <> __device__ __forceinline__ bf16 from_float_int<bf16>(float x)
{
    uint32_t u = __float_as_uint(x);
    bf16 r;
    if ((u & 0x7fffffffu) > 0x7f800000u) { r.v = (uint16_t)((u >> 16) | 0x40u); return r; }
    u += 0x7fffu + ((u >> 16) & 1u);
    r.v = (uint16_t)(u >> 16);
    return r;
}

static inline bool dtype_ok(int dtype) { return dtype == MDX_F32 || dtype == MDX_BF16; }
static inline size_t elem_bytes(int dtype) { return dtype == MDX_F32 ? 4 : 2; }
static inline int vec_elems(int dtype) { return dtype == MDX_F32 ? 4 : 8; }       // elements of a 16-byte channel vector

// a channels-last map [B][H][W][C] whose threads own whole 16-byte channel vectors and index its pixels in 32 bits
static inline int nhwc_map_ok(int B, int C, int H, int W, int dtype)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !dtype_ok(dtype)) return MDX_ERR_BAD_SHAPE;
    if (C % vec_elems(dtype)) return MDX_ERR_BAD_SHAPE;
    if ((long long)B * H * W >= (1ll << 31)) return MDX_ERR_BAD_SHAPE;
    return MDX_OK;
}

// ---- dispatch: f is a generic lambda that launches; it gets the storage type(s) as tags and the switch as a std::bool_constant:
//          dispatch_dtype(dtype, [&](auto t) { using T = typename decltype(t)::type;  hipLaunchKernelGGL((k<T>), ..., (const T *)x, ...); });
//      so that the argument list of a launch is written once.  false: no such instantiation, nothing was launched.
template <typename T> struct type_tag { using type = T; };

template <typename F> static inline bool dispatch_dtype(int dtype, F &&f)
{
    if (dtype == MDX_F32) f(type_tag<float>{});
    else if (dtype == MDX_BF16) f(type_tag<bf16>{});
    else return false;
    return true;
}

// the (in, out) pairs the decoder glue is built for: a float32 map never feeds a bfloat16 one
template <typename F> static inline bool dispatch_dtype_pair(int in_dtype, int out_dtype, F &&f)
{
    if (in_dtype == MDX_F32 && out_dtype == MDX_F32) f(type_tag<float>{}, type_tag<float>{});
    else if (in_dtype == MDX_BF16 && out_dtype == MDX_BF16) f(type_tag<bf16>{}, type_tag<bf16>{});
    else if (in_dtype == MDX_BF16 && out_dtype == MDX_F32) f(type_tag<bf16>{}, type_tag<float>{});
    else return false;
    return true;
}

template <typename F> static inline void dispatch_flag(bool flag, F &&f)
{
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

template <typename F> static inline bool dispatch_dtype_flag(int dtype, bool flag, F &&f)
{
    return dispatch_dtype(dtype, [&](auto t) { dispatch_flag(flag, [&](auto b) { f(t, b); }); });
}

}  // namespace mdx
