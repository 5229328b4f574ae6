// digest.hip -- a 64-bit digest of every weight tensor, computed on the device (mdx/optim.py: WeightDigest), gfx950.
//
// Data-parallel ranks must hold the same weights after every step, and a resumed run must read the weight files its state file was
// written beside; neither can be seen from a loss curve.  One read-only pass over the weights gives each tensor one 64-bit word
// that two ranks (model_tool/parallel.py: check_replicas) or a run and a file (model_tool/logger.py) compare for equality.  The
// work split is adam.hip's: a device table, a {tensor, chunk} block map, 4096 words per block of 256 threads, uint4 where the
// tensor's pointer is 16-byte aligned, a scalar path otherwise and for a tensor's tail.
//
//   digest(tensor) = sum over storage index i = 0 .. n - 1 of hash32(i, word[i]),  modulo 2^64
//
// The words are read as words, never as floats: NaN payloads and the sign of zero count.  Integer addition is associative, so the
// block sums may arrive in any order (one vector global atomic per block) and the result has no tolerance.  The position enters
// through i, so two exchanged elements change the digest.  i is taken modulo 2^32: a tensor of 2^32 words or more is not refused,
// its words 2^32 apart merely share their index.
#include "mdx_multi_tensor.hpp"

namespace mdx {

struct DigestTensor {
    const uint32_t *w;        // the tensor's dense storage, as words
    long long n;
};
static_assert(sizeof(DigestTensor) == 16, "the digest's table entry is 16 bytes (include/mdx.h)");

// A multiplicative spread of the index, then murmur3's 32-bit finaliser (include/mdx.h states the recipe).
__device__ __forceinline__ unsigned long long digest_one(uint32_t i, uint32_t u)
{
    uint32_t k = u ^ (i * 0x9E3779B1u);
    k ^= k >> 16;
    k *= 0x85EBCA6Bu;
    k ^= k >> 13;
    k *= 0xC2B2AE35u;
    k ^= k >> 16;
    return (unsigned long long)k;
}

__global__ __launch_bounds__(256) void digest_words_kernel(const DigestTensor *__restrict__ tab, int first,
                                                           const int2 *__restrict__ blockmap, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long lds[4];
    const int2 bm = blockmap[blockIdx.x];                 // (tensor of this launch, chunk)
    const DigestTensor t = tab[first + bm.x];
    const long long base = (long long)bm.y * MT_CHUNK;
    constexpr int K = MT_CHUNK / (256 * 4);
    unsigned long long acc = 0;
    if ((((uintptr_t)t.w) & 15) == 0 && base + MT_CHUNK <= t.n) {      // a whole aligned chunk: every load in flight first
        uint4 U[K];
#pragma unroll
        for (int k = 0; k < K; ++k) U[k] = *reinterpret_cast<const uint4 *>(t.w + base + ((long long)k * 256 + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t i = (uint32_t)(base + ((long long)k * 256 + threadIdx.x) * 4);
            acc += ((digest_one(i, U[k].x) + digest_one(i + 1u, U[k].y)) + digest_one(i + 2u, U[k].z)) + digest_one(i + 3u, U[k].w);
        }
    } else {
        for (int k = 0; k < K; ++k) {
            const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
            for (long long j = i; j < i + 4 && j < t.n; ++j) acc += digest_one((uint32_t)j, t.w[j]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out + first + bm.x, ((lds[0] + lds[1]) + lds[2]) + lds[3]);
}

// The sums are added into out, so it is cleared first -- by a launch, not by hipMemsetAsync: with the memset captured into a
// hipGraph in front of the pass, the graph's first replay was right and its second returned other sums for the same weights
// (LABNOTES, "The weight digests").
__global__ __launch_bounds__(256) void digest_clear_kernel(unsigned long long *__restrict__ out, int count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = 0;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_digest_table_entry_bytes(void) { return sizeof(DigestTensor); }

MDX_EXPORT int mdx_digest_words(const void *table, int first, int count, const void *blockmap, int nblocks, uint64_t *out,
                                void *stream)
{
    if (!out) return MDX_ERR_NULL_POINTER;
    if (int rc = check_plan(table, first, count, blockmap, nblocks)) return rc;
    if (!aligned(out, sizeof(uint64_t))) return MDX_ERR_MISALIGNED;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "atomicAdd's 64-bit type");
    // the entry point clears its own slice: the block sums are added into it, and a caller (or a replayed graph) never zeroes
    hipLaunchKernelGGL(digest_clear_kernel, dim3((count + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long *>(out) + first, count);
    if (int rc = check_launch()) return rc;
    hipLaunchKernelGGL(digest_words_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, (const DigestTensor *)table, first,
                       (const int2 *)blockmap, reinterpret_cast<unsigned long long *>(out));
    return check_launch();
}
