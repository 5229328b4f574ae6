// loss_stats.hip -- statistics of the maps the fused loss path leaves behind, computed on the device (mdx/loss_stats.py: LossStats), gfx950.
//
// After every step outputs[("automask", s)] holds the per-pixel arg-min channel (uint8 [B,H,W]: which pixels the auto-mask removed,
// which source frame won the minimum) and outputs[("disp", s)] the disparity of every scale.  The two silent failures of this loss --
// a stationary scene whose every pixel is masked, a disparity that collapses to a constant -- show in these maps alone.  One read-only
// pass over them gives every (scale, image) a record -- how many pixels each channel won, how many indices are corrupt, the sum, the
// sum of squares, the smallest and the largest of the finite disparities, the count of the others -- and every scale a history entry
// that stays on the device, so that a run watched at every step still reads the host once per epoch.
//
// Two launches for all scales of a step, ordered by the stream alone, in tensor_stats.hip's manner: every block's partial record into
// the block's own slot, then one block per scale, a wave per image, adds the slots of each image in a fixed order.  Block b of pass 1
// IS slot b; the block map -- {scale, image, chunk, index or disparity} per block -- is built once on the host (mdx_loss_stats_plan)
// and kept on the device; the map pointers travel as kernel arguments, since they change from step to step.  A NULL map still has its
// slots: its blocks store the empty partial.  No atomics and nothing to clear -- every slot, record and history entry is overwritten
// (or advanced) by exactly one thread -- so the same inputs give the same bits at every launch and a replayed graph has no state of
// its own (LABNOTES, "hipMemsetAsync inside a captured graph").
#include "mdx_common.hpp"

namespace mdx {

constexpr int LOSS_CHUNK_INDEX = 4096;        // pixels of an index map per block: one 16-byte vector per thread
constexpr int LOSS_CHUNK_DISP = 4096;         // disparity elements per block: four float4 per thread
constexpr int LOSS_BINS = 2 * MDX_MAX_SRC;
static_assert(LOSS_BINS == 8, "a thread counts its winners in the eight bytes of one 64-bit word");
static_assert(LOSS_CHUNK_INDEX == 256 * 16 && LOSS_CHUNK_DISP % (256 * 4) == 0, "the chunks are whole vectors per thread");

// One record: a (scale, image)'s (mdx_loss_stats) and a block's partial, which has the same fields over one chunk of ONE of the two
// maps -- except that a partial keeps the extrema as ordered keys (below), where "no finite element" is min > max.
struct LossRecord {
    double disp_sum, disp_sumsq;
    uint32_t disp_min, disp_max;              // the record: the bits of the floats; a partial: the keys
    uint32_t winner[LOSS_BINS];
    uint32_t bad_index, disp_nonfinite, index_present, disp_present;
};
static_assert(sizeof(LossRecord) == sizeof(mdx_loss_stats) && sizeof(LossRecord) == 72, "include/mdx.h: mdx_loss_stats");
static_assert(sizeof(mdx_loss_stats_history) == 152, "include/mdx.h: mdx_loss_stats_history");

struct LossMaps {                             // kernel argument of pass 1
    const uint8_t *idx[MDX_MAX_SCALES];
    const float *disp[MDX_MAX_SCALES];
    long long hw[MDX_MAX_SCALES];             // h[s] * w[s]
    long long HW;                             // H * W, < 2^32
    uint32_t limit;                           // an index >= limit is corrupt: 2S with the auto-mask, S without
};

struct LossFinish {                           // kernel argument of pass 2
    long long base[MDX_MAX_SCALES];           // first slot of scale s
    int cd[MDX_MAX_SCALES];                   // disparity chunks per image of scale s
    int ci;                                   // index chunks per image
    int B, S, automask;
    long long HW;
    double static_share;
};

// The order of finite floats as an order of unsigned words, -0 below +0, denormals included whatever the denormal mode.
__device__ __forceinline__ uint32_t float_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return (key & 0x80000000u) ? key ^ 0x80000000u : ~key; }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// What a thread carries; the neutral element of every field is its initial value.
struct LossAcc {
    double sum = 0.0, sumsq = 0.0;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    uint32_t nonfinite = 0, bad = 0;
    uint32_t win[LOSS_BINS] = {0, 0, 0, 0, 0, 0, 0, 0};
};

__device__ __forceinline__ void loss_disp(LossAcc &a, float x)
{
    const uint32_t bits = __float_as_uint(x);
    const bool finite = (bits & 0x7F800000u) != 0x7F800000u;       // from the exponent bits: Inf and every NaN payload
    const uint32_t key = float_key(bits);
    a.sum += finite ? (double)x : 0.0;
    a.sumsq += finite ? (double)x * (double)x : 0.0;               // the product of two floats is exact in double
    a.kmin = finite ? umin(a.kmin, key) : a.kmin;
    a.kmax = finite ? umax(a.kmax, key) : a.kmax;
    a.nonfinite += finite ? 0u : 1u;
}

// A thread sees at most 16 pixels: their winners are counted in the eight bytes of `bins`, byte c for channel c.
__device__ __forceinline__ void loss_index(unsigned long long &bins, uint32_t &bad, uint32_t v, uint32_t limit)
{
    const bool legal = v < limit;                                  // limit <= 8
    bins += legal ? 1ull << ((v & 7u) * 8u) : 0ull;
    bad += legal ? 0u : 1u;
}

__device__ __forceinline__ void loss_index_word(unsigned long long &bins, uint32_t &bad, uint32_t word, uint32_t limit)
{
    loss_index(bins, bad, word & 0xFFu, limit);
    loss_index(bins, bad, (word >> 8) & 0xFFu, limit);
    loss_index(bins, bad, (word >> 16) & 0xFFu, limit);
    loss_index(bins, bad, word >> 24, limit);
}

// 256 threads: wave shuffles, four LDS slots, a fixed order.  The result is valid in thread 0.
struct LossLds { double sum[4], sumsq[4]; uint32_t kmin[4], kmax[4], nonfinite[4], bad[4], win[LOSS_BINS][4]; };

__device__ __forceinline__ void loss_wave_reduce(LossAcc &a)          // the result is valid in the wave's lane 0
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.sum += __shfl_down(a.sum, off, 64);
        a.sumsq += __shfl_down(a.sumsq, off, 64);
        a.kmin = umin(a.kmin, __shfl_down(a.kmin, off, 64));
        a.kmax = umax(a.kmax, __shfl_down(a.kmax, off, 64));
        a.nonfinite += __shfl_down(a.nonfinite, off, 64);
        a.bad += __shfl_down(a.bad, off, 64);
#pragma unroll
        for (int c = 0; c < LOSS_BINS; ++c) a.win[c] += __shfl_down(a.win[c], off, 64);
    }
}

__device__ __forceinline__ void loss_block_reduce(LossAcc &a, LossLds &lds)
{
    loss_wave_reduce(a);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        lds.sum[wv] = a.sum; lds.sumsq[wv] = a.sumsq;
        lds.kmin[wv] = a.kmin; lds.kmax[wv] = a.kmax;
        lds.nonfinite[wv] = a.nonfinite; lds.bad[wv] = a.bad;
#pragma unroll
        for (int c = 0; c < LOSS_BINS; ++c) lds.win[c][wv] = a.win[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.sum = ((lds.sum[0] + lds.sum[1]) + lds.sum[2]) + lds.sum[3];
        a.sumsq = ((lds.sumsq[0] + lds.sumsq[1]) + lds.sumsq[2]) + lds.sumsq[3];
        a.kmin = umin(umin(lds.kmin[0], lds.kmin[1]), umin(lds.kmin[2], lds.kmin[3]));
        a.kmax = umax(umax(lds.kmax[0], lds.kmax[1]), umax(lds.kmax[2], lds.kmax[3]));
        a.nonfinite = ((lds.nonfinite[0] + lds.nonfinite[1]) + lds.nonfinite[2]) + lds.nonfinite[3];
        a.bad = ((lds.bad[0] + lds.bad[1]) + lds.bad[2]) + lds.bad[3];
#pragma unroll
        for (int c = 0; c < LOSS_BINS; ++c) a.win[c] = ((lds.win[c][0] + lds.win[c][1]) + lds.win[c][2]) + lds.win[c][3];
    }
}

__device__ __forceinline__ void loss_store(LossRecord *__restrict__ out, const LossAcc &a, uint32_t dmin, uint32_t dmax,
                                           uint32_t index_present, uint32_t disp_present)
{
    LossRecord r;
    r.disp_sum = a.sum; r.disp_sumsq = a.sumsq;
    r.disp_min = dmin; r.disp_max = dmax;
#pragma unroll
    for (int c = 0; c < LOSS_BINS; ++c) r.winner[c] = a.win[c];
    r.bad_index = a.bad; r.disp_nonfinite = a.nonfinite;
    r.index_present = index_present; r.disp_present = disp_present;
    *out = r;
}

// Pass 1.  Block b: chunk bm.z of image bm.y of scale bm.x's index map (bm.w == 0) or disparity (bm.w == 1) -> partials[b].
// Image bm.y of an index map starts at idx + bm.y * H * W, which is 16-byte aligned only when H * W allows it: the vector path asks
// the image's base, not the map's.  A NULL map: the empty partial, which says "absent".
__global__ __launch_bounds__(256) void loss_stats_partials_kernel(LossMaps maps, const int4 *__restrict__ blockmap,
                                                                  LossRecord *__restrict__ partials)
{
    __shared__ LossLds lds;
    const int4 bm = blockmap[blockIdx.x];
    LossAcc a;
    uint32_t index_present = 0, disp_present = 0;
    if (bm.w == 0) {
        const uint8_t *__restrict__ map = maps.idx[bm.x];
        if (map) {
            index_present = 1;
            const uint8_t *__restrict__ img = map + (long long)bm.y * maps.HW;
            const long long base = (long long)bm.z * LOSS_CHUNK_INDEX + (long long)threadIdx.x * 16;
            unsigned long long bins = 0;
            if ((((uintptr_t)img) & 15) == 0 && (long long)(bm.z + 1) * LOSS_CHUNK_INDEX <= maps.HW) {     // whole and aligned
                const uint4 v = *reinterpret_cast<const uint4 *>(img + base);
                loss_index_word(bins, a.bad, v.x, maps.limit);
                loss_index_word(bins, a.bad, v.y, maps.limit);
                loss_index_word(bins, a.bad, v.z, maps.limit);
                loss_index_word(bins, a.bad, v.w, maps.limit);
            } else {
                for (long long j = base; j < base + 16 && j < maps.HW; ++j) loss_index(bins, a.bad, img[j], maps.limit);
            }
#pragma unroll
            for (int c = 0; c < LOSS_BINS; ++c) a.win[c] = (uint32_t)(bins >> (8 * c)) & 0xFFu;
        }
    } else {
        const float *__restrict__ map = maps.disp[bm.x];
        if (map) {
            disp_present = 1;
            const long long n = maps.hw[bm.x];
            const float *__restrict__ img = map + (long long)bm.y * n;
            const long long base = (long long)bm.z * LOSS_CHUNK_DISP;
            constexpr int K = LOSS_CHUNK_DISP / (256 * 4);
            if ((((uintptr_t)img) & 15) == 0 && base + LOSS_CHUNK_DISP <= n) {          // whole and aligned: every load in flight first
                float4 D[K];
#pragma unroll
                for (int k = 0; k < K; ++k) D[k] = *reinterpret_cast<const float4 *>(img + base + ((long long)k * 256 + threadIdx.x) * 4);
#pragma unroll
                for (int k = 0; k < K; ++k) { loss_disp(a, D[k].x); loss_disp(a, D[k].y); loss_disp(a, D[k].z); loss_disp(a, D[k].w); }
            } else {
                for (int k = 0; k < K; ++k) {
                    const long long i = base + ((long long)k * 256 + threadIdx.x) * 4;
                    for (long long j = i; j < i + 4 && j < n; ++j) loss_disp(a, img[j]);
                }
            }
        }
    }
    loss_block_reduce(a, lds);
    if (threadIdx.x == 0) loss_store(partials + blockIdx.x, a, a.kmin, a.kmax, index_present, disp_present);
}

// Pass 2.  Block s: scale s; wave v of its four takes the images v, v + 4, ...  Image b's slots are base[s] + b * (ci + cd[s])
// onwards, the index chunks first; lane l takes slots lo + l, lo + l + 64, ..., then the fixed tree of loss_wave_reduce, and lane 0
// writes the image's record: no barrier between the images.  What a pass does to the scale's history entry does not depend on the
// order of the images -- sums of integers, "any", the largest share and the smallest range, all of ONE pass number -- so each
// wave's lane 0 gathers its images' part, the four parts meet in LDS in a fixed order, and thread 0 advances the entry.
struct LossPass {                             // one pass's part of a history entry; all-zero is "nothing seen"
    unsigned long long win[LOSS_BINS];
    uint32_t images, statics, bad, ranged;
    double max_share, min_range;              // min_range counts when ranged != 0
};

__device__ __forceinline__ void loss_pass_add(LossPass &p, const LossPass &q)
{
#pragma unroll
    for (int c = 0; c < LOSS_BINS; ++c) p.win[c] += q.win[c];
    p.images += q.images; p.statics += q.statics; p.bad |= q.bad;
    p.max_share = q.max_share > p.max_share ? q.max_share : p.max_share;
    if (q.ranged && (!p.ranged || q.min_range < p.min_range)) p.min_range = q.min_range;
    p.ranged |= q.ranged;
}

__global__ __launch_bounds__(256) void loss_stats_finish_kernel(LossFinish f, const LossRecord *__restrict__ partials,
                                                                LossRecord *__restrict__ records,
                                                                mdx_loss_stats_history *__restrict__ history)
{
    __shared__ LossPass parts[4];
    const int s = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per_image = f.ci + f.cd[s];
    LossPass mine = {};
    for (int b = wv; b < f.B; b += 4) {
        const long long lo = f.base[s] + (long long)b * per_image;
        LossAcc a;
        for (int i = lane; i < per_image; i += 64) {
            const LossRecord p = partials[lo + i];
            a.sum += p.disp_sum; a.sumsq += p.disp_sumsq;
            a.kmin = umin(a.kmin, p.disp_min); a.kmax = umax(a.kmax, p.disp_max);
            a.nonfinite += p.disp_nonfinite; a.bad += p.bad_index;
#pragma unroll
            for (int c = 0; c < LOSS_BINS; ++c) a.win[c] += p.winner[c];
        }
        loss_wave_reduce(a);
        if (lane == 0) {
            const uint32_t index_present = partials[lo].index_present;            // one pointer per scale: every slot says the same
            const uint32_t disp_present = partials[lo + f.ci].disp_present;
            const bool any_finite = a.kmin <= a.kmax;
            const float dmin = any_finite ? __uint_as_float(key_bits(a.kmin)) : 0.0f;
            const float dmax = any_finite ? __uint_as_float(key_bits(a.kmax)) : 0.0f;
            loss_store(records + (long long)s * f.B + b, a, __float_as_uint(dmin), __float_as_uint(dmax), index_present, disp_present);
            mine.bad |= (a.bad > 0 || a.nonfinite > 0) ? 1u : 0u;
            if (index_present) {
                mine.images += 1;
                uint32_t masked = 0;
#pragma unroll
                for (int c = 0; c < LOSS_BINS; ++c) {
                    mine.win[c] += a.win[c];
                    masked += (f.automask && c < f.S) ? a.win[c] : 0u;
                }
                if (f.automask) {
                    mine.statics += (double)masked >= f.static_share * (double)f.HW ? 1u : 0u;
                    const double share = (double)masked / (double)f.HW;
                    mine.max_share = share > mine.max_share ? share : mine.max_share;
                }
            }
            if (disp_present && any_finite) {
                const double range = (double)dmax - (double)dmin;
                if (!mine.ranged || range < mine.min_range) mine.min_range = range;
                mine.ranged = 1;
            }
        }
    }
    if (!history) return;
    if (lane == 0) parts[wv] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    loss_pass_add(mine, parts[1]);
    loss_pass_add(mine, parts[2]);
    loss_pass_add(mine, parts[3]);
    mdx_loss_stats_history h = history[s];
    h.passes += 1;
    h.images += mine.images;
#pragma unroll
    for (int c = 0; c < LOSS_BINS; ++c) h.winner_total[c] += (long long)mine.win[c];
    if (mine.bad) {
        h.bad_passes += 1;
        if (h.first_bad_pass == 0) h.first_bad_pass = h.passes;
    }
    if (mine.statics) {
        h.static_images += mine.statics;
        if (h.first_static_pass == 0) h.first_static_pass = h.passes;
        h.last_static_pass = h.passes;
    }
    if (mine.max_share > h.max_masked_share) {                      // strictly: the first pass of a tie stays
        h.max_masked_share = mine.max_share;
        h.max_masked_pass = h.passes;
    }
    if (mine.ranged && (h.min_disp_range_pass == 0 || mine.min_range < h.min_disp_range)) {
        h.min_disp_range = mine.min_range;
        h.min_disp_range_pass = h.passes;
    }
    history[s] = h;
}

static inline long long chunks(long long n, int chunk) { return (n + chunk - 1) / chunk; }

// NULL, then shape: what both passes and the plan ask of the sizes.
static int loss_shapes(int nscales, int B, int H, int W, const int *h, const int *w)
{
    if (!h || !w) return MDX_ERR_NULL_POINTER;
    if (nscales < 1 || nscales > MDX_MAX_SCALES || B < 1 || H < 1 || W < 1) return MDX_ERR_BAD_SHAPE;
    if ((long long)H * W >= (1ll << 32)) return MDX_ERR_BAD_SHAPE;
    for (int s = 0; s < nscales; ++s)
        if (h[s] < 1 || w[s] < 1) return MDX_ERR_BAD_SHAPE;
    return MDX_OK;
}

// -> the number of blocks = slots, or 0 when it does not fit an int; base[s]: scale s's first slot, cd[s]: its disparity chunks.
static int loss_layout(int nscales, int B, int H, int W, const int *h, const int *w, long long *base, int *cd, int *ci)
{
    const long long ni = chunks((long long)H * W, LOSS_CHUNK_INDEX);
    long long total = 0;
    for (int s = 0; s < nscales; ++s) {
        const long long nd = chunks((long long)h[s] * w[s], LOSS_CHUNK_DISP);
        if (ni + nd >= (1ll << 31)) return 0;
        base[s] = total;
        cd[s] = (int)nd;
        total += (long long)B * (ni + nd);
        if (total >= (1ll << 31)) return 0;
    }
    *ci = (int)ni;
    return (int)total;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_loss_stats_partial_bytes(void) { return sizeof(LossRecord); }
MDX_EXPORT size_t mdx_loss_stats_record_bytes(void) { return sizeof(mdx_loss_stats); }
MDX_EXPORT size_t mdx_loss_stats_history_bytes(void) { return sizeof(mdx_loss_stats_history); }
MDX_EXPORT size_t mdx_loss_stats_blockmap_entry_bytes(void) { return sizeof(int4); }
MDX_EXPORT int mdx_loss_stats_index_chunk(void) { return LOSS_CHUNK_INDEX; }
MDX_EXPORT int mdx_loss_stats_disp_chunk(void) { return LOSS_CHUNK_DISP; }

MDX_EXPORT int mdx_loss_stats_plan(int nscales, int B, int H, int W, const int *h, const int *w, void *blockmap)
{
    const int st = loss_shapes(nscales, B, H, W, h, w);
    if (st != MDX_OK) return st;
    long long base[MDX_MAX_SCALES];
    int cd[MDX_MAX_SCALES], ci = 0;
    const int total = loss_layout(nscales, B, H, W, h, w, base, cd, &ci);
    if (total < 1) return MDX_ERR_BAD_SHAPE;
    if (blockmap) {
        int4 *bm = (int4 *)blockmap;
        for (int s = 0; s < nscales; ++s)
            for (int b = 0; b < B; ++b) {
                for (int c = 0; c < ci; ++c) *bm++ = make_int4(s, b, c, 0);
                for (int c = 0; c < cd[s]; ++c) *bm++ = make_int4(s, b, c, 1);
            }
    }
    return total;
}

MDX_EXPORT int mdx_loss_stats_partials(int nscales, int B, int H, int W, int S, int automask, const int *h, const int *w,
                                       const uint8_t *const *idx, const float *const *disp, const void *blockmap, int nblocks,
                                       void *partials, void *stream)
{
    if (!idx || !disp || !blockmap || !partials) return MDX_ERR_NULL_POINTER;
    const int st = loss_shapes(nscales, B, H, W, h, w);
    if (st != MDX_OK) return st;
    if (S < 1 || S > MDX_MAX_SRC || (automask != 0 && automask != 1) || nblocks < 1) return MDX_ERR_BAD_SHAPE;
    LossFinish f;
    if (loss_layout(nscales, B, H, W, h, w, f.base, f.cd, &f.ci) != nblocks) return MDX_ERR_BAD_SHAPE;      // not this plan's map
    if (!aligned(partials, sizeof(double))) return MDX_ERR_MISALIGNED;
    for (int s = 0; s < nscales; ++s)
        if (!aligned(disp[s], sizeof(float))) return MDX_ERR_MISALIGNED;
    LossMaps m;
    for (int s = 0; s < MDX_MAX_SCALES; ++s) {
        m.idx[s] = s < nscales ? idx[s] : nullptr;
        m.disp[s] = s < nscales ? disp[s] : nullptr;
        m.hw[s] = s < nscales ? (long long)h[s] * w[s] : 0;
    }
    m.HW = (long long)H * W;
    m.limit = (uint32_t)(automask ? 2 * S : S);
    hipLaunchKernelGGL(loss_stats_partials_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, m, (const int4 *)blockmap,
                       (LossRecord *)partials);
    return check_launch();
}

MDX_EXPORT int mdx_loss_stats_finish(int nscales, int B, int H, int W, int S, int automask, const int *h, const int *w,
                                     double static_share, const void *partials, void *records, void *history, void *stream)
{
    if (!partials || !records) return MDX_ERR_NULL_POINTER;
    const int st = loss_shapes(nscales, B, H, W, h, w);
    if (st != MDX_OK) return st;
    if (S < 1 || S > MDX_MAX_SRC || (automask != 0 && automask != 1)) return MDX_ERR_BAD_SHAPE;
    if (!(static_share > 0.0 && static_share <= 1.0)) return MDX_ERR_BAD_SHAPE;                 // a NaN fails both comparisons
    LossFinish f;
    if (loss_layout(nscales, B, H, W, h, w, f.base, f.cd, &f.ci) < 1) return MDX_ERR_BAD_SHAPE;
    if (!aligned(partials, sizeof(double)) || !aligned(records, sizeof(double)) || !aligned(history, sizeof(double)))
        return MDX_ERR_MISALIGNED;
    for (int s = nscales; s < MDX_MAX_SCALES; ++s) { f.base[s] = 0; f.cd[s] = 0; }
    f.B = B; f.S = S; f.automask = automask;
    f.HW = (long long)H * W;
    f.static_share = static_share;
    hipLaunchKernelGGL(loss_stats_finish_kernel, dim3(nscales), dim3(256), 0, (hipStream_t)stream, f, (const LossRecord *)partials,
                       (LossRecord *)records, (mdx_loss_stats_history *)history);
    return check_launch();
}
