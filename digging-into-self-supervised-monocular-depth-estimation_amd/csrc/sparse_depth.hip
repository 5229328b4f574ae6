// sparse_depth.hip -- sparse lidar supervision: a depth term beside the fused loss, forward and gradient, all scales at once (gfx950).
//
// THE TERM (mdx.functional.sparse_depth_loss, mdx.composite.sparse_depth_loss; include/mdx.h: mdx_sparse_depth_*)
//   disp_k  float32 contiguous [B,1,h_k,w_k], k < nscales (1..MDX_MAX_SCALES);  gt  float32 contiguous [B,1,gh,gw], 0 = no return;
//   gh >= h_k and gw >= w_k for every k.
//   A ground-truth pixel (b,Y,X) is VALID when gt > lo && gt < hi, both strict: NaN, +-inf, negative values (lo >= 0) and values
//   equal to a bound are invalid.  n = the valid pixels of the whole batch.
//   Per valid pixel and scale:
//     u   = the bilinear sample of disp_k at (Y,X) on the gh x gw grid, align_corners=False: up_tap / up_combine(premul=false) of
//           mdx_device.hpp -- the element itself when the sizes are equal;
//     sd  = scaled_disp(u, a, b), a = 1/max_depth, b = 1/min_depth - 1/max_depth, formed as disparity2depth forms them;
//     r   = -log(sd) - log(gt)                      (log depth - log gt; evaluated as -log(sd * gt) with the product taken exactly)
//     rho = sqrt(r^2 + eps^2) - eps                 (Charbonnier in log depth: smooth, so float32 rounding cannot flip a gradient's
//                                                    sign at r ~ 0)
//   Per scale:  L_k = (sum over the valid pixels of rho) / max(n, 1), the sum in double in a fixed order;
//   out[k] = L_k as float32, out[nscales] = n as float32 (exact up to 2^24 valid pixels).
//   Gradient:  dL_k / d disp_k[b,i,j] = gout[k] / max(n,1) * sum_valid (r / sqrt(r^2+eps^2)) * (-b / sd) * wy(Y,i) * wx(X,j),
//   wy / wx the tap weights up_tap gives; gout is a DEVICE array of nscales floats, so nothing synchronises.
//   n == 0: every L_k is 0 and every gradient element is written as 0.  A non-finite or non-positive sd under a VALID pixel makes
//   that L_k (and the gradients it reaches) NaN: carried, not clamped, as the monitor does.  A non-finite disparity that only
//   invalid pixels touch changes nothing.
//
// Forward, two launches: a block takes SD_CHUNK ground-truth pixels of one image -- each of its waves 256 at a time, as one float4 per
// lane where the image's base is 16-byte aligned and the 256 are whole, element by element otherwise -- and a wave that finds no
// valid pixel among its 256 goes on before it touches any disparity (KITTI's maps are ~95 % zeros); the valid ones are queued and
// worked off 64 at a time, one per lane.  The block's sums (a double per scale, the count) go to the block's own workspace slot;
// one finishing block adds the slots in a fixed order.
// Backward, one launch per scale, a GATHER: a disparity pixel walks the ground-truth pixels whose taps reach it -- the row and
// column range taken conservatively from the scale ratio, then membership and weights decided by up_tap itself (t.i0 == i ||
// t.i1 == i, which covers the clamp at 0 and the far edge where i1 == i0 and both weights land on one pixel) -- re-derives u, sd, r
// there and adds the contributions in double in a fixed order.  G lanes share a pixel (1 at scale 0's ~4 x 4 walk, a whole wave at
// ~31 x 31) and meet in a fixed shuffle tree.  No floating-point atomics, every output element written by a plain store, nothing to
// clear: the same inputs give the same bits at every launch and every graph replay.
#include <cmath>

#include "mdx_common.hpp"
#include "mdx_device.hpp"

namespace mdx {

constexpr int SD_CHUNK = 4096;                // ground-truth pixels per block of the forward pass
constexpr int SD_SUB = 256;                   // per wave and turn: one float4 per lane
constexpr int SD_QUEUE = 64 + SD_SUB;          // a wave's queue of valid pixels: fewer than 64 left over + one turn's 256
constexpr int SD_LOOK = 4;                    // walk positions a lane of the backward pass loads before it looks at any of them
constexpr int SD_DEFER = 8;                   // valid pixels a lane can have noted when the wave works the lists off
static_assert(SD_LOOK <= SD_DEFER, "one round of looks fits the list");
static_assert(SD_CHUNK % (4 * SD_SUB) == 0, "the four waves of a block take whole turns");

struct SdGeom {                               // kernel argument of every pass
    const float *disp[MDX_MAX_SCALES];
    int h[MDX_MAX_SCALES], w[MDX_MAX_SCALES];
    const float *gt;
    int nscales, B, gh, gw;
    unsigned ghw;                             // gh * gw; B * gh * gw < 2^32
    float a, b, lo, hi, eps;
};

MDX_DEV bool sd_valid(float g, float lo, float hi) { return g > lo && g < hi; }          // a NaN fails both

// The taps of destination `dst`; equal sizes: the element itself with weight 1.
MDX_DEV UpTap sd_tap(bool same, float scale, int dst, int n)
{
    if (!same) return up_tap(scale, dst, n);
    UpTap t;
    t.i0 = t.i1 = dst; t.l0 = 1.0f; t.l1 = 0.0f;
    return t;
}

MDX_DEV float sd_sample(const float *__restrict__ img, int w, const UpTap &ty, const UpTap &tx, bool same)
{
    const unsigned r0 = (unsigned)ty.i0 * (unsigned)w, r1 = (unsigned)ty.i1 * (unsigned)w;
    if (same) return img[r0 + tx.i0];
    return up_combine(img[r0 + tx.i0], img[r0 + tx.i1], img[r1 + tx.i0], img[r1 + tx.i1], ty, tx, false);
}

// What a valid pixel contributes: rho = sqrt(r^2 + eps^2) - eps and g = d rho / d r = r / sqrt(r^2 + eps^2), r = -log(sd * gt).  In
// float32, the product taken exactly (p + e == sd * gt: fma), so that r keeps its relative accuracy where it matters -- near 0,
// where log(p) ~ p - 1 and g still moves with r; far from 0 g is +-1 to rounding.  An sd that is not a positive finite number: NaN.
struct SdTerm { float rho, g; };

MDX_DEV SdTerm sd_term(float sd, float gt, float eps)
{
    SdTerm t;
    if (!(sd > 0.0f) || sd == INFINITY) { t.rho = t.g = NAN; return t; }
    const float p = sd * gt;
    const float e = __builtin_fmaf(sd, gt, -p);
    const float r = -(logf(p) + e / p);
    const float root = sqrtf(r * r + eps * eps);
    t.rho = root - eps;
    t.g = r / root;
    return t;
}

MDX_DEV double block_sum_256(double v, double (*lds)[MDX_MAX_SCALES + 1], int k)         // valid in thread 0
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6][k] = v;
    __syncthreads();
    return ((lds[0][k] + lds[1][k]) + lds[2][k]) + lds[3][k];
}

// what one lane of a wave wrote to LDS is read by another lane of the same wave: order the two for the compiler and the hardware
MDX_DEV void wave_lds_handover()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One valid pixel (index j of image b, value v) -> every scale's rho onto acc.
MDX_DEV void sd_consume(const SdGeom &g, unsigned b, unsigned j, float v, double (&acc)[MDX_MAX_SCALES], double &count)
{
    const int Y = (int)(j / (unsigned)g.gw), X = (int)(j - (unsigned)Y * (unsigned)g.gw);
    count += 1.0;
#pragma unroll
    for (int k = 0; k < MDX_MAX_SCALES; ++k) {
        if (k >= g.nscales) break;
        const int h = g.h[k], w = g.w[k];
        const bool same = h == g.gh && w == g.gw;
        const UpTap ty = sd_tap(same, (float)h / (float)g.gh, Y, h), tx = sd_tap(same, (float)w / (float)g.gw, X, w);
        const float u = sd_sample(g.disp[k] + (size_t)b * h * w, w, ty, tx, same);
        acc[k] += (double)sd_term(scaled_disp(u, g.a, g.b), v, g.eps).rho;
    }
}

// Forward, pass 1.  Block x: chunk x % chunks of image x / chunks -> slots[x * (nscales + 1) ...] = {sum of rho per scale, count}.
// A wave reads 256 pixels per turn and queues the valid ones in LDS (ballot + prefix count: the order of the pixels is kept); the
// arithmetic runs on whole batches of 64 queued pixels, one per lane, so a map that is 95 % zeros costs its valid pixels and not
// 64 lanes per valid pixel.  Lane l of the wave takes the queue's entries l, l + 64, ...: a fixed order.
__global__ __launch_bounds__(256) void sparse_depth_partials_kernel(SdGeom g, unsigned chunks, double *__restrict__ slots)
{
    __shared__ double lds[4][MDX_MAX_SCALES + 1];
    __shared__ unsigned queue_j[4][SD_QUEUE];
    __shared__ float queue_v[4][SD_QUEUE];
    const unsigned b = blockIdx.x / chunks, c = blockIdx.x - b * chunks;
    const float *__restrict__ img = g.gt + (size_t)b * g.ghw;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1ull;                              // the lanes before this one
    const bool base16 = (((uintptr_t)img) & 15) == 0;
    double acc[MDX_MAX_SCALES] = {0.0, 0.0, 0.0, 0.0};
    double count = 0.0;
    unsigned pending = 0;                                                                // queued and not consumed: the wave as one
    for (int turn = wv; turn < SD_CHUNK / SD_SUB; turn += 4) {
        const unsigned long long first = (unsigned long long)c * SD_CHUNK + (unsigned long long)turn * SD_SUB;
        if (first >= g.ghw) break;
        const unsigned long long j0 = first + (unsigned)lane * 4u;
        float v[4];
        if (base16 && first + SD_SUB <= g.ghw) {
            const float4 q = *reinterpret_cast<const float4 *>(img + j0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = j0 + e < g.ghw ? img[j0 + e] : NAN;      // past the image: never valid
        }
        const bool any = sd_valid(v[0], g.lo, g.hi) || sd_valid(v[1], g.lo, g.hi) || sd_valid(v[2], g.lo, g.hi) ||
                         sd_valid(v[3], g.lo, g.hi);
        if (__ballot(any) == 0ull) continue;                                             // the wave as one: no disparity is touched
#pragma unroll
        for (int e = 0; e < 4; ++e) {                                                    // fewer than 64 pending + at most 256 new
            const bool ok = sd_valid(v[e], g.lo, g.hi);
            const unsigned long long mask = __ballot(ok);
            if (ok) {
                const unsigned pos = pending + (unsigned)__popcll(mask & below);
                queue_j[wv][pos] = (unsigned)(j0 + e);
                queue_v[wv][pos] = v[e];
            }
            pending += (unsigned)__popcll(mask);
        }
        wave_lds_handover();
        unsigned head = 0;
        for (; pending - head >= 64; head += 64) sd_consume(g, b, queue_j[wv][head + lane], queue_v[wv][head + lane], acc, count);
        if (head) {                                                                      // the rest, fewer than 64, to the front
            const unsigned rest = pending - head;
            const unsigned tj = lane < rest ? queue_j[wv][head + lane] : 0u;             // read at >= 64, written below 64
            const float tv = lane < rest ? queue_v[wv][head + lane] : 0.0f;
            wave_lds_handover();
            if (lane < rest) { queue_j[wv][lane] = tj; queue_v[wv][lane] = tv; }
            pending = rest;
        }
    }
    wave_lds_handover();
    if ((unsigned)lane < pending) sd_consume(g, b, queue_j[wv][lane], queue_v[wv][lane], acc, count);
    double *__restrict__ slot = slots + (size_t)blockIdx.x * (g.nscales + 1);
#pragma unroll
    for (int k = 0; k < MDX_MAX_SCALES; ++k) {
        if (k >= g.nscales) break;                                                       // uniform: the barrier inside is safe
        const double s = block_sum_256(acc[k], lds, k);
        if (threadIdx.x == 0) slot[k] = s;
    }
    const double n = block_sum_256(count, lds, MDX_MAX_SCALES);
    if (threadIdx.x == 0) slot[g.nscales] = n;
}

// Forward, pass 2.  One block: thread t adds the slots t, t + 256, ... in that order, then the fixed tree of block_sum_256.
__global__ __launch_bounds__(256) void sparse_depth_finish_kernel(int nscales, unsigned nslots, const double *__restrict__ slots,
                                                                  float *__restrict__ out)
{
    __shared__ double lds[4][MDX_MAX_SCALES + 1];
    double acc[MDX_MAX_SCALES + 1] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned s = threadIdx.x; s < nslots; s += 256) {
        const double *__restrict__ slot = slots + (size_t)s * (nscales + 1);
#pragma unroll
        for (int k = 0; k <= MDX_MAX_SCALES; ++k) acc[k] += k <= nscales ? slot[k] : 0.0;
    }
    double total[MDX_MAX_SCALES + 1], n = 0.0;
#pragma unroll
    for (int k = 0; k <= MDX_MAX_SCALES; ++k) {
        total[k] = block_sum_256(acc[k], lds, k);
        n = k == nscales ? total[k] : n;
    }
    if (threadIdx.x != 0) return;
    const double d = n > 1.0 ? n : 1.0;
#pragma unroll
    for (int k = 0; k < MDX_MAX_SCALES; ++k)
        if (k < nscales) out[k] = (float)(total[k] / d);
    out[nscales] = (float)n;
}

// The ground-truth rows (or columns) that reach disparity row i, EXACTLY: src = s * (Y + 0.5) - 0.5 in [i - 1, i + 1), s = n / gn,
// taken in double and widened by one on both sides -- conservative -- and then trimmed from both ends by up_tap itself: what
// belongs is contiguous (src does not fall as Y grows), and up_tap alone decides it, the clamp at 0 and the far edge included.
MDX_DEV bool sd_member(float s, int Y, int n, int i)
{
    const UpTap t = up_tap(s, Y, n);
    return t.i0 == i || t.i1 == i;
}

MDX_DEV void sd_range(bool same, float s, int i, int n, int gn, int &first, int &last)
{
    if (same) { first = last = i; return; }
    const double inv = (double)gn / (double)n;
    const double lo = ((double)i - 0.5) * inv - 0.5, hi = ((double)i + 1.5) * inv - 0.5;
    int a = (int)floor(lo) - 1, b = (int)ceil(hi) + 1;
    a = a < 0 ? 0 : a;
    b = b > gn - 1 ? gn - 1 : b;
    while (a <= b && !sd_member(s, a, n, i)) ++a;
    while (b >= a && !sd_member(s, b, n, i)) --b;
    first = a; last = b;                                                                 // first > last: nothing reaches the row
}

MDX_DEV float sd_weight(const UpTap &t, int i) { return (t.i0 == i ? t.l0 : 0.0f) + (t.i1 == i ? t.l1 : 0.0f); }

// Backward of scale k.  G lanes per disparity pixel: lane q of the G takes the positions q, q + G, ... of the pixel's walk -- the
// rectangle of ground-truth pixels that reach it, row by row -- in that order, SD_LOOK of them per round with their loads in flight
// together (a look is one dependent load from the Infinity Cache: one at a time, the walk is a chain of latencies).  The walk only
// LOOKS: a valid pixel is noted in the lane's own LDS list, and when a lane of the wave could not take another round (and at the
// end) the wave works its lists off together, each lane in the order it noted them.  So the arithmetic runs a few times per walk
// instead of at every look at which any of 64 lanes saw a valid pixel; a dense map fills every list at once and loses nothing.
template <int G>
__global__ __launch_bounds__(256) void sparse_depth_bwd_kernel(SdGeom g, int k, const float *__restrict__ out,
                                                               const float *__restrict__ gout, float *__restrict__ ddisp)
{
    __shared__ unsigned noted_t[SD_DEFER][256];                                          // the walk position, < 2^32
    __shared__ float noted_v[SD_DEFER][256];
    const int h = g.h[k], w = g.w[k];
    const unsigned hw = (unsigned)h * (unsigned)w;
    const unsigned long long npix = (unsigned long long)g.B * hw;
    const unsigned long long pix = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) / G;
    const unsigned q = threadIdx.x & (G - 1);
    const bool live = pix < npix;
    const bool same = h == g.gh && w == g.gw;
    const float sy = (float)h / (float)g.gh, sx = (float)w / (float)g.gw;
    int i = 0, j = 0, Y0 = 0, X0 = 0;
    unsigned nc = 0;
    unsigned long long walk = 0;                                                         // a dead lane walks nothing
    const float *__restrict__ gimg = g.gt, *__restrict__ dimg = g.disp[k];
    if (live) {
        const unsigned b = (unsigned)(pix / hw), p = (unsigned)(pix - (unsigned long long)b * hw);
        i = (int)(p / (unsigned)w);
        j = (int)(p - (unsigned)i * (unsigned)w);
        int Y1, X1;
        sd_range(same, sy, i, h, g.gh, Y0, Y1);
        sd_range(same, sx, j, w, g.gw, X0, X1);
        if (Y1 >= Y0 && X1 >= X0) {
            nc = (unsigned)(X1 - X0 + 1);
            walk = (unsigned long long)(Y1 - Y0 + 1) * nc;                               // <= gh * gw < 2^32
        }
        gimg += (size_t)b * g.ghw;
        dimg += (size_t)b * hw;
    }
    unsigned long long t = q;
    unsigned row = nc ? q / nc : 0u, col = nc ? q - row * nc : 0u;
    double acc = 0.0;
    int noted = 0;
    const auto work_off = [&]() {
        for (int e = 0; __any(e < noted); ++e) {
            if (e >= noted) continue;
            const unsigned at = noted_t[e][threadIdx.x], at_row = at / nc;               // noted: nc > 0
            const int Y = Y0 + (int)at_row, X = X0 + (int)(at - at_row * nc);
            const float gv = noted_v[e][threadIdx.x];
            const UpTap ty = sd_tap(same, sy, Y, h), tx = sd_tap(same, sx, X, w);
            const float sd = scaled_disp(sd_sample(dimg, w, ty, tx, same), g.a, g.b);
            const float coef = sd_term(sd, gv, g.eps).g * (-g.b / sd);
            acc += (double)coef * ((double)sd_weight(ty, i) * (double)sd_weight(tx, j));
        }
        noted = 0;
    };
    while (__any(t < walk)) {
        float gv[SD_LOOK];
        unsigned at[SD_LOOK];
#pragma unroll
        for (int u = 0; u < SD_LOOK; ++u) {
            gv[u] = NAN;                                                                 // past the walk: never valid
            at[u] = (unsigned)t;
            if (t < walk) {
                gv[u] = gimg[(unsigned)(Y0 + (int)row) * (unsigned)g.gw + (unsigned)(X0 + (int)col)];
                t += G;
                col += G;
                while (col >= nc) { col -= nc; ++row; }
            }
        }
#pragma unroll
        for (int u = 0; u < SD_LOOK; ++u) {                                              // noted <= SD_DEFER - SD_LOOK on entry
            if (sd_valid(gv[u], g.lo, g.hi)) {
                noted_t[noted][threadIdx.x] = at[u]; noted_v[noted][threadIdx.x] = gv[u];
                ++noted;
            }
        }
        if (__any(noted > SD_DEFER - SD_LOOK)) work_off();
    }
    work_off();
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) acc += __shfl_down(acc, off, G);
    if (live && q == 0) {
        const double n = (double)out[g.nscales];
        ddisp[pix] = (float)((double)gout[k] / (n > 1.0 ? n : 1.0) * acc);
    }
}

static inline unsigned long long sd_chunks(long long ghw) { return (unsigned long long)((ghw + SD_CHUNK - 1) / SD_CHUNK); }

// the slots of the forward pass, or 0 for sizes the passes refuse
static unsigned long long sd_slots(int nscales, int B, int gh, int gw)
{
    if (nscales < 1 || nscales > MDX_MAX_SCALES || B < 1 || gh < 1 || gw < 1) return 0;
    if ((long long)gh * gw >= (1ll << 32) || (long long)B * ((long long)gh * gw) >= (1ll << 32)) return 0;
    const unsigned long long slots = (unsigned long long)B * sd_chunks((long long)gh * gw);
    return slots < (1ull << 31) ? slots : 0;
}

// lanes per disparity pixel of the backward walk, from its size: about (2 gh/h + 1) x (2 gw/w + 1) ground-truth pixels
static int sd_group(int h, int w, int gh, int gw)
{
    if (h == gh && w == gw) return 1;
    const double walk = (2.0 * gh / h + 1.0) * (2.0 * gw / w + 1.0);
    return walk <= 32.0 ? 1 : walk <= 128.0 ? 4 : walk <= 512.0 ? 16 : 64;
}

// the entries of a pointer array that may be read: those of a legal nscales (an illegal one is refused as a shape right after)
static inline int sd_entries(int nscales) { return nscales >= 1 && nscales <= MDX_MAX_SCALES ? nscales : 0; }

// NULL, then shape: what both passes ask.  Fills g.
static int sd_check(int nscales, int B, const int *h, const int *w, const float *const *disp, const float *gt, int gh, int gw,
                    double min_depth, double max_depth, float lo, float hi, double eps, const void *out, SdGeom *g)
{
    if (!h || !w || !disp || !gt || !out) return MDX_ERR_NULL_POINTER;
    for (int k = 0; k < sd_entries(nscales); ++k)
        if (!disp[k]) return MDX_ERR_NULL_POINTER;
    if (sd_slots(nscales, B, gh, gw) == 0) return MDX_ERR_BAD_SHAPE;
    for (int k = 0; k < nscales; ++k)
        if (h[k] < 1 || w[k] < 1 || gh < h[k] || gw < w[k]) return MDX_ERR_BAD_SHAPE;
    if (!(min_depth > 0.0) || !(max_depth > min_depth) || !(lo < hi) || !(eps > 0.0) || !std::isfinite(eps)) return MDX_ERR_BAD_SHAPE;
    const double min_disp = 1.0 / max_depth, max_disp = 1.0 / min_depth;                 // as disparity2depth (csrc/ops.hip)
    g->a = (float)min_disp;
    g->b = (float)(max_disp - min_disp);
    for (int k = 0; k < MDX_MAX_SCALES; ++k) {
        g->disp[k] = k < nscales ? disp[k] : nullptr;
        g->h[k] = k < nscales ? h[k] : 0;
        g->w[k] = k < nscales ? w[k] : 0;
    }
    g->gt = gt;
    g->nscales = nscales; g->B = B; g->gh = gh; g->gw = gw;
    g->ghw = (unsigned)((long long)gh * gw);
    g->lo = lo; g->hi = hi; g->eps = (float)eps;
    return MDX_OK;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_sparse_depth_workspace_bytes(int nscales, int B, int gh, int gw)
{
    return (size_t)sd_slots(nscales, B, gh, gw) * (size_t)(nscales + 1) * sizeof(double);
}

MDX_EXPORT int mdx_sparse_depth_fwd(int nscales, int B, const int *h, const int *w, const float *const *disp, const float *gt,
                                    int gh, int gw, double min_depth, double max_depth, float lo, float hi, double eps, float *out,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    SdGeom g;
    const int st = sd_check(nscales, B, h, w, disp, gt, gh, gw, min_depth, max_depth, lo, hi, eps, out, &g);
    if (st != MDX_OK) return st;
    if (!workspace || workspace_bytes < mdx_sparse_depth_workspace_bytes(nscales, B, gh, gw)) return MDX_ERR_WORKSPACE;
    if (!aligned(workspace, sizeof(double)) || !aligned(gt, sizeof(float)) || !aligned(out, sizeof(float))) return MDX_ERR_MISALIGNED;
    for (int k = 0; k < nscales; ++k)
        if (!aligned(disp[k], sizeof(float))) return MDX_ERR_MISALIGNED;
    const unsigned chunks = (unsigned)sd_chunks((long long)gh * gw);
    const unsigned nslots = (unsigned)sd_slots(nscales, B, gh, gw);
    hipLaunchKernelGGL(sparse_depth_partials_kernel, dim3(nslots), dim3(256), 0, (hipStream_t)stream, g, chunks, (double *)workspace);
    hipLaunchKernelGGL(sparse_depth_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nscales, nslots,
                       (const double *)workspace, out);
    return check_launch();
}

MDX_EXPORT int mdx_sparse_depth_bwd(int nscales, int B, const int *h, const int *w, const float *const *disp, const float *gt,
                                    int gh, int gw, double min_depth, double max_depth, float lo, float hi, double eps,
                                    const float *out, const float *gout, float *const *ddisp, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!gout || !ddisp) return MDX_ERR_NULL_POINTER;
    for (int k = 0; k < sd_entries(nscales); ++k)
        if (!ddisp[k]) return MDX_ERR_NULL_POINTER;
    SdGeom g;
    const int st = sd_check(nscales, B, h, w, disp, gt, gh, gw, min_depth, max_depth, lo, hi, eps, out, &g);
    if (st != MDX_OK) return st;
    // checked as the header says, and never touched: the recomputing gather keeps nothing between its launches (the argument is
    // there so that the store-pass form -- per-pixel coefficients, then the sums -- fits behind the same prototype)
    if (!workspace || workspace_bytes < mdx_sparse_depth_workspace_bytes(nscales, B, gh, gw)) return MDX_ERR_WORKSPACE;
    if (!aligned(workspace, sizeof(double)) || !aligned(gt, sizeof(float)) || !aligned(out, sizeof(float)) ||
        !aligned(gout, sizeof(float)))
        return MDX_ERR_MISALIGNED;
    for (int k = 0; k < nscales; ++k)
        if (!aligned(disp[k], sizeof(float)) || !aligned(ddisp[k], sizeof(float))) return MDX_ERR_MISALIGNED;
    for (int k = 0; k < nscales; ++k) {
        const int G = sd_group(h[k], w[k], gh, gw);
        const unsigned long long threads = (unsigned long long)B * h[k] * w[k] * G;      // < 2^38
        const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
        hipStream_t s = (hipStream_t)stream;
        if (G == 1) hipLaunchKernelGGL(sparse_depth_bwd_kernel<1>, grid, block, 0, s, g, k, out, gout, ddisp[k]);
        else if (G == 4) hipLaunchKernelGGL(sparse_depth_bwd_kernel<4>, grid, block, 0, s, g, k, out, gout, ddisp[k]);
        else if (G == 16) hipLaunchKernelGGL(sparse_depth_bwd_kernel<16>, grid, block, 0, s, g, k, out, gout, ddisp[k]);
        else hipLaunchKernelGGL(sparse_depth_bwd_kernel<64>, grid, block, 0, s, g, k, out, gout, ddisp[k]);
    }
    return check_launch();
}
