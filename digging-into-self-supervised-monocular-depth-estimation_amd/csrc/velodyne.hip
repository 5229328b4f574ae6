// velodyne.hip -- velodyne ground truth on the GPU: model_utility.point2depth -> resize_nearest -> fliplr -> float32 for a ragged
// batch of scans (include/mdx.h, mdx_velodyne_depth; the semantics are stated there and in DESIGN.md).
//
// Three launches, the kernel boundaries are the only ordering:
//   velo_mark_kernel    one thread per point: project in float64, store the point's pixel (-1: dropped) and float32 depth, and
//                       store 0 into the four scratch cells the point will vote on (every writer stores the same 0)
//   velo_vote_kernel    one thread per point: integer atomics on those cells -- atomicMax(last[pixel], i + 1),
//                       atomicAdd(count[g], 1), atomicMax(first[g], INT_MAX - i) (= the smallest i), atomicMax(near[g], ~key(d))
//                       (= the smallest d; key: the float's bits mapped to an unsigned integer of the same order)
//   velo_gather_kernel  one thread per output pixel: nearest-neighbour index, flip, last[pixel] -> that point's depth, overridden
//                       by near[g] iff count[g] >= 2 and the group's first point lies on this pixel
// Maxima, minima and counts of integers do not depend on the order in which the atomics arrive: the result is the same bits at
// every call.  The scratch is never cleared as a whole (16 bytes per native pixel: 89 MB for 12 KITTI frames, of which the points
// touch 3 %): a pixel nothing voted on holds whatever the allocator left there, and the gather believes last[pixel] = i + 1 only
// if i < n and point i's stored pixel IS this pixel -- true exactly when the cell was cleared and voted on in this call.  A pixel
// that passes has a voted g as well, so count / first / near need no test of their own.
#include <limits.h>
#include <string.h>
#include "mdx_common.hpp"

namespace mdx {

struct VeloJob {
    mdx_velodyne_job j;
    int *pix;            // [n]   pixel r*w + c of point i, -1 when dropped
    float *val;          // [n]   its depth, clamped at 0, float32
    int *cells;          // [4][h*w]: last (by pixel), count, first, near (by g)
};

struct VeloJobs {
    VeloJob job[MDX_VELO_JOBS];
};

// float bits -> unsigned integer with the same order (negative floats below positive ones)
__device__ __forceinline__ unsigned velo_key(float f)
{
    const unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float velo_unkey(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ int velo_group(int p, int w)
{
    const int r = p / w;
    return r * (w - 1) + (p - r * w);          // the reference's sub2ind + 1: (r, 0) and (r-1, w-1) coincide
}

__global__ __launch_bounds__(256) void velo_mark_kernel(const VeloJobs a)
{
    const VeloJob &J = a.job[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.j.n) return;
    const float *q = J.j.points + (size_t)i * J.j.stride;
    const float xf = q[0], yf = q[1], zf = q[2];
    int p = -1;
    float d32 = 0.0f;
    if (xf >= 0.0f) {                                               // (a NaN x is dropped, as numpy's velo[:, 0] >= 0 drops it)
        const double x = xf, y = yf, z = zf;
        const double *P = J.j.P;
        const double X = P[0] * x + P[1] * y + P[2] * z + P[3];
        const double Y = P[4] * x + P[5] * y + P[6] * z + P[7];
        const double Z = P[8] * x + P[9] * y + P[10] * z + P[11];
        const double c = rint(X / Z) - 1.0, r = rint(Y / Z) - 1.0;  // round half to even, as np.round
        // decided on the doubles: NaN and +-inf fail, and only values inside [0, w) x [0, h) are ever converted
        if (c >= 0.0 && r >= 0.0 && c < (double)J.j.w && r < (double)J.j.h) {
            p = (int)r * J.j.w + (int)c;
            const double d = J.j.vel_depth ? x : Z;
            d32 = d < 0.0 ? 0.0f : (float)d;                        // clamping is monotone: it commutes with the group minimum
        }
    }
    J.pix[i] = p;
    J.val[i] = d32;
    if (p >= 0) {
        const size_t hw = (size_t)J.j.h * J.j.w, g = velo_group(p, J.j.w);     // (4 * hw may pass int32)
        J.cells[p] = 0;
        J.cells[hw + g] = 0;
        J.cells[2 * hw + g] = 0;
        J.cells[3 * hw + g] = 0;
    }
}

__global__ __launch_bounds__(256) void velo_vote_kernel(const VeloJobs a)
{
    const VeloJob &J = a.job[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= J.j.n) return;
    const int p = J.pix[i];
    if (p < 0) return;
    const size_t hw = (size_t)J.j.h * J.j.w, g = velo_group(p, J.j.w);
    atomicMax(&J.cells[p], i + 1);                                   // last point on the pixel (0: none)
    atomicAdd(&J.cells[hw + g], 1);                                  // members of the group
    atomicMax(&J.cells[2 * hw + g], INT_MAX - i);                    // its first member
    atomicMax((unsigned *)&J.cells[3 * hw + g], ~velo_key(J.val[i]));   // its smallest depth
}

// resize_nearest's source index of output k: clip(rint((k + 0.5) * n_in / n_out - 0.5), 0, n_in - 1), in float64, numpy's order
__device__ __forceinline__ int velo_nearest(int k, int n_in, int n_out)
{
    if (n_in == n_out) return k;
    const double s = rint(((double)k + 0.5) * (double)n_in / (double)n_out - 0.5);
    return s < 0.0 ? 0 : (s > (double)(n_in - 1) ? n_in - 1 : (int)s);
}

__global__ __launch_bounds__(256) void velo_gather_kernel(const VeloJobs a)
{
    const VeloJob &J = a.job[blockIdx.y];
    const int gw = J.j.gw;
    const unsigned o = blockIdx.x * 256u + threadIdx.x;
    if (o >= (unsigned)(J.j.gh * gw)) return;
    const int R = (int)(o / (unsigned)gw), C = (int)o - R * gw;
    const int w = J.j.w, n = J.j.n;
    const size_t hw = (size_t)J.j.h * w;
    const int r = velo_nearest(R, J.j.h, J.j.gh), c = velo_nearest(J.j.flip ? gw - 1 - C : C, w, gw);
    const int p = r * w + c;
    float v = 0.0f;
    if (n > 0) {
        const int i = J.cells[p] - 1;
        if ((unsigned)i < (unsigned)n && J.pix[i] == p) {            // the cell was cleared and voted on in this call
            v = J.val[i];
            const size_t g = (size_t)(r * (w - 1) + c);
            const int head = INT_MAX - J.cells[2 * hw + g];
            if (J.cells[hw + g] >= 2 && (unsigned)head < (unsigned)n && J.pix[head] == p)
                v = velo_unkey(~(unsigned)J.cells[3 * hw + g]);
        }
    }
    J.j.out[o] = v;
}

static inline size_t velo_round16(size_t v) { return (v + 15) & ~(size_t)15; }

static inline size_t velo_job_bytes(long long n, long long h, long long w)
{
    return velo_round16((size_t)n * 8) + velo_round16((size_t)(h * w) * 16);
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_velodyne_workspace_bytes(int count, int nmax, int hmax, int wmax)
{
    if (count < 0 || nmax < 0 || nmax > INT_MAX - 256 || hmax < 1 || wmax < 2 || (long long)hmax * wmax > INT_MAX) return 0;
    return (size_t)count * velo_job_bytes(nmax, hmax, wmax);
}

MDX_EXPORT int mdx_velodyne_depth(const mdx_velodyne_job *jobs, int count, void *workspace, size_t workspace_bytes, void *stream)
{
    if (count < 0) return MDX_ERR_BAD_SHAPE;
    if (!jobs) return MDX_ERR_NULL_POINTER;
    size_t need = 0;
    for (int k = 0; k < count; ++k) {
        const mdx_velodyne_job &J = jobs[k];
        if (J.n < 0 || J.n > INT_MAX - 256 || J.h < 1 || J.w < 2 || J.gh < 1 || J.gw < 1) return MDX_ERR_BAD_SHAPE;
        if ((long long)J.h * J.w > INT_MAX || (long long)J.gh * J.gw > INT_MAX) return MDX_ERR_BAD_SHAPE;
        if (J.stride != 3 && J.stride != 4) return MDX_ERR_UNSUPPORTED;
        if (!J.out || (J.n > 0 && !J.points)) return MDX_ERR_NULL_POINTER;
        need += velo_job_bytes(J.n, J.h, J.w);
    }
    if (count == 0) return MDX_OK;
    if (!workspace || workspace_bytes < need) return MDX_ERR_WORKSPACE;
    if (!aligned(workspace, 16)) return MDX_ERR_MISALIGNED;
    hipStream_t st = (hipStream_t)stream;
    char *at = (char *)workspace;
    for (int first = 0; first < count; first += MDX_VELO_JOBS) {
        const int nj = count - first < MDX_VELO_JOBS ? count - first : MDX_VELO_JOBS;
        VeloJobs a;
        memset(&a, 0, sizeof(a));
        int max_n = 0, max_out = 0;
        for (int k = 0; k < nj; ++k) {
            VeloJob &V = a.job[k];
            V.j = jobs[first + k];
            V.pix = (int *)at;
            V.val = (float *)(at + (size_t)V.j.n * 4);
            at += velo_round16((size_t)V.j.n * 8);
            V.cells = (int *)at;
            at += velo_round16((size_t)V.j.h * V.j.w * 16);
            max_n = V.j.n > max_n ? V.j.n : max_n;
            max_out = V.j.gh * V.j.gw > max_out ? V.j.gh * V.j.gw : max_out;
        }
        if (max_n > 0) {
            const dim3 grid((unsigned)(max_n + 255) / 256, nj);
            hipLaunchKernelGGL(velo_mark_kernel, grid, dim3(256), 0, st, a);
            hipLaunchKernelGGL(velo_vote_kernel, grid, dim3(256), 0, st, a);
        }
        hipLaunchKernelGGL(velo_gather_kernel, dim3((unsigned)(((long long)max_out + 255) / 256), nj), dim3(256), 0, st, a);
    }
    return check_launch();
}
