// stereo_hints.hip -- stereo proxy depth: a semi-global matcher over a rectified pair, left-right checked, as depth hints (gfx950).
//
// THE DEFINITION is the one of include/mdx.h ("stereo proxy depth", items 1-10; mdx.functional.stereo_hints is the GPU form,
// mdx.composite.stereo_hints the plain-torch one): direction from T[b,0,3], float32 luma, 9 x 7 census, Hamming cost (31 outside),
// eight path recursions with penalties P1 / P2, S = their sum, first minima d0 and dR, the left-right check, a float32 parabola,
// depth = (K[b,0,0] * |T[b,0,3]|) / dsub.  Integers are exact; the floats are formed in the order stated there.
//
// THE FORM, twelve launches on one stream:
//   luma      one thread per pixel of either image                                     -> workspace luma maps
//   census    one thread per pixel of either image, 62 clamped reads of the luma map    -> workspace census maps (uint64)
//   8 x path  ONE WAVE PER PATH LINE, lanes hold disparities (D = 64: one per lane; D = 128: lane l holds 2l and 2l+1, so the
//             d-1 / d+1 neighbours of one are the other register or the adjacent lane's and no seam lies inside a register pair).
//             Per step: the cost from the two census maps (one wave-uniform 8-byte read, one per-lane read of adjacent words, a
//             popcount; the cost volume is never stored), the neighbours by DPP wave shifts, m by a DPP row reduction and one
//             readlane, then S[p, :] -- 128 / 256 contiguous bytes per wave -- written (first pass) or read, added to and written
//             (the other seven).  The next position's census words and this position's S are asked for before the dependent
//             min-chain of the step, so the walk waits for arithmetic and not for memory.  Every wave owns its line: each element
//             of S has exactly one writer per launch, and no launch depends on the order in which other waves arrive.
//   winners   one wave per pixel: d0 and dR as a wave minimum of (S << 8 | d) -- the smallest S, then the smallest d -- and the
//             parabola by lane 0                                                          -> workspace d0, dR; dsub into `disp`
//   outputs   one thread per pixel: the left-right check, disp / depth / valid.
// Bytes at D disparities over n = B*H*W pixels: S is 2 n D bytes; the path passes move (1 + 2*7) * 2 n D (2.83 GB at 12 x 192 x 640,
// D = 64), the winners read S twice.  A row sweep that carried three downward paths at once would halve the path traffic at the
// price of three chains per wave; it is not built (LABNOTES "Stereo proxy depth").
// No atomics, no host synchronisation, nothing to clear: capturable, and the same inputs give the same bits at every call.
#include <cmath>

#include "mdx_common.hpp"
#include "mdx_device.hpp"

namespace mdx {

constexpr int SH_BORDER_COST = 31;            // the cost of a match that leaves the image
constexpr int SH_ABSENT = 1 << 14;            // stands for the d-1 / d+1 term past the ends of the range: never the minimum
constexpr int SH_MAX_P2 = 190;                // 62 + P2 fits a byte
constexpr int SH_MAX_SIDE = 32767;

struct ShGeom {                               // kernel argument of every pass
    const float *target, *partner, *K, *T;
    int B, H, W, D, P1, P2;
    unsigned n;                               // B * H * W; n * D < 2^31
    uint16_t *S;                              // [B][H][W][D]
    unsigned long long *cen[2];               // [B][H][W], target / partner
    float *lum[2];                            // [B][H][W]
    uint8_t *d0, *dR;                         // [B][H][W]
    float *disp, *depth;
    uint8_t *valid;
};

// +1 / -1: where the match lies; 0: a sample without a usable baseline (zero, NaN, +-inf)
MDX_DEV int sh_dir(const float *T, int b)
{
    const float t = T[b * 16 + 3];
    if (!(fabsf(t) <= 3.402823466e+38f)) return 0;
    return t > 0.f ? 1 : t < 0.f ? -1 : 0;
}

// wave64 minimum that stays in the VALU, as wave_sum_dpp_lane63 (mdx_device.hpp): row_shr 1/2/4/8, row_bcast:15, row_bcast:31; a lane
// whose source lies outside its row (or a row outside the mask) keeps its own value.  Every lane must be active.  -> wave-uniform
MDX_DEV int sh_wave_min(int v)
{
#define MDX_DPP_MIN(ctrl, rowmask) v = min(v, __builtin_amdgcn_update_dpp(v, v, ctrl, rowmask, 0xf, false))
    MDX_DPP_MIN(0x111, 0xf);
    MDX_DPP_MIN(0x112, 0xf);
    MDX_DPP_MIN(0x114, 0xf);
    MDX_DPP_MIN(0x118, 0xf);
    MDX_DPP_MIN(0x142, 0xa);
    MDX_DPP_MIN(0x143, 0xc);
#undef MDX_DPP_MIN
    return __builtin_amdgcn_readlane(v, 63);
}

// lane l <- lane l-1 (lane 0: SH_ABSENT) and lane l <- lane l+1 (lane 63: SH_ABSENT): wave_shr:1 / wave_shl:1
MDX_DEV int sh_from_below(int v) { return __builtin_amdgcn_update_dpp(SH_ABSENT, v, 0x138, 0xf, 0xf, false); }
MDX_DEV int sh_from_above(int v) { return __builtin_amdgcn_update_dpp(SH_ABSENT, v, 0x130, 0xf, 0xf, false); }

__global__ void __launch_bounds__(256) stereo_hints_luma_kernel(ShGeom g)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= 2u * g.n) return;
    const unsigned which = i >= g.n ? 1u : 0u, j = i - which * g.n;
    const unsigned hw = (unsigned)g.H * (unsigned)g.W, b = j / hw, p = j - b * hw;
    const float *src = (which ? g.partner : g.target) + (size_t)b * 3u * hw + p;
    g.lum[which][j] = (0.299f * src[0] + 0.587f * src[hw]) + 0.114f * src[2u * hw];
}

__global__ void __launch_bounds__(256) stereo_hints_census_kernel(ShGeom g)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= 2u * g.n) return;
    const unsigned which = i >= g.n ? 1u : 0u, j = i - which * g.n;
    const int H = g.H, W = g.W;
    const unsigned hw = (unsigned)H * (unsigned)W, b = j / hw, p = j - b * hw;
    const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
    const float *L = g.lum[which] + (size_t)b * hw;
    const float centre = L[p];
    unsigned long long word = 0;
    for (int dy = -3; dy <= 3; ++dy) {
        const int yy = min(max(y + dy, 0), H - 1);
#pragma unroll
        for (int dx = -4; dx <= 4; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int xx = min(max(x + dx, 0), W - 1);
            word = (word << 1) | (L[(unsigned)yy * (unsigned)W + (unsigned)xx] < centre ? 1ull : 0ull);
        }
    }
    g.cen[which][j] = word;
}

// The costs of position (y,x) for this lane's DPL disparities.  ct / cs: the census maps of the sample.
template <int DPL>
MDX_DEV void sh_cost(const unsigned long long *ct, const unsigned long long *cs, int W, int y, int x, int dir, int lane, int (&C)[DPL])
{
    const unsigned row = (unsigned)y * (unsigned)W;
    const unsigned long long t = ct[row + (unsigned)x];
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
        const int xs = x + dir * (lane * DPL + j);
        const bool inside = (unsigned)xs < (unsigned)W;
        const unsigned long long s = inside ? cs[row + (unsigned)xs] : 0ull;
        C[j] = inside ? __builtin_popcountll(t ^ s) : SH_BORDER_COST;
    }
}

// One path direction (dy,dx): a wave walks one line from the pixel whose predecessor lies outside the image to the far edge.
template <int DPL>
__global__ void __launch_bounds__(256) stereo_hints_path_kernel(ShGeom g, int dy, int dx, int first)
{
    constexpr int D = 64 * DPL;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    const int H = g.H, W = g.W, P1 = g.P1, P2 = g.P2;
    const unsigned lines = dy == 0 ? (unsigned)H : dx == 0 ? (unsigned)W : (unsigned)(W + H - 1);
    if (wave >= lines * (unsigned)g.B) return;                                            // whole waves leave
    const int b = (int)(wave / lines), l = (int)(wave - (unsigned)b * lines);
    int y, x;
    if (dy == 0) { y = l; x = dx > 0 ? 0 : W - 1; }
    else if (dx == 0) { x = l; y = dy > 0 ? 0 : H - 1; }
    else if (l < W) { x = l; y = dy > 0 ? 0 : H - 1; }
    else { const int k = l - W + 1; x = dx > 0 ? 0 : W - 1; y = dy > 0 ? k : H - 1 - k; }   // k = 1 .. H-1
    const int dir = sh_dir(g.T, b);
    const size_t img = (size_t)b * (unsigned)H * (unsigned)W;
    uint16_t *S = g.S + img * D + (unsigned)(lane * DPL);
    const unsigned long long *ct = g.cen[0] + img, *cs = g.cen[1] + img;

    if (dir == 0) {                                                                        // a dead sample: S is all zeros
        if (first)
            for (; (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W; y += dy, x += dx)
#pragma unroll
                for (int j = 0; j < DPL; ++j) S[(size_t)((unsigned)y * (unsigned)W + (unsigned)x) * D + j] = 0;
        return;
    }

    int C[DPL], L[DPL];
    sh_cost<DPL>(ct, cs, W, y, x, dir, lane, C);
    bool start = true;
    for (;;) {
        uint16_t *at = S + (size_t)((unsigned)y * (unsigned)W + (unsigned)x) * D;
        int sum[DPL];
#pragma unroll
        for (int j = 0; j < DPL; ++j) sum[j] = first ? 0 : (int)at[j];
        const int ny = y + dy, nx = x + dx;
        const bool more = (unsigned)ny < (unsigned)H && (unsigned)nx < (unsigned)W;        // wave-uniform
        int Cn[DPL];
#pragma unroll
        for (int j = 0; j < DPL; ++j) Cn[j] = 0;
        if (more) sh_cost<DPL>(ct, cs, W, ny, nx, dir, lane, Cn);
        if (start) {
#pragma unroll
            for (int j = 0; j < DPL; ++j) L[j] = C[j];
            start = false;
        } else if (DPL == 1) {
            const int m = sh_wave_min(L[0]);
            const int side = min(sh_from_below(L[0]), sh_from_above(L[0])) + P1;
            L[0] = C[0] + min(min(L[0], side), m + P2) - m;
        } else {
            const int m = sh_wave_min(min(L[0], L[DPL - 1]));
            const int even = min(sh_from_below(L[DPL - 1]), L[DPL - 1]) + P1;              // d = 2l: 2l-1 is lane l-1's odd one
            const int odd = min(L[0], sh_from_above(L[0])) + P1;                           // d = 2l+1: 2l+2 is lane l+1's even one
            const int l0 = C[0] + min(min(L[0], even), m + P2) - m;
            const int l1 = C[DPL - 1] + min(min(L[DPL - 1], odd), m + P2) - m;
            L[0] = l0; L[DPL - 1] = l1;
        }
#pragma unroll
        for (int j = 0; j < DPL; ++j) at[j] = (uint16_t)(sum[j] + L[j]);
        if (!more) break;
        y = ny; x = nx;
#pragma unroll
        for (int j = 0; j < DPL; ++j) C[j] = Cn[j];
    }
}

// d0, dR and the sub-pixel disparity of one pixel per wave.
template <int DPL>
__global__ void __launch_bounds__(256) stereo_hints_winner_kernel(ShGeom g)
{
    constexpr int D = 64 * DPL;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    if (wave >= g.n) return;
    const int W = g.W;
    const unsigned hw = (unsigned)g.H * (unsigned)W, b = wave / hw, p = wave - b * hw;
    const int y = (int)(p / (unsigned)W), x = (int)(p - (unsigned)y * (unsigned)W);
    const int dir = sh_dir(g.T, (int)b);
    if (dir == 0) {
        if (lane == 0) { g.d0[wave] = 0; g.dR[wave] = 0; g.disp[wave] = 0.f; }
        return;
    }
    const uint16_t *Simg = g.S + (size_t)b * hw * D;
    const uint16_t *Sp = Simg + (size_t)p * D;
    int k0 = 0x7fffffff, kr = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < DPL; ++j) {
        const int d = lane * DPL + j;
        k0 = min(k0, ((int)Sp[d] << 8) | d);
        const int col = x - dir * d;
        if ((unsigned)col < (unsigned)W) kr = min(kr, ((int)Simg[(size_t)((unsigned)y * (unsigned)W + (unsigned)col) * D + d] << 8) | d);
    }
    k0 = sh_wave_min(k0);
    kr = sh_wave_min(kr);                                                                   // d = 0 is always inside
    if (lane == 0) {
        const int d0 = k0 & 255;
        float dsub = (float)d0;
        if (d0 > 0 && d0 < D - 1) {
            const float a = (float)Sp[d0 - 1], m = (float)Sp[d0], c = (float)Sp[d0 + 1];
            const float den = (a + c) - 2.f * m;
            if (den > 0.f) dsub = (float)d0 + (a - c) / (2.f * den);
        }
        g.d0[wave] = (uint8_t)d0;
        g.dR[wave] = (uint8_t)(kr & 255);
        g.disp[wave] = dsub;
    }
}

__global__ void __launch_bounds__(256) stereo_hints_output_kernel(ShGeom g)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= g.n) return;
    const int W = g.W;
    const unsigned hw = (unsigned)g.H * (unsigned)W, b = i / hw, p = i - b * hw;
    const int x = (int)(p % (unsigned)W);
    const int dir = sh_dir(g.T, (int)b);
    const int d0 = (int)g.d0[i];
    const int xm = x + dir * d0;
    bool ok = dir != 0 && d0 >= 1 && (unsigned)xm < (unsigned)W;
    if (ok) {
        const int back = (int)g.dR[i - (unsigned)x + (unsigned)xm];
        ok = abs(back - d0) <= 1;
    }
    const float dsub = g.disp[i];
    const float num = g.K[b * 16] * fabsf(g.T[b * 16 + 3]);
    g.disp[i] = ok ? dsub : 0.f;
    g.depth[i] = ok ? num / dsub : 0.f;
    g.valid[i] = ok ? 1 : 0;
}

static inline size_t sh_round8(size_t v) { return (v + 7) & ~(size_t)7; }

// the pixels of a call, or 0 for sizes it refuses
static unsigned sh_pixels(int B, int H, int W, int D)
{
    if (B < 1 || H < 1 || W < 1 || H > SH_MAX_SIDE || W > SH_MAX_SIDE || (D != 64 && D != 128)) return 0;
    const long long n = (long long)B * H * W;
    return n * D < (1ll << 31) ? (unsigned)n : 0;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_stereo_hints_workspace_bytes(int B, int H, int W, int D)
{
    const size_t n = sh_pixels(B, H, W, D);
    if (n == 0) return 0;
    return n * (size_t)D * sizeof(uint16_t) + 2 * n * sizeof(unsigned long long) + 2 * sh_round8(n * sizeof(float)) + 2 * sh_round8(n);
}

MDX_EXPORT int mdx_stereo_hints(const float *target, const float *partner, const float *K, const float *T, int B, int H, int W, int D,
                                int P1, int P2, float *disp, float *depth, unsigned char *valid, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    if (!target || !partner || !K || !T || !disp || !depth || !valid) return MDX_ERR_NULL_POINTER;
    const unsigned n = sh_pixels(B, H, W, D);
    if (n == 0 || !(0 < P1 && P1 < P2 && P2 <= SH_MAX_P2)) return MDX_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < mdx_stereo_hints_workspace_bytes(B, H, W, D)) return MDX_ERR_WORKSPACE;
    if (!aligned(workspace, 8) || !aligned(target, sizeof(float)) || !aligned(partner, sizeof(float)) || !aligned(K, sizeof(float)) ||
        !aligned(T, sizeof(float)) || !aligned(disp, sizeof(float)) || !aligned(depth, sizeof(float)))
        return MDX_ERR_MISALIGNED;
    ShGeom g;
    g.target = target; g.partner = partner; g.K = K; g.T = T;
    g.B = B; g.H = H; g.W = W; g.D = D; g.P1 = P1; g.P2 = P2; g.n = n;
    char *at = (char *)workspace;
    g.S = (uint16_t *)at;                  at += (size_t)n * D * sizeof(uint16_t);
    g.cen[0] = (unsigned long long *)at;   at += (size_t)n * sizeof(unsigned long long);
    g.cen[1] = (unsigned long long *)at;   at += (size_t)n * sizeof(unsigned long long);
    g.lum[0] = (float *)at;                at += sh_round8((size_t)n * sizeof(float));
    g.lum[1] = (float *)at;                at += sh_round8((size_t)n * sizeof(float));
    g.d0 = (uint8_t *)at;                  at += sh_round8(n);
    g.dR = (uint8_t *)at;
    g.disp = disp; g.depth = depth; g.valid = valid;
    hipStream_t s = (hipStream_t)stream;
    const dim3 block(256);
    const dim3 both((2u * n + 255u) / 256u), each((n + 255u) / 256u), waves((n + 3u) / 4u);
    hipLaunchKernelGGL(stereo_hints_luma_kernel, both, block, 0, s, g);
    hipLaunchKernelGGL(stereo_hints_census_kernel, both, block, 0, s, g);
    static const int steps[8][2] = {{0, 1}, {0, -1}, {1, 0}, {-1, 0}, {1, 1}, {1, -1}, {-1, 1}, {-1, -1}};
    for (int r = 0; r < 8; ++r) {
        const int dy = steps[r][0], dx = steps[r][1];
        const unsigned lines = (dy == 0 ? (unsigned)H : dx == 0 ? (unsigned)W : (unsigned)(W + H - 1)) * (unsigned)B;
        const dim3 grid((lines + 3u) / 4u);
        if (D == 64) hipLaunchKernelGGL(stereo_hints_path_kernel<1>, grid, block, 0, s, g, dy, dx, r == 0 ? 1 : 0);
        else hipLaunchKernelGGL(stereo_hints_path_kernel<2>, grid, block, 0, s, g, dy, dx, r == 0 ? 1 : 0);
    }
    if (D == 64) hipLaunchKernelGGL(stereo_hints_winner_kernel<1>, waves, block, 0, s, g);
    else hipLaunchKernelGGL(stereo_hints_winner_kernel<2>, waves, block, 0, s, g);
    hipLaunchKernelGGL(stereo_hints_output_kernel, each, block, 0, s, g);
    return check_launch();
}
