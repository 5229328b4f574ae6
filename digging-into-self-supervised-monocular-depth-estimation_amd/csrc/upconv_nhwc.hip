// upconv_nhwc.hip -- the decoder's last stage convolution on the LOW-resolution map, gfx950 MFMA.
//
// model_layer/depth_decoder.py, stage 0, second ConvBlock: conv3x3(ReflectionPad2d(1)(nearest_x2(ELU(raw + bias)))) of a 16-channel
// map, the only stage convolution without a skip connection.  Its input is a 4x replicated copy, so the output pixel (2Y+py, 2X+px)
// reads, through kernel row ky, the low-resolution row Y + off(py, ky) with off(p, k) = floor((p + k - 1) / 2):
//     py = 0: {-1, 0, 0}      py = 1: {0, 0, +1}                                            (columns alike)
// Each of the four output phases (py, px) is therefore a 2x2 convolution of the low-resolution map whose four 16 x 16 matrices
// Wq[py][px][dy][dx] are sums of the 3x3 taps that land on the same pixel, and the reflection pad of the x2 map is a clamp of the
// low-resolution index (row -1 -> x2 row 1 -> row 0; row 2h -> x2 row 2h-2 -> row h-1).  4/9 of the flops, a quarter of the input,
// and neither the padded x2 copy nor its gradient map is ever written.
//
//   forward   a wave owns 16 pixels of a low-resolution row and walks down a run of rows with a 3 x 3 window of ELU'd channel
//             vectors in registers; D[co][pixel] = Wq (A operand, 64 registers, formed once per wave from the 3x3 weight) x window
//             (B operand: the lane's own 16-byte load, contraction index permuted to match), 64 v_mfma_f32_16x16x4_f32 a row, four
//             16-byte stores per lane.
//   dgrad     the transpose as a gather: the low-resolution pixel (Yv, Xv) collects the 4 x 4 output-gradient pixels
//             (2Yv-1.., 2Xv-1..), each through one transposed Wq.  The clamp's transpose -- border pixels also receive what the
//             virtual row -1 / h and column -1 / w would -- is the same gather at the virtual index, added into the same
//             accumulators (rows: wave-uniform; columns: the two border lanes of the first / last strip).  Times ELU', stored;
//             d(bias) as one partial per wave.
//   wgrad     G[py][px][dy][dx] = sum gy (x) a over runs of pixel quads, 16 accumulator tiles in registers (thinconv_nhwc.hip's
//             scheme), block partials; the finishing pass adds them in a fixed order, recombines
//             gw[ky][kx] = sum over the phases of G[py][px][off(py, ky)][off(px, kx)] and finishes d(bias).  No atomics.
#include <type_traits>

#include "nhwc_common.hpp"

namespace mdx {
namespace nhwc {

typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : __expf(x) - 1.0f; }   // glue_nhwc.hip's expression
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }
__device__ __forceinline__ v4f load4(const float *p) { return *reinterpret_cast<const v4f *>(p); }
__device__ __forceinline__ void store4(float *p, v4f v) { *reinterpret_cast<v4f *>(p) = v; }
__device__ __forceinline__ v4f elu4(v4f r, v4f b)
{
    return (v4f){elu1(r.x + b.x), elu1(r.y + b.y), elu1(r.z + b.z), elu1(r.w + b.w)};
}

// which of a phase's two offsets (0: p - 1, 1: p) kernel tap k lands on: off(p, k) - (p - 1)
__host__ __device__ constexpr int tap_slot(int p, int k) { return (p + k + 1) / 2 - p; }

// Wq[py][px][dy][dx][c] for one lane: the sum of the taps t[ky][kx][c] that land there, in (ky, kx) order
__device__ __forceinline__ void presum(const float (&t)[3][3][4], float (&wq)[2][2][2][2][4])
{
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
        for (int px = 0; px < 2; ++px)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float s[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
                bool any[2][2] = {{false, false}, {false, false}};
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int dy = tap_slot(py, ky), dx = tap_slot(px, kx);
                        s[dy][dx] = any[dy][dx] ? s[dy][dx] + t[ky][kx][c] : t[ky][kx][c];
                        any[dy][dx] = true;
                    }
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) wq[py][px][dy][dx][c] = s[dy][dx];
            }
}

constexpr int UC_WAVES = 4;                    // waves per block, forward and data gradient: one (image, row run, strip) each
constexpr int UC_PIX = 16;                     // low-resolution pixels of a strip

struct UpItem { int b, y0, y1, strip; bool any; };
__device__ __forceinline__ UpItem up_item(int B, int h, int rows_per_wave, int nstrips, int nruns)
{
    UpItem it;
    const long long g = (long long)blockIdx.x * UC_WAVES + (threadIdx.x >> 6);
    it.any = g < (long long)B * nruns * nstrips;
    it.strip = (int)(g % nstrips);
    const long long r = g / nstrips;
    const int run = (int)(r % nruns);
    it.b = it.any ? (int)(r / nruns) : 0;
    it.y0 = run * rows_per_wave;
    it.y1 = it.y0 + rows_per_wave < h ? it.y0 + rows_per_wave : h;
    return it;
}

// ---- forward: raw [B][h][w][16], out [B][2h][2w][16] -----------------------------------------------------------------------------
__global__ __launch_bounds__(64 * UC_WAVES) void up_conv3x3_fwd_kernel(const float *__restrict__ raw, const float *__restrict__ bias,
                                                                       const float *__restrict__ wt, long wso, long wsc, long wsy,
                                                                       long wsx, float *__restrict__ out, int B, int h, int w,
                                                                       int rows_per_wave, int nstrips, int nruns)
{
    const UpItem it = up_item(B, h, rows_per_wave, nstrips, nruns);
    if (!it.any) return;
    const int lane = threadIdx.x & 63, p = lane & 15, cq = lane >> 4;
    // A operand of chunk c: Wq[co = lane % 16][ci = 4 * (lane / 16) + c]; the B operand's four contraction slots of chunk c are then
    // the channels 4 * cq + c of the lane's pixel = component c of its 16-byte load
    float wq[2][2][2][2][4];
    {
        float t[3][3][4];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int c = 0; c < 4; ++c) t[ky][kx][c] = wt[p * wso + (4 * cq + c) * wsc + ky * wsy + kx * wsx];
        presum(t, wq);
    }
    const v4f bv = (v4f){bias[4 * cq], bias[4 * cq + 1], bias[4 * cq + 2], bias[4 * cq + 3]};
    const int X = it.strip * UC_PIX + p;
    const int xs[3] = {clampi(X - 1, w), clampi(X, w), clampi(X + 1, w)};
    const float *img = raw + (size_t)it.b * h * w * 16 + 4 * cq;
    auto load_row = [&](int Y, v4f (&r)[3]) {
        const float *row = img + (size_t)clampi(Y, h) * w * 16;
#pragma unroll
        for (int d = 0; d < 3; ++d) r[d] = load4(row + (size_t)xs[d] * 16);
    };
    v4f win[3][3], nxt[3];
    load_row(it.y0 - 1, win[0]);
    load_row(it.y0, win[1]);
    load_row(it.y0 + 1, win[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) win[r][d] = elu4(win[r][d], bv);
    const int H2 = 2 * h, W2 = 2 * w;
    for (int Y = it.y0; Y < it.y1; ++Y) {
        load_row(Y + 2, nxt);                            // in flight under this row's MFMAs
        v4f acc[2][2];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) acc[py][px] = (v4f){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ry = 0; ry < 3; ++ry)
#pragma unroll
            for (int rx = 0; rx < 3; ++rx)
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int py = 0; py < 2; ++py)
#pragma unroll
                        for (int px = 0; px < 2; ++px) {
                            const int dy = ry - py, dx = rx - px;            // window row ry = offset ry - 1 = (py - 1) + dy
                            if (dy < 0 || dy > 1 || dx < 0 || dx > 1) continue;
                            acc[py][px] = __builtin_amdgcn_mfma_f32_16x16x4f32(wq[py][px][dy][dx][c], win[ry][rx][c], acc[py][px], 0, 0, 0);
                        }
        // D[co][pixel]: the lane holds co = 4 * cq + v of pixel p
        if (X < w) {
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px)
                    store4(out + (((size_t)it.b * H2 + 2 * Y + py) * W2 + 2 * X + px) * 16 + 4 * cq, acc[py][px]);
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            win[0][d] = win[1][d];
            win[1][d] = win[2][d];
            win[2][d] = elu4(nxt[d], bv);
        }
    }
}

// ---- data gradient: gy [B][2h][2w][16] -> graw [B][h][w][16], bias_part [waves][16] ----------------------------------------------
// The gradient row R = 2P+1 (odd) or 2P+2 (even) reaches the low-resolution rows P (through r = R - 2P = 1, 2) and P + 1 (r = -1, 0):
// a wave walks the gradient rows 2 y0 - 1 .. 2 y1 of its run once, each row's four 16-byte loads a row ahead of its MFMAs, with the
// accumulator of row P (cur) and of row P + 1 (nxt) alive.  The clamp's transpose: row -1's accumulator is added to row 0's, row
// h's to row h-1's; column -1's share is the border lane's own gradient pixel 0 through the s = 2 matrices, column w's its pixel
// 2w-1 through the s = -1 matrices (two more operands, first / last strip only).
__global__ __launch_bounds__(64 * UC_WAVES) void up_conv3x3_dgrad_kernel(const float *__restrict__ gy, const float *__restrict__ raw,
                                                                         const float *__restrict__ bias, const float *__restrict__ wt,
                                                                         long wso, long wsc, long wsy, long wsx, float *__restrict__ graw,
                                                                         float *__restrict__ bias_part, int B, int h, int w,
                                                                         int rows_per_wave, int nstrips, int nruns)
{
    const UpItem it = up_item(B, h, rows_per_wave, nstrips, nruns);
    if (!it.any) return;
    const int lane = threadIdx.x & 63, p = lane & 15, cq = lane >> 4;
    // The gradient pixel (2Yv + r, 2Xv + s), r, s = -1 .. 2, reaches (Yv, Xv) through Wq[py][dy]^T with r = py - 2 * off:
    // r = -1: (py 1, off +1)   0: (0, 0)   1: (1, 0)   2: (0, -1).  A operand of chunk c: Wq[co = 4 * cq + c][ci = lane % 16].
    float vq[4][4][4];
    {
        float t[3][3][4], wq[2][2][2][2][4];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int c = 0; c < 4; ++c) t[ky][kx][c] = wt[(4 * cq + c) * wso + p * wsc + ky * wsy + kx * wsx];
        presum(t, wq);
        constexpr int PH[4] = {1, 0, 1, 0}, SL[4] = {1, 1, 0, 0};
#pragma unroll
        for (int ri = 0; ri < 4; ++ri)
#pragma unroll
            for (int si = 0; si < 4; ++si)
#pragma unroll
                for (int c = 0; c < 4; ++c) vq[ri][si][c] = wq[PH[ri]][PH[si]][SL[ri]][SL[si]][c];
    }
    const v4f bv = (v4f){bias[4 * cq], bias[4 * cq + 1], bias[4 * cq + 2], bias[4 * cq + 3]};
    const int X = it.strip * UC_PIX + p, H2 = 2 * h, W2 = 2 * w;
    const bool in_map = X < w;
    const bool edge_strip = it.strip == 0 || it.strip == nstrips - 1;
    const bool first_col = X == 0, last_col = X == w - 1;
    // the lane's four gradient columns 2X - 1 .. 2X + 2: offsets clamped into the map, validity a property of the lane
    int col[4];
    bool col_ok[4];
#pragma unroll
    for (int si = 0; si < 4; ++si) {
        const int S = 2 * X + si - 1;
        col_ok[si] = in_map && S >= 0 && S < W2;
        col[si] = clampi(S, W2) * 16;
    }
    const float *gimg = gy + (size_t)it.b * H2 * W2 * 16 + 4 * cq;
    const v4f zero = (v4f){0.f, 0.f, 0.f, 0.f};
    auto load_row = [&](int R, v4f (&g)[4]) {              // R clamped: a row outside the map is loaded (in bounds) and not used
        const float *row = gimg + (size_t)clampi(R, H2) * W2 * 16;
#pragma unroll
        for (int si = 0; si < 4; ++si) g[si] = load4(row + col[si]);
    };
    // one gradient row into the accumulator(s) it reaches: RA = r + 1 of the row towards row P, RB towards row P + 1
    auto row_step = [&](auto ra, auto rb, v4f (&g)[4], bool to_cur, bool to_nxt, v4f &cur, v4f &nxt) {
        constexpr int RA = decltype(ra)::value, RB = decltype(rb)::value;
#pragma unroll
        for (int si = 0; si < 4; ++si) g[si] = col_ok[si] ? g[si] : zero;
        v4f e[2] = {zero, zero};
        if (edge_strip) {
            e[0] = last_col ? g[2] : zero;                 // virtual column w: pixel 2w - 1 through s = -1
            e[1] = first_col ? g[1] : zero;                // virtual column -1: pixel 0 through s = 2
        }
        if (to_cur && to_nxt) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int si = 0; si < 4; ++si) {
                    cur = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RA][si][c], g[si][c], cur, 0, 0, 0);
                    nxt = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RB][si][c], g[si][c], nxt, 0, 0, 0);
                }
            if (edge_strip) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        cur = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RA][3 * k][c], e[k][c], cur, 0, 0, 0);
                        nxt = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RB][3 * k][c], e[k][c], nxt, 0, 0, 0);
                    }
            }
        } else {
            // a run's first and last rows and the map's borders: one target only
            if (to_cur) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int si = 0; si < 4; ++si) cur = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RA][si][c], g[si][c], cur, 0, 0, 0);
#pragma unroll
                    for (int k = 0; k < 2; ++k) cur = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RA][3 * k][c], e[k][c], cur, 0, 0, 0);
                }
            }
            if (to_nxt) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#pragma unroll
                    for (int si = 0; si < 4; ++si) nxt = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RB][si][c], g[si][c], nxt, 0, 0, 0);
#pragma unroll
                    for (int k = 0; k < 2; ++k) nxt = __builtin_amdgcn_mfma_f32_16x16x4f32(vq[RB][3 * k][c], e[k][c], nxt, 0, 0, 0);
                }
            }
        }
    };
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    v4f cur = zero, nxt = zero, g0[4], g1[4];
    load_row(2 * it.y0 - 1, g0);
    for (int P = it.y0 - 1; P < it.y1; ++P) {
        // row P collects (P in the run, or the virtual row -1 above row 0); row P + 1 collects (in the run, or the virtual row h)
        const bool to_cur = P >= it.y0 || P < 0, to_nxt = P + 1 < it.y1 || P + 1 >= h;
        const size_t at = (((size_t)it.b * h + (P < it.y0 ? it.y0 : P)) * w + (in_map ? X : w - 1)) * 16 + 4 * cq;
        const v4f rv = load4(raw + at);
        load_row(2 * P + 2, g1);
        if (P >= 0) row_step(std::integral_constant<int, 2>(), std::integral_constant<int, 0>(), g0, to_cur, to_nxt, cur, nxt);
        load_row(2 * P + 3, g0);
        if (P + 1 < h) row_step(std::integral_constant<int, 3>(), std::integral_constant<int, 1>(), g1, to_cur, to_nxt, cur, nxt);
        if (P + 1 >= h) cur += nxt;                        // the virtual row h lands on row h - 1
        if (P >= it.y0) {
            // D[ci][pixel]: the lane holds ci = 4 * cq + v of pixel p
            v4f o;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float pre = rv[v] + bv[v];
                o[v] = !(pre > 0.f) ? cur[v] * __expf(pre) : cur[v];
                bsum[v] += in_map ? o[v] : 0.f;
            }
            if (in_map) store4(graw + at, o);
        }
        cur = P < 0 ? cur + nxt : nxt;                     // the virtual row -1 lands on row 0
        nxt = zero;
    }
    // d(bias): this wave's sum over its pixels, the 16 pixel lanes of a channel group added in a fixed (butterfly) order
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        float s = bsum[v];
        s += __shfl_xor(s, 8, 64);
        s += __shfl_xor(s, 4, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        bsum[v] = s;
    }
    if (p == 0) {
        const size_t g = (size_t)blockIdx.x * UC_WAVES + (threadIdx.x >> 6);
        store4(bias_part + g * 16 + 4 * cq, (v4f){bsum[0], bsum[1], bsum[2], bsum[3]});
    }
}

// ---- weight gradient: part [blocks][(py, px, dy, dx)][co][ci] ----------------------------------------------------------------------
constexpr int UW_WAVES = 8;                    // waves per block
constexpr int UW_ROUND = 4;                    // accumulator tiles that cross the LDS together

__global__ __launch_bounds__(64 * UW_WAVES) void up_conv3x3_wgrad_kernel(const float *__restrict__ gy, const float *__restrict__ raw,
                                                                         const float *__restrict__ bias, int B, int h, int w,
                                                                         int quads_per_wave, float *__restrict__ part)
{
    __shared__ float lds[UW_WAVES][UW_ROUND][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = lane >> 4, j = lane & 15;                       // pixel of the quad, channel
    const int wq4 = w / 4, W2 = 2 * w;
    const long long nquads = (long long)B * h * wq4;
    const long long q0 = ((long long)blockIdx.x * UW_WAVES + wave) * quads_per_wave;
    const long long q1 = q0 + quads_per_wave < nquads ? q0 + quads_per_wave : nquads;
    v4f acc[2][2][2][2];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t >> 3][(t >> 2) & 1][(t >> 1) & 1][t & 1] = (v4f){0.f, 0.f, 0.f, 0.f};
    if (q0 < q1) {
        const float bj = bias[j];
        int qx = (int)(q0 % wq4);
        const long long row0 = q0 / wq4;
        int Y = (int)(row0 % h), b = (int)(row0 / h);
        // A: gy[co = j] of the quad's pixel k in the four phases; B: the 3 x 3 clamped window of a = ELU(raw + bias)[ci = j]
        auto load_a = [&](float (&a)[2][2]) {
            const float *g = gy + (((size_t)b * 2 * h + 2 * Y) * W2 + 2 * (qx * 4 + k)) * 16 + j;
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px) a[py][px] = g[((size_t)py * W2 + px) * 16];
        };
        auto load_b = [&](float (&bw)[3][3]) {
            const int X = qx * 4 + k;
#pragma unroll
            for (int ry = 0; ry < 3; ++ry) {
                const float *row = raw + ((size_t)b * h + clampi(Y + ry - 1, h)) * w * 16 + j;
#pragma unroll
                for (int rx = 0; rx < 3; ++rx) bw[ry][rx] = row[(size_t)clampi(X + rx - 1, w) * 16];
            }
        };
        float a0[2][2], b0[3][3];
        load_a(a0);
        load_b(b0);
        for (long long q = q0; q < q1; ++q) {
            float a1[2][2] = {{0.f, 0.f}, {0.f, 0.f}}, b1[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            if (++qx == wq4) {
                qx = 0;
                if (++Y == h) { Y = 0; ++b; }
            }
            if (q + 1 < q1) {                            // the next quad's thirteen loads are issued before this quad's MFMAs
                load_a(a1);
                load_b(b1);
            }
#pragma unroll
            for (int ry = 0; ry < 3; ++ry)
#pragma unroll
                for (int rx = 0; rx < 3; ++rx) b0[ry][rx] = elu1(b0[ry][rx] + bj);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
#pragma unroll
                    for (int py = 0; py < 2; ++py)
#pragma unroll
                        for (int px = 0; px < 2; ++px)
                            acc[py][px][dy][dx] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[py][px], b0[py + dy][px + dx], acc[py][px][dy][dx], 0, 0, 0);
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
                for (int px = 0; px < 2; ++px) a0[py][px] = a1[py][px];
#pragma unroll
            for (int ry = 0; ry < 3; ++ry)
#pragma unroll
                for (int rx = 0; rx < 3; ++rx) b0[ry][rx] = b1[ry][rx];
        }
    }
    // D[co][ci]: lane holds rows 4 * (lane / 16) + v, column lane % 16; the block's waves are added in wave order
    float *dst = part + (size_t)blockIdx.x * 16 * 256;
#pragma unroll
    for (int t0 = 0; t0 < 16; t0 += UW_ROUND) {
#pragma unroll
        for (int u = 0; u < UW_ROUND; ++u) {
            const int t = t0 + u;
            const v4f d = acc[t >> 3][(t >> 2) & 1][(t >> 1) & 1][t & 1];
#pragma unroll
            for (int v = 0; v < 4; ++v) lds[wave][u][(4 * k + v) * 16 + j] = d[v];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < UW_ROUND * 256; e += 64 * UW_WAVES) {
            float s = lds[0][e >> 8][e & 255];
#pragma unroll
            for (int u = 1; u < UW_WAVES; ++u) s += lds[u][e >> 8][e & 255];
            dst[t0 * 256 + e] = s;
        }
        __syncthreads();
    }
}

// gw[co][ci][ky][kx] (the weight's strides) = sum over the blocks and the four phases of part[.][(py, px, slot(py, ky), slot(px, kx))][co][ci];
// the last block: gbias[c] = sum over the data gradient's waves of bias_part[.][c].  16 elements x 64 sub-sums a block, fixed order.
constexpr int UF_S = 64;
__global__ __launch_bounds__(16 * UF_S) void up_conv3x3_finish_kernel(const float *__restrict__ part, int nblk,
                                                                      const float *__restrict__ bias_part, int nwaves, long wso, long wsc,
                                                                      long wsy, long wsx, float *__restrict__ gw, float *__restrict__ gbias)
{
    __shared__ float lds[UF_S / 4][16];
    const int cl = threadIdx.x % 16, sl = threadIdx.x / 16;
    const bool for_bias = blockIdx.x == gridDim.x - 1;
    const int e = blockIdx.x * 16 + cl;                            // weight element (tap, co, ci)
    const int tap = e >> 8, r = e & 255, ky = tap / 3, kx = tap % 3;
    float s = 0.f;
    if (for_bias) {
        for (int i0 = sl; i0 < nwaves; i0 += UF_S * 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * UF_S;
                v[u] = i < nwaves ? bias_part[(size_t)i * 16 + cl] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    } else {
        int tile[4];
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
            for (int px = 0; px < 2; ++px) tile[py * 2 + px] = (((py * 2 + px) * 2 + tap_slot(py, ky)) * 2 + tap_slot(px, kx)) * 256 + r;
        // four blocks' partials in flight per thread and round (a loop of single loads is a chain of round trips)
        for (int i0 = sl; i0 < nblk; i0 += UF_S * 4) {
            float v[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * UF_S;
                const float *pb = part + (size_t)(i < nblk ? i : 0) * 16 * 256;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[u][q] = i < nblk ? pb[tile[q]] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) s += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
        }
    }
    s += __shfl_down(s, 32, 64);
    s += __shfl_down(s, 16, 64);
    if ((threadIdx.x & 63) < 16) lds[threadIdx.x >> 6][cl] = s;
    __syncthreads();
    if (threadIdx.x < 16) {
        float tot = 0.f;
#pragma unroll
        for (int u = 0; u < UF_S / 4; ++u) tot += lds[u][cl];
        if (for_bias)
            gbias[cl] = tot;
        else
            gw[(r >> 4) * wso + (r & 15) * wsc + ky * wsy + kx * wsx] = tot;
    }
}

struct UpGeom { int nstrips, rows_per_wave, nruns, blocks; long long waves; int wblocks, quads_per_wave; };
static inline UpGeom up_geom(int B, int h, int w)
{
    UpGeom g;
    g.nstrips = (w + UC_PIX - 1) / UC_PIX;
    // forward / data gradient: three waves per SIMD are resident (144 / 168 VGPRs); no more waves than that over the chip, so that
    // there is no second, part-filled round, and a run of at least four rows each (a run pays two halo rows and the weights)
    const long long rows = (long long)B * g.nstrips * h;
    long long rpw = (rows + 3071) / 3072;
    if (rpw < 4) rpw = 4;
    if (rpw > h) rpw = h;
    g.rows_per_wave = (int)rpw;
    g.nruns = (h + g.rows_per_wave - 1) / g.rows_per_wave;
    g.waves = (long long)B * g.nruns * g.nstrips;
    g.blocks = (int)((g.waves + UC_WAVES - 1) / UC_WAVES);
    // weight gradient: two blocks of eight waves per CU, runs of at least 8 quads (shorter: the partials cost more than they hide)
    const long long nquads = (long long)B * h * (w / 4);
    long long qpw = (nquads + 4095) / 4096;
    if (qpw < 8) qpw = 8;
    g.quads_per_wave = (int)qpw;
    g.wblocks = (int)((nquads + qpw * UW_WAVES - 1) / (qpw * UW_WAVES));
    return g;
}

}  // namespace nhwc
}  // namespace mdx

using namespace mdx;
using namespace mdx::nhwc;

static int up_args_ok(int B, int h, int w)
{
    if (B <= 0 || h <= 0 || w <= 0 || w % 4) return MDX_ERR_BAD_SHAPE;
    if ((long long)B * h * w * 64 >= (1ll << 40)) return MDX_ERR_BAD_SHAPE;                  // elements of the x2 map
    if (h >= (1 << 29) || w >= (1 << 29)) return MDX_ERR_BAD_SHAPE;                           // 2h + 2, 2w + 2 in an int
    return MDX_OK;
}

MDX_EXPORT size_t mdx_up_conv3x3_workspace_bytes(int B, int h, int w)
{
    if (up_args_ok(B, h, w)) return 0;
    const UpGeom g = up_geom(B, h, w);
    return ((size_t)g.wblocks * 16 * 256 + (size_t)g.blocks * UC_WAVES * 16) * sizeof(float);
}

// raw [B][h][w][16], out [B][2h][2w][16], float32 channels-last, 16-byte aligned; bias [16]; weight element (co, ci, ky, kx) at
// weight[co * s_o + ci * s_c + ky * s_y + kx * s_x]
MDX_EXPORT int mdx_up_conv3x3_fwd(const float *raw, const float *bias, const float *weight, int64_t s_o, int64_t s_c, int64_t s_y,
                                  int64_t s_x, float *out, int B, int h, int w, void *stream)
{
    if (!raw || !bias || !weight || !out) return MDX_ERR_NULL_POINTER;
    const int bad = up_args_ok(B, h, w);
    if (bad) return bad;
    if (!aligned(raw, 16) || !aligned(out, 16) || !aligned(bias, 4) || !aligned(weight, 4)) return MDX_ERR_MISALIGNED;
    const UpGeom g = up_geom(B, h, w);
    hipLaunchKernelGGL(up_conv3x3_fwd_kernel, dim3(g.blocks), dim3(64 * UC_WAVES), 0, (hipStream_t)stream, raw, bias, weight, (long)s_o,
                       (long)s_c, (long)s_y, (long)s_x, out, B, h, w, g.rows_per_wave, g.nstrips, g.nruns);
    return check_launch();
}

MDX_EXPORT int mdx_up_conv3x3_bwd(const float *gy, const float *raw, const float *bias, const float *weight, int64_t s_o, int64_t s_c,
                                  int64_t s_y, int64_t s_x, float *graw, float *gbias, float *gweight, int64_t g_o, int64_t g_c,
                                  int64_t g_y, int64_t g_x, int B, int h, int w, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!gy || !raw || !bias || !weight || !graw || !gbias || !gweight || !workspace) return MDX_ERR_NULL_POINTER;
    const int bad = up_args_ok(B, h, w);
    if (bad) return bad;
    if (workspace_bytes < mdx_up_conv3x3_workspace_bytes(B, h, w)) return MDX_ERR_WORKSPACE;
    if (!aligned(gy, 16) || !aligned(raw, 16) || !aligned(graw, 16) || !aligned(bias, 4) || !aligned(workspace, 16) ||
        !aligned(weight, 4) || !aligned(gweight, 4) || !aligned(gbias, 4))
        return MDX_ERR_MISALIGNED;
    const UpGeom g = up_geom(B, h, w);
    float *part = (float *)workspace, *bias_part = part + (size_t)g.wblocks * 16 * 256;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(up_conv3x3_dgrad_kernel, dim3(g.blocks), dim3(64 * UC_WAVES), 0, st, gy, raw, bias, weight, (long)s_o, (long)s_c,
                       (long)s_y, (long)s_x, graw, bias_part, B, h, w, g.rows_per_wave, g.nstrips, g.nruns);
    hipLaunchKernelGGL(up_conv3x3_wgrad_kernel, dim3(g.wblocks), dim3(64 * UW_WAVES), 0, st, gy, raw, bias, B, h, w, g.quads_per_wave, part);
    hipLaunchKernelGGL(up_conv3x3_finish_kernel, dim3(9 * 16 + 1), dim3(16 * UF_S), 0, st, part, g.wblocks, bias_part, (int)g.waves,
                       (long)g_o, (long)g_c, (long)g_y, (long)g_x, gweight, gbias);
    return check_launch();
}
