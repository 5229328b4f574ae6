// hint_select.hip -- depth hints: keep a proxy depth only where it reprojects better than the network's own depth (gfx950).
//
// THE DEFINITION is the one of include/mdx.h ("depth-hint selection"; mdx.functional.hint_select is the GPU form,
// mdx.composite.hint_select the plain-torch one): per pixel the ReprojectionLoss of the partner warped with the hint depth and with
// the depth the step forms from its finest disparity, keep = hint > 0 && l_hint < l_pred (strict), sel = keep ? hint : 0, and per
// sample the counts (hints, kept).  Every float is formed by the functions of mdx_device.hpp / photo_common.hpp that the
// fine-grained ops and the fused photometric kernels use, so l_hint and l_pred carry the bits of those chains.
//
// THE FORM, two launches on one stream:
//   select   one 256-thread block per 64 x 8 tile of one sample, tiles in the XCD-aware order of photo_common.hpp.
//            stage 0  the target tile + 1-pixel halo -> LDS (16-byte loads, every load issued before the first LDS write);
//                     threads 0..11 form P = (K @ T)[:3] of the sample into LDS.
//            stage 1  every thread warps up to three tile + halo positions TWICE: the pixel's ray is formed once, scaled by the
//                     hint and by the predicted depth, projected and sampled from the same partner planes.  A halo position
//                     outside the image is the reflected position inside it and is warped there.  The 8-byte tap loads of a
//                     depth's three positions and three channels are all issued before the first is consumed.
//            stage 2  per pixel the target's window statistics once, the window statistics of the two warped tiles against them,
//                     SSIM + L1, the compare; sel (and l_hint / l_pred on request) by one plain store each; the block's two
//                     counts by wave ballots -> one int pair per tile in the workspace.
//   counts   one block per sample adds its tiles' pairs (integers: the order cannot matter) -> counts[b] = (hints, kept).
// LDS: 9 planes of 10 x 66 floats = 23.8 KB per block.  No atomics, every output element has one writer, the workspace is
// written before it is read, no host synchronisation: capturable, and the same inputs give the same bits at every call.
// No index is formed from an unclamped float: the only float -> int conversions are make_tap's, behind fminf(fmaxf(.)) (a NaN
// becomes 0 there), and up_tap's, whose argument does not depend on the data.
#include <type_traits>

#include "photo_common.hpp"

namespace mdx {

constexpr int HS_NPIX = (FX * FY + NT - 1) / NT;   // tile + halo positions per thread in stage 1 (3)
constexpr int HS_ROWS = TY / (NT / 64);            // adjacent output rows per thread in stage 2 (2)

struct HsArgs {
    const float *target, *partner, *K, *invK, *T, *hint, *disp;
    int B, H, W, h, w;
    float disp_a, disp_b;
    bool premul, fast_w, fast_h;
    float *sel, *l_hint, *l_pred;
    int *partial;                                  // [tiles][2], tiles of a sample contiguous
    int *counts;                                   // [B][2]
};

struct HsPx { int ly, lx, px, py; bool valid; };

// position i of the tile + halo: its LDS slot and the image pixel it stands for (reflected when outside)
MDX_DEV HsPx hs_px(int i, int x0, int y0, int H, int W)
{
    HsPx p;
    p.valid = i < FX * FY;
    const int ii = p.valid ? i : 0;
    p.ly = ii / FX;
    p.lx = ii - p.ly * FX;
    const int gx = x0 + p.lx - 1, gy = y0 + p.ly - 1;
    p.valid = p.valid && gx <= W && gy <= H;         // beyond the reflected ring: never read
    p.px = p.valid ? reflect(gx, W) : 0;
    p.py = p.valid ? reflect(gy, H) : 0;
    return p;
}

__global__ __launch_bounds__(NT, 4) void hint_select_kernel(HsArgs a)
{
    __shared__ float s_t[3][FY][FX];
    __shared__ float s_x[2][3][FY][FX];              // the partner warped with the hint (0) and with the predicted depth (1)
    __shared__ float s_P[12];
    __shared__ int s_cnt[NT / 64][2];

    const int H = a.H, W = a.W;
    const size_t HW = (size_t)H * W;
    const TileId tile = tile_id();
    const int b = tile.b, x0 = tile.tx * TX, y0 = tile.ty * TY;
    const int tid = threadIdx.x;
    const float *tgt_b = a.target + (size_t)b * 3 * HW, *par_b = a.partner + (size_t)b * 3 * HW;
    const float *hint_b = a.hint + (size_t)b * HW, *disp_b = a.disp + (size_t)b * a.h * a.w;

    // ---- stage 0 ----
    {
        float (*const dst[3])[FX] = {s_t[0], s_t[1], s_t[2]};
        const float *const planes[3] = {tgt_b, tgt_b + HW, tgt_b + 2 * HW};
        load_plane_tiles<1, 3>(dst, planes, H, W, x0, y0, tid);
    }
    if (tid < 12) {
        // ATen's small-matrix bmm as compose_projection_kernel restates it: acc = 0; acc += K[r][k] * T[k][j], each rounded
        const int j = tid & 3, r = tid >> 2;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float prod = a.K[b * 16 + r * 4 + k] * a.T[b * 16 + k * 4 + j];
            acc = acc + prod;
        }
        s_P[tid] = acc;
    }
    __syncthreads();

    // ---- stage 1: both warps of the tile + halo ----
    {
        const float *invK_b = a.invK + b * 16;
        Norm2 nd;
        nd.w = make_normdiv(W - 1, a.fast_w);
        nd.h = make_normdiv(H - 1, a.fast_h);
        auto warp_stage = [&](auto np_tag) {
            constexpr int NP = decltype(np_tag)::value;
            HsPx hp[NP];
            float ray[NP][3], dep[NP][2];
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                hp[k] = hs_px(tid + k * NT, x0, y0, H, W);
                const float up = upsample_at(disp_b, a.h, a.w, H, W, hp[k].py, hp[k].px, a.premul);
                dep[k][0] = at32(hint_b, (unsigned)(hp[k].py * W + hp[k].px));
                dep[k][1] = 1.0f / scaled_disp(up, a.disp_a, a.disp_b);
                pixel_ray(invK_b, (float)hp[k].px, (float)hp[k].py, ray[k]);
            }
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                Tap t[NP];
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const float d = dep[k][f];
                    const Proj pr = project_point(s_P, d * ray[k][0], d * ray[k][1], d * ray[k][2], 1.0f, nd, 1e-7f);
                    t[k] = make_tap(pr.gx, pr.gy, H, W);
                }
                Corners cn[NP][3];
#pragma unroll
                for (int k = 0; k < NP; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) cn[k][c] = load_corners(par_b + c * HW, H, W, t[k]);
#pragma unroll
                for (int k = 0; k < NP; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (hp[k].valid) s_x[f][c][hp[k].ly][hp[k].lx] = sample(cn[k][c], t[k]);
            }
        };
        // FX*FY = 660 positions = two full rounds of the block plus 148: only the waves that own part of the rest run a third
        const int third = __builtin_amdgcn_readfirstlane((tid & ~63) + (HS_NPIX - 1) * NT < FX * FY);
        if (third) warp_stage(std::integral_constant<int, HS_NPIX>{});
        else warp_stage(std::integral_constant<int, HS_NPIX - 1>{});
    }
    __syncthreads();

    // ---- stage 2: the two losses from LDS, the compare, the outputs ----
    const int tx = tid & 63, px = x0 + tx;
    int n_hint = 0, n_kept = 0;
#pragma unroll
    for (int q = 0; q < HS_ROWS; ++q) {
        const int r = HS_ROWS * (tid >> 6) + q;
        const int py = y0 + r;
        const bool valid = px < W && py < H;
        const unsigned p = (unsigned)((valid ? py : 0) * W + (valid ? px : 0));
        const float hv = at32(hint_b, p);
        float y9[3][9];
        TargetStats ts[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 9; ++k) y9[c][k] = s_t[c][r + k / 3][tx + k % 3];
            ts[c] = target_stats(y9[c]);
        }
        float rl[2];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            float ss[3], ad[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float x9[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) x9[k] = s_x[f][c][r + k / 3][tx + k % 3];
                ss[c] = clamp01(ssim_raw(pred_stats(x9, y9[c]), ts[c]));
                ad[c] = fabsf(y9[c][4] - x9[4]);
            }
            rl[f] = reprojection_combine(ss, ad);
        }
        const bool has = valid && hv > 0.f;
        const bool keep = has && rl[0] < rl[1];           // strict; false when either side is a NaN
        if (valid) {
            at32(a.sel + (size_t)b * HW, p) = keep ? hv : 0.f;
            if (a.l_hint) at32(a.l_hint + (size_t)b * HW, p) = rl[0];
            if (a.l_pred) at32(a.l_pred + (size_t)b * HW, p) = rl[1];
        }
        n_hint += __builtin_popcountll(__ballot(has));    // wave-uniform
        n_kept += __builtin_popcountll(__ballot(keep));
    }
    if ((tid & 63) == 0) { s_cnt[tid >> 6][0] = n_hint; s_cnt[tid >> 6][1] = n_kept; }
    __syncthreads();
    if (tid < 2) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) t += s_cnt[k][tid];
        a.partial[2u * tile.linear + (unsigned)tid] = t;
    }
}

// counts[b] = the sums of the sample's tile pairs
__global__ __launch_bounds__(NT) void hint_select_counts_kernel(const int *__restrict__ partial, int tiles_per_sample,
                                                                int *__restrict__ counts)
{
    __shared__ int s[NT / 64][2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int *mine = partial + (size_t)b * tiles_per_sample * 2;
    int n0 = 0, n1 = 0;
    for (int i = tid; i < tiles_per_sample; i += NT) { n0 += mine[2 * i]; n1 += mine[2 * i + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { n0 += __shfl_down(n0, off, 64); n1 += __shfl_down(n1, off, 64); }
    if ((tid & 63) == 0) { s[tid >> 6][0] = n0; s[tid >> 6][1] = n1; }
    __syncthreads();
    if (tid < 2) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < NT / 64; ++k) t += s[k][tid];
        counts[2 * b + tid] = t;
    }
}

// the tiles of a call, or 0 for sizes it refuses
static size_t hs_tiles(int B, int H, int W, int h, int w)
{
    if (B < 1 || H < 2 || W < 2 || h < 1 || w < 1 || h > H || w > W) return 0;
    if ((long long)H * W >= (1ll << 30) || (long long)B * H * W >= (1ll << 31)) return 0;
    if ((H + TY - 1) / TY > 65535 || B > 65535) return 0;
    return (size_t)((W + TX - 1) / TX) * (size_t)((H + TY - 1) / TY) * (size_t)B;
}

}  // namespace mdx

using namespace mdx;

MDX_EXPORT size_t mdx_hint_select_workspace_bytes(int B, int H, int W, int h, int w)
{
    return hs_tiles(B, H, W, h, w) * 2 * sizeof(int);
}

MDX_EXPORT int mdx_hint_select(const float *target, const float *partner, const float *K, const float *invK, const float *T,
                               const float *hint, const float *disp, int B, int H, int W, int h, int w, double min_depth,
                               double max_depth, float *sel, float *l_hint, float *l_pred, int *counts, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!target || !partner || !K || !invK || !T || !hint || !disp || !sel || !counts) return MDX_ERR_NULL_POINTER;
    const size_t tiles = hs_tiles(B, H, W, h, w);
    if (tiles == 0 || !(min_depth > 0.0) || !(max_depth > min_depth)) return MDX_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < mdx_hint_select_workspace_bytes(B, H, W, h, w)) return MDX_ERR_WORKSPACE;
    const void *floats[] = {target, partner, K, invK, T, hint, disp, sel, l_hint, l_pred, counts};
    for (const void *p : floats)
        if (!aligned(p, sizeof(float))) return MDX_ERR_MISALIGNED;
    // stage 0 reads the target planes through load_plane_tiles' 16-byte loads (photo_abi.hip refuses the same way)
    if (!aligned(workspace, 8) || !aligned(target, 16)) return MDX_ERR_MISALIGNED;
    HsArgs a;
    a.target = target; a.partner = partner; a.K = K; a.invK = invK; a.T = T; a.hint = hint; a.disp = disp;
    a.B = B; a.H = H; a.W = W; a.h = h; a.w = w;
    // disparity2depth's constants as mdx_desc_init forms them: Python doubles, rounded to f32 where they meet the tensor
    const double min_disp = 1.0 / max_depth, max_disp = 1.0 / min_depth;
    a.disp_a = (float)min_disp;
    a.disp_b = (float)(max_disp - min_disp);
    a.premul = H + W <= 128;
    a.fast_w = div_verified(W - 1);
    a.fast_h = div_verified(H - 1);
    a.sel = sel; a.l_hint = l_hint; a.l_pred = l_pred;
    a.partial = (int *)workspace;
    a.counts = counts;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY, B);
    hipLaunchKernelGGL(hint_select_kernel, grid, dim3(NT), 0, s, a);
    hipLaunchKernelGGL(hint_select_counts_kernel, dim3(B), dim3(NT), 0, s, (const int *)a.partial, (int)(grid.x * grid.y), counts);
    return check_launch();
}
