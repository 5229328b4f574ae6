// check_loss_stats_host.cpp -- the host half of csrc/loss_stats.hip as a stand-alone program, for a sanitizer build: the plan (the
// only host code of the pass that writes memory) against the recipe of include/mdx.h, and every refusal, none of which reaches a HIP
// call.  Needs no GPU.
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         digging-into-self-supervised-monocular-depth-estimation_amd/csrc/loss_stats.hip tools/check_loss_stats_host.cpp \
//         -o tools/check_loss_stats_host_bin && tools/check_loss_stats_host_bin
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../include/mdx.h"

static int failures = 0;
#define EXPECT(what, want)                                                                              \
    do {                                                                                                \
        const int got_ = (what);                                                                        \
        if (got_ != (want)) { printf("FAIL %s:%d %s = %d, want %d\n", __FILE__, __LINE__, #what, got_, (int)(want)); ++failures; } \
    } while (0)

int main(void)
{
    const int ci = mdx_loss_stats_index_chunk(), cd = mdx_loss_stats_disp_chunk();
    EXPECT((int)mdx_loss_stats_record_bytes(), 72);
    EXPECT((int)mdx_loss_stats_partial_bytes(), 72);
    EXPECT((int)mdx_loss_stats_history_bytes(), 152);
    EXPECT((int)mdx_loss_stats_blockmap_entry_bytes(), 16);

    // the plan, written into a heap buffer of exactly its size: the sanitizer sees one entry too many
    struct Case { int n, B, H, W; int h[4], w[4]; };
    const Case cases[] = {{1, 1, 4, 4, {4}, {4}}, {2, 3, 6, 10, {6, 3}, {10, 5}}, {4, 2, 64, 160, {64, 32, 16, 8}, {160, 80, 40, 20}},
                          {2, 1, 4, ci / 4 + 1, {4, 2}, {cd / 4 + 1, cd / 4}}, {4, 12, 192, 640, {192, 96, 48, 24}, {640, 320, 160, 80}},
                          {3, 2, 1, 1, {1, 7, 1}, {1, 3 * cd, 1}}};
    for (const Case &c : cases) {
        long long want = 0;
        for (int s = 0; s < c.n; ++s)
            want += (long long)c.B * (((long long)c.H * c.W + ci - 1) / ci + ((long long)c.h[s] * c.w[s] + cd - 1) / cd);
        EXPECT(mdx_loss_stats_plan(c.n, c.B, c.H, c.W, c.h, c.w, NULL), (int)want);
        std::vector<int> map((size_t)want * 4, -1);
        EXPECT(mdx_loss_stats_plan(c.n, c.B, c.H, c.W, c.h, c.w, map.data()), (int)want);
        long long at = 0;
        for (int s = 0; s < c.n; ++s)
            for (int b = 0; b < c.B; ++b)
                for (int kind = 0; kind < 2; ++kind) {
                    const long long chunks = kind ? ((long long)c.h[s] * c.w[s] + cd - 1) / cd : ((long long)c.H * c.W + ci - 1) / ci;
                    for (int k = 0; k < chunks; ++k, ++at)
                        if (map[at * 4] != s || map[at * 4 + 1] != b || map[at * 4 + 2] != k || map[at * 4 + 3] != kind) {
                            printf("FAIL plan entry %lld\n", at);
                            ++failures;
                        }
                }
        EXPECT((int)(at == want), 1);
    }

    // refusals: NULL, then shape, then alignment -- with pointers that are never followed
    void *fake = (void *)4096, *odd = (void *)4100;
    int h[2] = {4, 2}, w[2] = {4, 2}, zero[2] = {4, 0};
    const uint8_t *idx[2] = {(const uint8_t *)4096, NULL};
    const float *disp[2] = {NULL, (const float *)8192}, *disp_odd[2] = {NULL, (const float *)8194};
    const int nb = mdx_loss_stats_plan(2, 2, 4, 4, h, w, NULL);
    EXPECT(nb, 8);
    EXPECT(mdx_loss_stats_plan(2, 2, 4, 4, NULL, w, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_plan(5, 2, 4, 4, h, w, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_plan(2, 2, 65536, 65536, h, w, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_plan(1, 1 << 20, 65535, 65535, h, w, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, NULL, disp, fake, nb, fake, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, NULL, fake, nb, fake, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp, NULL, nb, fake, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp, fake, nb, NULL, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 0, 1, h, w, idx, disp, fake, nb, NULL, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 0, 1, h, w, idx, disp, fake, nb, odd, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 5, 1, h, w, idx, disp, fake, nb, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, zero, idx, disp, fake, nb, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp, fake, 0, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp, fake, nb + 1, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp, fake, nb, odd, NULL), MDX_ERR_MISALIGNED);
    EXPECT(mdx_loss_stats_partials(2, 2, 4, 4, 2, 1, h, w, idx, disp_odd, fake, nb, fake, NULL), MDX_ERR_MISALIGNED);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.9, NULL, fake, fake, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.9, fake, NULL, fake, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.0, fake, NULL, odd, NULL), MDX_ERR_NULL_POINTER);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.0, fake, fake, odd, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 1.5, fake, fake, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, (double)NAN, fake, fake, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_finish(2, 0, 4, 4, 2, 1, h, w, 0.9, fake, fake, fake, NULL), MDX_ERR_BAD_SHAPE);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.9, odd, fake, fake, NULL), MDX_ERR_MISALIGNED);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.9, fake, odd, NULL, NULL), MDX_ERR_MISALIGNED);
    EXPECT(mdx_loss_stats_finish(2, 2, 4, 4, 2, 1, h, w, 0.9, fake, fake, odd, NULL), MDX_ERR_MISALIGNED);
    printf(failures ? "%d FAILURES\n" : "check_loss_stats_host: ok (%d)\n", failures);
    return failures ? 1 : 0;
}
