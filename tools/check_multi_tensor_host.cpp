// check_multi_tensor_host.cpp -- the host halves of csrc/adam.hip, ema.hip, digest.hip and tensor_stats.hip as a stand-alone
// program, for a sanitizer build: every refusal of every entry point and the order of the refusals (null < shape < value <
// alignment < per-gradient null), one line per call, so that the outputs of two builds can be compared line for line.  No refusal
// reaches a HIP call and no pointer is followed, the gradient-pointer array (a heap block of exactly `count` entries) aside.
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         digging-into-self-supervised-monocular-depth-estimation_amd/csrc/{adam,ema,digest,tensor_stats}.hip \
//         tools/check_multi_tensor_host.cpp -o tools/check_multi_tensor_host_bin && tools/check_multi_tensor_host_bin
// The one ACCEPTED call (the statistics pass with a null gradient pointer) goes on to a launch over pointers that do not exist; it is
// made only where there is no GPU, and the launch's failure is then the expected status.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "../include/mdx.h"

struct Args {
    const void *table = (const void *)4096, *blockmap = (const void *)4096, *guard = NULL;
    void *partials = (void *)4096, *record = (void *)4096, *out = (void *)4096, *records = (void *)4096, *history = (void *)4096;
    const int *offsets = (const int *)4096;
    int first = 0, count = 2, nblocks = 3;
    bool no_grads = false;                // the array itself is NULL
    int null_grad = -1;                   // this entry of the array is NULL
    double decay = 0.999, max_grad_norm = 1.0;
};
typedef std::function<int(const Args &, const float *const *)> Entry;
typedef std::function<void(Args &)> Change;

static void *const ODD = (void *)4100;    // 4-byte but not 8-byte aligned
static std::map<int, int> tally;
static int failures = 0;

static const char *status_name(int s)
{
    return s == MDX_OK ? "OK" : s == MDX_ERR_NULL_POINTER ? "NULL_POINTER" : s == MDX_ERR_BAD_SHAPE ? "BAD_SHAPE"
         : s == MDX_ERR_MISALIGNED ? "MISALIGNED" : s == MDX_ERR_LAUNCH ? "LAUNCH" : "OTHER";
}

static void run(const char *entry, const Entry &fn, const char *what, const Change &change, int want)
{
    Args a;
    change(a);
    std::vector<const float *> grads((size_t)(a.count > 0 && a.count <= 384 ? a.count : 2), (const float *)8192);
    if (a.null_grad >= 0) grads[(size_t)a.null_grad] = NULL;
    const int got = fn(a, a.no_grads ? NULL : grads.data());
    ++tally[got];
    printf("%-26s %-44s %s%s\n", entry, what, status_name(got), got == want ? "" : "   <-- UNEXPECTED");
    failures += got != want;
}

int main(void)
{
    int gpus = 0;
    if (hipGetDeviceCount(&gpus) != hipSuccess) gpus = 0;
    (void)hipGetLastError();
    const int N = MDX_ERR_NULL_POINTER, S = MDX_ERR_BAD_SHAPE, M = MDX_ERR_MISALIGNED;
    printf("max_tensors %d chunk %d guard_record %d adam %d ema %d+%d digest %d stats %d/%d/%d/%d\n", mdx_adam_max_tensors(),
           mdx_adam_chunk(), (int)mdx_adam_guard_record_bytes(), (int)mdx_adam_table_entry_bytes(), (int)mdx_ema_table_entry_bytes(),
           (int)mdx_ema_record_bytes(), (int)mdx_digest_table_entry_bytes(), (int)mdx_tensor_stats_table_entry_bytes(),
           (int)mdx_tensor_stats_partial_bytes(), (int)mdx_tensor_stats_record_bytes(), (int)mdx_tensor_stats_history_bytes());

    const Entry step = [](const Args &a, const float *const *g) {
        return mdx_adam_step(a.table, a.first, a.count, g, a.blockmap, a.nblocks, NULL, 1e-3, 0.9, 0.999, 1e-8, NULL); };
    const Entry sumsq = [](const Args &a, const float *const *g) {
        return mdx_adam_grad_sumsq(a.table, a.first, a.count, g, a.blockmap, a.nblocks, (double *)a.partials, NULL); };
    const Entry guarded = [](const Args &a, const float *const *g) {
        return mdx_adam_step_guarded(a.table, a.first, a.count, g, a.blockmap, a.nblocks, NULL, 1e-3, 0.9, 0.999, 1e-8, a.record, NULL); };
    const Entry finish = [](const Args &a, const float *const *) {     // count: ntensors; nblocks: npartials
        return mdx_adam_guard_finish(a.table, a.count, (const double *)a.partials, a.nblocks, a.max_grad_norm, 1, a.record, NULL); };
    const Entry update = [](const Args &a, const float *const *) {
        return mdx_ema_update(a.table, a.first, a.count, a.blockmap, a.nblocks, a.decay, 1, a.record, a.guard, NULL); };
    const Entry tick = [](const Args &a, const float *const *) { return mdx_ema_tick(a.record, a.guard, NULL); };
    const Entry swap = [](const Args &a, const float *const *) {
        return mdx_ema_swap(a.table, a.first, a.count, a.blockmap, a.nblocks, NULL); };
    const Entry digest = [](const Args &a, const float *const *) {
        return mdx_digest_words(a.table, a.first, a.count, a.blockmap, a.nblocks, (uint64_t *)a.out, NULL); };
    const Entry stats = [](const Args &a, const float *const *g) {
        return mdx_tensor_stats_partials(a.table, a.first, a.count, g, a.blockmap, a.nblocks, a.partials, NULL); };
    const Entry stats_finish = [](const Args &a, const float *const *) {
        return mdx_tensor_stats_finish(a.first, a.count, a.offsets, a.partials, a.records, a.history, NULL); };

    // what every entry point that takes a plan refuses alike: (table, first, count, blockmap, nblocks)
    const struct { const char *name; Entry fn; } plans[] = {{"adam_step", step}, {"adam_grad_sumsq", sumsq}, {"adam_step_guarded", guarded},
        {"ema_update", update}, {"ema_swap", swap}, {"digest_words", digest}, {"tensor_stats_partials", stats}};
    for (const auto &p : plans) {
        run(p.name, p.fn, "table null", [](Args &a) { a.table = NULL; }, N);
        run(p.name, p.fn, "blockmap null", [](Args &a) { a.blockmap = NULL; }, N);
        run(p.name, p.fn, "count 0", [](Args &a) { a.count = 0; }, S);
        run(p.name, p.fn, "count -2", [](Args &a) { a.count = -2; }, S);
        run(p.name, p.fn, "count 385", [](Args &a) { a.count = 385; }, S);
        run(p.name, p.fn, "first -1", [](Args &a) { a.first = -1; }, S);
        run(p.name, p.fn, "nblocks 0", [](Args &a) { a.nblocks = 0; }, S);
        run(p.name, p.fn, "nblocks -1", [](Args &a) { a.nblocks = -1; }, S);
        run(p.name, p.fn, "table null < count 385", [](Args &a) { a.table = NULL; a.count = 385; }, N);
        run(p.name, p.fn, "blockmap null < first -1", [](Args &a) { a.blockmap = NULL; a.first = -1; }, N);
    }
    // the gradient pointers: the array, then (last of all) its entries -- refused by Adam, accepted by the statistics
    const struct { const char *name; Entry fn; bool adam, partials, record; } grads[] = {{"adam_step", step, true, false, false},
        {"adam_grad_sumsq", sumsq, true, true, false}, {"adam_step_guarded", guarded, true, false, true},
        {"tensor_stats_partials", stats, false, true, false}};
    for (const auto &p : grads) {
        run(p.name, p.fn, "grads null", [](Args &a) { a.no_grads = true; }, N);
        run(p.name, p.fn, "grads null < nblocks 0", [](Args &a) { a.no_grads = true; a.nblocks = 0; }, N);
        run(p.name, p.fn, "count 385 < a null gradient", [](Args &a) { a.count = 385; a.null_grad = 1; }, S);
        if (p.adam) {
            run(p.name, p.fn, "a null gradient (first)", [](Args &a) { a.null_grad = 0; }, N);
            run(p.name, p.fn, "a null gradient (last of 384)", [](Args &a) { a.count = 384; a.null_grad = 383; }, N);
        }
        if (p.partials) {
            run(p.name, p.fn, "partials null", [](Args &a) { a.partials = NULL; }, N);
            run(p.name, p.fn, "partials null < count 0", [](Args &a) { a.partials = NULL; a.count = 0; }, N);
            run(p.name, p.fn, "partials misaligned", [](Args &a) { a.partials = ODD; }, M);
            run(p.name, p.fn, "count 0 < partials misaligned", [](Args &a) { a.partials = ODD; a.count = 0; }, S);
            run(p.name, p.fn, "partials misaligned < a null gradient", [](Args &a) { a.partials = ODD; a.null_grad = 1; }, M);
        }
        if (p.record) {
            run(p.name, p.fn, "record null", [](Args &a) { a.record = NULL; }, N);
            run(p.name, p.fn, "record null < count 0", [](Args &a) { a.record = NULL; a.count = 0; }, N);
            run(p.name, p.fn, "record misaligned", [](Args &a) { a.record = ODD; }, M);
            run(p.name, p.fn, "nblocks -1 < record misaligned", [](Args &a) { a.record = ODD; a.nblocks = -1; }, S);
            run(p.name, p.fn, "record misaligned < a null gradient", [](Args &a) { a.record = ODD; a.null_grad = 1; }, M);
        }
    }
    if (gpus == 0)
        run("tensor_stats_partials", stats, "a null gradient: accepted, no GPU to launch", [](Args &a) { a.null_grad = 0; }, MDX_ERR_LAUNCH);
    else
        printf("%-26s %-44s not called: a GPU is present\n", "tensor_stats_partials", "a null gradient: accepted");

    run("adam_guard_finish", finish, "table null", [](Args &a) { a.table = NULL; }, N);
    run("adam_guard_finish", finish, "partials null", [](Args &a) { a.partials = NULL; }, N);
    run("adam_guard_finish", finish, "record null", [](Args &a) { a.record = NULL; }, N);
    run("adam_guard_finish", finish, "ntensors 0", [](Args &a) { a.count = 0; }, S);
    run("adam_guard_finish", finish, "npartials 0", [](Args &a) { a.nblocks = 0; }, S);
    run("adam_guard_finish", finish, "max_grad_norm NaN", [](Args &a) { a.max_grad_norm = (double)NAN; }, S);
    run("adam_guard_finish", finish, "record null < max_grad_norm NaN", [](Args &a) { a.record = NULL; a.max_grad_norm = (double)NAN; }, N);
    run("adam_guard_finish", finish, "max_grad_norm NaN < record misaligned", [](Args &a) { a.record = ODD; a.max_grad_norm = (double)NAN; }, S);
    run("adam_guard_finish", finish, "partials misaligned", [](Args &a) { a.partials = ODD; }, M);
    run("adam_guard_finish", finish, "record misaligned", [](Args &a) { a.record = ODD; }, M);

    run("ema_update", update, "record null", [](Args &a) { a.record = NULL; }, N);
    run("ema_update", update, "record null < count 385", [](Args &a) { a.record = NULL; a.count = 385; }, N);
    run("ema_update", update, "decay NaN", [](Args &a) { a.decay = (double)NAN; }, S);
    run("ema_update", update, "decay 1", [](Args &a) { a.decay = 1.0; }, S);
    run("ema_update", update, "decay 1.5", [](Args &a) { a.decay = 1.5; }, S);
    run("ema_update", update, "decay -1e-9", [](Args &a) { a.decay = -1e-9; }, S);
    run("ema_update", update, "decay inf", [](Args &a) { a.decay = (double)INFINITY; }, S);
    run("ema_update", update, "table null < decay NaN", [](Args &a) { a.table = NULL; a.decay = (double)NAN; }, N);
    run("ema_update", update, "decay NaN < record misaligned", [](Args &a) { a.decay = (double)NAN; a.record = ODD; }, S);
    run("ema_update", update, "record misaligned", [](Args &a) { a.record = ODD; }, M);
    run("ema_update", update, "guard record misaligned", [](Args &a) { a.guard = ODD; }, M);
    run("ema_tick", tick, "record null", [](Args &a) { a.record = NULL; }, N);
    run("ema_tick", tick, "record null < guard record misaligned", [](Args &a) { a.record = NULL; a.guard = ODD; }, N);
    run("ema_tick", tick, "record misaligned", [](Args &a) { a.record = ODD; }, M);
    run("ema_tick", tick, "guard record misaligned", [](Args &a) { a.guard = ODD; }, M);

    run("digest_words", digest, "out null", [](Args &a) { a.out = NULL; }, N);
    run("digest_words", digest, "out null < count 0", [](Args &a) { a.out = NULL; a.count = 0; }, N);
    run("digest_words", digest, "out misaligned", [](Args &a) { a.out = ODD; }, M);
    run("digest_words", digest, "first -1 < out misaligned", [](Args &a) { a.out = ODD; a.first = -1; }, S);

    run("tensor_stats_finish", stats_finish, "offsets null", [](Args &a) { a.offsets = NULL; }, N);
    run("tensor_stats_finish", stats_finish, "partials null", [](Args &a) { a.partials = NULL; }, N);
    run("tensor_stats_finish", stats_finish, "records null", [](Args &a) { a.records = NULL; }, N);
    run("tensor_stats_finish", stats_finish, "records null < count 385", [](Args &a) { a.records = NULL; a.count = 385; }, N);
    run("tensor_stats_finish", stats_finish, "first -1", [](Args &a) { a.first = -1; }, S);
    run("tensor_stats_finish", stats_finish, "count 0", [](Args &a) { a.count = 0; }, S);
    run("tensor_stats_finish", stats_finish, "count -2", [](Args &a) { a.count = -2; }, S);
    run("tensor_stats_finish", stats_finish, "count 385", [](Args &a) { a.count = 385; }, S);
    run("tensor_stats_finish", stats_finish, "count 385 < records misaligned", [](Args &a) { a.count = 385; a.records = ODD; }, S);
    run("tensor_stats_finish", stats_finish, "partials misaligned", [](Args &a) { a.partials = ODD; }, M);
    run("tensor_stats_finish", stats_finish, "records misaligned", [](Args &a) { a.records = ODD; }, M);
    run("tensor_stats_finish", stats_finish, "history misaligned", [](Args &a) { a.history = ODD; }, M);

    int calls = 0;
    for (const auto &t : tally) {
        printf("%d x %s\n", t.second, status_name(t.first));
        calls += t.second;
    }
    printf(failures ? "%d calls, %d UNEXPECTED\n" : "check_multi_tensor_host: ok (%d calls)\n", calls, failures);
    return failures ? 1 : 0;
}
