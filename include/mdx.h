/*
 * mdx.h -- C-ABI of the MI355X (gfx950) photometric hot path: libmdx_hip.so
 *
 * Drop-in boundary for the self-supervised depth training step of
 * russellgeum/Digging-into-Self-Supervised-Monocular-Depth-Estimation:
 *   model_tool/processor.py:139-163  compute.image2warping
 *   model_tool/processor.py:166-218  compute.compute_loss
 *   model_layer/warp.py:12-39,193-269, model_loss/model_loss.py:11-116 (the ops those two call)
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory (hipMalloc / a torch CUDA tensor's
 *     data_ptr) unless the parameter is named host_*;
 *   - float32, contiguous, NCHW planar; indices uint8;
 *   - the caller allocates every input, output and workspace; the library never allocates, frees or
 *     keeps a pointer after return; outputs are fully overwritten;
 *   - kernels are enqueued on `stream` (a hipStream_t, NULL = default stream) and the call returns
 *     without synchronising; re-entrant, no global mutable state;
 *   - return 0 on success, a negative mdx_status otherwise (never throws, never aborts).
 *
 * Numerics: every per-pixel result reproduces the reference's CPU path (PyTorch ATen, CPU) bit for
 * bit -- see DESIGN.md "pinned operation orders"; reductions and gradients agree to <= 1e-4 rel.
 */
#ifndef MDX_H
#define MDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_VERSION 510
#define MDX_MAX_SRC 4
#define MDX_MAX_SCALES 4

typedef enum mdx_status {
    MDX_OK = 0,
    MDX_ERR_BAD_SHAPE = -1,       /* non-positive size, S out of range, h/w not H>>k, W or H < 4 */
    MDX_ERR_NULL_POINTER = -2,    /* a required pointer is NULL */
    MDX_ERR_WORKSPACE = -3,       /* workspace missing or too small */
    MDX_ERR_LAUNCH = -4,          /* hipGetLastError() after launch was not hipSuccess */
    MDX_ERR_UNSUPPORTED = -5,     /* flag/mode combination not implemented */
    MDX_ERR_MISALIGNED = -6       /* pointer not 4-byte (float) / 8-byte (workspace) aligned */
} mdx_status;

/* flags */
#define MDX_FLAG_AUTOMASK 1u       /* channels [ident(0..S-1), reproj(0..S-1)] (processor.py:186-196) */
#define MDX_FLAG_UPSAMPLE_PREMUL 2u /* ATen's small-output bilinear kernel (H+W <= 128); set by mdx_desc_init */
#define MDX_FLAG_FASTDIV_W 4u      /* W-1 is in the verified constant-division table (set by mdx_desc_init) */
#define MDX_FLAG_FASTDIV_H 8u      /* H-1 likewise */

/* Problem descriptor of one scale of the step. */
typedef struct mdx_desc {
    int32_t B, H, W;      /* images, full resolution (opt.height, opt.width) */
    int32_t h, w;         /* disparity resolution of this scale: outputs[("disp", s)] is [B,1,h,w] */
    int32_t S;            /* number of source frames: len(opt.frame_ids) - 1, 1..MDX_MAX_SRC */
    uint32_t flags;
    float disp_a, disp_b; /* scaled_disp = disp_a + disp_b*disp (warp.py:34-37), f32-rounded */
} mdx_desc;

/* S source images, each [B,3,H,W] (inputs[("color", frame_id, 0)], order of opt.frame_ids[1:]) */
typedef struct mdx_sources {
    const float *img[MDX_MAX_SRC];
} mdx_sources;

/* Fills a descriptor; computes disp_a/disp_b from (min_depth, max_depth) exactly as
 * warp.py:34-37 does (Python doubles, rounded to f32), and sets MDX_FLAG_UPSAMPLE_PREMUL. */
int mdx_desc_init(mdx_desc *d, int B, int H, int W, int h, int w, int S, int automask,
                  double min_depth, double max_depth);

int mdx_version(void);
const char *mdx_status_string(int status);

/* ------------------------------------------------------------------------------------------
 * Fused path (what the training step runs)
 * ---------------------------------------------------------------------------------------- */

/* P[b] = (K[b] @ T[b])[:3,:]   replaces warp.py:260.  K,T [B,4,4] -> P [B,3,4]. */
int mdx_compose_projection(const float *K, const float *T, int B, float *P, void *stream);

/* Identity (auto-mask) losses, hoisted out of the scale loop because they do not depend on the
 * scale: ident[b,f] = ReprojectionLoss(color_f, target)   replaces processor.py:187-191.
 * target [B,3,H,W], ident out [B,S,H,W] (noise NOT added here). */
int mdx_identity_loss(const mdx_desc *d, const float *target, const mdx_sources *src, float *ident,
                      void *stream);

size_t mdx_photometric_workspace_bytes(const mdx_desc *d);

/* One scale of image2warping + compute_loss, forward   replaces processor.py:141-162,172-204,212.
 *   disp [B,1,h,w]; target [B,3,H,W]; invK [B,4,4]; P [S,B,3,4]; ident [B,S,H,W]; noise [B,S,H,W]
 *   (ident/noise only with MDX_FLAG_AUTOMASK; noise is the N(0,1) draw of processor.py:195).
 * Outputs: idx [B,H,W] uint8 (arg-min channel, torch.min's first-minimum rule);
 *          loss_sum [1] float = sum over B,H,W of to_optimise (divide by B*H*W for .mean()); NULL skips
 *          the finishing pass and leaves one double per tile at the start of the workspace;
 * optional (NULL to skip): to_opt [B,H,W]; depth [B,1,H,W]; warp [S,B,3,H,W]; reproj [B,S,H,W];
 *          coef [B,3,H,W,3] (9*B*H*W floats) = the SSIM coefficient triplets (alpha,beta,gamma) per colour
 *          channel of each pixel's
 *          arg-min frame, zero where an identity channel won -- hand coef (or, without it, warp) to
 *          mdx_photometric_bwd. */
int mdx_photometric_fwd(const mdx_desc *d, const float *disp, const float *target,
                        const mdx_sources *src, const float *invK, const float *P,
                        const float *ident, const float *noise, uint8_t *idx, float *loss_sum,
                        float *to_opt, float *depth, float *warp, float *reproj, float *coef,
                        void *workspace, size_t workspace_bytes, void *stream);

/* Measurement hook: a pair of hipEvent_t handles that the *_timed entry points record on `stream` immediately
 * before and immediately after the FUSED kernel of the call (not around its small finishing passes), so that a
 * caller can time that kernel inside a real training step.  mdx_event_* are thin wrappers over hipEventCreate /
 * hipEventDestroy / hipEventSynchronize + hipEventElapsedTime for callers without a HIP binding. */
typedef struct mdx_timing { void *start, *stop; } mdx_timing;
void *mdx_event_create(void);
void mdx_event_destroy(void *event);
int mdx_event_elapsed_us(void *start, void *stop, float *us);   /* waits for `stop` */

/* mdx_photometric_fwd / mdx_photometric_bwd with the hook (t == NULL: exactly the plain call). */
int mdx_photometric_fwd_timed(const mdx_desc *d, const float *disp, const float *target,
                              const mdx_sources *src, const float *invK, const float *P,
                              const float *ident, const float *noise, uint8_t *idx, float *loss_sum,
                              float *to_opt, float *depth, float *warp, float *reproj, float *coef,
                              void *workspace, size_t workspace_bytes, void *stream, const mdx_timing *t);

/* Backward of the above for d(loss)/d(to_optimise[b,y,x]) = g_const * (*g_dev) on every pixel
 * (g_dev may be NULL = 1).  Needs only the inputs and idx; `warp` (optional, [S,B,3,H,W]) is the forward's
 * warped-colour output -- when given the kernel reads it instead of re-warping the 2-pixel halo; `coef`
 * (optional, [B,3,H,W,3]) is the forward's coefficient output -- with it the backward skips the window
 * statistics altogether and needs no `warp` (it re-samples a pixel's own warped colour from the corners it
 * gathers for the gradient; `warp` is ignored when `coef` is given).
 * Outputs: gdisp [B,1,h,w]; gP [S,B,3,4] (d loss / d P; chain to T with K^T outside).  Passing NULL for BOTH
 * runs the fused kernel alone and leaves its raw per-tile outputs in the workspace (timing aid). */
int mdx_photometric_bwd(const mdx_desc *d, const float *disp, const float *target,
                        const mdx_sources *src, const float *invK, const float *P,
                        const uint8_t *idx, const float *warp, const float *coef, float g_const,
                        const float *g_dev, float *gdisp, float *gP, void *workspace, size_t workspace_bytes,
                        void *stream);
int mdx_photometric_bwd_timed(const mdx_desc *d, const float *disp, const float *target,
                        const mdx_sources *src, const float *invK, const float *P,
                        const uint8_t *idx, const float *warp, const float *coef, float g_const,
                        const float *g_dev, float *gdisp, float *gP, void *workspace, size_t workspace_bytes,
                        void *stream, const mdx_timing *t);

/* ------------------------------------------------------------------------------------------
 * Training step: every scale, forward AND gradient, in one launch
 *   replaces the scale loops of processor.py:140-163 and :167-204,212 plus their autograd backward.
 * Everything downstream of sum(to_optimise) is linear in the upstream gradient, so the kernel returns the
 * gradients for a UNIT upstream: d loss / d disp_s = g_s * gdisp[s], d loss / d P = sum_s g_s * gP[s]
 * where g_s = d loss / d loss_sum[s] (the caller's autograd multiplies; nothing else is kept for backward).
 * ---------------------------------------------------------------------------------------- */
typedef struct mdx_train_desc {
    int32_t B, H, W;                 /* images, full resolution */
    int32_t S;                       /* source frames, 1..MDX_MAX_SRC */
    int32_t nscales;                 /* len(opt.scales), 1..MDX_MAX_SCALES */
    uint32_t flags;                  /* as mdx_desc.flags */
    float disp_a, disp_b;            /* as mdx_desc */
    int32_t h[MDX_MAX_SCALES], w[MDX_MAX_SCALES];   /* outputs[("disp", s)] is [B,1,h[s],w[s]] */
    int32_t rows_per_chunk;          /* rows one wave walks; 0 = chosen by the library */
} mdx_train_desc;

int mdx_train_desc_init(mdx_train_desc *d, int B, int H, int W, int S, int nscales, const int32_t *h,
                        const int32_t *w, int automask, double min_depth, double max_depth, int rows_per_chunk);
size_t mdx_photometric_train_workspace_bytes(const mdx_train_desc *d);

/* disp, P, noise, idx, gdisp, to_opt: HOST arrays of nscales DEVICE pointers.
 *   disp[s] [B,1,h[s],w[s]]; P[s] [S,B,3,4] (the same pointer for every scale unless the pose depends on the
 *   scale); noise[s], ident [B,S,H,W] (MDX_FLAG_AUTOMASK only); target [B,3,H,W]; invK [B,4,4].
 * Outputs: idx[s] [B,H,W] uint8; loss_sum [nscales]; gdisp[s] [B,1,h[s],w[s]]; gP [nscales,S,B,3,4];
 *   optional depth0 [B,1,H,W] (depth of scale 0, outputs[("depth",0,0)]); optional to_opt (array may be NULL,
 *   entries may be NULL) [B,H,W].
 * gdisp == NULL and gP == NULL (both): every scale's FORWARD alone -- loss sums, indices, depth0, to_opt -- in one
 *   launch: what the validation loop (model_train.py:75-79, under torch.no_grad()) and model_test.py need.
 * t (optional): events recorded right before / after the fused kernel. */
int mdx_photometric_train(const mdx_train_desc *d, const float *const *disp, const float *target,
                          const mdx_sources *src, const float *invK, const float *const *P, const float *ident,
                          const float *const *noise, uint8_t *const *idx, float *loss_sum, float *const *gdisp,
                          float *gP, float *depth0, float *const *to_opt, void *workspace, size_t workspace_bytes,
                          void *stream, const mdx_timing *t);

/* ------------------------------------------------------------------------------------------
 * What the scales of one step share, once per step (csrc/photo_prologue.hip)
 *   processor.py:187-191 (identity losses), model_loss.py:28-33 (the target's SSIM window statistics, evaluated
 *   nscales * S times per step by the reference), processor.py:194-204 (identity + 1e-5 * randn and, since the identity
 *   channels come first and torch.min keeps the first minimum, the best identity channel of each pixel).
 * Outputs: tstat [B,H,W,6] = (mu_y[3], sigma_y[3]) per pixel; with MDX_FLAG_AUTOMASK per scale bidfi[s] [B,H,W,2] =
 *   (best identity value as float32, its channel index as int32); optional ident [B,S,H,W].
 * noise: HOST array of nscales device pointers [B,S,H,W] (injected draws: parity), or NULL: N(0,1) drawn in the kernel
 *   (Philox4x32-10 + Box-Muller) from rng_state = DEVICE {uint64 seed, uint64 offset}; advance_rng != 0 adds one to the
 *   offset afterwards (mdx_photometric_train_pre does so itself when it is handed rng_state). */
int mdx_photometric_prologue(const mdx_train_desc *d, const float *target, const mdx_sources *src,
                             const float *const *noise, unsigned long long *rng_state, int advance_rng,
                             float *ident, float *tstat, float *const *bidfi, void *stream);

/* mdx_photometric_train with the prologue's outputs in place of ident / noise: the kernel loads the target statistics
 * and the best identity channel (32 B per pixel and scale) instead of re-deriving / re-reading them.  Same outputs, bit
 * for bit.  rng_state (optional): its offset is advanced by the finishing kernel -- the next step (also the next replay
 * of a captured graph) draws new noise. */
int mdx_photometric_train_pre(const mdx_train_desc *d, const float *const *disp, const float *target,
                              const mdx_sources *src, const float *invK, const float *const *P,
                              const float *tstat, const float *const *bidfi, unsigned long long *rng_state,
                              uint8_t *const *idx, float *loss_sum, float *const *gdisp, float *gP, float *depth0,
                              float *const *to_opt, void *workspace, size_t workspace_bytes, void *stream,
                              const mdx_timing *t);

/* Edge-aware smoothness   replaces model_loss.py:77-88,112-115 (processor.py:208).
 * disp [B,1,h,w], color [B,3,h,w] -> loss [1]; gdisp (optional) = d loss / d disp for unit upstream.
 * normalize = 1: SmoothLoss (disp / (mean_HW(disp) + 1e-7) first); 0: EdgeAwareSmooth on disp as given.
 * Two launches (MDX_VERSION 400; four before): a main pass on the disparity as given + a finishing pass that forms the
 * per-image mean from the main pass's partials. */
size_t mdx_smooth_workspace_bytes(int B, int h, int w);
int mdx_smooth_loss(int B, int h, int w, const float *disp, const float *color, int normalize, float *loss,
                    float *gdisp, void *workspace, size_t workspace_bytes, void *stream);

/* The same for every scale of a step, both passes launched once for all scales (the scale loop of processor.py:208):
 * h, w, disp, color, gdisp: HOST arrays of nscales entries (gdisp NULL or all entries given); loss [nscales]. */
size_t mdx_smooth_multi_workspace_bytes(int nscales, int B, const int32_t *h, const int32_t *w);
int mdx_smooth_loss_multi(int nscales, int B, const int32_t *h, const int32_t *w, const float *const *disp,
                          const float *const *color, int normalize, float *loss, float *const *gdisp,
                          void *workspace, size_t workspace_bytes, void *stream);

/* The scalar tail of the loss   processor.py:208-217 (scale_loss = mean + disp_smoothness * smooth / 2**scale; total = sum / len)
 * and its backward fan-out, one launch each way instead of ~20 / ~30 scalar launches + three whole-map passes per scale.
 * sums [nscales] = sum over the pixels of to_optimise (mdx_photometric_train), smooth [nscales] (mdx_smooth_loss_multi),
 * scale: HOST array opt.scales, pixels = B*H*W -> total [1].  Rounded op by op as ATen-GPU rounds the reference's expression.
 * bwd: g_total [1] (device), gd_photo / gd_smooth: HOST arrays of nscales device pointers (the unit-upstream gradients the two
 * kernels left), count[s] = elements of scale s -> gdisp[s] = gd_photo[s] * c1 + gd_smooth[s] * c2[s];
 * gP [nscales][nP] (optional) -> gP_out [nscales][nP] * c1 (per_scale_P) or their sum over the scales [nP]. */
int mdx_loss_total_fwd(int nscales, const float *sums, const float *smooth, const int32_t *scale, int64_t pixels,
                       double disp_smoothness, float *total, void *stream);
int mdx_loss_total_bwd(int nscales, const float *g_total, const int32_t *scale, int64_t pixels, double disp_smoothness,
                       const float *const *gd_photo, const float *const *gd_smooth, const int64_t *count,
                       float *const *gdisp, const float *gP, int nP, int per_scale_P, float *gP_out, void *stream);

/* The optimiser step   reference model_tool/loader.py:93-97 (torch.optim.Adam, no weight decay / amsgrad / maximize) in ONE launch
 * for every parameter of a group.  table: DEVICE array of { float *param, *exp_avg, *exp_avg_sq; const float *step; int64_t numel }
 * (mdx_adam_table_entry_bytes() each; step = the tensor's float32 step count, already incremented); one call takes entries
 * first .. first + count - 1, count <= mdx_adam_max_tensors(); grads: HOST array of count device pointers (they change from step
 * to step); blockmap: DEVICE array of nblocks { int32 tensor (0-based within the call), int32 chunk } covering every tensor in
 * chunks of mdx_adam_chunk() elements; lr_ptr: device float32 (a captured step's learning rate) or NULL (then lr).
 * Arithmetic: ATen's fused Adam, expression by expression (ATen/native/cuda/fused_adam_utils.cuh). */
int mdx_adam_max_tensors(void);
int mdx_adam_chunk(void);
size_t mdx_adam_table_entry_bytes(void);
int mdx_adam_step(const void *table, int first, int count, const float *const *grads, const void *blockmap, int nblocks,
                  const float *lr_ptr, double lr, double beta1, double beta2, double eps, void *stream);

/* The guarded step: clip by the global gradient norm and / or skip a step whose norm is not finite, decided on the device (a
 * captured loop cannot branch on the host).  Three launches instead of torch._foreach_add_(steps, 1) + mdx_adam_step, ordered by
 * the stream alone -- no atomics, no block waits for another:
 *   mdx_adam_grad_sumsq    table / first / count / grads / blockmap / nblocks as for mdx_adam_step (only numel is read); block b
 *                          writes the sum of g^2 over its chunk, squared and added in double, to partials[b] (DEVICE, nblocks
 *                          doubles, mdx_adam_guard_partials_bytes(nblocks)).  Several calls (more than mdx_adam_max_tensors()
 *                          tensors, several parameter groups) take disjoint slices of one partials buffer.
 *   mdx_adam_guard_finish  one block: adds partials[0 .. npartials - 1] in a fixed order and writes the DEVICE record
 *                          (mdx_adam_guard_record_bytes(), 8-byte aligned, zeroed once by the caller):
 *                            { float total_norm = (float)sqrt(sum);  float coef;  int32 skipped;  int32 reserved;
 *                              int64 steps;  int64 skipped_steps }
 *                          coef = min(1, max_grad_norm / (total_norm + 1e-6)) in float32, or exactly 1 when max_grad_norm <= 0
 *                          (no clipping); skipped = skip_nonfinite && !isfinite(total_norm).  steps += 1, skipped_steps +=
 *                          skipped.  Unless skipped it adds 1 to the step count of table entries 0 .. ntensors - 1 (step is the
 *                          count BEFORE this step here: the caller does not increment it).
 *   mdx_adam_step_guarded  mdx_adam_step reading the record: returns at once when skipped (parameters, moments and step counts keep
 *                          their bits), otherwise consumes g * coef -- one float32 multiply, rounded before Adam's own arithmetic;
 *                          coef == 1 gives mdx_adam_step's bits.  The gradients are never written.
 * A NaN max_grad_norm is MDX_ERR_BAD_SHAPE. */
size_t mdx_adam_guard_record_bytes(void);
size_t mdx_adam_guard_partials_bytes(int nblocks);
int mdx_adam_grad_sumsq(const void *table, int first, int count, const float *const *grads, const void *blockmap, int nblocks,
                        double *partials, void *stream);
int mdx_adam_guard_finish(const void *table, int ntensors, const double *partials, int npartials, double max_grad_norm,
                          int skip_nonfinite, void *record, void *stream);
int mdx_adam_step_guarded(const void *table, int first, int count, const float *const *grads, const void *blockmap, int nblocks,
                          const float *lr_ptr, double lr, double beta1, double beta2, double eps, const void *record, void *stream);

/* An exponential moving average of the weights, kept on the device (csrc/ema.hip; mdx.optim.WeightEMA): capturable with the step,
 * its decay warm-up and the guard's skip decided from device records.  table: DEVICE array of { float *live, *shadow; int64_t numel }
 * (mdx_ema_table_entry_bytes() each; the shadow has the live tensor's dense storage order); first / count / blockmap / nblocks as
 * for mdx_adam_step (count <= mdx_adam_max_tensors(), chunks of mdx_adam_chunk() elements).  record: DEVICE
 * { int64 updates; int64 held } (mdx_ema_record_bytes(), 8-byte aligned, zeroed once by the caller).
 *   mdx_ema_update  t = record.updates; d = warmup ? min(decay, (1 + t) / (10 + t)) : decay, in double; w = (float)(1 - d);
 *                   shadow = lerp(shadow, live, w) by ATen's rule in float32: w < 0.5 ? e + w * (p - e) : p - (p - e) * (1 - w).
 *                   The record is only read: several calls of one update (more than mdx_adam_max_tensors() tensors) see the same t.
 *                   guard_record: NULL, or the step guard's record (mdx_adam_guard_finish); when it says skipped, nothing is written.
 *   mdx_ema_tick    one thread, after the last mdx_ema_update of an update: updates += 1, or held += 1 when the guard record
 *                   says skipped.
 *   mdx_ema_swap    exchanges live and shadow bit for bit, in place; two calls are the identity.
 * A decay that is NaN or outside [0, 1) is MDX_ERR_BAD_SHAPE. */
size_t mdx_ema_table_entry_bytes(void);
size_t mdx_ema_record_bytes(void);
int mdx_ema_update(const void *table, int first, int count, const void *blockmap, int nblocks, double decay, int warmup,
                   const void *record, const void *guard_record, void *stream);
int mdx_ema_tick(void *record, const void *guard_record, void *stream);
int mdx_ema_swap(const void *table, int first, int count, const void *blockmap, int nblocks, void *stream);

/* A 64-bit digest of every weight tensor, computed on the device (csrc/digest.hip; mdx.optim.WeightDigest): what data-parallel ranks
 * compare after a step (model_tool/parallel.py: check_replicas) and what a checkpoint's state file records of the weight files
 * beside it.  table: DEVICE array of { const uint32_t *words; int64_t numel } (mdx_digest_table_entry_bytes() = 16 each; the tensor's
 * dense storage, read as 32-bit words); first / count / blockmap / nblocks as for mdx_adam_step (count <= mdx_adam_max_tensors(),
 * chunks of mdx_adam_chunk() words).  out: DEVICE array of at least first + count 64-bit words, 8-byte aligned.
 *   mdx_digest_words  out[first + t] = the digest of table entry first + t, t = 0 .. count - 1: the sum modulo 2^64, over storage
 *                     index i = 0 .. numel - 1, of the 32-bit hash of (i, u = word i):
 *                         k = u ^ ((uint32_t)i * 0x9E3779B1u);
 *                         k ^= k >> 16;  k *= 0x85EBCA6Bu;  k ^= k >> 13;  k *= 0xC2B2AE35u;  k ^= k >> 16;
 *                     The words are never read as floats: NaN payloads and the sign of zero count, an all-zero tensor has a
 *                     non-zero digest, two exchanged elements change it.  An integer sum: any order of the blocks gives the same
 *                     bits, there is no tolerance.  The call clears out[first .. first + count - 1] itself (a small launch
 *                     on `stream` in front of the pass): callers never zero, and the pair is capturable and replayable.
 * The index is taken modulo 2^32: a tensor of 2^32 words or more is not refused; its words 2^32 apart share their index.
 * A misaligned out is MDX_ERR_MISALIGNED. */
size_t mdx_digest_table_entry_bytes(void);
int mdx_digest_words(const void *table, int first, int count, const void *blockmap, int nblocks, uint64_t *out, void *stream);

/* Per-tensor gradient and weight statistics, computed on the device (csrc/tensor_stats.hip; mdx.optim.GradStats): where the step
 * guard knows one global norm, this read-only pass says which tensor.  table: DEVICE array of { const float *weight; int64_t numel }
 * (mdx_tensor_stats_table_entry_bytes() = 16 each; the parameter's dense storage); first / count / blockmap / nblocks as for
 * mdx_adam_step (count <= mdx_adam_max_tensors(), chunks of mdx_adam_chunk() elements); grads: HOST array of count device pointers
 * as for mdx_adam_grad_sumsq, except that an entry may be NULL: that parameter received no gradient in this pass.
 *   mdx_tensor_stats_partials  block b writes the record of its chunk -- an mdx_tensor_stats over the chunk's elements alone -- to
 *                              slot b of partials (DEVICE, nblocks slots of mdx_tensor_stats_partial_bytes() = 40, 8-byte aligned).
 *                              Several calls (more than mdx_adam_max_tensors() tensors) take disjoint slices of one partials buffer,
 *                              in table order, so that tensor t's slots are offsets[t] .. offsets[t + 1] - 1 of the whole buffer.
 *                              An element is finite when its exponent bits are not all ones; a square is formed and added in
 *                              double (exact, and 1e30 squared stays finite); a zero is +0 or -0; a magnitude is compared by its
 *                              bits, so denormals count whatever the denormal mode.  A NULL gradient: the weight half alone.
 *   mdx_tensor_stats_finish    one block per tensor first .. first + count - 1: adds the tensor's slots of partials (the WHOLE
 *                              buffer's base) in a fixed order -- offsets: DEVICE array of int32, one more than there are tensors --
 *                              and writes records[t] (DEVICE, mdx_tensor_stats_record_bytes() = 40 each, 8-byte aligned).  With
 *                              history (DEVICE, mdx_tensor_stats_history_bytes() = 56 each, 8-byte aligned, zeroed once by the
 *                              caller; or NULL) it advances history[t]: passes += 1; grad_nonfinite > 0 counts a bad pass and
 *                              sets first / last; weight_nonfinite > 0 sets first_bad_weight_pass once; a gradient that is present
 *                              and whose grad_sumsq exceeds max_grad_sumsq sets it and max_grad_pass (the first pass of a tie).
 * Every slot, record and history entry is written by exactly one thread with plain stores: no atomics, nothing to clear, the same
 * inputs give the same bits at every launch, and the pair is capturable and replayable.  Nothing but the three outputs is written. */
typedef struct mdx_tensor_stats {          /* 40 bytes */
    double grad_sumsq, weight_sumsq;       /* over FINITE elements only */
    float grad_absmax, weight_absmax;      /* over finite elements; 0 when there is none */
    uint32_t grad_nonfinite, weight_nonfinite, grad_zeros;   /* counts modulo 2^32 */
    uint32_t grad_present;                 /* 0: no gradient pointer was given; the grad_* fields are 0 */
} mdx_tensor_stats;

typedef struct mdx_tensor_stats_history {  /* 56 bytes; all-zero is the valid initial state */
    int64_t passes, bad_passes;            /* bad: grad_nonfinite > 0 */
    int64_t first_bad_pass, last_bad_pass; /* 1-based pass numbers of this tensor; 0 = never */
    int64_t first_bad_weight_pass;         /* first pass with weight_nonfinite > 0; 0 = never */
    double max_grad_sumsq;                 /* the largest grad_sumsq of a pass with a gradient; over finite elements, so finite */
    int64_t max_grad_pass;                 /* that pass; 0 = none yet (no gradient, or only zero ones) */
} mdx_tensor_stats_history;

size_t mdx_tensor_stats_table_entry_bytes(void);
size_t mdx_tensor_stats_partial_bytes(void);
size_t mdx_tensor_stats_record_bytes(void);
size_t mdx_tensor_stats_history_bytes(void);
int mdx_tensor_stats_partials(const void *table, int first, int count, const float *const *grads, const void *blockmap, int nblocks,
                              void *partials, void *stream);
int mdx_tensor_stats_finish(int first, int count, const int *offsets, const void *partials, void *records, void *history,
                            void *stream);

/* Statistics of the maps the fused loss path leaves behind, computed on the device (csrc/loss_stats.hip; mdx.loss_stats.LossStats):
 * which pixels the auto-mask removed and which source frame won the minimum, and the range of the disparity at every scale -- the
 * two places where a step that learns nothing (a stationary scene, a disparity collapsed to a constant) shows.  A read-only pass over
 * all scales of a step at once: nscales (1..MDX_MAX_SCALES), B, H, W >= 1 with H * W < 2^32, S (1..MDX_MAX_SRC), automask (0 / 1);
 * h, w: HOST arrays of nscales disparity sizes, each >= 1 and otherwise free; idx: HOST array of nscales device pointers to uint8
 * [B,H,W] arg-min channels, always full resolution; disp: HOST array of nscales device pointers to contiguous float32
 * [B,1,h[s],w[s]], 4-byte aligned.  An entry of idx or disp may be NULL: that half of the scale's records is 0 and says "absent".
 *   mdx_loss_stats_plan      -> the number of blocks of pass 1 = the number of partial slots (>= 1; MDX_ERR_BAD_SHAPE when it does
 *                            not fit an int); with blockmap (HOST, that many entries of mdx_loss_stats_blockmap_entry_bytes() = 16:
 *                            int32 {scale, image, chunk, 0 = index map / 1 = disparity}) it writes the map the caller copies to the
 *                            device once.  Scale after scale, image after image, per image ceil(H * W / mdx_loss_stats_index_chunk())
 *                            index chunks, then ceil(h[s] * w[s] / mdx_loss_stats_disp_chunk()) disparity chunks; a NULL map keeps
 *                            its slots.
 *   mdx_loss_stats_partials  block b writes the record of its chunk to slot b of partials (DEVICE, nblocks slots of
 *                            mdx_loss_stats_partial_bytes() = 72, 8-byte aligned); nblocks must be the plan's.  uint8 maps are read
 *                            as 16-byte vectors and disparities as float4 where the IMAGE's base (idx[s] + b * H * W) is 16-byte
 *                            aligned and the chunk is whole; element by element otherwise and in an image's tail.  An index
 *                            >= (automask ? 2S : S) counts as bad_index and in no winner.  A disparity element is finite when its
 *                            exponent bits are not all ones; it is added, and its square formed and added, in double; finite
 *                            elements are compared by value (-0 below +0, denormals whatever the denormal mode).
 *   mdx_loss_stats_finish    one block per scale, one of its four waves per image: adds each image's slots in a fixed order and
 *                            writes records[s * B + b] (DEVICE, mdx_loss_stats_record_bytes() = 72 each, 8-byte aligned).  With
 *                            history (DEVICE, nscales entries of mdx_loss_stats_history_bytes() = 152, 8-byte aligned, zeroed once
 *                            by the caller; or NULL) it advances history[s] as the struct below says.  static_share in (0, 1].
 * Refusals come before any HIP call: NULL pointers (the arrays, blockmap, partials, records), then shapes (a size out of range,
 * H * W >= 2^32, static_share outside (0, 1] or not finite, nblocks < 1 or not the plan's), then alignment.  Every slot, record and
 * history entry is written by exactly one thread with plain stores: no atomics, nothing to clear, the same inputs give the same
 * bits at every launch, and the pair is capturable and replayable.  Nothing but the three outputs is written. */
typedef struct mdx_loss_stats {            /* 72 bytes, per (scale, image) */
    double disp_sum, disp_sumsq;           /* over FINITE disparity elements; float -> double, squares formed in double */
    float disp_min, disp_max;              /* over finite elements, compared by value; 0 when there is none */
    uint32_t winner[2 * MDX_MAX_SRC];      /* winner[c] = pixels with idx == c.  automask: c < S are the identity channels (masked
                                              pixels), S <= c < 2S the warped sources; without automask c < S are the sources.
                                              0 for every c that is not legal */
    uint32_t bad_index;                    /* pixels with idx >= (automask ? 2S : S): a corrupt map */
    uint32_t disp_nonfinite;               /* exponent bits all ones */
    uint32_t index_present, disp_present;  /* 0: the pointer was NULL; that half's fields are 0 */
} mdx_loss_stats;

typedef struct mdx_loss_stats_history {    /* 152 bytes, per scale; all-zero is the valid initial state */
    int64_t passes, images;                /* images += B per pass with an index map */
    int64_t winner_total[2 * MDX_MAX_SRC]; /* sums of winner[] over passes and images */
    int64_t bad_passes, first_bad_pass;    /* a pass with bad_index > 0 or disp_nonfinite > 0 in any image; 1-based, 0 = never */
    int64_t static_images, first_static_pass, last_static_pass;
                                           /* automask only: an image is static when (double)masked >= static_share * (double)(H*W),
                                              masked = sum of winner[c < S] */
    double max_masked_share;               /* automask only: (double)masked / (double)(H*W), largest over images and passes */
    int64_t max_masked_pass;               /* that pass, the first of a tie; 0 = no masked pixel yet */
    double min_disp_range;                 /* (double)disp_max - (double)disp_min of an image with at least one finite element,
                                              smallest seen */
    int64_t min_disp_range_pass;           /* that pass, the first of a tie; 0 = none yet */
} mdx_loss_stats_history;

size_t mdx_loss_stats_partial_bytes(void);
size_t mdx_loss_stats_record_bytes(void);
size_t mdx_loss_stats_history_bytes(void);
size_t mdx_loss_stats_blockmap_entry_bytes(void);
int mdx_loss_stats_index_chunk(void);
int mdx_loss_stats_disp_chunk(void);
int mdx_loss_stats_plan(int nscales, int B, int H, int W, const int *h, const int *w, void *blockmap);
int mdx_loss_stats_partials(int nscales, int B, int H, int W, int S, int automask, const int *h, const int *w,
                            const uint8_t *const *idx, const float *const *disp, const void *blockmap, int nblocks, void *partials,
                            void *stream);
int mdx_loss_stats_finish(int nscales, int B, int H, int W, int S, int automask, const int *h, const int *w, double static_share,
                          const void *partials, void *records, void *history, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fine-grained ops behind the reference's model_layer / model_loss API (each differentiable)
 * ---------------------------------------------------------------------------------------- */

/* interpolate(x, H, W, "bilinear", align_corners=False)   warp.py:18-20.  x [BC,h,w] -> [BC,H,W] */
int mdx_interpolate_bilinear_fwd(const float *x, int BC, int h, int w, float *out, int H, int W,
                                 void *stream);
int mdx_interpolate_bilinear_bwd(const float *gout, int BC, int H, int W, float *gin, int h, int w,
                                 void *stream);

/* disparity2depth   warp.py:29-39.  sd/depth may be NULL.  bwd: gdisp = gsd*b + gdepth*(-b*depth^2) */
int mdx_disparity2depth_fwd(const float *disp, size_t n, double min_depth, double max_depth,
                            float *sd, float *depth, void *stream);
int mdx_disparity2depth_bwd(const float *disp, const float *gsd, const float *gdepth, size_t n,
                            double min_depth, double max_depth, float *gdisp, void *stream);

/* Depth2PointCloud.forward   warp.py:237-246.  depth [B,1,H,W], invK [B,4,4] -> cam [B,4,HW] */
int mdx_backproject_fwd(const float *depth, const float *invK, int B, int H, int W, float *cam,
                        void *stream);
int mdx_backproject_bwd(const float *gcam, const float *invK, int B, int H, int W, float *gdepth,
                        void *stream);

/* PointCloud2Pixel.forward   warp.py:259-269, with P = (K@T)[:3].  cam [B,4,HW] -> grid [B,H,W,2]
 * bwd: ggrid -> gcam [B,4,HW] (row 3 zero) and gP [B,3,4]. workspace: mdx_project_workspace_bytes */
size_t mdx_project_workspace_bytes(int B, int H, int W);
int mdx_project_fwd(const float *cam, const float *P, int B, int H, int W, float eps, float *grid,
                    void *stream);
int mdx_project_bwd(const float *cam, const float *P, const float *ggrid, int B, int H, int W,
                    float eps, float *gcam, float *gP, void *workspace, size_t workspace_bytes,
                    void *stream);

/* grid_sample(img, grid, "border", align_corners=True), bilinear   warp.py:12-14.
 * img [B,C,Hi,Wi], grid [B,Ho,Wo,2] -> out [B,C,Ho,Wo];  bwd -> ggrid (gimg optional, atomics) */
int mdx_grid_sample_border_fwd(const float *img, const float *grid, int B, int C, int Hi, int Wi,
                               int Ho, int Wo, float *out, void *stream);
int mdx_grid_sample_border_bwd(const float *img, const float *grid, const float *gout, int B, int C,
                               int Hi, int Wi, int Ho, int Wo, float *ggrid, float *gimg,
                               void *stream);

/* ReprojectionLoss.forward   model_loss.py:97-103 (SSIM 28-41).  pred,target [B,3,H,W] -> [B,1,H,W]
 * bwd: gout [B,1,H,W] -> gpred [B,3,H,W] (gtarget optional) */
int mdx_reprojection_loss_fwd(const float *pred, const float *target, int B, int H, int W,
                              float *out, void *stream);
int mdx_reprojection_loss_bwd(const float *pred, const float *target, const float *gout, int B,
                              int H, int W, float *gpred, float *gtarget, void *stream);
/* SSIM.forward alone   model_loss.py:28-41.  x,y [BC,H,W] -> [BC,H,W] */
int mdx_ssim_fwd(const float *x, const float *y, int BC, int H, int W, float *out, void *stream);
/* its backward (the reference's SSIM module is differentiable through autograd): gout [BC,H,W] -> gx and / or gy [BC,H,W] */
int mdx_ssim_bwd(const float *x, const float *y, const float *gout, int BC, int H, int W, float *gx, float *gy,
                 void *stream);

/* identity+noise, concat, per-pixel min   processor.py:194-204.  ident/noise/reproj [B,S,H,W]
 * -> combined [B,C,H,W] (optional), to_opt [B,H,W], idx [B,H,W] uint8 */
int mdx_min_automask_fwd(const float *ident, const float *noise, const float *reproj, int B, int S,
                         int H, int W, int automask, float *combined, float *to_opt, uint8_t *idx,
                         void *stream);

/* param2matrix   model_layer/warp.py:126-153 (with vector2translation :43-61, angle2rotation :65-122).
 * axisangle, translation [N,3] (the reference's [N,1,3]) -> M [N,4,4]; invert as in the reference.
 * bwd: gM [N,4,4] -> gaxisangle, gtranslation [N,3]. */
int mdx_param2matrix_fwd(const float *axisangle, const float *translation, int N, int invert, float *M, void *stream);
int mdx_param2matrix_bwd(const float *axisangle, const float *translation, const float *gM, int N, int invert,
                         float *gaxisangle, float *gtranslation, void *stream);

/* The pose network's output -> camera-to-camera matrices and projections for every source frame, one launch each way
 * (processor.py:61-83 slices + param2matrix, :143-160 K @ T): raw [M,F,6] = the pose head's 0.01-scaled output
 * (axis-angle | translation; pose_decoder.py:51-53); source s reads rows row0[s] .. row0[s]+B-1, entry frame[s], inverted if
 * invert[s] (HOST arrays of S entries); K [B,4,4] -> T [S,B,4,4], P [S,B,3,4] = (K @ T)[:, :3].
 * bwd: gP [S,B,3,4] and / or gT [S,B,4,4] (either may be NULL) -> graw [M,F,6] (entries no source reads: zeros). */
int mdx_pose_projection_fwd(const float *raw, int M, int F, const float *K, int B, int S, const int32_t *row0,
                            const int32_t *frame, const int32_t *invert, float *T, float *P, void *stream);
int mdx_pose_projection_bwd(const float *raw, int M, int F, const float *K, int B, int S, const int32_t *row0,
                            const int32_t *frame, const int32_t *invert, const float *gP, const float *gT, float *graw,
                            void *stream);

/* ---- network glue around the convolutions (no reference FFI: these replace torch op sequences of
 * model_layer/depth_decoder.py:44-47,96-106 and the ResNet stem max-pool, model_layer/depth_encoder.py) ----
 * dtype codes: 0 = float32, 1 = bfloat16 (storage; arithmetic is float32). */

/* out [B,C1+C2,u*h+2,u*w+2] = ReflectionPad2d(1)( cat( nearest_up_u( act(raw [B,C1,h,w] + bias [C1]) ), skip [B,C2,u*h,u*w] ) ),
 * u = upsample ? 2 : 1, act = elu ? ELU : identity; skip may be NULL when C2 == 0; bias (float32, may be NULL) is
 * the bias of the convolution that produced raw, when that convolution was run without it.
 * (in_dtype, out_dtype) in {(0,0), (1,1), (1,0)}; skip has in_dtype. */
int mdx_decoder_glue_fwd(const void *raw, const void *skip, const float *bias, void *out, int B, int C1, int C2, int h,
                         int w, int upsample, int elu, int in_dtype, int out_dtype, void *stream);
/* gout has out's shape / out_dtype; graw, gskip have the inputs' shapes / in_dtype (gskip NULL when C2 == 0);
 * dbias [C1] float32 = sum of graw over (b, y, x) (NULL to skip; needs the workspace, fixed summation order). */
size_t mdx_decoder_glue_workspace_bytes(int B, int C1, int h, int w);
int mdx_decoder_glue_bwd(const void *gout, const void *raw, const float *bias, void *graw, void *gskip, float *dbias,
                         int B, int C1, int C2, int h, int w, int upsample, int elu, int in_dtype, int out_dtype,
                         void *workspace, size_t workspace_bytes, void *stream);

/* MaxPool2d(3, stride 2, padding 1) on [BC,H,W] -> [BC,Ho,Wo], Ho = (H-1)/2+1; arg [BC,Ho,Wo] uint8 = window tap
 * (0..8, row-major) of the first maximum, consumed by the backward (a gather, no atomics). */
int mdx_maxpool3s2_fwd(const void *in, void *out, uint8_t *arg, int BC, int H, int W, int dtype, void *stream);
int mdx_maxpool3s2_bwd(const void *gout, const uint8_t *arg, void *gin, int BC, int H, int W, int dtype, void *stream);

/* Training-mode BatchNorm2d + residual add + ReLU of the ResNet blocks (model_layer/depth_encoder.py; the reference
 * gets them from torchvision): y = act(bn(x) [+ res]) with batch statistics over (B,H,W), running statistics updated
 * in place as torch.nn.functional.batch_norm(training=True) does (run_mean/run_var may both be NULL).
 * The tensors hold `groups` consecutive sub-batches of B images: x, res, y, dy, dx, dres [groups*B,C,H,W] float32
 * (dtype 0) or bfloat16 (dtype 1); each sub-batch is normalised with its own statistics and updates the running
 * statistics in turn -- what `groups` calls on the sub-batches do.  gamma, beta, statistics float32;
 * save_mean / save_invstd [groups,C] go from forward to backward.  One launch each way for maps up to 24 K elements
 * per channel and sub-batch, two per sub-batch above. */
size_t mdx_bn_workspace_bytes(int B, int C, int H, int W);
int mdx_bn_act_fwd(const void *x, const void *res, const float *gamma, const float *beta, float *run_mean,
                   float *run_var, void *y, float *save_mean, float *save_invstd, int B, int C, int H, int W,
                   int groups, float eps, float momentum, int relu, int dtype, void *workspace, size_t workspace_bytes,
                   void *stream);
/* dz = dy * (y > 0) when relu; dx, d(res) = dz (dres NULL when there was no residual); dgamma, dbeta [C] summed
 * over the sub-batches. */
int mdx_bn_act_bwd(const void *dy, const void *y, const void *x, const float *gamma, const float *save_mean,
                   const float *save_invstd, void *dx, void *dres, float *dgamma, float *dbeta, int B, int C, int H,
                   int W, int groups, int relu, int dtype, void *workspace, size_t workspace_bytes, void *stream);

/* EVAL-mode BatchNorm2d + residual add + ReLU (csrc/norm_infer.hip; model_layer/depth_encoder.py BatchNorm2d.act when the
 * module is not training): y = act(x * s + t [+ res]) per channel, s = gamma / sqrt(run_var + eps), t = beta - run_mean * s,
 * what torch.nn.functional.batch_norm(training=False) computes.  One launch, no workspace, no atomics; the running
 * statistics are read, never written.  x, res, y float32 (dtype 0) or bfloat16 (dtype 1); gamma, beta, run_mean, run_var
 * [C] float32; res may be NULL, every other pointer must not be; relu 0 / 1.
 * mdx_bn_act_infer: planar [B][C][H][W], any C and H * W, element-aligned pointers.
 * mdx_bn_act_nhwc_infer: channels-last [B][H][W][C]; C a multiple of 4 (float32) / 8 (bfloat16) and x, res, y 16-byte aligned,
 * else MDX_ERR_BAD_SHAPE / MDX_ERR_MISALIGNED (the caller then takes the planar entry point). */
int mdx_bn_act_infer(const void *x, const void *res, const float *gamma, const float *beta, const float *run_mean,
                     const float *run_var, void *y, int B, int C, int H, int W, float eps, int relu, int dtype,
                     void *stream);
int mdx_bn_act_nhwc_infer(const void *x, const void *res, const float *gamma, const float *beta, const float *run_mean,
                          const float *run_var, void *y, int B, int C, int H, int W, float eps, int relu, int dtype,
                          void *stream);

/* ---- the same network glue for CHANNELS-LAST maps (memory [B][H][W][C]; csrc/norm_nhwc.hip, csrc/glue_nhwc.hip) ----
 * What MIOpen's implicit-GEMM convolutions read and write without a layout transpose on either side.  Same operators,
 * same arithmetic and summation order per element as the planar entry points above; a thread owns one 16-byte channel
 * vector, so every channel count must be a multiple of 4 (float32) / 8 (bfloat16) and every map pointer 16-byte aligned
 * (else MDX_ERR_BAD_SHAPE / MDX_ERR_MISALIGNED: the caller then takes the planar entry points).
 *
 * mdx_bn_act_nhwc_*: model_layer/depth_encoder.py:27,95 (BatchNorm2d + ReLU + residual of every ResNet block).
 * x, res, y, dy, dx, dres [groups*B][H][W][C]; three launches each way (block partials, a float64 finalize pass, apply),
 * no atomics.  dy2 (may be NULL): a second upstream gradient of y, added on the way in -- a block's output feeds the next
 * block's first convolution AND its identity path, and autograd would otherwise spend one more pass over the map on
 * adding the two.  bwd with y NULL (relu, no residual: dres NULL; beta given): the ReLU mask is re-derived from x with the forward
 * pass's own expressions instead of being read -- one map less in each of the two passes (beta is read in that case only). */
size_t mdx_bn_nhwc_workspace_bytes(int B, int C, int H, int W, int groups, int dtype);
int mdx_bn_act_nhwc_fwd(const void *x, const void *res, const float *gamma, const float *beta, float *run_mean,
                        float *run_var, void *y, float *save_mean, float *save_invstd, int B, int C, int H, int W,
                        int groups, float eps, float momentum, int relu, int dtype, void *workspace,
                        size_t workspace_bytes, void *stream);
int mdx_bn_act_nhwc_bwd(const void *dy, const void *dy2, const void *y, const void *x, const float *gamma,
                        const float *beta, const float *save_mean, const float *save_invstd, void *dx, void *dres, float *dgamma,
                        float *dbeta, int B, int C, int H, int W, int groups, int relu, int dtype, void *workspace,
                        size_t workspace_bytes, void *stream);
/* mdx_bn_act_nhwc_bwd with dres on a float32 map forms dz = (dy [+ dy2]) * (y > 0) once: the statistics pass stores it to dres,
 * the apply pass reads dres and x only (eight map-sized streams, not ten; the same bits).  dres shares storage with no input.
 * mdx_bn_dz_once(0) switches this off process-wide (both passes form dz, as for bfloat16), for A/B runs and
 * tests; it returns the previous setting and must not race a launch. */
int mdx_bn_dz_once(int on);
/* The ResNet stem forward, relu(bn(x)) followed by MaxPool2d(3, 2, 1), as one operator (float32 only: dtype 1 is MDX_ERR_BAD_SHAPE
 * and the caller takes mdx_bn_act_nhwc_fwd + mdx_maxpool3s2_nhwc_fwd, whose results this equals bit for bit).  x, y
 * [groups*B][H][W][C]; pooled, arg [groups*B][Ho][Wo][C], Ho = (H - 1) / 2 + 1.  Workspace: mdx_bn_nhwc_workspace_bytes.  Three
 * launches: the statistics and finalize passes of mdx_bn_act_nhwc_fwd, then one pass that normalises the nine x taps of every
 * window, writes pooled and arg (first maximum wins, NaN propagates) and -- only when y is not NULL -- the map y itself, every pixel
 * once.  save_mean, save_invstd and arg are what mdx_bn_act_nhwc_bwd (y NULL) and mdx_maxpool3s2_nhwc_bwd take in the backward. */
int mdx_bn_pool_nhwc_fwd(const void *x, const float *gamma, const float *beta, float *run_mean, float *run_var, void *y,
                         void *pooled, uint8_t *arg, float *save_mean, float *save_invstd, int B, int C, int H, int W,
                         int groups, float eps, float momentum, int dtype, void *workspace, size_t workspace_bytes,
                         void *stream);
/* Between the pose decoder's convolutions  model_layer/pose_decoder.py:24-53 (the convolution runs without its bias).
 * bias_act: y = act(x + bias), x, y [B][H][W][C] channels-last (dtype 0 float32 / 1 bfloat16, C a multiple of the 16-byte vector),
 * bias [C] float32, relu 0 / 1.  bwd: dy, y -> dx, dbias [C]: one launch + a finishing pass over the block partials (workspace).
 * mean_bias: out [B][C] float32 = scale * (mean over H*W of x + bias) -- the head's spatial mean and 0.01 (pose_decoder.py:51-53);
 * any C.  bwd: gout [B][C] -> dx (x's dtype), dbias [C] (may be NULL). */
size_t mdx_bias_act_nhwc_workspace_bytes(int B, int C, int H, int W, int dtype);
int mdx_bias_act_nhwc_fwd(const void *x, const float *bias, void *y, int B, int C, int H, int W, int relu, int dtype, void *stream);
int mdx_bias_act_nhwc_bwd(const void *dy, const void *y, void *dx, float *dbias, int B, int C, int H, int W, int relu, int dtype,
                          void *workspace, size_t workspace_bytes, void *stream);
int mdx_mean_bias_nhwc_fwd(const void *x, const float *bias, float *out, int B, int C, int H, int W, float scale, int dtype,
                           void *stream);
int mdx_mean_bias_nhwc_bwd(const float *gout, void *dx, float *dbias, int B, int C, int H, int W, float scale, int dtype,
                           void *stream);

/* The networks' input   depth_encoder.py:89 ((x - 0.45) / 0.225) + processor.py:61-75 (the pose network's frame pairs concatenated
 * along the channels; this package: the pairs along the batch) written channels-last in one pass.  src: HOST array of
 * blocks * groups (1..2 each) device pointers, src[k * groups + g] a planar float32 [n][3][H][W] frame;
 * out [blocks * n][H][W][3 * groups] (dtype 0 float32 / 1 bfloat16) = (src - mean) * inv_std. */
int mdx_encoder_input_nhwc(const float *const *src, int blocks, int groups, int n, int H, int W, float mean, float inv_std,
                           void *out, int dtype, void *stream);

/* Weight gradient of the decoder's thin 3x3 convolutions   model_layer/depth_decoder.py:96-106 (16 output channels, 16 or 32 input
 * channels, on the two biggest maps): x [B][h+2][w+2][Cin] the reflection-padded input, gy [B][h][w][16], float32 channels-last,
 * w a multiple of 4 -> gweight, element (co, ci, ky, kx) at gweight[co * s_o + ci * s_c + ky * s_y + kx * s_x].  One MFMA launch
 * (v_mfma_f32_16x16x4_f32; operands loaded as they lie in memory) + a finishing pass over the block partials (fixed order). */
size_t mdx_thin_conv3x3_wgrad_workspace_bytes(int B, int Cin, int Cout, int h, int w);
int mdx_thin_conv3x3_wgrad(const float *x, const float *gy, float *gweight, int64_t s_o, int64_t s_c, int64_t s_y, int64_t s_x, int B,
                           int Cin, int Cout, int h, int w, void *workspace, size_t workspace_bytes, void *stream);

/* The decoder's last stage convolution on the low-resolution map (csrc/upconv_nhwc.hip; mdx.functional.up_conv3x3):
 *   out = conv3x3(ReflectionPad2d(1)(nearest_x2(ELU(raw + bias))), weight)          (no output bias)
 * raw, graw [B][h][w][16], out, gy [B][2h][2w][16], float32 channels-last, 16-byte aligned; bias, gbias [16]; weight and gweight
 * [16][16][3][3], element (co, ci, ky, kx) at [co * s_o + ci * s_c + ky * s_y + kx * s_x], each with its own strides.  Every output
 * phase (2Y+py, 2X+px) is a 2x2 convolution of the low-resolution map with pre-summed taps and a clamped index: neither the padded
 * x2 copy nor its gradient exists.  Forward one launch; backward three (data gradient with d(bias) partials, weight-gradient
 * partials, one finishing pass in a fixed order), no atomics: the same inputs give the same bits at every call; no host
 * synchronisation (capturable).  The workspace (mdx_up_conv3x3_workspace_bytes; 0 for sizes the calls refuse; 16-byte aligned) may
 * hold anything on entry.  Refusals, before anything is launched: MDX_ERR_NULL_POINTER; MDX_ERR_BAD_SHAPE (B or h < 1, w not a
 * positive multiple of 4, B*h*w >= 2^34); MDX_ERR_WORKSPACE; MDX_ERR_MISALIGNED. */
size_t mdx_up_conv3x3_workspace_bytes(int B, int h, int w);
int mdx_up_conv3x3_fwd(const float *raw, const float *bias, const float *weight, int64_t s_o, int64_t s_c, int64_t s_y, int64_t s_x,
                       float *out, int B, int h, int w, void *stream);
int mdx_up_conv3x3_bwd(const float *gy, const float *raw, const float *bias, const float *weight, int64_t s_o, int64_t s_c,
                       int64_t s_y, int64_t s_x, float *graw, float *gbias, float *gweight, int64_t g_o, int64_t g_c, int64_t g_y,
                       int64_t g_x, int B, int h, int w, void *workspace, size_t workspace_bytes, void *stream);

/* The decoder's disparity heads   model_layer/depth_decoder.py:73-74,108-110: sigmoid(Conv3x3(C -> 1)(x)) on a channels-last map.
 * x [B][h+2][w+2][C] = the reflection-padded input (mdx_decoder_glue_nhwc_fwd's output), dtype 0 float32 / 1 bfloat16, C a
 * power of two from 4 to 256; weight: float32, element (c, ky, kx) at
 * weight[c * w_stride_c + ky * w_stride_ky + kx * w_stride_kx] (planar [1,C,3,3]: 9, 3, 1; channels-last: 1, 3C, C);
 * bias [1] (may be NULL) -> disp [B][h][w] float32.  One launch.
 * bwd: gdisp, disp [B][h][w] -> gx (x's dtype and shape), gweight (the weight's strides), gbias [1] (may be NULL): one launch
 * that reads x once and writes gx once + a finishing pass over the block partials (fixed order, no atomics). */
size_t mdx_disp_head_nhwc_workspace_bytes(int B, int C, int h, int w, int dtype);
int mdx_disp_head_nhwc_fwd(const void *x, const float *weight, int64_t w_stride_c, int64_t w_stride_ky, int64_t w_stride_kx,
                           const float *bias, float *disp, int B, int C, int h, int w, int dtype, void *stream);
int mdx_disp_head_nhwc_bwd(const void *x, const float *weight, int64_t w_stride_c, int64_t w_stride_ky, int64_t w_stride_kx,
                           const float *gdisp, const float *disp, void *gx, float *gweight, float *gbias, int B, int C, int h,
                           int w, int dtype, void *workspace, size_t workspace_bytes, void *stream);
/* mdx_decoder_glue_nhwc_*: model_layer/depth_decoder.py:44-47,96-106.  raw [B][h][w][C1], skip [B][u*h][u*w][C2],
 * out / gout [B][u*h+2][u*w+2][C1+C2]; dtype pairs as mdx_decoder_glue_fwd. */
int mdx_decoder_glue_nhwc_fwd(const void *raw, const void *skip, const float *bias, void *out, int B, int C1, int C2,
                              int h, int w, int upsample, int elu, int in_dtype, int out_dtype, void *stream);
size_t mdx_decoder_glue_nhwc_workspace_bytes(int B, int C1, int h, int w, int in_dtype);
int mdx_decoder_glue_nhwc_bwd(const void *gout, const void *raw, const float *bias, void *graw, void *gskip,
                              float *dbias, int B, int C1, int C2, int h, int w, int upsample, int elu, int in_dtype,
                              int out_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* mdx_maxpool3s2_nhwc_*: the ResNet stem's MaxPool2d(3, 2, 1).  in / gin [B][H][W][C]; out, arg, gout [B][Ho][Wo][C];
 * gout2 (may be NULL): a second upstream gradient, added on the way in. */
int mdx_maxpool3s2_nhwc_fwd(const void *in, void *out, uint8_t *arg, int B, int C, int H, int W, int dtype,
                            void *stream);
int mdx_maxpool3s2_nhwc_bwd(const void *gout, const void *gout2, const uint8_t *arg, void *gin, int B, int C, int H,
                            int W, int dtype, void *stream);

/* Train-time depth monitor   replaces model_loss/model_metric.py:70-105 (called every step, model_train.py:69).
 * pred [B,1,h,w] (outputs[("depth",0,0)]), gt [B,1,gh,gw] (0 = no return); window rows r0:r1, cols c0:c1 (the Garg crop).
 * out [8] = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, number of valid pixels.  Bilinear resize to the ground truth's
 * size, clamp, batch-level median scaling (torch.median's lower median, exact), clamp, compute_depth_error -- the masked
 * pixels are compacted on the device and three radix-selection passes (11 / 11 / 10 bits) find the medians; nothing is
 * sorted and nothing leaves the device.  A NaN prediction at a valid window pixel makes all seven numbers NaN (as
 * torch.clamp and torch.median do); out[7] is still the number of valid pixels. */
size_t mdx_depth_monitor_workspace_bytes(int B, int r0, int r1, int c0, int c1);
int mdx_depth_monitor(const float *pred, int B, int h, int w, const float *gt, int gh, int gw, int r0, int r1, int c0,
                      int c1, float min_depth, float max_depth, float *out, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ---- image preparation on the GPU   replaces, per sample and frame, the Pillow / torchvision calls of
 * model_loader/kitti_mono.py:288-291 + 349-353 (transforms.Resize((H>>s, W>>s), Image.ANTIALIAS) of the original image
 * for every scale, ColorJitter, ToTensor) and kitti_mono.py:302-303 (FLIP_LEFT_RIGHT); same in kitti_stereo.py.
 * Bit-exact with Pillow (Resample.c, Blend.c, Convert.c, ImageEnhance.py) -- uint8 results, float32 = u8 / 255.
 * Jobs are HOST arrays of plain structs whose pointers are DEVICE pointers (except where noted); they are passed to the
 * kernels by value (resampling: packed, MDX_IMG_JOBS jobs sharing at most 16 plans per axis per launch; jitter:
 * MDX_JITTER_JOBS per launch), so the caller may free or reuse the array on return.  A call may hold any number of jobs. */
#define MDX_IMG_JOBS 72
#define MDX_JITTER_JOBS 56
#define MDX_JITTER_PARTIALS 128

/* taps per output sample of the Lanczos-3 plan in_size -> out_size (2*ceil(3*max(in/out,1)) + 1) */
int mdx_resample_ksize(int in_size, int out_size);
/* Resample.c precompute_coeffs + normalize_coeffs_8bpc: bounds [out_size][2] = (first source sample, number of taps),
 * kk [ksize][out_size] = 22-bit fixed-point weights, TAP-MAJOR (the transpose of Pillow's table, so that consecutive
 * outputs read consecutive weights).  HOST arrays (the caller uploads and caches them per size pair). */
int mdx_resample_plan(int in_size, int out_size, int *bounds, int *kk);
/* The same weights COLUMN-MAJOR for the rows form of the horizontal pass (round 4), which fetches a column's taps with scalar
 * loads and evaluates two neighbouring columns over the union of their windows: table [2][out_size][row] ints -- direction 0:
 * table[0][x][lead + t] = weight t of output x; direction 1 (flipped images): the weights of x in reverse order,
 * table[1][x][lead + t] = weight (n_x - 1 - t); everything else 0.  lead >= the largest offset between the windows of two
 * neighbouring outputs (either direction); row = lead + ksize + lead rounded up to 16, + 16: every 16-entry read of a pair's
 * union stays inside a row.  Call with table == NULL for the sizes (*lead, *row); HOST arrays, uploaded and cached by the
 * caller like the plan itself. */
int mdx_resample_plan_cols(int in_size, int out_size, int *lead, int *row, int *table);

typedef struct mdx_resample_job {
    const uint8_t *src;          /* interleaved RGB, rows of in_stride bytes (>= 3*in_w): the decoder's layout */
    const int *xbounds, *xkk;    /* plan in_w -> out_w (device copies) */
    const int *ybounds, *ykk;    /* plan in_h -> out_h */
    uint8_t *inter;              /* scratch, planar [3][in_h][out_w] */
    uint8_t *dst_u8;             /* planar [3][out_h][out_w], or NULL */
    float *dst_f32;              /* planar [3][out_h][out_w] = u8 / 255 (ToTensor), or NULL */
    int in_h, in_w, in_stride, flip;   /* flip: resize image.transpose(FLIP_LEFT_RIGHT) */
    int out_h, out_w, xksize, yksize;
    const int *xkc;              /* mdx_resample_plan_cols table of in_w -> out_w (device copy) or NULL: without it the */
    int xkc_lead, xkc_row;       /* horizontal pass runs in its general gather form (slower, same bytes)              */
} mdx_resample_job;
/* Image.resize((out_w, out_h), Image.LANCZOS): horizontal pass to uint8, then vertical pass. */
int mdx_resample_lanczos_u8(const mdx_resample_job *jobs, int njobs, void *stream);

typedef struct mdx_jitter_job {
    const uint8_t *src;          /* planar [3][h][w] */
    float *dst_f32;              /* planar [3][h][w] = u8 / 255, or NULL */
    uint8_t *dst_u8;             /* planar, or NULL (may alias src: each pixel is read before it is written) */
    unsigned long long *lsum;    /* scratch, MDX_JITTER_PARTIALS 8-byte words per job (partial sums of L for Contrast) */
    int h, w;
    int order[4];                /* 0 brightness, 1 contrast, 2 saturation, 3 hue, 4 = empty slot; each at most once */
    int hue_shift;               /* int(hue_factor * 255), added to the H byte modulo 256 */
    float brightness, contrast, saturation;   /* ImageEnhance factors */
} mdx_jitter_job;
/* torchvision ColorJitter on PIL images: the adjustments in `order`, uint8 after each. */
int mdx_color_jitter_u8(const mdx_jitter_job *jobs, int njobs, void *stream);

/* Unfused parity op: Pillow's convert() maps on planar uint8 [3][npix]: mode 0 RGB->HSV, 1 HSV->RGB, 2 RGB->L ([npix] out). */
int mdx_color_convert_u8(int mode, const uint8_t *src, uint8_t *dst, size_t npix, void *stream);

/* torchvision ToTensor on a uint8 image (kitti_mono.py:283,351; kitti_stereo.py:280-281): dst[i] = float32(src[i]) / 255
 * with the IEEE divide (NOT a multiplication by 1/255: that differs in the last bit for 126 of the 256 byte values).
 * src: n bytes, any layout; dst: n floats, 16-byte aligned. */
int mdx_to_tensor_u8(const uint8_t *src, float *dst, size_t n, void *stream);

/* ---- velodyne ground truth on the GPU   model_utility.point2depth (reference model_utility.py:128-197) -> resize_nearest
 * -> np.fliplr -> float32, for a ragged batch of scans; bit-equal to that host chain wherever no projected coordinate sits on
 * a rounding boundary (a half-integer u or v).  Per job, in file order i = 0..n-1:
 *   points with !(x >= 0) are dropped; (X, Y, Z) = P . (x, y, z, 1) in float64 (products summed left to right, no fma),
 *   c = rint(X/Z) - 1, r = rint(Y/Z) - 1, kept iff 0 <= c < w && 0 <= r < h as doubles (NaN and infinities fail);
 *   depth d = vel_depth ? x : Z, negative -> 0, cast to float32;
 *   pixel (r, c) takes the d of its kept point with the largest i; then, the reference's rule with its index arithmetic: for
 *   every g = r*(w-1) + c shared by >= 2 kept points, the pixel of the member with the smallest i receives the smallest d of the
 *   group ((r, 0) and (r-1, w-1) share a g);
 *   out[R][C] = map[ys[R]][xs[flip ? gw-1-C : C]], ys / xs = clip(rint((k + 0.5) * n_in / n_out - 0.5), 0, n_in - 1) in float64.
 * Three launches per MDX_VELO_JOBS jobs (project + clear the touched scratch cells; integer atomicMax / atomicAdd votes; one
 * thread per output pixel gathers): no float atomics, nothing depends on arrival order, the same bits at every call.  The
 * workspace needs NO clearing and may hold anything: a cell is believed only if the point it names lies on it.
 * Jobs are a HOST array (passed to the kernels by value); points / out are DEVICE pointers; no host synchronisation. */
#define MDX_VELO_JOBS 16
typedef struct mdx_velodyne_job {
    const float *points;         /* n rows of `stride` floats (x, y, z[, reflectance: never read]); may be NULL when n == 0 */
    float *out;                  /* [gh][gw], every element written (0 = no return) */
    double P[12];                /* 3x4 row-major: P_rect @ R_cam2rect @ velo2cam, formed on the host in float64 */
    int n, stride;               /* stride: 3 or 4 */
    int h, w;                    /* native image size, w >= 2 */
    int gh, gw;                  /* output size */
    int vel_depth, flip;
} mdx_velodyne_job;
/* bytes that `count` jobs of at most nmax points on native grids of at most hmax x wmax need (8 per point, 16 per pixel, each
 * job's share rounded up to 16); 0 for an argument outside the ranges mdx_velodyne_depth accepts */
size_t mdx_velodyne_workspace_bytes(int count, int nmax, int hmax, int wmax);
/* MDX_ERR_NULL_POINTER: jobs, an out, or points with n > 0 is NULL.  MDX_ERR_BAD_SHAPE: count < 0, n < 0, h < 1, w < 2, gh or
 * gw < 1, h*w or gh*gw beyond int32.  MDX_ERR_UNSUPPORTED: a stride other than 3 or 4.  MDX_ERR_WORKSPACE: workspace NULL or
 * smaller than the jobs need (the sum of their own shares).  MDX_ERR_MISALIGNED: workspace not 16-byte aligned.  All of them
 * before anything is launched.  count == 0 launches nothing. */
int mdx_velodyne_depth(const mdx_velodyne_job *jobs, int count, void *workspace, size_t workspace_bytes, void *stream);

/* ---- sparse lidar supervision: a depth term beside the fused loss (csrc/sparse_depth.hip; mdx.functional.sparse_depth_loss).
 * disp[k]: float32 contiguous [B,1,h[k],w[k]], k < nscales (1..MDX_MAX_SCALES); gt: float32 contiguous [B,1,gh,gw], 0 = no return;
 * gh >= h[k] and gw >= w[k].  A ground-truth pixel is VALID when gt > lo && gt < hi (strict: NaN, infinities and the bounds
 * themselves are invalid); n = the valid pixels of the batch.  Per valid pixel (b,Y,X) and scale:
 *   u = the bilinear sample of disp[k] at (Y,X) on the gh x gw grid, align_corners=False (the element itself when the sizes are equal),
 *   sd = a + b*u with a = 1/max_depth, b = 1/min_depth - 1/max_depth as mdx_disparity2depth_fwd forms them,
 *   r = -log(sd) - log(gt),  rho = sqrt(r^2 + eps^2) - eps.
 * out[k] = L_k = (sum of rho over the valid pixels, in double, in a fixed order) / max(n, 1); out[nscales] = n (float32: exact up to
 * 2^24).  n == 0: every L_k is 0.  An sd that is not a positive finite number under a valid pixel makes L_k NaN; a non-finite
 * disparity that only invalid pixels touch changes nothing.
 * mdx_sparse_depth_bwd: ddisp[k][b,i,j] = gout[k] / max(n,1) * sum over the valid pixels of (r / sqrt(r^2+eps^2)) * (-b / sd) *
 * wy(Y,i) * wx(X,j) -- a per-destination sum in a fixed order, every element written (0 where nothing reaches it); `out` is the
 * forward's (read for n), gout a DEVICE array of nscales floats.
 * h, w, disp, ddisp are HOST arrays; gt, out, gout, workspace and what disp / ddisp point to are DEVICE memory.  The forward is two
 * launches, the backward one per scale; no floating-point atomics, nothing to clear between calls, the same inputs give the same
 * bits at every call; no host synchronisation (capturable).  The workspace (mdx_sparse_depth_workspace_bytes; 0 for sizes the calls
 * refuse; 8-byte aligned; contents need not survive between the two calls) is asked for and checked by both, but only the forward
 * uses it: the backward as it is built (a recomputing gather) neither reads nor writes it, so the forward's buffer can be handed
 * over again; the argument is there for a form that stores per-pixel coefficients first.
 * Refusals, all before anything is launched, in this order: MDX_ERR_NULL_POINTER (h, w, disp, an entry of it, gt, out; bwd: gout,
 * ddisp, an entry of it); MDX_ERR_BAD_SHAPE (nscales out of range, a size < 1, gh < h[k] or gw < w[k], B*gh*gw >= 2^32,
 * min_depth <= 0, max_depth <= min_depth, !(lo < hi), eps not finite or <= 0); MDX_ERR_WORKSPACE (NULL or too small);
 * MDX_ERR_MISALIGNED (a float pointer not 4-byte, the workspace not 8-byte aligned). */
size_t mdx_sparse_depth_workspace_bytes(int nscales, int B, int gh, int gw);
int mdx_sparse_depth_fwd(int nscales, int B, const int *h, const int *w, const float *const *disp, const float *gt, int gh, int gw,
                         double min_depth, double max_depth, float lo, float hi, double eps, float *out, void *workspace,
                         size_t workspace_bytes, void *stream);
int mdx_sparse_depth_bwd(int nscales, int B, const int *h, const int *w, const float *const *disp, const float *gt, int gh, int gw,
                         double min_depth, double max_depth, float lo, float hi, double eps, const float *out, const float *gout,
                         float *const *ddisp, void *workspace, size_t workspace_bytes, void *stream);

/* ---- stereo proxy depth: a semi-global matcher over a rectified pair (csrc/stereo_hints.hip; mdx.functional.stereo_hints).
 * target, partner: float32 contiguous [B,3,H,W]; K, T: float32 [B,4,4] (scale-0 intrinsics; the target -> partner transform, the
 * loaders' inputs["stereo"]), read on the device; D = 64 or 128 disparities; integers 0 < P1 < P2 <= 190.  Per sample b:
 *  1. dir = +1 if T[b,0,3] > 0, -1 if < 0: the match of target (y,x) at disparity d is partner (y, x + dir*d).  T[b,0,3] zero or not
 *     finite: the sample's S, disp, depth and valid are all 0.
 *  2. luma  L = (0.299f*R + 0.587f*G) + 0.114f*B in float32, each operation rounded on its own.
 *  3. census over 9 wide x 7 high: 62 bits, bit = L(neighbour) < L(centre), neighbour coordinates clamped to the image.
 *  4. cost  C(y,x,d) = popcount(ct(y,x) ^ cs(y,x+dir*d)) if 0 <= x+dir*d < W, else 31.
 *  5. paths r in {(0,+-1), (+-1,0), (+-1,+-1)} as (row, column) steps: L_r(p,d) = C(p,d) where p-r lies outside the image, else
 *     C(p,d) + min(L_r(p-r,d), L_r(p-r,d-1)+P1, L_r(p-r,d+1)+P1, m+P2) - m with m = min_k L_r(p-r,k); the d-1 / d+1 terms are
 *     absent at d = 0 / d = D-1.  S = sum_r L_r (L_r <= 62+P2 <= 252, S <= 2016: 16 bits).
 *  6. d0(p) = argmin_d S(p,d), the smallest d on ties.
 *  7. dR(y,xr) = argmin_d S(y, xr - dir*d, d) over the d whose column lies inside the image, the smallest d on ties.
 *  8. valid: d0 >= 1 and 0 <= x+dir*d0 < W and |dR(y, x+dir*d0) - d0| <= 1.
 *  9. in float32: a = S(p,d0-1), m = S(p,d0), c = S(p,d0+1), den = (a + c) - 2*m; if 0 < d0 < D-1 and den > 0:
 *     dsub = d0 + (a - c) / (2*den), else dsub = d0.
 * 10. disp[b,0,y,x] = dsub where valid, else 0; depth = (K[b,0,0] * |T[b,0,3]|) / dsub where valid (the product first, the quotient
 *     correctly rounded), else 0; valid[b,0,y,x] = 1 / 0 (uint8).  Every element of the three outputs is written.
 * Workspace (mdx_stereo_hints_workspace_bytes; 0 for sizes the call refuses; 8-byte aligned): S lies at offset 0 as uint16
 * [B][H][W][D]; behind it, each rounded up to 8 bytes, the two census maps (uint64 [B][H][W], target then partner), the two luma maps
 * (float32 [B][H][W]), d0 and dR (uint8 [B][H][W]).  It may hold anything on entry: the first path pass writes S, the other seven
 * add to it, each element with one writer per launch.  12 launches (luma, census, 8 paths, the two winners, outputs), no
 * atomics, no host synchronisation (capturable); the same inputs give the same bits at every call.
 * Refusals, all before anything is launched, in this order: MDX_ERR_NULL_POINTER (target, partner, K, T, disp, depth, valid);
 * MDX_ERR_BAD_SHAPE (B, H or W < 1, H or W > 32767, D not 64 / 128, B*H*W*D >= 2^31, !(0 < P1 < P2 <= 190)); MDX_ERR_WORKSPACE
 * (NULL or too small); MDX_ERR_MISALIGNED (a float pointer not 4-byte, the workspace not 8-byte aligned). */
size_t mdx_stereo_hints_workspace_bytes(int B, int H, int W, int D);
int mdx_stereo_hints(const float *target, const float *partner, const float *K, const float *T, int B, int H, int W, int D, int P1,
                     int P2, float *disp, float *depth, unsigned char *valid, void *workspace, size_t workspace_bytes, void *stream);

/* ---- depth-hint selection: a proxy depth supervises a pixel only where it reprojects better than the network's own depth
 * (Watson et al. 2019; csrc/hint_select.hip; mdx.functional.hint_select, mdx.composite.hint_select).
 * target, partner: float32 contiguous [B,3,H,W]; K, invK, T: float32 [B,4,4] (scale-0 intrinsics, their inverse, the target ->
 * partner transform), read on the device; hint: float32 [B,1,H,W], 0 = no hint; disp: float32 [B,1,h,w], the step's finest
 * disparity, h <= H, w <= W.  Per pixel (b,y,x):
 *  1. u = the bilinear sample of disp at (y,x) on the H x W grid, align_corners=False (the element itself when the sizes are equal);
 *     d_pred = 1 / (a + b*u) with a = 1/max_depth, b = 1/min_depth - 1/max_depth as mdx_disparity2depth_fwd forms them.
 *  2. ray = invK[b,:3,:3] . (x, y, 1); P = (K[b] @ T[b])[:3] as mdx_compose_projection forms it.
 *  3. for d in (hint, d_pred): the point (d*ray, 1) through mdx_project_fwd's arithmetic (eps 1e-7) to a sampling position, the
 *     three partner planes sampled there as mdx_grid_sample_border_fwd samples them (bilinear, border, align_corners=True).  This
 *     is done over the whole map as given: a 0 (or any other value) in hint is warped like a depth.
 *  4. l_hint, l_pred = mdx_reprojection_loss_fwd of the two warped images against target: 0.85 * the channel mean of the clamped
 *     SSIM map (3 x 3 windows, reflect padding: a window position outside the image is the reflected position inside it, warped
 *     there) + 0.15 * the channel mean of |target - warped|.
 *  5. keep = hint > 0 && l_hint < l_pred.  Strict: a tie keeps nothing; a comparison with a NaN is false.
 *  6. sel[b,0,y,x] = keep ? hint : 0 (the hint's own bits); l_hint / l_pred [B,1,H,W] are written when the pointers are not NULL.
 *  7. counts[b] = (the pixels with hint > 0, the pixels kept) as int32 [B][2].
 * Every float is formed in the order of the calls named above, so l_hint and l_pred equal their chain bit for bit.  Where a
 * non-finite value of hint or of the upsampled disparity lies inside a pixel's 3 x 3 window that pixel's keep is unspecified (sel is
 * still 0 or the hint); every pixel farther away is unaffected.  No index is formed from an unclamped float: sampling positions are
 * clamped to the image (a NaN to 0) before they are converted.
 * Two launches (one 64 x 8 tile per block with its halo in LDS; one block per sample adds the tiles' integer counts), no atomics,
 * every output element written by one plain store, no host synchronisation (capturable); the same inputs give the same bits at
 * every call.  Workspace (mdx_hint_select_workspace_bytes; 0 for sizes the call refuses; 8-byte aligned): one int32 pair per tile;
 * it may hold anything on entry.
 * Refusals, all before anything is launched, in this order: MDX_ERR_NULL_POINTER (target, partner, K, invK, T, hint, disp, sel,
 * counts); MDX_ERR_BAD_SHAPE (B, h or w < 1, H or W < 2, h > H, w > W, H*W >= 2^30, B*H*W >= 2^31, B or ceil(H/8) > 65535,
 * min_depth <= 0, max_depth <= min_depth); MDX_ERR_WORKSPACE (NULL or too small); MDX_ERR_MISALIGNED (a float or count pointer not
 * 4-byte, the workspace not 8-byte, target not 16-byte aligned: its planes are read with 16-byte loads, and H*W*4 is a multiple of 16
 * wherever those loads are taken, W % 4 == 0). */
size_t mdx_hint_select_workspace_bytes(int B, int H, int W, int h, int w);
int mdx_hint_select(const float *target, const float *partner, const float *K, const float *invK, const float *T, const float *hint,
                    const float *disp, int B, int H, int W, int h, int w, double min_depth, double max_depth, float *sel,
                    float *l_hint, float *l_pred, int *counts, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MDX_H */
