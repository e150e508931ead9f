/* libr2dm_hip.so -- C ABI of the MI355X (gfx950) R2DM sampling engine.
 *
 * The reference (kazuto1011/r2dm) has no native code and no FFI; its only seam on the sampling path
 * is the Python call  prediction = self.model(x_t, cond)  plus the elementwise posterior update
 * around it.  This header is that seam expressed as a C ABI: what a ctypes / cffi / pybind stub in
 * the reference would bind to run the per-step hot path on hand-written HIP kernels.
 * Every entry point names the reference code it replaces (paths relative to the reference repo).
 *
 * Conventions
 *   - all tensors are fp32, NCHW, contiguous, in DEVICE memory owned by the caller (PyTorch);
 *   - the library never allocates device memory, never synchronises and enqueues everything on the
 *     `stream` it is given (a hipStream_t passed as void*; NULL = default stream);
 *   - a handle is bound to the current device of the creating thread and used from one host thread;
 *   - every function returns 0 on success and a non-zero code on failure; r2dm_last_error() then
 *     returns a thread-local human-readable message.
 */
#ifndef R2DM_HIP_H
#define R2DM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct r2dm_handle r2dm_handle;

/* Geometry of one EfficientUNet instance: the constructor arguments of
 * models/efficient_unet.py:194-211 that shape tensors (ring=True, dropout=0 always). */
typedef struct r2dm_config {
    int32_t in_channels;            /* 2: range + reflectance */
    int32_t out_channels;
    int32_t height, width;          /* resolution, e.g. 64 x 1024 */
    int32_t base_channels;          /* 64 */
    int32_t temb_channels;          /* 4 * base */
    int32_t channel_multiplier[4];  /* (1,2,4,8) */
    int32_t num_residual_blocks[4]; /* (3,3,3,3) */
    int32_t gn_num_groups;          /* 8 */
    float gn_eps;                   /* 1e-6 */
    int32_t attn_num_heads;         /* 8 */
    int32_t coord_channels;         /* channels of the constant coordinate encoding (32 @64x1024; 0 = none) */
    int32_t max_batch;              /* layer tilings are chosen for batches up to this size */
} r2dm_config;

/* One state-dict tensor the engine consumes, in the reference's naming (SURVEY.md appendix A.3,
 * without the "model." prefix), plus two host-precomputed constants:
 *   "__cenc"      (coord_channels, H, W)  FourierFeatures(coords)        models/encoding.py:141-146
 *   "__sin_freqs" (base_channels/2,)      sinusoid frequency table       models/ops.py:22-23          */
typedef struct r2dm_tensor_info {
    const char* key;
    int64_t numel; /* number of fp32 elements the caller must supply */
} r2dm_tensor_info;

const char* r2dm_last_error(void);
const char* r2dm_version(void);

/* -- lifetime ------------------------------------------------------------------------------- */
int r2dm_create(r2dm_handle** out, const r2dm_config* cfg);
void r2dm_destroy(r2dm_handle* h);

/* -- weights: replaces nn.Module.load_state_dict + .to(device) for the denoiser
 *    (utils/inference.py:80-83).  The caller allocates r2dm_blob_bytes() of device memory, binds it,
 *    then feeds every tensor listed by r2dm_tensor_at(); the engine repacks each into its
 *    kernel-friendly layout inside the blob (HIP kernels, asynchronous).  A blob filled on one GPU
 *    can be broadcast (RCCL) and bound on another GPU with an identical config: no per-rank load. */
int64_t r2dm_num_tensors(const r2dm_handle* h);
int r2dm_tensor_at(const r2dm_handle* h, int64_t index, r2dm_tensor_info* out);
size_t r2dm_blob_bytes(const r2dm_handle* h);
/* The blob's parts that are STATE, not weights (byte offset and size; a checksum of "the weights" leaves them out -- distributed.py):
 * the range-guard slots -- int32[2 * 256]: [0] the packers' "weight not finite" flag, which travels with the blob; [2 k + 1] site k's bound as
 * float bits, a running maximum raised by every forward: whoever adopts a blob clears [1 ..] on its own stream -- and the constant
 * coordinate map of in_conv (0 bytes without a coordinate encoding), which the first forward after a bind computes from the weights. */
int r2dm_blob_flag_region(const r2dm_handle* h, size_t* offset, size_t* bytes);
int r2dm_blob_cmap_region(const r2dm_handle* h, size_t* offset, size_t* bytes);

/* Fingerprint of the blob's LAYOUT as this handle planned it: every slot's key, offset and packing (algorithm, channel / pixel tile of
 * each convolution's packings -- they depend on max_batch, the device's CU count and experiment switches, not only on the
 * configuration) and the blob size.  A blob filled through one handle may be bound by another only if the two agree (the Python
 * wrapper compares them before it adopts a broadcast blob: a mismatch would run silently wrong convolutions -- ADVICE round 4). */
uint64_t r2dm_blob_layout_hash(const r2dm_handle* h);
int r2dm_bind_blob(r2dm_handle* h, void* dev_blob, size_t bytes);
int r2dm_load_tensor(r2dm_handle* h, int64_t index, const float* dev_src, int64_t numel, void* stream);

/* -- the denoiser: replaces EfficientUNet.forward (models/efficient_unet.py:269-295), called from
 *    p_step at models/diffusion/continuous_time.py:207 and discrete_time.py:139.
 *    x (B,in_channels,H,W), cond (B,) as float, out (B,out_channels,H,W). */
size_t r2dm_workspace_bytes(const r2dm_handle* h, int32_t batch);
int r2dm_unet_forward(r2dm_handle* h, const float* x, const float* cond, float* out, int32_t batch,
                      void* workspace, size_t workspace_bytes, void* stream);
/* What a forward at this batch in the handle's precision mode enqueues, from the sizing walk (host only: no GPU, no weights, the handle unchanged): one
 * text line per launch in enqueue order -- "layer | launch | out=<workspace offset, or dst> [| a convolution's kernel, tile, shape and fusions]
 * [| range sites it hands out, profiling class]".  Writes at most cap - 1 characters and a NUL to buf (may be NULL); *need = the size that holds all of it.
 * The dispatch tests compare it with tests/golden/forward_listing.json. */
int r2dm_forward_listing(const r2dm_handle* h, int32_t batch, char* buf, size_t cap, size_t* need);

/* -- the feature cache (DeepCache, Ma et al., CVPR 2024): between adjacent sampler steps the deep part of the U-Net changes slowly, so a "shallow" forward
 *    runs only the outermost `depth` levels and reads everything below them from what the last full forward left at the topmost skipped join.
 *    depth d in {1, 2, 3}: live are in_conv, stages [0, d) and [8 - d, 8), out_conv, the time embedding and ada_proj.  The cache, a caller-owned buffer of
 *    r2dm_cache_bytes(h, B, d) bytes (256-byte aligned), holds [output of stage 7 - d, as the walk stores it: fp32, or fp16 in the one-plane mode
 *    | the GroupNorm statistics slots of that join, where the walk fuses them | scratch of the drift reduction].  The library keeps no cache state: which
 *    forward filled the buffer, at which batch and in which precision mode, is the caller's to know (unet.py FeatureCache).
 *      mode 1 (store): the full forward -- the launches of r2dm_unet_forward in the same order, bit-identical `out` -- whose stage 7 - d writes its output
 *                      into the cache.  drift != NULL (device, 2 B doubles): the stage writes to the workspace as ever and r2dm_cache_store moves it into the
 *                      cache, leaving per sample {sum (fresh - old)^2, sum old^2} in drift -- one more pass over the tensor per full step.
 *      mode 2 (reuse): only the live stages run; stage 8 - d reads cat([cache, skip tensor]) and the join's statistics with the cached half in them.
 *    Non-zero (r2dm_last_error): depth outside 1..3, mode other than 1 / 2, cache too small or misaligned, batch > max_batch, and what r2dm_unet_forward refuses.
 *    workspace: as for r2dm_unet_forward (r2dm_workspace_bytes).  r2dm_forward_listing_cached: that walk's listing (host only; the cached tensor's line reads
 *    out=cache; range sites carry the numbers of the full walk). */
size_t r2dm_cache_bytes(const r2dm_handle* h, int32_t batch, int32_t depth);
int r2dm_unet_forward_cached(r2dm_handle* h, const float* x, const float* cond, float* out, int32_t batch, void* workspace, size_t workspace_bytes,
                             void* stream, void* cache, size_t cache_bytes, int32_t depth, int32_t mode, double* drift);
int r2dm_forward_listing_cached(const r2dm_handle* h, int32_t batch, int32_t depth, int32_t mode, char* buf, size_t cap, size_t* need);
/* cached <- fresh, bit for bit, (B, n_per_sample) values of fp32 (f16 = 0) or fp16 (f16 = 1), read once together with the values they replace:
 * sums[b] = {sum (fresh - old)^2, sum old^2}, differences and squares in float64 from the stored values.  partial: scratch of 2 * 512 * B doubles (per-block
 * sums; a second launch adds them in a fixed order: no atomics, the same bits from call to call).  Both tensors 16-byte aligned; any n_per_sample >= 1. */
int r2dm_cache_store(const void* fresh, void* cached_inout, int32_t batch, int64_t n_per_sample, int32_t f16, double* partial, double* sums, void* stream);

/* -- arithmetic of the convolutions / attention core on the 16-bit matrix pipe (tensors and accumulation are fp32 in every mode):
 *      pieces = 2 (default, parity mode): every fp32 operand v is split to 22 bits, v = h + 2^-11 l with h = RNE_f16(v),
 *                 l = RNE_f16(2^11 (v - h)); a product is xh wh + 2^-11 (xh wl + xl wh) -- 3 MFMA products, the l x l term
 *                 (2^-22 relative) dropped, two fp32 accumulators: conv_f16x2.hip (3x3), proj_f16x2.hip (1x1), attention.hip.
 *                 fp32-class BY MEASUREMENT (error vs fp64 at or below an fp32 FMA chain's), not bit-exact fp32 operands.
 *                 Operands pass through fp16 (|v| < 65504): weights are pre-scaled per layer by a power of two (max|w| into
 *                 [2^9, 2^10); undone exactly in the epilogue); a GroupNorm-normalised operand is bounded from the DATA
 *                 (|a| M + |d| with M >= max|x|: the square root of the largest statistics-slot energy, or the maximum the
 *                 streaming statistics kernel recorded); a raw operand's producer records max|output| (conv epilogues, fir_up2);
 *      pieces = 3 (parity mode, fp32 operand range): three bf16 pieces = exact 24-bit operands, 6 products (conv_bf16x3.hip)
 *                 for the 3x3 convolutions, the fp32-input MFMA for the 1x1 convolutions and the attention core;
 *      pieces = 1 (REDUCED precision, bulk sampling -- the reference's fp16 autocast mode, sample_and_save.py:70,
 *                 utils/option.py:49): the kernels of pieces = 2 with the h piece alone: one fp16 product per MAC.
 *    With pieces = 1 / 2 r2dm_check_range reports a violation of the fp16 operand range.
 *    h == NULL sets the mode of the single-kernel entries r2dm_conv2d_ring / r2dm_attention. */
int r2dm_set_conv_pieces(r2dm_handle* h, int32_t pieces);

/* Waits for `stream` and returns non-zero (r2dm_last_error explains) if, since the last call, a forward of `h` ran an
 * f16x2 convolution on operands that may have left the fp16 range -- its output is then not valid.  The Python wrapper
 * calls this after every stand-alone forward and once at the end of a sampling loop.  The recorded bounds are running maxima: a clean check leaves
 * them (nothing can have tripped unnoticed), a reported trip resets them. */
int r2dm_check_range(r2dm_handle* h, void* stream);

/* Per-site view of the guard (round 6; python -m r2dm_amd.check): a SITE is one guarded producer of a forward in walk order -- a GroupNorm's
 * output bound, or the recorded max|output| of a tensor that the next fp16-operand kernel reads raw (conv_f16x2 records the root of the largest sum of squares of four
 * neighbouring pixels: an upper bound of max|output|, at most twice it).  r2dm_range_sites copies the bounds
 * the LAST r2dm_check_range read (up to `cap`; *n = number of sites of the last forward, site 0 = shared slot) -- call r2dm_check_range
 * first; r2dm_range_site_name labels site k ("d_block1.residual_blocks.0.conv1: GroupNorm output bound ..."; valid until the next forward).
 * A bound >= 65504 is a trip.  Replaces nothing upstream: the reference runs fp32 / autocast and has no operand range to guard. */
int r2dm_range_sites(r2dm_handle* h, float* bounds, int32_t cap, int32_t* n);
const char* r2dm_range_site_name(r2dm_handle* h, int32_t k);

/* Test hook: raises the recorded operand bound to at least `bound` on `stream`, as a convolution input of that size would have
 * (tests/test_hip_range.py simulates a guard trip at a chosen step of a sampling loop with it). */
int r2dm_test_raise_range_bound(r2dm_handle* h, float bound, void* stream);

/* -- measurement aid (bench.py): when enabled, every convolution launch of a forward -- conv_f16x2_kernel (54 3x3 launches in
 *    the default mode; conv_bf16x3_* with pieces = 3), proj_f16x2_kernel (8 1x1 launches; conv_mfma_kernel with pieces = 3) and
 *    the two direct kernels (in_conv, out_conv), 64 launches per forward -- is bracketed by hipEvents recorded on the caller's stream.  r2dm_profile_read waits for them and returns the summed kernel time, the summed
 *    ALGORITHMIC flops (2*B*Cout*Cin*k*k*H*W per launch) and the number of launches, then resets. */
int r2dm_profile_enable(r2dm_handle* h, int32_t on);
int r2dm_profile_read(r2dm_handle* h, double* conv_ms, double* conv_flop, int64_t* launches);
/* same, per kernel class: [0] conv_f16x2_kernel, [1] conv_bf16x3_*, [2] conv_mfma_kernel / conv_direct_kernel */
int r2dm_profile_read_classes(r2dm_handle* h, double* ms3, double* flop3, int64_t* launches3);
/* what a bracketing event pair adds to the kernel between its events, measured on `stream` (medians of 33): the pair around nothing (marker processing)
 * and around an empty kernel (marker processing + one dispatch + that kernel's own microsecond); bench.py prints both next to the per-launch figures,
 * which rocprofv3's kernel durations (profiles/) do not contain. */
int r2dm_profile_event_overhead(r2dm_handle* h, void* stream, double* empty_pair_us, double* empty_kernel_pair_us);

/* -- posterior update: replaces the elementwise tail of p_step
 *    (continuous_time.py:208-229, discrete_time.py:140-177).  coef is (B,8) host-computed scalars,
 *    see r2dm_amd/diffusion.py for the slot meaning per mode.
 *    mode: 0 continuous DDPM, 1 continuous DDIM, 2 discrete DDPM, 3 discrete DDIM (eta=0, noise may
 *    be NULL), 4 discrete DDIM with noise.  objective: 0 eps, 1 v, 2 x_0.  clip < 0 disables clamping. */
int r2dm_posterior_step(const float* x_t, const float* prediction, const float* noise, const float* coef,
                        float* x_s, int32_t batch, int64_t per_sample, int32_t mode, int32_t objective,
                        float clip, void* stream);

/* -- data-consistent posterior update: the step of r2dm_posterior_step with a measurement written over the x_0 estimate (the null-space
 *    projection of DDNM, Wang et al. 2023, for a mask operator).  One pass in float32, not contracted; per element, in this order:
 *      x0  = as r2dm_posterior_step (eps: (x - s_t*pr)/a_t | v: a_t*x - s_t*pr | x_0: pr), clamped to [-clip, clip] (clip < 0: no clamp)
 *      x0  = m*y + (1 - m)*x0          y = known, m = mask: a per-pixel weight, not necessarily 0 / 1
 *      x_s = mode 0 (continuous DDPM): a_s*(x*(1 - c)/a_t + c*x0) + sd*z | mode 1 (continuous DDIM): a_s*x0 + c1*z + c2*((x - a_t*x0)/s_t)
 *    coef is the (B,8) row of r2dm_posterior_step.  mask has `mask_channels` channels (1 = broadcast over the `channels` planes of a
 *    sample, as in r2dm_repaint_blend).  With an all-zero mask the result is r2dm_posterior_step's, bit for bit.
 *    Refused (status 1, "posterior_step_known: ..." in r2dm_last_error, nothing launched): a null pointer (noise included); a mode other
 *    than 0 / 1 (discrete time is not built) or an objective other than 0 / 1 / 2; a batch outside [1, 65535]; per_sample or the plane
 *    per_sample / channels not a multiple of 4; mask_channels not 1 or `channels`; x_t, prediction, noise, known, mask or x_s not 16-byte
 *    aligned (all are read and written as quads), coef not 4-byte aligned. */
int r2dm_posterior_step_known(const float* x_t, const float* prediction, const float* noise, const float* known, const float* mask,
                              const float* coef, float* x_s, int32_t batch, int64_t per_sample, int32_t channels, int32_t mask_channels,
                              int32_t mode, int32_t objective, float clip, void* stream);

/* -- DPM-Solver++(2M) update (Lu et al. 2022: the second-order multistep solver of the probability-flow ODE in data-prediction form, on the
 *    half-log-SNR axis; continuous time).  One pass in float32, not contracted; per element, in this order:
 *      x0  = as r2dm_posterior_step (eps: (x - s_t*pr)/a_t | v: a_t*x - s_t*pr | x_0: pr), clamped to [-clip, clip] (clip < 0: no clamp)
 *      x_s = c_x*x + c_0*x0                         x0_prev NULL: a first-order row; c_1 is not read
 *      x_s = (c_x*x + c_0*x0) + c_1*x0_prev         otherwise
 *    coef is (B,8) = (a_t, s_t, c_x, c_0, c_1, 0, 0, 0), host-computed scalars in device memory (r2dm_amd/diffusion.py: _dpm_table).
 *    Both x_s and x0 are written; x0, the clamped estimate, is the next step's x0_prev.  x0 may be x0_prev's buffer (every element is read
 *    before the same thread writes it); no other aliasing of an output with an input or with the other output is supported.
 *    Refused (status 1, "dpm_step: ..." in r2dm_last_error, nothing launched): a null pointer other than x0_prev; an objective other than
 *    0 / 1 / 2; a batch outside [1, 65535]; per_sample not a multiple of 4; x_t, prediction, x0_prev, x_s or x0 not 16-byte aligned (all are
 *    read and written as quads), coef not 4-byte aligned; x_s equal to x_t, prediction, x0_prev or x0, or x0 equal to x_t or prediction. */
int r2dm_dpm_step(const float* x_t, const float* prediction, const float* x0_prev, const float* coef, float* x_s, float* x0, int32_t batch,
                  int64_t per_sample, int32_t objective, float clip, void* stream);

/* -- DPM-Solver++(2M) update with a measurement and a noise operand: completion on the multistep solver (DDNM's projection of the x_0
 *    estimate) and its stochastic member (SDE-DPM-Solver++(2M) with the table of eta = 1).  One pass in float32, not contracted; per element:
 *      x0  = as r2dm_posterior_step (eps: (x - s_t*pr)/a_t | v: a_t*x - s_t*pr | x_0: pr), clamped to [-clip, clip] (clip < 0: no clamp)
 *      x0  = m*y + (1 - m)*x0                   only when known (y) and mask (m) are given: both NULL or both non-NULL
 *      x_s = c_x*x + c_0*x0
 *      x_s = x_s + c_1*x0_prev                  only when x0_prev != NULL
 *      x_s = x_s + c_z*z                        only when noise (z) != NULL
 *    coef is (B,8) = (a_t, s_t, c_x, c_0, c_1, c_z, 0, 0) (r2dm_amd/diffusion.py: _dpm_table with eta).  Both x_s and x0 are written; x0 is
 *    the estimate AFTER the measurement has been written in: the history the next step extrapolates from.  mask has `mask_channels`
 *    channels (1 = broadcast over the `channels` planes of a sample), as in r2dm_posterior_step_known.  x0 may be x0_prev's buffer, as in
 *    r2dm_dpm_step; no other aliasing is supported.  With noise, known and mask NULL the result is r2dm_dpm_step's, bit for bit.
 *    Refused (status 1, "dpm_step_known: ..." in r2dm_last_error, nothing launched): everything r2dm_dpm_step refuses; what
 *    r2dm_posterior_step_known refuses about known, mask, channels and mask_channels (per_sample must divide into `channels` planes of a
 *    multiple of 4 elements, mask_channels 1 or `channels` -- with or without a measurement); exactly one of known / mask given; noise,
 *    known or mask not 16-byte aligned; x_s or x0 equal to noise, known or mask. */
int r2dm_dpm_step_known(const float* x_t, const float* prediction, const float* x0_prev, const float* noise, const float* known,
                        const float* mask, const float* coef, float* x_s, float* x0, int32_t batch, int64_t per_sample, int32_t channels,
                        int32_t mask_channels, int32_t objective, float clip, void* stream);

/* -- RePaint completion (models/diffusion/continuous_time.py:169-190 q_step_from_x_0 / q_step, :287-303 the
 *    known/unknown blend inside repaint()).  coef is (B,2) host-computed scalars.
 *    blend:  out = mask * (known*alpha + noise*sigma) + (1 - mask) * unknown,  coef = (alpha, sigma) at step s;
 *            mask has `mask_channels` channels (1 = broadcast over the `channels` planes of a sample).
 *    q_step: x_t = x_s * a_ts + std * noise,  coef = (alpha_t/alpha_s, sqrt(sigma_t^2 - a_ts^2 sigma_s^2)). */
int r2dm_repaint_blend(const float* known, const float* noise, const float* unknown, const float* mask,
                       const float* coef, float* out, int32_t batch, int64_t per_sample, int32_t channels,
                       int32_t mask_channels, void* stream);
int r2dm_q_step(const float* x_s, const float* noise, const float* coef, float* x_t, int32_t batch, int64_t per_sample,
                void* stream);

/* -- denoising loss: the value of GaussianDiffusion.p_loss between the denoiser call and the loss weight
 *    (models/diffusion/base.py:133-137), one pass over prediction, x_0, noise (batch, channels, plane) fp32 and the mask.
 *    objective: 0 eps (target = noise), 1 v (alpha * noise - sigma * x_0, coef (B,2) = (alpha, sigma) host-computed scalars; coef is read
 *    for this objective only), 2 x_0.  criterion: 0 l2, 1 l1, 2 huber (SmoothL1Loss, beta = 1).  mask: NULL (all ones) or
 *    (batch, mask_channels, plane) with mask_channels 1 (broadcast over the channels) or `channels`.
 *    num (batch, channels) fp64 = sum of loss * mask per plane; den (batch) fp64 = the sum of the mask over its own elements
 *    (channels * plane with no mask).  Sums are float64 in a fixed order (no atomics): bit-reproducible, and a sample's sums do not
 *    depend on the rest of the batch.  scratch: r2dm_diffusion_loss_scratch_bytes(batch, channels, plane) bytes (0 for an empty or
 *    oversized problem), 8-byte aligned.  The fp32 pointers must be 16-byte aligned when plane is a multiple of 4 (read as quads), else
 *    4-byte aligned; num and den 8-byte aligned. */
size_t r2dm_diffusion_loss_scratch_bytes(int32_t batch, int32_t channels, int64_t plane);
int r2dm_diffusion_loss(const float* prediction, const float* x_0, const float* noise, const float* mask, int32_t mask_channels,
                        const float* coef, int32_t objective, int32_t criterion, int32_t batch, int32_t channels, int64_t plane,
                        void* scratch, double* num, double* den, void* stream);

/* -- latent space: DDIM inversion / decoding from a given latent, and spherical interpolation of latents.
 *    r2dm_ddim_transfer moves x from noise level t to any level u along the deterministic DDIM line (u > t inverts, u < t decodes),
 *    without clipping.  coef is (B,4) = (alpha_t, sigma_t, alpha_u, sigma_u), host- or device-computed scalars in device memory.  Per
 *    element, float32, not contracted, x_0 and eps in the direct form of the objective (0 eps, 1 v, 2 x_0):
 *      eps: e = pr, x0 = (x - s_t*pr)/a_t | v: x0 = a_t*x - s_t*pr, e = s_t*x + a_t*pr | x_0: x0 = pr, e = (x - a_t*pr)/s_t
 *      x_u = a_u*x0 + s_u*e.
 *    per_sample must be a multiple of 4 and x_t, prediction, x_u 16-byte aligned.
 *    r2dm_slerp: per sample, over all per_sample elements, out[k][b] = fl32(c_a)*a[b] + fl32(c_b)*b[b] for each of the K weights w_k
 *    (HOST memory, 1 <= K <= 64, finite; values outside [0,1] extrapolate), out (K,batch,per_sample) fp32, coef64 (K,batch,2) fp64 =
 *    (c_a, c_b).  cos = <a,b>/sqrt(<a,a><b,b>) clamped to [-1,1], omega = acos(cos), c_a = sin((1-w)omega)/sin(omega), c_b =
 *    sin(w omega)/sin(omega); when 1 - cos^2 < 1e-10 or a norm is 0: the lerp pair (1-w, w).  The three sums are float64 sums of the
 *    float32 products in a fixed order (no atomics): bit-reproducible, and a sample's result does not depend on the rest of the batch.
 *    Two launches.  scratch: r2dm_slerp_scratch_bytes(batch, per_sample) bytes (0 for an empty, oversized or non-multiple-of-4
 *    problem), 8-byte aligned; a, b, out 16-byte aligned, per_sample a multiple of 4. */
int r2dm_ddim_transfer(const float* x_t, const float* prediction, const float* coef, float* x_u, int32_t batch, int64_t per_sample,
                       int32_t objective, void* stream);
size_t r2dm_slerp_scratch_bytes(int32_t batch, int64_t per_sample);
int r2dm_slerp(const float* a, const float* b, const float* weights, int32_t K, float* out, double* coef64, int32_t batch,
               int64_t per_sample, void* scratch, void* stream);

/* -- sample post-processing: LiDARUtility.denormalize/revert_depth/to_xyz + concat
 *    (utils/lidar.py:49-61,98-120; sample_and_save.py:52-57).  x (B,2,H,W) in [-1,1],
 *    ray_angles (2,H,W) [elevation, azimuth] in rad, out (B,5,H,W) = depth,x,y,z,reflectance. */
int r2dm_lidar_postprocess(const float* x, const float* ray_angles, float* out, int32_t batch, int32_t height,
                           int32_t width, float min_depth, float max_depth, void* stream);
/* ... with the checkpoint's depth coding (LiDARUtility.revert_depth, utils/lidar.py:95-112):
 *    depth_format 0 = "log_depth" (the entry above), 1 = "inverse_depth", 2 = "depth". */
int r2dm_lidar_postprocess_fmt(const float* x, const float* ray_angles, float* out, int32_t batch, int32_t height,
                               int32_t width, float min_depth, float max_depth, int32_t depth_format, void* stream);

/* -- BEV metrics of the evaluation script (metrics/bev.py; evaluate.py:22-41,131-196) ---------------------------------------
 * r2dm_bev_histogram: point_cloud_to_histogram on a batch -- the (x, y) occupancy histogram, bins x bins over the edges
 *    `edges` (bins + 1 fp32 values in device memory, as torch.linspace computes them), of the points with
 *    min_depth < |xyz| < max_depth.  layout 0: src (B,5,H,W) samples [depth, x, y, z, reflectance], xyz first masked by
 *    image_min_depth < depth < image_max_depth (points = H*W); layout 1: src (B,points,3).  hist (B,bins,bins) int32 counts,
 *    bit-identical to torch.histogramdd on the CPU; sum (bins,bins) int64 over the batch, or NULL.  bins <= 128.
 * r2dm_bev_hist_sum: sum (cells,) int64 of a batch of histograms hist (batch,cells), int32 (is_int32 = 1) or fp32 counts.
 * r2dm_bev_mmd: the three means of 1 - k over P x Q, P x P and Q x Q (out[3], fp64) of the RBF kernel
 *    k = exp(-|p - q|^2 / (2 sigma^2)) between the rows of p (np,bins) and q (nq,bins), each normalised by its sum;
 *    MMD = 2 out[0] - out[1] - out[2].  scratch: r2dm_bev_mmd_scratch_bytes() of device memory. */
int r2dm_bev_histogram(const float* src, int32_t layout, const float* edges, int32_t* hist, int64_t* sum, int32_t batch,
                       int64_t points, int32_t bins, float min_depth, float max_depth, float image_min_depth,
                       float image_max_depth, void* stream);
int r2dm_bev_hist_sum(const void* hist, int32_t is_int32, int64_t* sum, int64_t batch, int64_t cells, void* stream);
size_t r2dm_bev_mmd_scratch_bytes(int32_t np, int32_t nq);
int r2dm_bev_mmd(const float* p, const float* q, int32_t np, int32_t nq, int64_t bins, double sigma, void* scratch,
                 size_t scratch_bytes, double* out, void* stream);

/* -- FPD of the evaluation script: PointNet features and their distribution metrics (metrics/extractor/pointnet.py,
 *    metrics/distribution.py; evaluate.py:61-65,158-160,182-187) ------------------------------------------------------------------
 * The network is PointNet1(k = 16) in eval mode with every BatchNorm folded into the layer in front of it by the caller.
 * r2dm_pointnet_pack: w (cout, cin) fp32 -> packed (r2dm_pointnet_packed_bytes(), 16-byte aligned): the layer scaled by a power of
 *    two (max|w| into [2^9, 2^10)) and split into an fp16 piece and an fp16 residual, in matrix-core operand order.  wscale: two
 *    floats of device memory, [1] <- the inverse scale.  cout % 32 == 0, cin % 16 == 0.  *flag |= 4 if a weight is not finite.
 * r2dm_pointnet_trunk: one fused pass over the points of every cloud: 3 -> 64 (fp32 FMA, ReLU), 64 -> 128 (ReLU) and 128 -> 1024 on
 *    the fp16 matrix pipe (three products per MAC, fp32 accumulation), and the per-channel maximum over the points; only the maxima
 *    reach memory: scratch (r2dm_pointnet_scratch_bytes()) holds them as order-preserving integer keys of W3 h2 before the last
 *    layer's inverse scale and bias, which r2dm_pointnet_head applies.  Exact and the same bits on every call and for every order of
 *    the points.  layout 0: src (batch,5,H,W) samples [depth, x, y, z, reflectance], xyz x (image_min_depth < depth < image_max_depth) /
 *    divisor, points = H W, all kept; layout 1: src (batch,points,3); layout 2: src (batch,3,points).  trans: (batch,9) row-major 3 x 3
 *    applied as point @ trans, or NULL.  w1b: (64,4) rows [w0, w1, w2, bias]; b2 (128,).
 *    *flag |= 1 for a non-finite coordinate, |= 2 for an activation outside the fp16 operand range (65504): the results are then invalid.
 * r2dm_pointnet_head: per cloud x1 = max * w3_inv_scale + b3 (ReLU if stn), fc1 1024 -> 512 + ReLU, fc2 512 -> 256 + ReLU,
 *    fc3 256 -> outputs, plain fp32.  stn = 1: out (batch,9) = fc3 + identity (outputs = 9); stn = 0: out (batch,1808) =
 *    cat(x1, x2, x3, x4), outputs = 16.
 * r2dm_feature_moments: feats (rows,dim) fp32 -> mean (dim,) and unbiased covariance (dim,dim) in fp64, two passes, fixed order.
 * r2dm_poly_mmd: for each of `subsets` subsets, x = rows ix[s] of X and y = rows iy[s] of Y (subset_size int64 indices each, device
 *    memory, in range): out[s] = (sum_ij (x_i.y_j / dim + 1)^3, the same over x x x off the diagonal, over y x y off the diagonal),
 *    fp64 throughout, no subset_size^2 matrix.  scratch: r2dm_poly_mmd_scratch_bytes(), 256-byte aligned.
 * r2dm_feature_knn: the primitive of the k-NN manifold metrics (improved precision / recall, density / coverage).  x (m,dim), y (n,dim)
 *    fp32.  D2(i,j) = max(0, |x_i|^2 + |y_j|^2 - 2 x_i.y_j): every value widened to fp64 first, the norms summed in fp64 in a fixed
 *    order, the dot product on the fp64 matrix pipe in an order that is fixed per element and independent of the tiling.  For every
 *    row i over the admissible columns j (all of them; same = 1, which requires y == x and m == n, drops j == i -- by index, so a
 *    duplicate row is a neighbour at distance 0):
 *      kth2[i]   the k-th smallest D2 (needs k >= 1);
 *      min2[i], argmin[i]   the smallest D2 and its column, the lowest column on an equal computed value;
 *      count[i]  the number of columns with D2 <= y_radius2[j] (needs y_radius2 (n,) fp64; a NaN radius never counts).
 *    Each output may be NULL.  status: int64[1] of device memory, zeroed by the call, receives the number of rows of x or y (of x
 *    alone with same = 1) that hold a non-finite value; outputs that depend on such a row are unspecified, every other row's are those
 *    of a clean call, nothing faults.  chosen: NULL or HOST int32[2] <- the row tiles and the column splits of the launch.
 *    The same bits on every call, no floating-point atomics; row i's outputs depend neither on the other rows of x nor on the tiling
 *    or the number of column splits.  No m x n buffer: scratch (r2dm_feature_knn_scratch_bytes; 0 outside the limits) holds the norms
 *    and, per row and column split, a k-list, a minimum and a count; a second kernel merges the splits in split order.
 *    Limits: 1 <= dim <= 16384, 1 <= m, n <= 2^20, 0 <= k <= 16, at least k admissible columns; x and y 16-byte aligned when
 *    dim % 4 == 0, else 4-byte; kth2, min2, y_radius2, scratch and status 8-byte aligned.  A refusal returns 1 and sets
 *    r2dm_last_error before anything is launched or written.  Nothing is allocated, nothing synchronises. */
size_t r2dm_pointnet_packed_bytes(int32_t cout, int32_t cin);
int r2dm_pointnet_pack(const float* w, int32_t cout, int32_t cin, void* packed, float* wscale, int32_t* flag, void* stream);
size_t r2dm_pointnet_scratch_bytes(int32_t batch);
int r2dm_pointnet_trunk(const float* src, int32_t layout, int32_t batch, int64_t points, const float* trans, float image_min_depth,
                        float image_max_depth, float divisor, const float* w1b, const void* w2_packed, const float* w2_inv_scale, const float* b2,
                        const void* w3_packed, void* scratch, size_t scratch_bytes, int32_t* flag, void* stream);
int r2dm_pointnet_head(const void* scratch, const float* w3_inv_scale, const float* b3, int32_t stn, const float* fc1_w, const float* fc1_b,
                       const float* fc2_w, const float* fc2_b, const float* fc3_w, const float* fc3_b, int32_t outputs, float* out, int32_t batch,
                       void* stream);
int r2dm_feature_moments(const float* feats, int64_t rows, int32_t dim, double* mean, double* cov, void* stream);
size_t r2dm_poly_mmd_scratch_bytes(int32_t subsets, int32_t subset_size);
int r2dm_poly_mmd(const float* x, const float* y, const int64_t* ix, const int64_t* iy, int32_t subsets, int32_t subset_size, int32_t dim,
                  void* scratch, size_t scratch_bytes, double* out, void* stream);
size_t r2dm_feature_knn_scratch_bytes(int64_t m, int64_t n, int32_t dim, int32_t k);
int r2dm_feature_knn(const float* x, int64_t m, const float* y, int64_t n, int32_t dim, int32_t same, int32_t k, const double* y_radius2, double* kth2,
                     double* min2, int32_t* argmin, int32_t* count, void* scratch, size_t scratch_bytes, int64_t* status, int32_t* chosen,
                     void* stream);

/* -- FRD of the evaluation script and the segmentation of completion_demo.py: RangeNet-53 / -21 (metrics/extractor/rangenet.py) in eval
 *    mode, every BatchNorm folded into the layer in front of it by the caller ------------------------------------------------------
 * r2dm_rangenet_pack: w (cout, taps, cin) fp32 -> packed (r2dm_rangenet_packed_bytes(), 16-byte aligned): cout padded to 32 and cin to 16
 *    with zeros, the layer scaled by a power of two (max|w| into [2^9, 2^10)) and split into an fp16 piece and an fp16 residual, in
 *    matrix-core operand order.  wscale: two floats of device memory, [1] <- the inverse scale.  *flag |= 4 if a weight is not finite.
 * r2dm_rangenet_conv: one layer as an implicit GEMM on the fp16 matrix pipe (three products per MAC, fp32 accumulation):
 *    out = LeakyReLU_slope(conv(in) * inv_scale + bias) + add + add2 (add, add2: fp32 tensors of out's shape, or NULL; slope 1 = no
 *    activation), fp32 NCHW.  kind 0: 1 x 1; 1: 3 x 3 pad 1 (taps row-major); 2: 3 x 3 pad 1 stride (1,2), out width = width / 2;
 *    3 / 4: the even / odd output columns of the transposed 1 x 4, stride (1,2), pad (0,1) convolution (two taps: in[j] and in[j-1] /
 *    in[j] and in[j+1]), out width = 2 width, the other columns are left alone; 5: the stem, in = (batch,5,height,width) samples
 *    [depth, x, y, z, reflectance], each value (v - norm[c]) / norm[5 + c] * mask, mask (batch,1,height,width) of zeros and ones or NULL for
 *    min_depth < depth < max_depth; the raw values of a masked pixel are not used.  cin % 16 == 0 (stem: 5).
 *    *flag |= 1 for a non-finite value of an unmasked input pixel, |= 2 for an activation outside the fp16 operand range (65504): the
 *    results are then invalid.  The same bits on every call; a sample's result does not depend on the rest of the batch.
 * r2dm_rangenet_argmax: logits (batch,classes,pixels) -> labels (batch,pixels) int64, the lowest index on a tie. */
size_t r2dm_rangenet_packed_bytes(int32_t cout, int32_t cin, int32_t taps);
int r2dm_rangenet_pack(const float* w, int32_t cout, int32_t cin, int32_t taps, void* packed, float* wscale, int32_t* flag, void* stream);
int r2dm_rangenet_conv(const float* in, const float* mask, const float* norm, float min_depth, float max_depth, const void* packed,
                       const float* inv_scale, const float* bias, const float* add, const float* add2, float* out, int32_t batch, int32_t cin,
                       int32_t height, int32_t width, int32_t cout, int32_t kind, float slope, int32_t* flag, void* stream);
int r2dm_rangenet_argmax(const float* logits, int64_t* labels, int32_t batch, int32_t classes, int64_t pixels, void* stream);

/* -- rendering of generate.py (utils/render.py; generate.py:44-59) -------------------------------------------------------------
 * All arithmetic is fp32 with one rounding per operation.  The splat accumulates 64-bit fixed-point integers (scale from the
 * largest |value| of the call, taken on the device): the same bits on every call and for every order of the points.
 * r2dm_colorize: x (batch, pixels) -> out (batch, 3, pixels) uint8 = trunc(clamp(lut[trunc(clamp(x 256, 0, 255))] 255, 0, 255)),
 *    lut (256,3) fp32 in device memory.
 * r2dm_bilinear_rasterize: coords (B,N,2) [row, column], values (B,N,C) -> out (B,C,H,W): every point adds value x bilinear
 *    weight at its four neighbours (weights of clamped indices and products below 1e-3 are zero; non-finite coordinates add
 *    nothing).  ratio = 1 (C = 4): out (B,3,H,W) = sum_c / (sum_3 + 1e-8).  scratch: r2dm_rasterize_scratch_bytes(), 256-byte aligned.
 * r2dm_project_points: the per-point half of render_point_clouds: points (B,N,3), colors (B,N,3) or NULL (ones), view = 12 HOST
 *    floats (R row-major, then t): p' = (x, y, -z) R + t, pinhole projection with K = diag(f, f, 1), cx = cy = 0.5 ->
 *    uv (B,N,2) = size - size * projection, vals (B,N,4) = [w c0 m, w c1 m, w c2 m, w], w = exp(-3 |p'|), m the border mask.
 * r2dm_render_frames: generate.py's render() in one pass over x (frames,2,H,W) (depth / max_depth, reflectance; both in [0,1]):
 *    img (frames,3,2H,W) = turbo of the stacked channels / 255, bev (frames,3,size,size) = 1 - render_point_clouds(xyz, 1 - viridis(z)).
 *    trig (4,H,W): cos / sin of the elevation, cos / sin of the azimuth; turbo, viridis (256,3).  Frames are taken as many at a
 *    time as scratch (at least r2dm_render_frames_scratch_bytes(1, size), 256-byte aligned) holds. */
int r2dm_colorize(const float* x, const float* lut, uint8_t* out, int64_t batch, int64_t pixels, void* stream);
size_t r2dm_rasterize_scratch_bytes(int32_t batch, int32_t channels, int32_t height, int32_t width);
int r2dm_bilinear_rasterize(const float* coords, const float* values, float* out, int32_t batch, int64_t points, int32_t channels,
                            int32_t height, int32_t width, void* scratch, size_t scratch_bytes, int32_t ratio, void* stream);
int r2dm_project_points(const float* points, const float* colors, const float* view, float focal_length, int32_t size, float* uv,
                        float* vals, int64_t total_points, void* stream);
size_t r2dm_render_frames_scratch_bytes(int32_t frames, int32_t size);
int r2dm_render_frames(const float* x, const float* trig, const float* turbo, const float* viridis, float* img, float* bev,
                       int64_t frames, int32_t height, int32_t width, int32_t size, float min_depth, float max_depth,
                       const float* view, float focal_length, void* scratch, size_t scratch_bytes, void* stream);

/* -- surface normals and the training monitor's bird's-eye view (utils/render.py:145-236; train.py:227-239) ----------------------
 * r2dm_surface_normals: estimate_surface_normal on xyz (batch,3,height,width) fp32 -> normals (batch,3,height,width) fp32, one launch.
 *    The neighbour of pixel (h, w) at offset (dh, dw) is the pixel (clamp(h + dh, 0, height - 1), (w + dw) mod width): rows replicate,
 *    columns are circular (the azimuth seam is a neighbour like any other).  The eight offsets, k = 0 .. 7, are (-d,0) (-d,d) (0,d) (d,d)
 *    (d,0) (d,-d) (0,-d) (-d,-d).  With a the pixel's own point and p_k its k-th neighbour:
 *      V_k = p_k - a                                           (per component)
 *      |v| = sqrt((v0 v0 + v1 v1) + v2 v2)
 *      u x v = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)
 *    mode 0 ("closest"): dist_k = |V_k| + |V_(k+2)%8|; the smallest dist_k wins, the lowest k on a tie; n = V_k x V_(k+2)%8.
 *    mode 1 ("mean"):    c_k = V_k x V_(k+2)%8; n = (((c_0 + c_1) + c_2) + ... + c_7) / 8 (per component).
 *    normals = n / (|n| + 1e-8f) (per component).  Everything is fp32 with one rounding per written operation (nothing contracted),
 *    sqrt and the division correctly rounded, denormals kept: the result is a function of the input bits, the same on every call, and a
 *    sample's normals do not depend on the rest of the batch.  A pixel whose window is all zeros gives exactly 0.  A non-finite input
 *    makes the normals of the pixels whose window holds it unspecified and leaves every other pixel as it is.
 *    Limits: 1 <= d <= 8, d <= width, mode 0 or 1, height, width >= 1 (height < 2 d + 1 is fine: the rows replicate); fewer than 2^31
 *    tiles of 4 x 64 pixels over the batch.  Beyond them the call returns a status and launches nothing.  normals must not alias xyz.
 * r2dm_normal_frames: train.py's log_images view in one pass over metric (frames,1,height,width), the depth in metres:
 *      mask = min_depth < metric < max_depth                  (1 or 0)
 *      xyz  = ((((metric cos_phi) cos_theta) mask) / max_depth) mask, ((((metric cos_phi) sin_theta) mask) / max_depth) mask,
 *             (((metric sin_phi) mask) / max_depth) mask       (LiDARUtility.to_xyz, then / max_depth * mask)
 *      n    = the normal of r2dm_surface_normals(xyz, d, mode) at the pixel
 *      colour = (-n + 1) / 2
 *    colors (frames,3,height,width) = colour (NULL: not written); bev (frames,3,size,size) = render_point_clouds(xyz, colour) under the
 *    view (12 HOST floats, R row-major then t) and focal length of r2dm_project_points, splatted as r2dm_bilinear_rasterize does (64-bit
 *    fixed point, the same bits on every call).  A point whose coordinates or colour are not finite adds nothing.  trig (4,height,width):
 *    cos / sin of the elevation, cos / sin of the azimuth, as r2dm_render_frames takes them.  No xyz, normal or per-point tensor is written.
 *    Frames are taken as many at a time as scratch (at least r2dm_normal_frames_scratch_bytes(1, size), 256-byte aligned) holds; a
 *    frame's images do not depend on that number.  Limits: those of r2dm_surface_normals, max_depth > 0. */
int r2dm_surface_normals(const float* xyz, float* normals, int32_t batch, int32_t height, int32_t width, int32_t d, int32_t mode, void* stream);
size_t r2dm_normal_frames_scratch_bytes(int32_t frames, int32_t size);
int r2dm_normal_frames(const float* metric, const float* trig, float* colors, float* bev, int64_t frames, int32_t height, int32_t width,
                       int32_t size, float min_depth, float max_depth, int32_t d, int32_t mode, const float* view, float focal_length,
                       void* scratch, size_t scratch_bytes, void* stream);

/* -- raw scans to range images (data/kitti_360/kitti_360.py:34-93,164-165; the same in data/kitti_raw) -------------------------
 * r2dm_project_scans: load_points_as_images on a batch of scans held in one buffer: points (total,4) fp32 [x, y, z, reflectance]
 *    in device memory (16-byte aligned), scan b = rows offsets[b] .. offsets[b + 1] - 1; offsets = batch + 1 HOST values, offsets[0] = 0,
 *    non-decreasing (an empty scan gives an empty image), read before the call returns.
 *    depth = sqrt((x x + y y) + z z) in fp32, one rounding per operation (np.linalg.norm), mask = min_depth <= depth <= max_depth.
 *    Column: floor(((-atan2(y, x)) / pi + 1) / 2 mod 1 * width), fp32.  Row, scan_unfolding = 0: floor((1 - (asin(z / depth) + 25 deg) /
 *    28 deg) * height), fp32 asin, the rest fp64 (numpy >= 2); scan_unfolding = 1: by the point's position in the file -- a delimiter is a
 *    point in the 1st quadrant whose predecessor (cyclically) is in the 4th; with D delimiters in the scan and seg of them at positions
 *    <= i: row 0 if seg = 0, else r = height - 1 - (D - seg) -> r if r >= 0, height - 1 if r = -1, 0 below (the reference's loop).  Both
 *    clipped to the grid.  Every cell keeps its NEAREST point, inside the depth window or not; among equal depths the lowest index wins
 *    (64-bit integer atomic min of depth bits : index): the same bits on every call and for every order of the launch.
 *    A point whose depth is not a finite number > 0 (NaN / inf coordinates, (0,0,0)) never wins a cell; under scan unfolding it still
 *    counts in the sequence (quadrant 0 where a comparison with NaN decides).
 *    layout 0: out (batch,6,height,out_width) [x, y, z, reflectance, depth, mask], layout 1: out (batch,5,height,out_width)
 *    [depth, x, y, z, reflectance] (r2dm_bev_histogram's layout 0); empty cells are 0.  apply_mask = 1 multiplies every value by the mask
 *    (the dataset builder), 0 leaves them (the function's raw return value).  out_width <= width writes column j from source column
 *    floor((j + 0.5) width / out_width) (F.interpolate, mode "nearest-exact").
 *    scratch: r2dm_project_scratch_bytes() of device memory (0: geometry refused), 256-byte aligned.
 *    Limits: batch <= 65535; fewer than 2^31 points and fewer than 2^31 cells over the batch. */
size_t r2dm_project_scratch_bytes(int64_t total_points, int32_t batch, int32_t height, int32_t width, int32_t scan_unfolding);
int r2dm_project_scans(const float* points, const int64_t* offsets, float* out, int32_t batch, int32_t height, int32_t width,
                       int32_t out_width, int32_t scan_unfolding, float min_depth, float max_depth, int32_t apply_mask, int32_t layout,
                       void* scratch, size_t scratch_bytes, void* stream);

/* -- range images to point clouds: the inverse of r2dm_project_scans (Velodyne .bin rows out of samples) -----------------------
 * r2dm_unproject: a batch of range images -> the batch's valid pixels as [x, y, z, reflectance] rows, compacted into ONE buffer:
 *    points (batch*height*width,4) fp32 capacity in device memory (16-byte aligned), scan b = rows offsets[b] .. offsets[b + 1] - 1;
 *    offsets = batch + 1 int64 values written to DEVICE memory (offsets[batch] = the number of points; read them after the stream
 *    has run); index (batch*height*width) int32 or NULL: row i's pixel h*width + w inside its scan.
 *    Order, a part of the contract: position p in [0, height*width) of a scan is pixel h = p / width and
 *    w = p % width (row_start = NULL: image order) or w = (row_start[h] - p % width) mod width (scan order: row_start = height int32
 *    values in device memory, the last column of row h whose azimuth is >= 0; rows top to bottom, the azimuth rising from 0 inside a
 *    row, so that a ring ends in the 4th quadrant and the next starts in the 1st -- the delimiter r2dm_project_scans counts under
 *    scan_unfolding); the valid positions keep that order.  The same bits on every call: no atomics, no block waits for another.
 *    layout 0: src (batch,2,height,width), the model's sample in [-1,1]; the point is r2dm_lidar_postprocess_fmt's, bit for bit
 *    (ray_angles (2,height,width), min_depth, max_depth, depth_format as there); valid: inside the depth window (that entry's xyz
 *    mask is 1), keep_min < depth < keep_max, x, y, z finite.  layout 1: src (batch,5,height,width) [depth, x, y, z, reflectance]
 *    (r2dm_lidar_postprocess's output, r2dm_project_scans' layout 1), values copied; valid: keep_min < depth < keep_max, x, y, z
 *    finite; ray_angles, min_depth, max_depth, depth_format unused.  NaN never compares true: such a pixel is dropped.
 *    scratch: r2dm_unproject_scratch_bytes() of device memory (0: geometry refused), 256-byte aligned.  No host synchronisation.
 *    Limits: batch <= 65535; fewer than 2^31 pixels over the batch. */
size_t r2dm_unproject_scratch_bytes(int32_t batch, int32_t height, int32_t width);
int r2dm_unproject(const float* src, int32_t layout, const float* ray_angles, const int32_t* row_start, float* points, int32_t* index,
                   int64_t* offsets, int32_t batch, int32_t height, int32_t width, float min_depth, float max_depth,
                   int32_t depth_format, float keep_min, float keep_max, void* scratch, size_t scratch_bytes, void* stream);

/* -- post-processing of the segmentation: the kNN label filter of RangeNet++ and the CRF-RNN refinement of SqueezeSeg
 *    (metrics/extractor/rangenet.py:197-405), one launch each, zero padding at every image edge (no wrap at the azimuth seam) -----------
 * r2dm_knn_vote: depth (batch,1,height,width) fp32, label (batch,height,width) int64 -> out (batch,height,width) int64.
 *    A depth that is not finite is read as -1.  With the K = kh kw window offsets o in row-major order: the neighbour depth n_o(p) is the
 *    depth at p + o, 0 outside the image and +inf where it is negative; jump_o(p) = |n_o(p) - depth(p)| inside the image, 0 outside;
 *    dist_o(p) = sum over the window offsets q, row-major, of weight[q] * jump_o(p + q), in fp32 with one rounding per operation from an
 *    accumulator of 0 (weight: (kh,kw) fp32 in device memory, 1 - the normalised Gaussian).  The k smallest dist_o win, ties to the lowest
 *    o (a NaN, which only a zero weight can produce, is the largest); a winner with dist > cutoff votes for nothing (cutoff <= 0: never),
 *    a neighbour outside the image carries label 0.  out(p) = the class with the most votes, the lowest on a tie, 0 without votes.
 *    A label outside [0, classes) sets *flag |= 1 and votes for nothing.  The result is a function of the input bits; an image's labels
 *    do not depend on the rest of the batch.  Limits: kh, kw odd and <= 7, 1 <= k <= min(K, 8), classes <= 32, batch <= 65535.
 * r2dm_crf_iter: one mean-field iteration q_out = unary - compat . (ws * smooth_gamma(S) + wa * mask * appearance(S mask) * smooth_alpha(S)),
 *    S = softmax of q_in over the classes; q_in, unary, q_out (batch,classes,height,width), xyz (batch,3,height,width), mask
 *    (batch,1,height,width), all fp32; q_out must not alias an input.  smooth_t(S)[c](p) = sum over o != 0 of kernel_t[c][o] S[c](p + o);
 *    appearance(X)[c](p) = sum over o != 0 of X[c](p + o) exp(-|xyz(p + o) - xyz(p)|^2 / beta[c]), everything 0 outside the image.
 *    params, fp32 in device memory: kernel_gamma (classes,kh,kw) | kernel_alpha (classes,kh,kw) | ws (classes) | wa (classes) |
 *    beta (classes) = 2 theta_beta^2 | compat (classes,classes), row = output class.  uniform_beta != 0: beta[0] holds for every class and
 *    the exponentials are taken once per neighbour.  Sums run in a fixed order: the same bits on every call, independent of the batch.
 *    Limits: kh, kw odd and <= 7, classes <= 32, batch <= 65535. */
int r2dm_knn_vote(const float* depth, const int64_t* label, const float* weight, int64_t* out, int32_t batch, int32_t height, int32_t width,
                  int32_t kh, int32_t kw, int32_t k, int32_t classes, float cutoff, int32_t* flag, void* stream);
int r2dm_crf_iter(const float* q_in, const float* unary, const float* xyz, const float* mask, const float* params, float* q_out, int32_t batch,
                  int32_t classes, int32_t height, int32_t width, int32_t kh, int32_t kw, int32_t uniform_beta, void* stream);

/* -- completion metrics: how good an inpainted scan is (beam-level upsampling of held-out scans, the second results table of the R2DM
 *    paper; the reference has no code for it) ---------------------------------------------------------------------------------------------
 * r2dm_completion_error: pred, target (batch,5,plane) fp32 in the sample layout [depth, x, y, z, reflectance] (planes 0 and 4 are read),
 *    known (batch,1,plane) fp32 zeros and ones (the RePaint mask).  Per sample, with U = {known == 0}, G = {lo < target depth < hi},
 *    P = {lo < pred depth < hi} (a NaN depth is in neither), E = U & G, Bo = E & P and r^ = pred depth on P, else 0:
 *    out (batch,10) fp64 = |U|, |E|, |Bo|, |U & P \ G|, sum_E |r^ - r|, sum_E (r^ - r)^2, sum_Bo |dr|, sum_Bo dr^2, sum_E |drho|, sum_E drho^2.
 *    Every fp32 value is widened to fp64 first (exact differences); sums are fp64 in a fixed order (no atomics): bit-reproducible, and a
 *    sample's numbers do not depend on the rest of the batch.  scratch: the bytes the _scratch_bytes function returns for (batch, plane)
 *    (0 for an empty or oversized problem), 8-byte aligned like out.  The fp32 pointers must be 16-byte aligned when plane is a multiple
 *    of 4 (read as quads), else 4-byte aligned.
 * r2dm_confusion_matrix: pred, target (batch,pixels) int64 labels, mask NULL or (batch,pixels) fp32 (0 skips the pixel) ->
 *    counts (batch,classes,classes) int64, [b][target][pred], zeroed by the call.  One int32 table per block in LDS, merged with 64-bit
 *    integer atomics: exact, independent of any order.  An unmasked label outside [0, classes) indexes nothing and is counted in *bad
 *    (int64 in device memory, zeroed by the call).  Limits: 1 <= classes <= 64, batch <= 65535, batch * pixels <= 2^40.
 * r2dm_fill_beams: the interpolation baselines.  x, out (batch,channels,height,width) fp32, rows (batch,height) bytes (non-zero = the
 *    beam is known).  A known row is copied.  For a pixel (h, w) of an unknown row, `up` / `dn` are the nearest known rows above / below
 *    (no wrap); an endpoint is usable if it exists and x[b][0][row][w] != nodata.  mode 0 (nearest): every channel from the usable endpoint
 *    at the smaller row distance, `up` on a tie.  mode 1 (linear): with both usable a + (b - a) * t, t = float(h - up) / float(dn - up), in
 *    fp32 with IEEE division and no contraction; with one usable a copy of it.  No usable endpoint: nodata in every channel.  out must
 *    not alias x.  Limits: batch, height <= 65535.
 * r2dm_ensemble_score: K completions ("members") of each scan scored as an ensemble.  samples (batch,members,5,plane) fp32 in the sample
 *    layout, a scan's members adjacent (planes 0 and 4 are read); target, known, lo, hi, U, G, E as for r2dm_completion_error.  Member k
 *    returns at a pixel iff lo < d_k < hi (NaN is in neither); r^_k = d_k then, else 0; n = the returning members; g = [pixel in G]; a NaN
 *    member reflectance counts as 0.  With K = members and m = (1/K) sum_k r^_k:
 *    raw (batch,13) fp64 = |U|, |E|, sum_E sum_k |r^_k - r|, sum_E sum_{k<l} |r^_k - r^_l|, sum_E (m - r)^2,
 *      sum_E (1/(K-1)) sum_k (r^_k - m)^2 (0 at K = 1), the same four sums for reflectance (on the stored values), sum_U (n/K - g)^2,
 *      sum_E n/K, sum_{U \ G} n/K.  Un-normalised: CRPS = (raw[2]/K - raw[3]/K^2) / |E|, which is the mean absolute error at K = 1.
 *    member (batch,2,members) fp64 = sum_E |r^_k - r| and sum_E |rho_k - rho| per member, in member order.
 *    rank (batch,members+1) int64 = over E the histogram of #{k : r^_k < r}, zeroed by the call (int32 table per block in LDS, 64-bit
 *      integer atomics: exact in any order).
 *    maps NULL or (batch,8,plane) fp32, written for every pixel: n/K; over the returning members the mean, the population standard
 *      deviation (two-pass; 0 if n < 2), the median (even n: the fp64 mean of the two middle values), the minimum and the maximum of depth
 *      (0 if n = 0); the mean and the population standard deviation of reflectance over all members.  fp64, rounded once to fp32.  maps
 *      must not overlap an input.
 *    Every fp32 value is widened to fp64 first.  Per pixel and channel the members are sorted ascending and every sum over members runs in
 *    sorted order, the pair term as sum_{i=1}^{K-1} i (K - i) (x_(i+1) - x_(i)): everything but `member` is bit-identical under any
 *    permutation of the members.  Float sums run in a fixed order (per-block partials added in index order by a second kernel, no float
 *    atomics): the same bits on every call, and a scan's numbers do not depend on the batch.  scratch: the bytes the _scratch_bytes
 *    function returns for (batch, members, plane) (0 for an empty or oversized problem); scratch, raw, member and rank 8-byte aligned; the
 *    fp32 pointers 16-byte aligned when plane is a multiple of 4, else 4-byte aligned.  Limits: batch <= 65535, 1 <= members <= 64,
 *    plane <= 2^40, samples of at most 2^40 elements.
 * r2dm_ensemble_coherence: the same ensemble scored across pixels -- what the energy score and the variogram score are made of.  samples
 *    (batch,members,5,height,width), target, known, lo, hi, U, G, E as for r2dm_ensemble_score.  Per channel c (0 depth, 1 reflectance)
 *    the values v_i, i in [0, K]: for i < K member i's (depth d if lo < d < hi, else 0; reflectance as stored, NaN read as 0), v_K the
 *    target's, as stored.  Every fp32 value is widened to fp64 first.
 *    counts (batch,2) fp64 = |U|, |E|.
 *    dist NULL or (batch,2,K+1,K+1) fp64: dist[b][c][i][j] = sum over E of (v_i - v_j)^2, in the difference form; the full matrix, the
 *      diagonal an exact 0, [i][j] and [j][i] equal bit for bit.
 *    vario NULL or (batch,2,offsets,4) fp64, the variogram of order 0.5: for offset (dh, dw) over the ordered pairs p = (h, w) in E,
 *      q = (h + dh, (w + dw) mod width) in E with 0 <= h + dh < height (azimuth wraps, elevation does not), with
 *      a = sqrt|v_K at p - v_K at q| and m = (1/K) sum_k sqrt|v_k at p - v_k at q| (members added in member order, IEEE fp64 sqrt):
 *      the number of pairs, sum (a - m)^2, sum a^2, sum m^2.
 *    offsets_hw: a HOST pointer to (offsets,2) int32 (dh, dw), read before the call returns.  A part whose pointer is NULL is skipped.
 *    No float atomics: per-block partials are added in index order by a second kernel, their number depends on (height, width) alone --
 *    the same bits on every call, a scan's numbers do not depend on the batch.  The order in which pixels enter dist[i][j] does not
 *    depend on (i, j): permuting the members permutes the rows and columns of dist bit for bit (vario is not promised to be invariant).
 *    scratch: the bytes the _scratch_bytes function returns (0 for an empty or oversized problem); scratch, counts, dist and vario 8-byte
 *    aligned, the fp32 pointers as for r2dm_ensemble_score.  Limits: batch <= 65535, 1 <= members <= 64, height, width >= 1,
 *    height * width < 2^31, 0 <= offsets <= 16, every offset with |dh| < height, |dw| < width and not both 0, samples of at most 2^40
 *    elements. */
size_t r2dm_ensemble_coherence_scratch_bytes(int32_t batch, int32_t members, int32_t height, int32_t width, int32_t offsets);
int r2dm_ensemble_coherence(const float* samples, const float* target, const float* known, float lo, float hi, int32_t batch, int32_t members,
                            int32_t height, int32_t width, const int32_t* offsets_hw, int32_t offsets, void* scratch, double* counts,
                            double* dist, double* vario, void* stream);
size_t r2dm_ensemble_score_scratch_bytes(int32_t batch, int32_t members, int64_t plane);
int r2dm_ensemble_score(const float* samples, const float* target, const float* known, float lo, float hi, int32_t batch, int32_t members,
                        int64_t plane, void* scratch, double* raw, double* member, int64_t* rank, float* maps, void* stream);
size_t r2dm_completion_error_scratch_bytes(int32_t batch, int64_t plane);
int r2dm_completion_error(const float* pred, const float* target, const float* known, float lo, float hi, int32_t batch, int64_t plane,
                          void* scratch, double* out, void* stream);
int r2dm_confusion_matrix(const int64_t* pred, const int64_t* target, const float* mask, int32_t batch, int64_t pixels, int32_t classes,
                          int64_t* counts, int64_t* bad, void* stream);
int r2dm_fill_beams(const float* x, const uint8_t* rows, float* out, int32_t batch, int32_t channels, int32_t height, int32_t width,
                    float nodata, int32_t mode, void* stream);

/* -- geometry metrics: nearest neighbours between point clouds, the search behind Chamfer distance, F-score and COV / MMD / 1-NNA (the
 *    reference has no code for them) ------------------------------------------------------------------------------------------------------
 * r2dm_nn_pairs: a (a_total,4), b (b_total,4) fp32 rows [x, y, z, .] (16-byte aligned; the fourth value is not read) hold a_clouds /
 *    b_clouds clouds, cloud k = rows [offsets[k], offsets[k+1]) (int64, clouds + 1 values, in device memory like everything here).
 *    pairs (num_pairs,2) int64 [ia, ib].  For every pair and both directions (a -> b: every point of cloud ia against cloud ib; b -> a
 *    the reverse) the squared distance to the nearest neighbour, d^2 = (ax-bx)^2 + (ay-by)^2 + (az-bz)^2 evaluated in fp32 in this
 *    difference form (dx*dx, then two FMAs; never |a|^2 + |b|^2 - 2ab), and the neighbour's index inside its cloud, the lowest one on an
 *    exact fp32 tie; against an empty cloud +inf and -1.
 *    d2_ab / d2_ba: NULL or one fp32 per point of the pair's query cloud, pair p's values starting at out_ab[p] / out_ba[p] (int64,
 *    num_pairs values; the caller sizes the buffers as the sum of the query counts); idx_ab / idx_ba: NULL or int32 alike (only with d2).
 *    sums (num_pairs,8) fp64 = [sum d^2, sum d, #{d <= tau}] of a -> b, the same of b -> a, |cloud ia|, |cloud ib|; d = sqrt(d^2) in
 *    fp64, d <= tau tested as d^2 <= tau^2 in fp64.  Sums are fp64 in a fixed order (per-block partials added in order by a second
 *    kernel, no floating-point atomics): bit-reproducible, and a pair's numbers do not depend on the other pairs of the call.
 *    status (2) int64, zeroed by the call: [0] points with a non-finite coordinate met as a query (their results are not valid),
 *    [1] pairs whose index is outside [0, clouds) or whose offsets are not 0 <= begin <= end <= total with end - begin <= max_points
 *    (nothing is read through them; their eight sums are NaN).
 *    max_points: an upper bound of the points of any cloud of a pair, 1 to 2^21; it sizes the grid (2 num_pairs x ceil(max_points / 1024)
 *    blocks, at most 2^31 - 1) and the scratch (the bytes the _scratch_bytes function returns; 0 for an empty or oversized problem),
 *    8-byte aligned like sums and status. */
size_t r2dm_nn_pairs_scratch_bytes(int64_t num_pairs, int64_t max_points);
int r2dm_nn_pairs(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                  int64_t b_clouds, int64_t b_total, const int64_t* pairs, int64_t num_pairs, int64_t max_points, double tau, float* d2_ab,
                  int32_t* idx_ab, const int64_t* out_ab, float* d2_ba, int32_t* idx_ba, const int64_t* out_ba, void* scratch, double* sums,
                  int64_t* status, void* stream);

/* -- voxel occupancy: which cells of a grid clouds occupy -- voxel IoU / precision / recall / F1 of a pair of clouds, and the occupancy scores of
 *    an ensemble of K clouds against a target (the reference has no code for them) -----------------------------------------------------------
 * r2dm_voxel_occupancy: clouds as for r2dm_nn_pairs; a holds the member clouds, b the target clouds (they may be one allocation).
 *    The voxel of a point (x, y, z) at size s is (floor(x / s), floor(y / s), floor(z / s)), each quotient an IEEE round-to-nearest fp32
 *    division (never a reciprocal multiply: it would move points on a cell face); the grid is axis-aligned and anchored at the origin.
 *    A point counts if its three coordinates are finite and every floor(q) lies in [-2^20, 2^20), compared in floating point; the others
 *    are not inserted and are counted in status.
 *    A group g is the target cloud targets[g] (int64 index into b) and the K member clouds members[g][0..K) (int64 indices into a; a cloud
 *    may serve any number of groups).  With V(X) the set of voxels of cloud X, o(v) = [v in V(T)], c(v) = #{k: v in V(M_k)} and U the union
 *    of the K + 1 sets, per group and size, int64, zeroed by the call:
 *      member_out (G,S,K,2)   = |V(M_k)|, |V(M_k) n V(T)|
 *      hist_out   (G,S,2,K+1) = #{v in U: o(v) = o, c(v) = c}    ([0][0] is 0)
 *    A pair of clouds is K = 1: hist[1][1] the intersection, hist[0][1] the voxels of the member alone, hist[1][0] of the target alone.
 *    Only integers are summed, by integer atomics: the outputs do not depend on the order of the points or on the schedule, bit for bit.
 *    sizes: S HOST floats, each finite and > 0; 1 <= S <= 8.  1 <= K <= 63 (a voxel's membership mask has 64 bits, bit 63 the target's).
 *    max_group_points: an upper bound of the points of any group, target and members together, 1 to 2^27.  Per (group, size) the call keeps
 *    an open-addressing hash set of 63-bit voxel keys with one membership mask per slot in scratch, of capacity = the power of two
 *    >= 2 * max_group_points (a load factor of at most 0.5 whatever the data): r2dm_voxel_occupancy_scratch_bytes = 16 * groups * sizes *
 *    capacity + 8 * groups rounded up to 16 bytes; 0 for an empty problem or one beyond the limits (groups <= 65535, groups * sizes *
 *    capacity <= 2^36 slots).  scratch, a and b are 16-byte aligned, everything else 8-byte aligned.
 *    status (4) int64, zeroed by the call: [0] points with a non-finite coordinate (once per group they are part of), [1] points outside
 *    the grid (once per group and size), [2] groups with a cloud index outside [0, clouds), offsets that are not 0 <= begin <= end <=
 *    total, or more than max_group_points points (nothing is read through them, their outputs stay 0), [3] inserts that found no slot
 *    (cannot happen at this load factor: the probe loop is bounded so that a defect shows as a status and not as a hang).
 *    Nothing is allocated, nothing synchronises. */
size_t r2dm_voxel_occupancy_scratch_bytes(int64_t groups, int64_t sizes, int64_t max_group_points);
int r2dm_voxel_occupancy(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                         int64_t b_clouds, int64_t b_total, const int64_t* members, const int64_t* targets, int64_t groups, int64_t num_members,
                         const float* sizes, int64_t num_sizes, int64_t max_group_points, void* scratch, int64_t* member_out, int64_t* hist_out,
                         int64_t* status, void* stream);

/* -- earth mover's distance between clouds of equal size (the reference has no code for it) ------------------------------------------------
 * r2dm_emd_pairs: clouds and pairs as for r2dm_nn_pairs.  For a pair of clouds A, B of n points each,
 *    EMD = (1/n) min over permutations s of sum_i |a_i - b_s(i)| (Euclidean, metres).  The solver is a forward auction with
 *    epsilon-scaling (Jacobi rounds, one workgroup per pair, costs c = sqrt(d^2) in fp32 with d^2 in the difference form above); it does
 *    not promise the minimum.  Per pair, out (num_pairs,4) fp64 = [emd, lower, rounds, converged]: emd the true cost of the returned
 *    permutation, lower = (1/n) (sum_i min_j (c_ij + p_j) - sum_j p_j) from the final prices p, a lower bound of EMD for any p (weak
 *    duality), both summed in fp64 in a fixed order from sqrt in fp64 of the fp32 d^2: lower <= EMD <= emd, and in exact arithmetic
 *    emd - lower <= eps.  Bit-reproducible; a pair's numbers do not depend on the other pairs of the call.
 *    eps: the bid increment of the last phase, metres per point; finite, > 0 and a normal fp32 number.  A pair with
 *    eps < 2^-18 * (diagonal of the two clouds' joint bounding box) is refused on the device: an increment could vanish in fp32.
 *    max_rounds >= 1: bidding rounds of a pair over all phases; a pair that needs more ends with converged = 0.
 *    assignment: NULL or (num_pairs, max_points) int32, s(i) for i < n and -1 beyond; prices: NULL or fp32 alike, p_j and NaN beyond.
 *    A pair that ends without an answer has emd = lower = NaN, converged = 0, assignment -1 and prices NaN throughout, and rounds = 0,
 *    or max_rounds at the round cap.  scratch: num_pairs int64 (r2dm_emd_pairs_scratch_bytes; 0 for an empty or oversized problem),
 *    per pair the code 0 = solved, 1..5 = the reasons below.  status (5) int64, zeroed by the call, counts the pairs per reason:
 *    [0] an index outside [0, clouds), offsets that are not 0 <= begin <= end <= total, more than max_points points, or n = 0;
 *    [1] the two clouds differ in size; [2] a non-finite coordinate (or a bounding box whose diagonal overflows fp32); [3] eps below
 *    its floor; [4] the round cap.  Nothing is read through an index or offset that does not check out.
 *    max_points: 1 to r2dm_emd_max_points() = 3072 (48 bytes of LDS per point).  Nothing is allocated, nothing synchronises. */
int64_t r2dm_emd_max_points(void);
size_t r2dm_emd_pairs_scratch_bytes(int64_t num_pairs, int64_t max_points);
int r2dm_emd_pairs(const float* a, const int64_t* a_offsets, int64_t a_clouds, int64_t a_total, const float* b, const int64_t* b_offsets,
                   int64_t b_clouds, int64_t b_total, const int64_t* pairs, int64_t num_pairs, int64_t max_points, double eps, int64_t max_rounds,
                   int32_t* assignment, float* prices, double* out, void* scratch, int64_t* status, void* stream);

/* -- single kernels, exported for per-op parity tests against the oracle -------------------- */
/* ops.Conv2d(ring) 3x3 / 1x1 (models/ops.py:149-173) with optional fused GroupNorm-affine(+SiLU)
 * prologue (aff: (B,Cin,2) or NULL; prologue 0 none, 1 affine, 2 affine+SiLU) and optional
 * residual-add + scale epilogue.  w is OIHW; w_packed is caller scratch of r2dm_conv_packed_elems(). */
int64_t r2dm_conv_packed_elems(int32_t cout, int32_t cin, int32_t ksize, int32_t batch, int32_t height,
                               int32_t width);
int r2dm_conv2d_ring(const float* x, const float* w, const float* bias, float* w_packed, const float* aff,
                     int32_t prologue, const float* residual, const float* scale, float* y, int32_t batch,
                     int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t ksize, void* stream);
/* The same launch (same selection, packing and test hooks) with the fields that otherwise only the engine's walk sets:
 *   x1, c1         second input allocation holding the LAST c1 of the cin channels (x then holds the first cin - c1): the up path's concat without
 *                  a copy; c1 = 0 and x1 = NULL: one source
 *   res_broadcast  1: residual is ONE (cout, H, W) map added to every sample
 *   stat           fused GroupNorm statistics of y: (batch, stat_groups, r2dm_conv_stat_slots(height, width), 2) doubles [sum, sum of squares];
 *                  this launch writes groups [stat_goff, stat_goff + cout / stat_cpg) of stat_cpg = 8 | 16 | 32 | 64 channels; NULL: none
 *   range          device int[2]: [1] takes the running maximum of a bound on |y| as float bits -- the exact max|y|, except from conv_f16x2.hip,
 *                  which records sqrt(largest four-pixel energy) (1 + 1e-6): max|y| <= bound <= 2 max|y|; NULL: no record
 *   reverse        1: descending tile walk (conv_f16x2.hip, proj_f16x2.hip)
 *   chosen         HOST int32[3] (or NULL) <- algorithm (ConvAlgo), output channels per tile, image rows per tile of the selected kernel
 * Returns 1 -- before anything is launched or written -- for every combination the selected kernel would refuse, ignore, or that would leave the
 * sink: statistics from a kernel that emits none (the 32-channel fp32 tile, the few-output direct kernel) or for groups that do not fit; x1 / range
 * on the direct kernels; a concat seam off the kernel's chunk boundary; reverse on a kernel without the descending walk; c1 outside [0, cin). */
int32_t r2dm_conv_stat_slots(int32_t height, int32_t width);
int r2dm_conv2d_ring_ex(const float* x, const float* x1, int32_t c1, const float* w, const float* bias, float* w_packed, const float* aff,
                        int32_t prologue, const float* residual, int32_t res_broadcast, const float* scale, float* y, double* stat,
                        int32_t stat_groups, int32_t stat_goff, int32_t stat_cpg, int32_t* range, int32_t reverse, int32_t* chosen, int32_t batch,
                        int32_t cin, int32_t cout, int32_t height, int32_t width, int32_t ksize, void* stream);
/* nn.GroupNorm / AdaGN statistics folded to y = x*a + d (models/efficient_unet.py:72; ops.py:176-200).
 * gamma/beta (C,) or NULL; ada (B,2C) [scale|shift] or NULL; partial: scratch of
 * r2dm_group_norm_scratch_bytes(); aff out (B,C,2); stats out (B,G,2) mean/rstd or NULL. */
size_t r2dm_group_norm_scratch_bytes(int32_t batch, int32_t groups);
int r2dm_group_norm_affine(const float* x, const float* gamma, const float* beta, const float* ada, void* scratch,
                           float* aff, float* stats, int32_t batch, int32_t channels, int32_t height,
                           int32_t width, int32_t groups, float eps, void* stream);
int r2dm_affine_act(const float* x, const float* aff, float* y, int32_t batch, int32_t channels, int64_t hw,
                    int32_t silu, void* stream);
/* The same fold from a statistics sink the producers' epilogues filled -- stat: (B, groups, slots, 2) doubles [sum, sum of squares], every slot written --
 * i.e. the finalize kernel of the engine's walk alone (the consumer-side fold of conv_f16x2.hip repeats its arithmetic bit for bit); no range flag.
 * Kernel-level test hook, like r2dm_affine_act. */
int r2dm_group_norm_from_stats(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, float* aff, float* stats,
                               int32_t batch, int32_t channels, int32_t height, int32_t width, int32_t groups, float eps, void* stream);
/* ops.Resample(down=2) / (up=2) (models/ops.py:52-146) */
int r2dm_fir_down2(const float* x, float* y, int32_t batch, int32_t channels, int32_t height, int32_t width,
                   void* stream);
int r2dm_fir_up2(const float* x, float* y, int32_t batch, int32_t channels, int32_t height, int32_t width,
                 void* stream);
/* ops.Resample(down=2) that also leaves the GroupNorm statistics of its OUTPUT (nn.GroupNorm(groups, C) behind it:
 * models/efficient_unet.py:95-97 behind :135) in the convolution epilogues' slot grid -- stat: (B, groups, slots, 2) doubles
 * [sum, sum of squares], slots = r2dm_fir_down2_stat_slots() (0: geometry not supported, call r2dm_fir_down2); every slot is
 * written, the sums of a (sample, group) over ALL its slots are the group's moments.  Kernel-level test hook of the engine's path. */
int32_t r2dm_fir_down2_stat_slots(int32_t channels, int32_t groups, int32_t height, int32_t width);
int r2dm_fir_down2_stats(const float* x, float* y, double* stat, int32_t batch, int32_t channels, int32_t groups,
                         int32_t height, int32_t width, void* stream);
/* The down stages' Conv3x3(ring) + ops.Resample(down=2) (models/efficient_unet.py:132-136) with the FIR FIRST: r2dm_down_planes writes the nine
 * filtered planes per channel the stride-2 convolution reads -- planes: (B, 9 C, H/2, W/2), plane (ky 3 + kx) C + c; height % 4 == 0,
 * width % 8 == 0 --, r2dm_down_gemm runs that pass and the (Cout, 9 Cin) product with the bias scaled by the FIR's row factor (7/8 on the first
 * and last output row): y (B, Cout, H/2, W/2) = Resample(down=2)(Conv2d(x, w, bias)).  w is OIHW; w_packed: caller scratch of 9 cin cout + 64 floats;
 * planes: caller scratch of B 9 cin (H/2) (W/2) floats; cin % 32 == 0, cout % 64 == 0, height % 8 == 0, width % 128 == 0.  stat (optional): the
 * GroupNorm statistics of y in the convolution epilogues' slot grid, (B, groups, r2dm_down_gemm_stat_slots(), 2) doubles (0 slots: not available).
 * More than half of the nine planes are copies of each other (kx = 0 is kx = 2 one column to the left; V[2][i] = V[0][i + 1] away from the border rows):
 * r2dm_down_phase_planes writes every distinct plane once -- planes: (B, 2 phases [kx = 2 | kx = 1], C, H + 3 rows, W/2 + 4), r2dm_down_phase_planes_floats(C, H, W)
 * floats per sample; a channel's rows are V[0][0 .. H/2), V[1][0 .. H/2), V[2][0], V[2][H/2 - 2], V[2][H/2 - 1]; a row's column j is at float 4 + j and float 3 of a
 * phase-0 row holds column W/2 - 1 -- and r2dm_down_gemm runs that pass and maps the nine taps onto it in its loader.  r2dm_down_gemm_nine runs the product over all
 * nine planes (r2dm_down_planes' pass): the same bits.  Both take `planes` sized for nine.
 * The engine takes the pair in the default precision; R2DM_DOWN_GEMM (read at r2dm_create): 1 (default) = the phase planes, 9 = all nine planes, 0 = Conv3x3 +
 * fir_down2. */
int r2dm_down_planes(const float* x, float* planes, int32_t batch, int32_t channels, int32_t height, int32_t width, void* stream);
int r2dm_down_phase_planes(const float* x, float* planes, int32_t batch, int32_t channels, int32_t height, int32_t width, void* stream);
int64_t r2dm_down_phase_planes_floats(int32_t channels, int32_t height, int32_t width); /* per sample; 0: geometry not supported */
int r2dm_down_gemm_nine(const float* x, const float* w, const float* bias, float* w_packed, float* planes, float* y, double* stat,
                        int32_t batch, int32_t cin, int32_t cout, int32_t groups, int32_t height, int32_t width, void* stream);
int32_t r2dm_down_gemm_stat_slots(int32_t cin, int32_t cout, int32_t groups, int32_t height, int32_t width);
int r2dm_down_gemm(const float* x, const float* w, const float* bias, float* w_packed, float* planes, float* y, double* stat,
                   int32_t batch, int32_t cin, int32_t cout, int32_t groups, int32_t height, int32_t width, void* stream);
/* The range guard's other producers, one kernel (or the streaming pair) each with the record the engine's walk gives them -- range: device int32[2] or NULL,
 * [1] takes the running maximum as float bits (positive floats order like their bit patterns, a NaN above all), [0] is never written.  Everything else is the
 * entry of the same name without _ex (R2DM_TEST_IO16 and R2DM_FIR_UP_WIDE included), whose outputs the record does not change:
 *   r2dm_group_norm_affine_ex      the bound of gn_bound (csrc/gn_math.h) on |a x + d| with M = the exact max|x| of each group (the streaming pass records it)
 *   r2dm_group_norm_from_stats_ex  the same bound with M = sqrt(largest slot energy) (1 + 1e-6) of each group
 *   r2dm_fir_up2_ex                max|y| of the values as STORED (an fp16 store that overflows records +inf)
 *   r2dm_down_planes_ex, r2dm_down_phase_planes_ex  max|plane value| (the maximum over the distinct planes is the maximum over all nine: the same bits)
 * Kernel-level test hooks (tests/test_hip_range_producers.py). */
int r2dm_group_norm_affine_ex(const float* x, const float* gamma, const float* beta, const float* ada, void* scratch, float* aff, float* stats, int32_t batch,
                              int32_t channels, int32_t height, int32_t width, int32_t groups, float eps, void* stream, int32_t* range);
int r2dm_group_norm_from_stats_ex(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, float* aff, float* stats,
                                  int32_t batch, int32_t channels, int32_t height, int32_t width, int32_t groups, float eps, void* stream, int32_t* range);
/* r2dm_group_norm_from_stats_ex with the AdaGN rows where the engine has them: sample b's [scale(C) | shift(C)] at ada + b ada_stride (the packed
 * (B, ada_rows) output of the projection launch; _ex is ada_stride = 2 C).  Returns 1 for ada with ada_stride < 2 C. */
int r2dm_group_norm_from_stats_strided(const double* stat, int32_t slots, const float* gamma, const float* beta, const float* ada, int64_t ada_stride, float* aff,
                                       float* stats, int32_t batch, int32_t channels, int32_t height, int32_t width, int32_t groups, float eps, void* stream,
                                       int32_t* range);
int r2dm_fir_up2_ex(const float* x, float* y, int32_t batch, int32_t channels, int32_t height, int32_t width, void* stream, int32_t* range);
int r2dm_down_planes_ex(const float* x, float* planes, int32_t batch, int32_t channels, int32_t height, int32_t width, void* stream, int32_t* range);
int r2dm_down_phase_planes_ex(const float* x, float* planes, int32_t batch, int32_t channels, int32_t height, int32_t width, void* stream, int32_t* range);
/* attention core of nn.MultiheadAttention on channel-major qkv (B,3C,N) -> (B,C,N)
 * (models/efficient_unet.py:34-38,46) */
int r2dm_attention(const float* qkv, float* out, int32_t batch, int32_t channels, int32_t heads, int32_t tokens,
                   void* stream);
/* time embedding: cond (B,) -> SiLU(time_embedding(cond)) (B,T)  (models/efficient_unet.py:232-237);
 * hidden: (B,T) scratch */
int r2dm_time_embedding(const float* cond, const float* freqs, const float* w1, const float* b1, const float* w2,
                        const float* b2, float* act, float* hidden, int32_t batch, int32_t base, int32_t temb,
                        void* stream);
/* all AdaGN projections of one forward in one launch (models/ops.py:190-200: Linear(SiLU(temb), 2C) of every residual block, packed row-wise):
 * out (B, rows) = act (B, T) w^T (rows, T) + bias (rows,), fp64 accumulation.  Returns 1 for a null pointer, batch, temb or rows < 1, and -- the
 * kernel loads 16 bytes at a time where temb % 256 == 0 -- for an act or w that is not 16-byte aligned then.  Kernel-level test hook. */
int r2dm_ada_proj(const float* act, const float* w, const float* bias, float* out, int32_t batch, int32_t temb, int32_t rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* R2DM_HIP_H */
