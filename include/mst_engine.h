/* mst_engine.h -- C ABI of the MI355X denoising engine (libmst_engine.so).
 *
 * The reference (hlcdyy/diffusion-based-motion-style-transfer) is 100 % Python and has no
 * FFI/operator interface of its own, so nothing here mirrors an existing
 * binding; each entry point instead REPLACES a group of reference Python functions, cited per
 * function below as file:line under the reference root.  The library is called only from the
 * boundary package (diffusion-based-motion-style-transfer_amd/_native.py via ctypes), never from
 * user scripts.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; mst_last_error() then returns a
 *     thread-local, NUL-terminated description.
 *   - all pointers named *_dev are device (HBM) pointers owned by the caller (PyTorch tensors);
 *     *_host are host pointers.  The engine owns only its weights copy and workspace.
 *   - all work is enqueued on the hipStream_t passed as `void* stream` (NULL = default stream)
 *     and is stream-ordered; one host thread per handle.
 *   - tensors use the reference's layouts: clips are float32 [B, F, 1, T] (F = njoints*nfeats,
 *     T contiguous), timesteps are int64 [B].
 */
#ifndef MST_ENGINE_H
#define MST_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mst_engine mst_engine;     /* one MDM-shaped denoiser (weights + workspace)     */
typedef struct mst_schedule mst_schedule; /* one (possibly respaced) diffusion process' tables */

typedef struct mst_config {
    int32_t feats;       /* F = njoints * nfeats, e.g. 263 (humanml), 181 (stylexia), 190 (bandai) */
    int32_t max_frames;  /* largest T the engine must accept (<= 223; tokens S = T + 1)            */
    int32_t max_rows;    /* largest number of clips through the transformer at once
                            (= 2 * batch under classifier-free guidance)                           */
    int32_t latent_dim;  /* must be 512  (utils/parser_util.py default; model_util.py:160-167)     */
    int32_t num_heads;   /* must be 4    (hard-coded in utils/model_util.py:160-167)               */
    int32_t ff_size;     /* must be 1024 (same)                                                    */
    int32_t num_layers;  /* 1..16 (default 8)                                                      */
    int32_t clip_dim;    /* width of the text embedding, 512                                       */
    int32_t pe_len;      /* rows of the positional table (5000, mdm_forstyledataset.py:388)        */
    int32_t device;      /* HIP device ordinal                                                     */
} mst_config;

/* -------------------------------------------------------------------------------------------
 * lifetime
 * ----------------------------------------------------------------------------------------- */
const char* mst_last_error(void);
int  mst_version(void);
const char* mst_source_hash(void);   /* hash of csrc/ + this header the library was compiled from (stale-build check) */
int  mst_engine_create(const mst_config* cfg, mst_engine** out);
void mst_engine_destroy(mst_engine* e);

/* Copy one parameter (float32, device memory) into the engine, converting dense matrices to the
 * engine's padded f16 operand layout.  `name` is the key of the tensor in an MDM state dict
 * (model/mdm_forstyledataset.py:183-270), i.e. the reference checkpoint layout:
 *   seqTransEncoder.layers.{i}.self_attn.in_proj_weight [1536,512] / in_proj_bias
 *   seqTransEncoder.layers.{i}.self_attn.out_proj.weight [512,512] / .bias
 *   seqTransEncoder.layers.{i}.linear1.weight [1024,512] / .bias, linear2.weight [512,1024] / .bias
 *   seqTransEncoder.layers.{i}.norm1.weight/.bias, norm2.weight/.bias
 *   input_process.poseEmbedding.weight [512,F] / .bias      (InputProcess  :425-449)
 *   output_process.poseFinal.weight   [F,512] / .bias       (OutputProcess :452-478)
 *   embed_timestep.time_embed.0.weight/.bias, .2.weight/.bias (TimestepEmbedder :408-422)
 *   embed_text.weight [512,clip_dim] / .bias                (:258)
 *   sequence_pos_encoder.pe [pe_len,512]                    (PositionalEncoding :387-404)
 * For StyleDiffusion the caller passes its own `seqTransEncoder.*` tensors and the frozen prior's
 * (`motion_enc.mdm_model.*`) projections, which is exactly what StyleDiffusion.forward (:602-625)
 * reads.  Replaces: nn.Module.load_state_dict / .to(device) for this path.
 * Stream contract: the f16 copies are written on `stream`.  The fused kernels' pre-packed copies (fragment streams of W_in and of
 * W_out | W1 | W2) are produced lazily on the stream of the FIRST mst_forward / mst_sample_loop after an upload (for a loop: the
 * engine's loop stream, which is ordered behind the caller's stream); a caller that uploads on one stream and samples on another
 * orders the two itself, exactly as for the plain copies. */
int mst_load_weight(mst_engine* e, const char* name, const float* src_dev,
                    const int64_t* shape, int32_t ndim, void* stream);
/* The 12 tensors of EVERY encoder layer in one call (one launch per 8 layers): srcs_host_array = num_layers x 12 device pointers, per
 * layer in the order in_proj_weight, in_proj_bias, out_proj.weight, out_proj.bias, linear1.weight, linear1.bias, linear2.weight,
 * linear2.bias, norm1.weight, norm1.bias, norm2.weight, norm2.bias.  Same result as the 12 x num_layers mst_load_weight calls; what
 * a fine-tune iteration does after every optimizer step (train/training_loop.py:297-303 updates all 96).  Not in precise mode. */
int mst_load_layers(mst_engine* e, const float* const* srcs_host_array, void* stream);
/* 0 when every tensor of the list above has been loaded. */
int mst_weights_complete(const mst_engine* e);

/* -------------------------------------------------------------------------------------------
 * schedule: replaces GaussianDiffusion.__init__'s tables as consumed through
 * _extract_into_tensor (diffusion/gaussian_diffusion.py:183-219, :1605-1618) and
 * _WrappedModel's timestep_map (diffusion/respace.py:129-134).
 * `tables_host` is float32 [MST_NTAB][num_steps] in the order of mst_table below: the float64
 * numpy tables cast to float32, exactly what `.float()` at gaussian_diffusion.py:1615 yields.
 * ----------------------------------------------------------------------------------------- */
enum mst_table {
    MST_TAB_SQRT_AC = 0,        /* sqrt_alphas_cumprod                */
    MST_TAB_SQRT_1M_AC = 1,     /* sqrt_one_minus_alphas_cumprod      */
    MST_TAB_COEF1 = 2,          /* posterior_mean_coef1               */
    MST_TAB_COEF2 = 3,          /* posterior_mean_coef2               */
    MST_TAB_LOGVAR = 4,         /* log-variance of the configured var type
                                   (FIXED_SMALL: posterior_log_variance_clipped) */
    MST_TAB_SQRT_RECIP_AC = 5,  /* sqrt_recip_alphas_cumprod          */
    MST_TAB_SQRT_RECIPM1_AC = 6,/* sqrt_recipm1_alphas_cumprod        */
    MST_TAB_AC = 7,             /* alphas_cumprod                     */
    MST_TAB_AC_PREV = 8,        /* alphas_cumprod_prev                */
    MST_NTAB = 9
};
int  mst_schedule_create(int32_t num_steps, const float* tables_host,
                         const int32_t* timestep_map_host, int32_t device, mst_schedule** out);
void mst_schedule_destroy(mst_schedule* s);
/* The variance row of the schedule, float32 [num_steps] on the host: p_mean_var["variance"] of p_mean_variance
 * (gaussian_diffusion.py:366-385) -- posterior_variance for FIXED_SMALL (exactly 0 at index 0), append(posterior_variance[1],
 * betas[1:]) for FIXED_LARGE.  It is NOT exp(MST_TAB_LOGVAR).  Only condition_mean reads it (:463-467: mean += variance * gradient),
 * so only a guided MST_SAMPLER_DDPM step needs it, and such a step on a schedule without the row is refused by name.  An entry of
 * its own: mst_schedule_create's signature and the MST_TAB_* layout are unchanged. */
int  mst_schedule_set_variance(mst_schedule* s, const float* variance_host);

/* -------------------------------------------------------------------------------------------
 * conditioning: replaces embed_text(mask_cond(encode_text(...))) of StyleDiffusion.forward
 * (:611-615, :592-600) / MDM.forward (:324-327).  CLIP itself stays outside; `text_emb_dev` is its
 * float32 [batch, clip_dim] output.  keep_dev (float32 [batch], may be NULL = all ones) is the
 * cond mask: 0 drops the text embedding of that clip (y['uncond'] / the Bernoulli mask).
 * With cfg != 0 the engine prepares a doubled batch: rows [0,batch) conditional, rows
 * [batch, 2*batch) unconditional (model/cfg_sampler.py:36-43).  The projection is constant over a
 * sampling loop, so it is computed here once instead of once per step.
 * ----------------------------------------------------------------------------------------- */
int mst_set_text(mst_engine* e, const float* text_emb_dev, const float* keep_dev,
                 int32_t batch, int32_t cfg, void* stream);
/* The training-mode mask_cond (model/mdm_forstyledataset.py:288-296 / :592-600: `cond * (1. - bernoulli(ones(bs) * p))`) with the
 * mask handed over as drawn: drop_dev float32 [batch], 1 = the clip's text embedding is dropped.  Same projection, one
 * elementwise launch less on the caller's side than masking first and calling mst_set_text. */
int mst_set_text_dropped(mst_engine* e, const float* text_emb_dev, const float* drop_dev, int32_t batch, void* stream);

/* -------------------------------------------------------------------------------------------
 * one model evaluation: replaces StyleDiffusion.forward / MDM.forward (:602-625, :315-364) and,
 * with cfg != 0, ClassifierFreeSampleModel.forward (model/cfg_sampler.py:36-43).
 *   x_dev      float32 [batch, F, 1, frames]
 *   t_dev      int64 [batch] ORIGINAL-process timesteps (after timestep_map)
 *   scale_dev  float32 [batch] guidance scale (cfg only)
 *   out_dev    float32 [batch, F, 1, frames]
 * mst_set_text must have been called for this batch/cfg.
 * ----------------------------------------------------------------------------------------- */
int mst_forward(mst_engine* e, const float* x_dev, const int64_t* t_dev, const float* scale_dev,
                int32_t batch, int32_t frames, int32_t cfg, float* out_dev, void* stream);

/* -------------------------------------------------------------------------------------------
 * sampling loop / single step: replaces p_sample_loop(_progressive), ddim_sample_loop
 * (_progressive) (diffusion/gaussian_diffusion.py:644-794, :948-1082) with p_mean_variance
 * (:311-424), p_sample (:532-585 / inpainting_gaussian_diffusion.py:25-64) and ddim_sample
 * (inpainting_gaussian_diffusion.py:125-177) fused into the output-projection kernel.
 * Runs diffusion indices t_start, t_start-1, ..., t_end (t_start == t_end: one step).
 * ----------------------------------------------------------------------------------------- */
/* MST_SAMPLER_DDIM_REVERSE: ddim_reverse_sample (gaussian_diffusion.py:910-946), x_t -> x_{t+1}, the deterministic DDIM step run
 * upward (DDIM inversion).  Its index range is inclusive and ASCENDING, 0 <= t_start <= t_end <= n - 1: the loop visits t_start,
 * t_start + 1, ..., t_end and leaves x at index t_end + 1.  eta must be 0 ("Reverse ODE only for deterministic path", :923).  The
 * step has no noise term: noise_mode, seed and mask_noise are ignored and noise_dev may be NULL.  alphas_cumprod_next[t] (:193) is
 * read as MST_TAB alphas_cumprod[t + 1], and 0 at t == n - 1: the schedule's table layout is unchanged. */
/* MST_SAMPLER_PLMS: plms_sample (gaussian_diffusion.py:1084-1166), Pseudo Linear Multistep of order 1..4.  It carries a history of
 * up to three earlier epsilons between steps, so it has an entry point of its own, mst_sample_loop_plms below: mst_sample_loop
 * refuses this id by that name, and mst_step_backward refuses it (the reference has no `_with_grad` form of plms_sample). */
enum { MST_SAMPLER_DDPM = 0, MST_SAMPLER_DDIM = 1, MST_SAMPLER_DDIM_REVERSE = 2, MST_SAMPLER_PLMS = 3 };
enum { MST_NOISE_BUFFER = 0, MST_NOISE_PHILOX = 1 };

typedef struct mst_loop_args {
    int32_t batch;                  /* clips B                                                   */
    int32_t frames;                 /* T                                                         */
    int32_t cfg;                    /* classifier-free guidance: cond/uncond as one 2B batch     */
    int32_t sampler;                /* MST_SAMPLER_*                                             */
    int32_t mask_noise;             /* 1: InpaintingGaussianDiffusion (noise *= 1 - mask)        */
    int32_t clip_denoised;          /* clamp x0-hat to [-1, 1] (callers pass 0)                  */
    int32_t noise_mode;             /* MST_NOISE_*                                               */
    int32_t t_start, t_end;         /* inclusive, t_start >= t_end >= 0 (DDIM_REVERSE: t_start <= t_end) */
    float   eta;                    /* DDIM eta                                                  */
    uint64_t seed;                  /* Philox key (MST_NOISE_PHILOX)                             */
    const float* scale_dev;         /* [B] guidance scale (cfg)                                  */
    const float* inpainting_mask_dev;   /* [B,F,1,T] float32 0/1, or NULL                        */
    const float* inpainted_motion_dev;  /* [B,F,1,T], or NULL (blend needs both)                 */
    const float* noise_dev;         /* MST_NOISE_BUFFER: [nsteps][B,F,1,T], step j at j*B*F*T    */
    float* x_dev;                   /* [B,F,1,T]: x_{t_start} on entry, final sample on exit     */
    float* xstart_dump_dev;         /* optional [nsteps][B,F,1,T]: x0-hat of every step          */
} mst_loop_args;

int mst_sample_loop(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, void* stream);

/* -----------------------------------------------------------------------------------------
 * The PLMS sampler: plms_sample_loop (gaussian_diffusion.py:1168-1279) as native calls.
 * A chain is the sequence of steps that share one history.  Step k of a chain (k = steps_done + the step's position in this call):
 *   k == 0 and order > 1   the Pseudo Improved Euler step: TWO model evaluations, at (x, t) and at (x_mid, t - 1); run from the
 *                          host as two model-output-only passes and two small elementwise kernels, once per chain;
 *   otherwise              the multistep step with cur_order = min(order, k + 1), fused into the output projection like the other
 *                          samplers' steps.  cur_order and the ring slots are read on the device, so one captured graph serves every
 *                          order and every position in a chain.
 * hist_dev is a ring of three fp32 slots [3][B,F,1,T] in caller-owned memory (B rows under CFG too, not 2B): chain step k writes its
 * eps into slot k % 3 and reads the newest earlier ones from slots (k - 1) % 3, (k - 2) % 3, (k - 3) % 3.  (During the Euler step
 * slot 1 holds the chain's original x.)  The history is eps, never eps' or the second evaluation's eps.  It may be NULL for order 1.
 * The index range is descending as for MST_SAMPLER_DDIM.  a->sampler, eta, noise_mode, seed, noise_dev and mask_noise are ignored (the
 * step has no noise term); noise_dev may be NULL.  xstart_dump_dev entry j is the x0-hat of the call's step j (first evaluation).
 * A k-step call equals k one-step calls with steps_done carried forward, bit for bit (x and the ring).
 * Refused, each by name: order outside 1..4; steps_done < 0; hist_dev NULL with order > 1; a chain that STARTS at index 0 with
 * order > 1 -- the reference evaluates the model at t - 1 = -1 there, which silently wraps to the last table entry; this library
 * refuses instead.
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_plms_args {
    int32_t order;                  /* 1..4                                                            */
    int32_t steps_done;             /* chain steps taken by earlier calls; 0 starts a chain            */
    float*  hist_dev;               /* [3][B,F,1,T] float32 eps ring (may be NULL when order == 1)     */
} mst_plms_args;
int mst_sample_loop_plms(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_plms_args* pl, void* stream);


/* -----------------------------------------------------------------------------------------
 * Guided sampling: the `cond_fn` argument of p_sample / ddim_sample and their loops (condition_mean, gaussian_diffusion.py:454-467,
 * called at :577-580 and inpainting_gaussian_diffusion.py:59-62; condition_score, :484-506, called at :821-824 and igd:150-153).
 * g = grad log p(y | x_t), float32 [B,F,1,T] (B rows under CFG too, not 2B), enters the fused step behind the model output:
 *   MST_SAMPLER_DDPM   mean += variance_t g (the row of mst_schedule_set_variance), then the noise term;
 *   MST_SAMPLER_DDIM   eps = (srac x - pred) / srm1ac; eps -= sqrtf(1 - abar_t) g; pred' = srac x - srm1ac eps; eps re-derived from
 *                      pred'; sample = pred' sqrt(abar_prev) + dir eps'' + sigma noise.
 * The x0-hat dump holds the UNGUIDED x0-hat (the reference returns out_orig["pred_xstart"], :847 / igd:177).  Blend, conversion,
 * clip, noise and noise mask are those of mst_sample_loop; so are slices, CFG, style slots, precise mode, graph replay and profiling.
 *   MST_GUIDE_GRADIENT  grad_dev is g for ONE step (a Python cond_fn does not depend on the model output: the caller evaluates
 *                       it on x_t first).  t_start must equal t_end.
 *   MST_GUIDE_TARGET    g = weight[b] mask (a_t target - x_t), computed inside the step kernel from operands that are constant over
 *                       the loop: target_dev [B,F,1,T], mask_dev [B,F,1,T] or NULL (all ones), weight_dev [B]; a_t = 1, or
 *                       MST_TAB_SQRT_AC at the step's index when follow_schedule != 0 (a Gaussian log-likelihood around
 *                       sqrt(abar_t) target: a soft keyframe / trajectory constraint).  A k-step call equals k one-step calls bit
 *                       for bit, and one captured graph serves every step.
 * Refused, each by name: MST_GUIDE_GRADIENT with t_start != t_end; any guide with MST_SAMPLER_DDIM_REVERSE (ddim_reverse_sample
 * has no cond_fn, :910-919) or MST_SAMPLER_PLMS (guided PLMS is not built); a guided MST_SAMPLER_DDPM step on a schedule without the
 * variance row; a NULL grad_dev (gradient kind), target_dev or weight_dev (target kind).
 * ----------------------------------------------------------------------------------------- */
enum { MST_GUIDE_GRADIENT = 1, MST_GUIDE_TARGET = 2 };
typedef struct mst_guide_args {
    int32_t kind;                   /* MST_GUIDE_GRADIENT or MST_GUIDE_TARGET                          */
    int32_t follow_schedule;        /* target kind: a_t = sqrt(abar_t) instead of 1                    */
    const float* grad_dev;          /* gradient kind: [B,F,1,T] float32                                */
    const float* target_dev;        /* target kind: [B,F,1,T] float32                                  */
    const float* mask_dev;          /* target kind: [B,F,1,T] float32, or NULL for all ones            */
    const float* weight_dev;        /* target kind: [B] float32                                        */
} mst_guide_args;
int mst_sample_loop_guided(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_guide_args* g, void* stream);

/* -----------------------------------------------------------------------------------------
 * Clips of any length: overlapping windows, stitched behind every step (csrc/mst_window.h).  No reference counterpart: the reference
 * cuts the content clip at max_frames (sample/demo_style_transfer.py:37-38, :184).  The feature rows are frame-local (root velocities,
 * everything else relative to the root), so rows [s, s + W) of a long clip are the rows of the sub-clip; a long clip [C,F,1,L] is cut
 * into windows [N,F,1,W] of the model's own length, all windows of all clips are sampled as one batch, and after every step the frames
 * that two or more windows share are replaced, in all of them, by one weighted mean.
 * The plan (host arrays, uploaded once by mst_window_plan_create): clip c is clip_len[c] frames long and owns windows
 * clip_win0[c] .. clip_win0[c + 1] - 1 (clip_win0 has clips + 1 entries, 0 .. windows); window n covers long frames
 * win_start[n] .. win_start[n] + window - 1 of its clip.  A clip no longer than the window has one window at 0 (frames from its length
 * on are zero padding).  Refused, each by name: a clip length outside 1 .. long_frames; long_frames above mst_window_max_frames()
 * (4096, what the stages around the sampler take); a clip without a window; starts that are negative or not strictly ascending;
 * start + window > max(length, window); an uncovered frame below the length.
 *   mst_window_unfold   long_dev [C,F,1,L] -> win_dev [N,F,1,W]; window frames at or past the clip's length get 0.0.
 *   mst_window_stitch   win_dev in place.  Per (clip, feature, long frame), K = the covering windows in ascending order: |K| == 1: not
 *                       touched; all of K hold the same bits: kept (inpainted rows stay bit-exact); otherwise
 *                       v = (sum_K h x) / (sum_K h) with h(i) = min(i + 1, W - i) at local frame i, in fp32 in ascending window order,
 *                       stored into every window of K.  long_out_dev != NULL: also the fold, [C,F,1,L] -- the single covering value or
 *                       v below the clip's length, exactly 0.0 from there on.  One thread per element, no atomics.
 *   mst_sample_loop_windows   mst_sample_loop on the N windows with a stitch behind every step: the slice streams join, the stitch runs
 *                       on the loop stream, the slices fork again.  Every step is enqueued from the host and reads x from memory (no graph
 *                       replay, no chained frame rows, no fused embed: each would hand the next step rows the stitch has since changed),
 *                       so an n-step call equals n one-step mst_sample_loop calls with mst_window_stitch between them, bit for bit.
 *                       The last stitch also writes the long clips where mst_window_plan_set_fold has named a buffer (NULL: no fold).
 *                       Refused, each by name: any sampler but MST_SAMPLER_DDIM; eta != 0 (for the deterministic step x_{t-1} is linear
 *                       in x_t and x0-hat, so windows that start from one long x_T hold identical values on shared frames after every
 *                       stitch, and the mean is a mean over x0-hat alone); batch != the plan's windows; frames != the plan's window; a
 *                       plan on another device.  It takes no guide: mst_window_sample_loop does.  It is no implementation of its own:
 *                       the deterministic subset of mst_window_sample_loop, over the same code, with its two refusals in front.
 *   mst_window_noise    extends mst_philox_normal to windows: out_dev [nsteps,N,F,1,W], the layout an MST_NOISE_BUFFER loop reads (step
 *                       j at j * N*F*W).  Entry j = unfold(Z_j), Z_j [C,F,1,L] = mst_philox_normal(C, F, L, seed, step0 + j): element
 *                       (c, f, l) is component l & 3 of the four normals of counter (l >> 2, f, c, step0 + j) under `seed` -- the noise
 *                       is drawn in LONG-clip coordinates, so every window that covers a long frame receives the same bits for it
 *                       (the in-kernel draw is keyed by the window, and the stitch's mean would shrink the variance on shared frames).
 *                       Every element is written; window frames at or past the clip's length get 0.0.  One draw per long quad, no
 *                       atomics.  Refused, each by name: a null plan, a null out, feats < 1, nsteps < 1, more elements than one launch
 *                       takes.
 *   mst_window_sample_loop   extends mst_sample_loop_windows by the noise term and by mst_sample_loop_guided's guide (g may be NULL):
 *                       MST_SAMPLER_DDPM, or MST_SAMPLER_DDIM at any eta.  With noise drawn by mst_window_noise x_{t-1} stays linear
 *                       in (x_t, x0-hat, noise), so the windows still agree on shared frames after every stitch.  The same launch
 *                       sequence as mst_sample_loop_windows (host-enqueued steps, join, stitch, fork), so an n-step call equals n
 *                       one-step mst_sample_loop / mst_sample_loop_guided calls with mst_window_stitch between them, bit for bit.
 *                       Refused, each by name: any other sampler (PLMS and MST_SAMPLER_DDIM_REVERSE over windows are not built);
 *                       MST_NOISE_PHILOX where the step has a noise term (MST_SAMPLER_DDPM, or eta != 0), and a missing noise buffer
 *                       there; batch != the plan's windows; frames != the plan's window; a plan on another device; what
 *                       mst_sample_loop_guided refuses of a guide (MST_GUIDE_GRADIENT: t_start == t_end).
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_window_plan mst_window_plan;
int  mst_window_max_frames(void);
int  mst_window_plan_create(const int32_t* clip_len, const int32_t* clip_win0, const int32_t* win_start, int32_t clips, int32_t windows,
                            int32_t window, int32_t long_frames, int32_t device, mst_window_plan** out);
void mst_window_plan_destroy(mst_window_plan* p);
int  mst_window_plan_set_fold(mst_window_plan* p, float* long_out_dev);
int  mst_window_unfold(const mst_window_plan* p, const float* long_dev, int32_t feats, float* win_dev, void* stream);
int  mst_window_stitch(const mst_window_plan* p, float* win_dev, int32_t feats, float* long_out_dev, void* stream);
int  mst_sample_loop_windows(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_window_plan* p, void* stream);
int  mst_window_noise(const mst_window_plan* p, int32_t feats, uint64_t seed, uint32_t step0, int32_t nsteps, float* out_dev, void* stream);
int  mst_window_sample_loop(mst_engine* e, const mst_schedule* s, const mst_loop_args* a, const mst_window_plan* p,
                            const mst_guide_args* g /* may be NULL */, void* stream);

/* Number of independent clip slices (1..3) mst_sample_loop runs on separate streams for this
 * batch of `frames`-frame clips (frames <= 0: the engine's max_frames; the policy depends on the
 * token-row count, so pass the loop's own frame count when it is below the cap): clips never interact (no cross-sample op in
 * mdm_forstyledataset.py:602-625), so slices overlap each other's launch gaps, prologues and
 * tails.  Chosen per call from the tile count (one slice when every tile of the batch is
 * resident at once, up to three beyond that and on the small-tile path); MST_STREAMS=1..3 in
 * the environment at engine creation fixes it.  Per-launch work = batch / slices clips. */
int mst_loop_slices(const mst_engine* e, int32_t batch, int32_t cfg, int32_t frames);

/* -------------------------------------------------------------------------------------------
 * stand-alone elementwise kernels for callers that bring their own model callable
 * (any nn.Module passed to p_sample / ddim_sample / q_sample):
 *   mst_q_sample        diffusion/gaussian_diffusion.py:267-285,
 *                       diffusion/inpainting_gaussian_diffusion.py:6-23
 *   mst_step_epilogue   gaussian_diffusion.py:341-349 (blend), :387-412 (mean/variance),
 *                       :569-585 / inpainting_gaussian_diffusion.py:51-63 (p_sample),
 *                       inpainting_gaussian_diffusion.py:157-177 (ddim_sample),
 *                       gaussian_diffusion.py:910-946 (ddim_reverse_sample: sampler MST_SAMPLER_DDIM_REVERSE, eta 0,
 *                       noise_dev never read and may be NULL)
 * t_dev is int64 [batch] of indices into the schedule.  sample_out_dev / xstart_out_dev may be NULL.
 *
 * THE CALLER IS TRUSTED.  Every tensor operand of this section (and of mst_step_backward, mst_plms_epilogue / mst_plms_euler below)
 * is read as base + i over batch * per_clip float32 elements, the scale / weight vectors over `batch`: nothing here can see a
 * tensor's shape, and no check that would cost a synchronisation is made.  A broadcastable mask, a one-element scale or a
 * one-clip motion must be expanded to full size BEFORE the call; the Python handles do that (engine.py `_operand`, the table in
 * DESIGN.md section 1, "Drop-in boundary"), other callers owe the same.
 * ----------------------------------------------------------------------------------------- */
int mst_q_sample(const mst_schedule* s, const float* x_start_dev, const float* noise_dev,
                 const float* mask_dev, const int64_t* t_dev, int32_t batch, int64_t per_clip,
                 float* out_dev, void* stream);

int mst_step_epilogue(const mst_schedule* s, const float* model_out_dev, const float* x_dev,
                      const float* noise_dev, const float* mask_dev, const float* motion_dev,
                      const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t sampler,
                      float eta, int32_t mask_noise, int32_t clip_denoised,
                      float* sample_out_dev, float* xstart_out_dev, void* stream);

/* The same step for a model that predicts something else than x_start (enum ModelMeanType, gaussian_diffusion.py:69-76; branch
 * :398-412): mean_type 0 = x_start, 1 = epsilon (x0-hat = sqrt_recip_alphas_cumprod x - sqrt_recipm1_alphas_cumprod out, :426-431),
 * 2 = previous x (x0-hat = out / coef1 - coef2 / coef1 x, :433-441; the posterior mean is then the model output itself, :399-403).
 * As in the reference the inpainting blend (:341-349) acts on the raw model output, in front of the conversion. */
int mst_step_epilogue_mt(const mst_schedule* s, const float* model_out_dev, const float* x_dev,
                         const float* noise_dev, const float* mask_dev, const float* motion_dev,
                         const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t sampler, int32_t mean_type,
                         float eta, int32_t mask_noise, int32_t clip_denoised,
                         float* sample_out_dev, float* xstart_out_dev, void* stream);

/* mst_step_epilogue_mt with a guide (p_sample / ddim_sample with a cond_fn for callers that bring their own model: gaussian_diffusion.py
 * :577-580 with condition_mean :454-467, :821-824 with condition_score :484-506, then :828-846).  g as in mst_sample_loop_guided, with
 * per-clip indices t_dev; weight_dev is [batch].  xstart_out_dev receives the UNGUIDED x0-hat.  sampler: MST_SAMPLER_DDPM or
 * MST_SAMPLER_DDIM (the others are refused by name, as is MST_SAMPLER_DDPM on a schedule without the variance row). */
int mst_step_epilogue_guided(const mst_schedule* s, const float* model_out_dev, const float* x_dev,
                             const float* noise_dev, const float* mask_dev, const float* motion_dev,
                             const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t sampler, int32_t mean_type,
                             float eta, int32_t mask_noise, int32_t clip_denoised, const mst_guide_args* g,
                             float* sample_out_dev, float* xstart_out_dev, void* stream);

/* plms_sample for callers that bring their own model (gaussian_diffusion.py:1084-1166), elementwise on [batch][per_clip] tensors.
 *   mst_plms_epilogue   the multistep step: cur_order 1..4, e1 / e2 / e3 the history NEWEST FIRST (only cur_order - 1 are read, the
 *                       rest may be NULL).  Outputs, any of which may be NULL: sample (t != 0 ? mean : pred), xstart (x0-hat, after
 *                       blend / conversion / clip), eps_out (what the history takes).  eps_out may alias e3 and sample may alias x.
 *                       first_half != 0: the first half of the Euler step that opens a chain instead -- sample is
 *                       x_mid = pred sqrt(abar_prev) + sqrt(1 - abar_prev) eps (from pred itself); cur_order, e1..e3 are ignored.
 *   mst_plms_euler      the second half: model_out is the model at (x_mid, t - 1), x the chain's original input, eps the first
 *                       evaluation's; tables at t - 1 for eps2, at t for the update.  Every t must be >= 1.  sample may alias x_mid.
 * mean_type as mst_step_epilogue_mt; mask / motion: the inpainting pair, both or neither. */
int mst_plms_epilogue(const mst_schedule* s, const float* model_out_dev, const float* x_dev, const float* mask_dev, const float* motion_dev,
                      const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t mean_type, int32_t clip_denoised, int32_t cur_order,
                      int32_t first_half, const float* e1_dev, const float* e2_dev, const float* e3_dev, float* sample_out_dev,
                      float* xstart_out_dev, float* eps_out_dev, void* stream);
int mst_plms_euler(const mst_schedule* s, const float* model_out_dev, const float* x_mid_dev, const float* x_dev, const float* eps_dev,
                   const float* mask_dev, const float* motion_dev, const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t mean_type,
                   int32_t clip_denoised, float* sample_out_dev, void* stream);


/* Standard-normal fill with the engine's Philox stream (the generator MST_NOISE_PHILOX uses
 * inside the fused step), so a caller can reproduce in-loop noise: element (clip, f, t) of step
 * `step`.  Replaces th.randn / th.randn_like draws (gaussian_diffusion.py:754, :569). */
/* Backward of mst_step_epilogue for the `*_with_grad` samplers (diffusion/inpainting_gaussian_diffusion.py:66-123,
 * :179-239; the fine-tune objective keeps every x0-hat in the autograd graph, gaussian_diffusion.py:1364-1378):
 *     d_model_out = (g_pred + g_sample * d sample / d pred) * (1 - mask)
 * g_sample / g_pred: upstream gradients of the two outputs, either may be NULL (= zero).  has_blend: the forward blended
 * with (mask, motion).  pred_clipped_dev: NULL, or -- when the forward ran with clip_denoised (the reference signature's default,
 * gaussian_diffusion.py:389-395) -- its x0-hat output: the clamp's gradient mask (zero where the prediction saturated at +-1). */
/* MST_SAMPLER_DDIM_REVERSE is refused: the reference has no `_with_grad` form of ddim_reverse_sample. */
int mst_step_backward(const mst_schedule* s, const float* g_sample_dev, const float* g_pred_dev, const float* mask_dev,
                      int32_t has_blend, const int64_t* t_dev, int32_t batch, int64_t per_clip, int32_t sampler, float eta,
                      const float* pred_clipped_dev, float* d_model_out_dev, void* stream);

/* K13 of SURVEY section 2.1 -- the reductions of the fine-tune objective, one launch each way:
 * mst_masked_l2: `masked_l2` (gaussian_diffusion.py:223-235) of a, b [n][feats][1][frames] with a frame mask
 *   [n][1][1][frames]; a_stride / mask_stride = elements between consecutive samples (0 = broadcast, the
 *   `.expand(num_step, ...)` of :1380).  g == NULL: out[n] = loss; g != NULL ([n] upstream gradient): out = dL/db
 *   ([n][feats][1][frames]; dL/da is its negative).
 * mst_text_cosine: `(1 - cosine_similarity(f / |f|, m / |m|, eps = 1e-6)).mean()` (:1384-1388) of two [batch][dim]
 *   matrices.  g == NULL: out[0] = loss; g != NULL ([1]): out = dL/dm ([batch][dim]). */
int mst_masked_l2(const float* a_dev, int64_t a_stride, const float* b_dev, const float* mask_dev, int64_t mask_stride,
                  int32_t n, int32_t feats, int32_t frames, const float* g_dev, float* out_dev, void* stream);
int mst_text_cosine(const float* f_dev, const float* m_dev, int32_t batch, int32_t dim, const float* g_dev, float* out_dev,
                    void* stream);

int mst_philox_normal(float* out_dev, int32_t batch, int32_t feats, int32_t frames, uint64_t seed,
                      uint32_t step, void* stream);

/* -------------------------------------------------------------------------------------------
 * The variational-bound evaluation on timestep-batched rows (csrc/mst_vb.h): calc_bpd_loop (gaussian_diffusion.py:1547-1602) visits
 * its timesteps independently of each other, so (clip, timestep) pairs are packed into full model batches.  A ROW r is the pair
 * (clip_dev[r], t_dev[r]), both int64 [rows], in any order.  x_start / mask / motion are per CLIP ([N][per_clip], gathered by
 * clip_dev[r]); x_t, the model output, a noise buffer, x0-hat are per ROW ([rows][per_clip]).
 *   mst_vb_diffuse   q_sample on gathered operands (gaussian_diffusion.py:267-285, :1573-1574; inpainting_gaussian_diffusion.py:6-23):
 *                    out[r] = sqrt_ac[t] x_start[clip] + sqrt_1m_ac[t] z (1 - mask[clip]), the expression of mst_q_sample bit for bit.
 *                    mask_dev may be NULL.  noise_dev: z as [rows][per_clip], or NULL -- z is then drawn: row r gets
 *                    mst_philox_normal(N, feats, frames, seed, step = t[r])[clip[r]], so the noise of a (clip, timestep) pair does not
 *                    depend on the packing; feats * frames must be per_clip.
 *   mst_vb_terms     _vb_terms_bpd (:1281-1314 with p_mean_variance :341-412, losses.py:12-77) and the two MSEs of the loop
 *                    (:1586-1588): out_dev [rows][4] = (vb term in bits, mean (x0hat - x_start)^2, mean (eps - z)^2, rms of x0-hat) over
 *                    ALL per_clip elements (mean_flat: no frame mask, as the reference).  The inpainting blend acts on the raw output,
 *                    then mean_type (as mst_step_epilogue_mt), then clip_denoised.  t != 0: normal_kl(true posterior, model posterior);
 *                    true_logvar_dev is posterior_log_variance_clipped as float32 [num_steps] (the schedule's log-variance row is the
 *                    MODEL's: they differ under FIXED_LARGE); for mean types 0 and 1 the means' difference is coef1 (x_start - x0hat).
 *                    t == 0: minus discretized_gaussian_log_likelihood, evaluated in double.  z: noise_dev, or NULL and the draw of
 *                    mst_vb_diffuse.  xstart_out_dev ([rows][per_clip]) may be NULL.  Sums are accumulated in double in a fixed order,
 *                    one workgroup per row, no atomics: a row's four numbers do not depend on the other rows of the call.
 *   mst_vb_prior     _prior_bpd (:1529-1545): out_dev[n] = mean_flat(normal_kl(sqrt_ac_last x_start[n], log_1m_ac_last, 0, 0)) / ln 2,
 *                    the two scalars being sqrt_alphas_cumprod[-1] and log_one_minus_alphas_cumprod[-1] as float32 (the second is
 *                    no row of enum mst_table); the schedule names the device the launch goes to.
 * THE CALLER IS TRUSTED as in the stand-alone elementwise section: every operand is read as base + i over its full size, no check that
 * would cost a synchronisation is made, and clip_dev[r] in [0, N), t_dev[r] in [0, num_steps) are the caller's to check (the Python
 * handles do).  Refused here by name: null operands, rows / batch / per_clip < 1, an unknown mean_type, a draw without feats / frames
 * or with feats * frames != per_clip, a mask without a motion in mst_vb_terms.
 * ----------------------------------------------------------------------------------------- */
int mst_vb_diffuse(const mst_schedule* s, const float* x_start_dev, const float* noise_dev, const float* mask_dev,
                   const int64_t* clip_dev, const int64_t* t_dev, int32_t rows, int64_t per_clip, int32_t feats, int32_t frames,
                   uint64_t seed, float* out_dev, void* stream);
int mst_vb_terms(const mst_schedule* s, const float* true_logvar_dev, const float* x_start_dev, const float* x_t_dev,
                 const float* model_out_dev, const float* noise_dev, const float* mask_dev, const float* motion_dev,
                 const int64_t* clip_dev, const int64_t* t_dev, int32_t rows, int64_t per_clip, int32_t feats, int32_t frames,
                 uint64_t seed, int32_t mean_type, int32_t clip_denoised, float* out_dev, float* xstart_out_dev, void* stream);
int mst_vb_prior(const mst_schedule* s, const float* x_start_dev, int32_t batch, int64_t per_clip, float sqrt_ac_last, float log_1m_ac_last, float* out_dev,
                 void* stream);

/* -------------------------------------------------------------------------------------------
 * Training path of the TRAINABLE encoder stack: StyleDiffusion.seqTransEncoder, 8 x
 * nn.TransformerEncoderLayer(d_model=512, nhead=4, dim_feedforward=1024, dropout=0.1, gelu),
 * model/mdm_forstyledataset.py:539-546, called at :622 inside the graph that
 * few_shot_style_finetune_losses (diffusion/gaussian_diffusion.py:1317-1399) back-propagates
 * through.  Replaces the torch autograd graph of that call:
 *   mst_train_forward   forward in model.train() semantics: dropout p at the four sites of each
 *                       layer (attention probabilities, out-proj output, FFN hidden, FFN output),
 *                       masks drawn from a counter-based generator keyed by `seed`; writes the
 *                       activation tape into caller-owned memory of mst_train_tape_bytes() bytes.
 *   mst_train_backward  given dL/d(h_out): dL/d(h_in) and the 96 parameter gradients, ACCUMULATED
 *                       (+=) into the caller's float32 buffers.  `grads` is a HOST array of
 *                       num_layers*12 device pointers in nn.TransformerEncoderLayer parameter order:
 *                       self_attn.in_proj_weight, .in_proj_bias, self_attn.out_proj.weight, .bias,
 *                       linear1.weight, .bias, linear2.weight, .bias, norm1.weight, .bias,
 *                       norm2.weight, .bias.  grads == NULL: no parameter gradients (frozen stack, input
 *                       gradient only).  rows / S / p_drop / seed must repeat the forward's.
 * DYNAMIC RANGE of d_out (the same for mst_train_model_backward's d_out and mst_motion_encoder_backward's d_mu): ONE
 * power of two per call brings max |d_out| into [16, 32), and every f16 operand of the backward pass lives behind it.
 * The magnitude of the whole cotangent is therefore free (2^-30 is as accurate as 1), but its range INSIDE one call is
 * f16's: a clip or token whose cotangent lies 2^-k below the call's largest entry meets f16 subnormals from k = 18 on and
 * rounds to zero from about k = 29 on.  Supported: k <= 16 (R = 16: dL/d(h_in) of every clip within 1.5e-3 of float64; measured
 * 3.7e-4 at k = 12, as at k = 0, and 1.4e-3 at k = 16, the edge); beyond, that clip's dL/d(h_in) degrades as f16's gradual
 * underflow does, by about 2x per bit -- 2e-2 at 2^-20, 0.25 at 2^-24 -- while the parameter gradients, sums dominated by
 * the large clips, keep their accuracy.  The fine-tune objective stays within 2^3.4 (chained steps and the text-to-motion
 * batch in one pass; DESIGN section 5 has the table).  Cotangents of wider range belong in separate calls: the gradient
 * buffers accumulate.
 * h_in, h_out, d_out, d_in: float32 [rows][S][512] (clip-major; the reference's [S, B, 512] permuted).
 * key_keep: NULL, or uint8 [rows][S] with 0 marking padding keys -- the inverse of the `src_key_padding_mask`
 * the frozen MotionEncoder passes to its own 8-layer stack (model/mdm_forstyledataset.py:90-124); every clip
 * must keep at least one key.
 * The engine's weights are the ones last uploaded with mst_load_weight.
 * mst_dropout_mask: the keep-multipliers (0 or 1/(1-p)) of the first n elements of site
 * (layer, site 0..3) -- lets a test rebuild the masked forward exactly in PyTorch.
 * ----------------------------------------------------------------------------------------- */
int64_t mst_train_tape_bytes(const mst_engine* e, int32_t rows, int32_t S);
int mst_train_forward(mst_engine* e, const float* h_in_dev, int32_t rows, int32_t S, float p_drop,
                      uint64_t seed, const uint8_t* key_keep_dev, void* tape_dev, float* h_out_dev,
                      void* stream);
int mst_train_backward(mst_engine* e, const void* tape_dev, const float* d_out_dev, int32_t rows,
                       int32_t S, float p_drop, uint64_t seed, const uint8_t* key_keep_dev,
                       float* d_in_dev, float* const* grads_host_array, void* stream);
/* The whole denoiser as one training node: StyleDiffusion.forward / MDM.forward in train mode
 * (model/mdm_forstyledataset.py:602-625, :315-364): conditioning token (timestep MLP + text projection, text set with
 * mst_set_text as for mst_forward), pose embedding + positional rows, PositionalEncoding's dropout p_pe (:404) on the
 * assembled sequence, the trainable stack (p_drop), output projection.  Backward returns dL/dx and accumulates the 96
 * stack gradients (the projections, the timestep MLP and the text projection are frozen in every shipped script).
 * x, out, d_out, d_x: float32 [batch][feats][1][frames]; t_idx: int64 [batch] original-process timesteps.
 * clip0 / tape_clips (tape_clips <= 0: the tape is this call's own): the call writes clips [clip0, clip0 + batch) of a tape laid out
 * for tape_clips clips, and draws the dropout masks those clips have in a pass over the WHOLE tape with the same seed.  For model calls
 * whose inputs are cut from each other's graphs -- the chained x0-hat steps of the fine-tune objective (gaussian_diffusion.py:1364-1378:
 * `x.detach()` between steps) -- so that ONE mst_train_model_backward over tape_clips clips differentiates all of them (their forward
 * passes are sequential, their backward passes independent). */
int mst_train_model_forward(mst_engine* e, const float* x_dev, const int64_t* t_idx_dev, int32_t batch,
                            int32_t frames, float p_drop, float p_pe, uint64_t seed, void* tape_dev,
                            float* out_dev, int32_t clip0, int32_t tape_clips, void* stream);
int mst_train_model_backward(mst_engine* e, const void* tape_dev, const float* d_out_dev, int32_t batch,
                             int32_t frames, float p_drop, float p_pe, uint64_t seed, float* d_x_dev,
                             float* const* grads_host_array, void* stream);
/* MotionEncoder.forward (model/mdm_forstyledataset.py:90-124), the frozen "semantic discriminator" of the fine-tune
 * objective (gaussian_diffusion.py:1340-1343), as one native call each way:
 *     frames = mdm_model.input_process(x);  seq = pos_encoder(cat(muQuery, sigmaQuery, frames));
 *     mu = seqTransEncoder(seq, src_key_padding_mask=~keep)[0]
 * x_dev [batch][feats][1][frames]; mu_query / sigma_query [512]; key_keep_dev [batch][frames + 2] bytes (1 = real key,
 * the two query tokens first); mu_out_dev [batch][512].  Dropout (p_drop in the layers, p_pe behind the positional rows) is
 * counter-based from `seed` as in mst_train_forward.  The backward call returns dL/dx only: every parameter on this path
 * is frozen (train/finetune_style_diffusion.py:256, load_motion_enc :579-588).  The engine must hold the encoder's own
 * layers and the prior's pose embedding / positional table, with max_frames >= frames + 1. */
int mst_motion_encoder_forward(mst_engine* e, const float* x_dev, const float* mu_query_dev, const float* sigma_query_dev,
                               const uint8_t* key_keep_dev, int32_t batch, int32_t frames, float p_drop, float p_pe,
                               uint64_t seed, void* tape_dev, float* mu_out_dev, void* stream);
int mst_motion_encoder_backward(mst_engine* e, const void* tape_dev, const float* d_mu_dev, const uint8_t* key_keep_dev,
                                int32_t batch, int32_t frames, float p_drop, float p_pe, uint64_t seed, float* d_x_dev,
                                void* stream);

/* Data-parallel fine-tuning (BASELINE.json configs[3]; the reference is single-device, train/training_loop.py:73).
 * Make `stream` wait until every kernel that writes layer `layer`'s 12 gradient tensors in the MOST RECENT
 * mst_train_backward / mst_train_model_backward call (grads != NULL) has finished.  The backward calls only ENQUEUE
 * work; a reducer calls this right after the backward call returns, layer num_layers-1 first, and launches that
 * layer's gradient all-reduce on `stream`: it then runs on the GPU while the layers below are still being
 * differentiated. */
int mst_train_wait_layer_grads(mst_engine* e, int32_t layer, void* stream);
int mst_dropout_mask(uint64_t seed, int32_t layer, int32_t site, float p, uint64_t n, float* out_dev,
                     void* stream);

/* -------------------------------------------------------------------------------------------
 * Optimizer step of the fine-tune loop: `self.mp_trainer.optimize(self.opt)`,
 * train/training_loop.py:196-200 -> diffusion/fp16_util.py:208-223 (`_compute_norms`: one
 * `.item()` sync per tensor for grad and param norms) + torch.optim.AdamW.step (training_loop.py:96).
 * ONE launch over all tensors: AdamW update in place (torch's arithmetic: decoupled weight decay,
 * step_size = lr/(1-b1^t), denom = sqrt(v)/sqrt(1-b2^t) + eps) and norms_dev[0] += sum g^2,
 * norms_dev[1] += sum p^2 of the parameters BEFORE the update (what the reference logs).
 * All pointer arrays are HOST arrays of device pointers; workspace_dev holds the device-side tables
 * (mst_adamw_workspace_bytes).  `step` is the 1-based step count of these tensors.
 * `upload_tables` != 0: (re)write the device-side tables from the host arrays before the launch (one
 * stream synchronisation + two small copies).  The OWNER of the workspace decides: it must pass 1 on the
 * first call with a workspace, whenever any pointer / size changed since the tables were last written
 * into THIS workspace allocation, and whenever the workspace memory may have been reused in between;
 * 0 re-uses the tables already there (the steady state: torch's caching allocator returns the same
 * blocks every iteration).  The library keeps no state of its own about workspaces.
 * ----------------------------------------------------------------------------------------- */
int64_t mst_adamw_workspace_bytes(int32_t n_tensors, const int64_t* numel_host);
int mst_adamw_step(int32_t n_tensors, float* const* params, const float* const* grads,
                   float* const* exp_avg, float* const* exp_avg_sq, const int64_t* numel_host, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int32_t step,
                   float* norms_dev, void* workspace_dev, int64_t workspace_bytes, int32_t upload_tables,
                   void* stream);

/* -------------------------------------------------------------------------------------------
 * Post-sampling tensor ops, one launch (sample/demo_style_transfer.py:265-267,
 * train/finetune_style_diffusion.py:331-332):
 *     sample = dataset.inv_transform(sample.cpu().permute(0, 2, 3, 1)).float()   dataset.py:478-479
 *     joints = recover_from_ric(sample, n_joints)                                 motion_process.py:444-461
 * sample_dev: [batch][feats][1][frames] float32 normalised hml_vec (the samplers' output layout),
 * mean_dev / std_dev: [feats]; out_dev: [batch][1][frames][joints][3].  The clip never leaves the GPU.
 * ----------------------------------------------------------------------------------------- */
int mst_recover_from_ric(const float* sample_dev, const float* mean_dev, const float* std_dev, int32_t batch,
                         int32_t feats, int32_t frames, int32_t joints, float* out_dev, void* stream);
/* Longest clip mst_recover_from_ric takes on the current device: the kernel keeps five fp32 rows of `frames` entries in dynamic LDS,
 * so this is min(4096, shared memory per block / 20 bytes); longer clips are refused on the host.  -1 when the device cannot be asked. */
int mst_recover_max_frames(void);

/* -------------------------------------------------------------------------------------------
 * Joint-space guidance, one launch, one workgroup per clip: the log-likelihood of world-space joint positions of a denoised clip and
 * its gradient.  This is what a with-grad cond_fn (diffusion/gaussian_diffusion.py:469-482, :508-530; called from
 * diffusion/inpainting_gaussian_diffusion.py:66-123, :179-239) evaluates on p_mean_var["pred_xstart"] when the constraint is on joints:
 *     p       = recover_from_ric(x0 * std + mean, joints)       data_loaders/humanml/scripts/motion_process.py:389-410, :444-461
 *     logp[b] = -1/2 scale[b] sum_{t < len_b, j, c} weight (p - target)^2
 *     grad    = d logp / d x0   (normalised features: the std[f] factor is included)
 * x0_dev, grad_dev: [batch][feats][1][frames] float32, the samplers' layout; mean_dev / std_dev: [feats]; feats >= 4 + 3 (joints - 1):
 * the 263-feature HumanML row at 22 joints and the 9 J + 1 position-rotation row both qualify.  target_dev, weight_dev:
 * [batch][frames][joints][3], weight >= 0 per axis, 0 = unconstrained (the target is then not used).  scale_dev: [batch].
 * lengths_dev: [batch] int32, 0 <= len <= frames, or NULL; the kernel clamps the values into that range.  positions_dev:
 * [batch][frames][joints][3] or NULL.  The yaw quaternion is (cos a, 0, sin a, 0) with the full angle, as the reference has it.
 * The reverse pass is written by hand in the same launch; its three suffix sums and the forward map's three prefix sums are workgroup
 * scans in double with a fixed order, no atomics: a clip's result is the same bits alone, anywhere in a batch and from run to run.
 * Channels the map does not read and frames at or past a clip's length receive exact zeros, and what such frames hold changes no output.
 * Refused here: null operands, batch / frames / joints < 1, feats too small for the joints, frames above mst_joint_guide_max_frames.
 * ----------------------------------------------------------------------------------------- */
int mst_joint_guide(const float* x0_dev, const float* mean_dev, const float* std_dev, const float* target_dev, const float* weight_dev,
                    const float* scale_dev, const int32_t* lengths_dev, int32_t batch, int32_t feats, int32_t frames, int32_t joints,
                    float* logp_dev, float* grad_dev, float* positions_dev, void* stream);
/* Longest clip mst_joint_guide takes on the current device: the kernel keeps 32 bytes a frame in dynamic LDS (three double rows, two
 * fp32 rows), so this is min(2040, (shared memory per block - 128) / 32) -- above the 223 frames of the training node; longer clips
 * are refused on the host.  -1 when the device cannot be asked. */
int mst_joint_guide_max_frames(void);

/* -------------------------------------------------------------------------------------------
 * Foot-skate cleanup of joint clips, one launch, one workgroup per clip: the reference's remove_fs
 * (data_loaders/humanml/common/bvh_utils.py:1685-1809) with get_foot_contact_by_vel_acc (:1591-1639, use_vel3 = 0; thr is its
 * 0.003, use_window its window refinement), get_foot_contact_by_vel3 (:1642-1682, use_vel3 != 0) and Butterworth (:1872-1916;
 * filter_before = use_butterworth, cut-off 3; filter_after = after_butterworth, cut-off 2.5; dt = 1/20).  What
 * sample/demo_style_transfer.py:310-313 does to every clip it writes is two calls of this.
 * glb_dev: [batch][frames][joints][3] float32 (mst_recover_from_ric's output); out_dev: the same shape, may be glb_dev; NULL: only the
 * contacts and velocities are computed.
 * ref_dev: [ref_batch][frames][joints][3], ref_batch 1 or batch, the motion the contacts are detected on; NULL: the clip itself as it
 * is on entry.  It must not overlap out_dev.  lengths_dev: [batch] int32, 2 <= len <= frames, or NULL (every clip `frames` long):
 * every stage sees frames 0 .. len-1 only, later frames are copied through.  foot_ids_host: four distinct joint indices, host memory.
 * contacts_dev: [batch][frames][4] int32 or NULL; foot_vels_dev: [batch][frames-1][4] float32 or NULL (speeds for vel3, y-velocities
 * otherwise; zero from len-1 on).  workspace_dev: 8 * batch * (frames-1) * joints * 3 bytes when a filter is on, else unused.
 * The caller is trusted for the shapes and for the VALUES of lengths_dev (the kernel clamps them into 2..frames, so no access leaves
 * the clip); the Python handle checks both.  Refused here: frames < 2 (the reference raises IndexError), frames above
 * mst_remove_fs_max_frames, duplicate or out-of-range foot ids, a filter without its workspace.
 * ----------------------------------------------------------------------------------------- */
int mst_remove_fs(const float* glb_dev, const float* ref_dev, int32_t ref_batch, const int32_t* lengths_dev, int32_t batch,
                  int32_t frames, int32_t joints, const int32_t* foot_ids_host, int32_t use_vel3, float thr, int32_t use_window,
                  int32_t force_on_floor, int32_t interp_length, int32_t filter_before, int32_t filter_after, float* out_dev,
                  int32_t* contacts_dev, float* foot_vels_dev, double* workspace_dev, int64_t workspace_bytes, void* stream);
/* Longest clip mst_remove_fs takes at this joint count: never below mst_recover_max_frames, so that whatever mst_recover_from_ric returns
 * can be cleaned.  The kernel keeps two byte maps of 4 * frames contacts in LDS (32 KB at the cap of 4096) and the filter's forward
 * result in the caller's workspace, so today the bound is the same for every joint count.  -1 for joints < 1. */
int mst_remove_fs_max_frames(int32_t joints);

/* -------------------------------------------------------------------------------------------
 * Joint rotations fitted to joint positions, two launches: the optimisation inside the reference's fit_joints_bvh
 * (data_loaders/humanml/common/bvh_utils.py:1811-1846) -- InverseKinematics_hmlvec (common/Kinematics.py:30-91; the starting point is
 * recover_root_rot_pos_this, :8-27) stepping torch.optim.Adam (lr 1e-3, betas 0.9 / 0.999, eps 1e-8) `iters` times through
 * Skeleton.forward_kinematics_real_cont6d (common/skeleton.py:200-222) under the Geman-McClure loss at sigma 100 -- and the conversion
 * that follows it (cont6d2q, common/rotation.py:744-776; the root joint times the normalised r_rot_quat).  Every frame is an
 * optimisation of its own (6 * joints + 7 parameters) and runs in one lane from its first iteration to its last.
 * data_dev: the position-rotation vector, feats = 9 * joints + 1 per frame, element (b, t, f) at
 * data_dev[b * stride_batch + t * stride_frame + f * stride_feat] (strides in elements: [batch][frames][feats] is (frames * feats,
 * feats, 1); the samplers' [batch][feats][1][frames] is (feats * frames, 1, frames)); mean_dev / std_dev: [feats], both or neither,
 * applied as x * std + mean.  target_dev: [batch][frames][joints][3], the positions to fit.  lengths_dev: [batch] int32 or NULL;
 * frames at or beyond a clip's length take no step (their outputs are those of the starting point, their loss and gradient zero).
 * parents_host: [joints], parents[0] ignored, 0 <= parents[j] < j; offsets_host: [joints][3], row 0 ignored.
 * Outputs: cont6d_dev [batch][frames][joints][6], r_pos_dev [batch][frames][3], r_rot_quat_dev [batch][frames][4] (as optimised, not
 * normalised), positions_dev [batch][frames][joints][3] (forward kinematics of the fit), joint_quats_dev [batch][frames][joints][4];
 * optional (NULL: not written) frame_loss_dev [batch][frames][2], the loss of the first and of the last iteration, each before its
 * update, and grad_dev [batch][frames][6 * joints + 7], the gradient of the last iteration (cont6d, r_pos, r_rot_quat).
 * The quirk: the reference builds its local positions in the storage autograd saved as x_raw for the backward of x_raw / |x_raw|, so
 * its gradient on the first three 6D components is g / n - s (g . s) / n^3 with s the joint's offset (for the root: the frame's r_pos)
 * where the true gradient has x_raw.  true_gradient = 0 reproduces the reference, != 0 gives the true gradient.
 * Refused here: joints < 2 or above mst_fit_joints_max_joints, a parents array that is not a tree rooted at 0 with parents[j] < j,
 * iters < 1, feats != 9 * joints + 1, frames < 1 or above mst_fit_joints_max_frames, one of mean / std without the other.
 * ----------------------------------------------------------------------------------------- */
int mst_fit_joints(const float* data_dev, int64_t stride_batch, int64_t stride_frame, int64_t stride_feat, const float* mean_dev,
                   const float* std_dev, const float* target_dev, const int32_t* lengths_dev, int32_t batch, int32_t frames,
                   int32_t feats, int32_t joints, const int32_t* parents_host, const float* offsets_host, int32_t iters,
                   int32_t true_gradient, float* cont6d_dev, float* r_pos_dev, float* r_rot_quat_dev, float* positions_dev,
                   float* joint_quats_dev, float* frame_loss_dev, float* grad_dev, void* stream);
/* Most joints mst_fit_joints takes: a 64-lane workgroup keeps 21 * joints + 21 floats a lane in LDS (24 joints: 134 400 bytes). */
int mst_fit_joints_max_joints(void);
/* Longest clip mst_fit_joints takes: the starting point's three running sums keep three fp32 rows of `frames` entries in LDS, 48 KB at
 * the cap of 4096, the same for every joint count.  -1 for joints outside 2 .. mst_fit_joints_max_joints. */
int mst_fit_joints_max_frames(int32_t joints);

/* -------------------------------------------------------------------------------------------
 * Joint positions (and rotations) encoded into the model's feature rows, one launch, one workgroup per clip: the reference's
 * process_file_with_rotation (data_loaders/humanml/common/bvh_utils.py:1091-1287; mode 0, POSROT: 9 * joints + 1 features, the layout
 * mst_fit_joints reads) and process_file (bvh_utils.py:898-1088; mode 1, HML: 12 * joints - 1 features, 263 at 22 joints), followed by
 * process_np_motion's z-normalisation and zero padding (data_loaders/humanml/data/dataset.py:484-519).  The stages -- floor, origin,
 * initial facing (quatbetween, common/rotation.py:97-108), the smoothed root rotation of Skeleton.inverse_kinematics_np
 * (common/skeleton.py:55-86; gaussian_filter1d at sigma 20, 161 taps summed in double, index clamped into the clip; qbetween,
 * common/quaternion.py:421-431), in HML the chain IK (skeleton.py:88-103, every chain restarting from the frame's root quaternion),
 * root velocities, local pose, local velocities and foot contacts -- all run over a clip's own length.
 * positions_dev: [batch][frames][joints][3] float32; rotations_dev: [batch][frames][joints][4] (w, x, y, z), NULL allowed in HML.  Neither
 * is written (the reference mutates its arguments).  lengths_dev: [batch] int32, 2 <= len <= frames, or NULL; the kernel clamps the
 * values into 2..frames, so no access leaves a clip (the Python handle checks them).  mean_dev / std_dev: [feats], both or neither, applied
 * as (row - mean) / std.  Host arrays: face_ids_host[4] = r_hip, l_hip, sdr_r, sdr_l; foot_ids_host[4] = fid_l[0], fid_l[1], fid_r[0],
 * fid_r[1] (HML; may be NULL in POSROT); the kinematic chains flattened into chains_host with chain c at
 * chains_host[chain_starts_host[c] .. chain_starts_host[c + 1]) (HML; num_chains = 0 allowed in POSROT); raw_offsets_host[joints][3]
 * (HML), the unit bone directions.  feet_thre: the squared-displacement threshold of the contacts.
 * Outputs: sample_dev [batch][feats][1][frames_out], the samplers' layout: row t < min(len - 1, frames_out) of a clip, exact zeros from
 * there on (a longer clip is cut); lengths_out_dev [batch] int32 = min(len - 1, frames_out); optional (NULL: not written)
 * global_positions_dev and local_positions_dev [batch][frames][joints][3] and l_velocity_dev [batch][frames - 1][2], zero past a clip.
 * Stated deviation: the arcsin argument of the root's angular velocity is clamped into [-1, 1] (the reference returns NaN past 1).
 * Refused here: frames < 2 or above mst_encode_max_frames, joints outside 2..24, frames_out < 1, a face or foot id out of range, a face id
 * named twice, a chain that does not start at a joint already placed (joint 0 or an earlier chain's) or that names a joint twice as a
 * child, POSROT without rotations, HML without foot ids, chains or raw offsets, one of mean / std without the other.
 * ----------------------------------------------------------------------------------------- */
int mst_encode_motion(const float* positions_dev, const float* rotations_dev, const int32_t* lengths_dev, const float* mean_dev,
                      const float* std_dev, int32_t batch, int32_t frames, int32_t joints, int32_t mode, const int32_t* face_ids_host,
                      const int32_t* foot_ids_host, const int32_t* chains_host, const int32_t* chain_starts_host, int32_t num_chains,
                      const float* raw_offsets_host, float feet_thre, int32_t frames_out, float* sample_dev, int32_t* lengths_out_dev,
                      float* global_positions_dev, float* local_positions_dev, float* l_velocity_dev, void* stream);
/* Longest clip mst_encode_motion takes: the kernel keeps the per-frame forward direction (two fp32 rows) and one root quaternion a frame
 * in LDS, 24 bytes a frame -- 48 KB at the cap of 2048 -- and recomputes a neighbouring frame's positions from the input, so today the
 * bound is the same for every joint count and both modes.  -1 for joints outside 2..24 or a mode that is neither 0 nor 1. */
int mst_encode_max_frames(int32_t joints, int32_t mode);

/* -------------------------------------------------------------------------------------------
 * Motion files.  What is left on the host is text: one parse of a BVH file into an array of channel values, one formatting pass out of
 * one (utils/bvh.py).  Everything between runs here.
 *
 * mst_bvh_decode: what the reference's read_bvh does after the text is parsed (data_loaders/humanml/common/bvh_utils.py:222-295), for a
 * batch of clips of one hierarchy in one launch, one workgroup per clip: Euler degrees -> radians -> eul2q (utils/rotation.py:344-361
 * over angle_axis_to_quat, :327-341; sinf / cosf) in the file's rotation order, q(e0, axis0) (x) (q(e1, axis1) (x) q(e2, axis2)); the
 * sign continuity of remove_quat_discontinuities (:666-683) as a prefix parity over the full-rate frames (wave ballot, per-wave carries
 * through LDS, a carry across rounds of 256 frames); the [phase::stride] sub-sampling; quat_fk (:646-663: qnorm, file order).
 * channels_dev: [batch][frames][channels] float32, not written.  lengths_dev: [batch] int32, 1 <= len <= frames, or NULL; the kernel
 * clamps into that range.  Host arrays over the file's joints, End Sites included: parents_host (joint 0 is the root, -1; parents[j] < j),
 * rot_cols_host / pos_cols_host (the column of a joint's first rotation / position channel, -1 for none: an End Site is the identity, a
 * joint without position channels stands at its offset), offsets_host [joints][3], order_host[3] (0 / 1 / 2 = X / Y / Z rotation, a
 * permutation).  scale multiplies offsets and position channels.  select_host: num_select <= 24 file joints in the caller's order, or
 * NULL / 0 for all of them.  workspace_dev: [batch][frames][joints][11] float32 (the raw local quaternion, global quaternion and global
 * position of the whole file skeleton; a lane reads only what it wrote itself).
 * Outputs over J = num_select or joints and frames_out = ceil((frames - phase) / stride): rotations_dev [batch][frames_out][J][4]
 * (w, x, y, z) -- the file's own signed local quaternion (Anim.quats, not normalised) where a joint's nearest selected ancestor is its file
 * parent or nothing is selected, qinv(gr[ancestor]) (x) gr[j] where joints between them were skipped, gr[j] where it has no selected
 * ancestor -- and positions_dev [batch][frames_out][J][3], the global positions: together what mst_encode_motion takes in POSROT.
 * Optional (NULL: not written): local_positions_dev (Anim.pos) and global_rotations_dev.  Frames at or past a clip's length: exact zeros.
 * Stated deviation: for a dot product of exactly 0 between neighbouring raw quaternions the reference takes the raw sign, the kernel keeps
 * the running one.
 * Refused here: joints outside 1 .. mst_bvh_max_joints, frames above mst_bvh_max_frames, channels outside 3 .. 6 * joints, a column outside
 * the channels, parents that are no tree in file order, an order that is no permutation, stride < 1, phase outside 0 .. stride - 1 or past
 * the frames, more than 24 selected joints, one out of range or named twice.
 * ----------------------------------------------------------------------------------------- */
int mst_bvh_decode(const float* channels_dev, const int32_t* lengths_dev, int32_t batch, int32_t frames, int32_t channels, int32_t joints,
                   const int32_t* parents_host, const int32_t* rot_cols_host, const int32_t* pos_cols_host, const float* offsets_host,
                   const int32_t* order_host, float scale, int32_t stride, int32_t phase, const int32_t* select_host, int32_t num_select,
                   float* workspace_dev, float* rotations_dev, float* positions_dev, float* local_positions_dev,
                   float* global_rotations_dev, void* stream);
/* Most file joints (End Sites included) mst_bvh_decode and mst_quats_to_channels take: the skeleton's tables ride in the kernel arguments
 * and a lane keeps one scan bit a joint in two 64-bit registers. */
int mst_bvh_max_joints(void);
/* Longest clip mst_bvh_decode takes.  Nothing a frame needs is kept in LDS, so the bound is the same for every joint count: one workgroup
 * walks a clip 256 frames a round, 64 rounds at the cap of 16384.  -1 for joints outside 1 .. mst_bvh_max_joints. */
int mst_bvh_max_frames(int32_t joints);

/* The numbers the reference's save_bvh formats (bvh_utils.py:588-612), one thread per clip, frame and joint: qnorm, q2eul of order[::-1]
 * (utils/rotation.py:364-382, its own formula set), degrees.  order: 0 = a 'zyx' file (q2eul 'xyz'; the default and what every caller in
 * the reference uses), 1 = an 'xzy' file (q2eul 'yzx'); q2eul has no formulas for another.  quats_dev: [batch][frames][joints][4], need
 * not be normalised; root_pos_dev: [batch][frames][3] -- JointFit.joint_quats and JointFit.r_pos as they are.  perm_host[joints]: output
 * slot -> joint, the writer's save_joint_seq (perm[0] = 0).  positions_dev: NULL, or [batch][frames][joints][3] for a file written with
 * positions=True.  out_dev: [batch][frames][3 + 3 * joints] -- the root position, then per slot the three angles in the file's channel
 * order -- or, with positions, [batch][frames][6 * joints]: per slot the position (the root's: root_pos) and the angles.
 * Refused here: joints outside 1 .. mst_bvh_max_joints, another order, a perm that is no permutation or does not start at the root. */
int mst_quats_to_channels(const float* quats_dev, const float* root_pos_dev, const float* positions_dev, const int32_t* perm_host,
                          int32_t batch, int32_t frames, int32_t joints, int32_t order, float* out_dev, void* stream);

/* The reference's uniform_skeleton_basic (data_loaders/humanml/scripts/motion_process.py:12-35) for a batch, one workgroup per clip, one
 * frame per lane: source offsets from frame 0 (Skeleton.get_offsets_joints, common/skeleton.py:43-51); the leg ratio from the largest
 * absolute component of the two leg offsets, not their norms (the reference's quirk, kept); the root scaled by it; the chain IK of
 * inverse_kinematics_np (:55-105; smooth_forward=False, frame 0's root quaternion the identity, every chain restarting from the root
 * quaternion); forward_kinematics_np (:130-151) with the target offsets.  positions_dev / out_dev: [batch][frames][joints][3], distinct;
 * lengths_dev: [batch] int32, 1 <= len <= frames, or NULL (clamped by the kernel); frames past a clip are exact zeros, as is a joint no
 * chain places.  Host arrays as in mst_encode_motion: face_ids_host[4], the flattened chains, raw_offsets_host[joints][3]; and
 * target_offsets_host[joints][3], leg_ids_host[2] (l_idx).  A zero-length bone divides by zero, here as in the reference.
 * Refused here: joints outside 2..24, frames above mst_retarget_max_frames, a face id out of range or named twice, a chain that does not
 * start at a placed joint or names a joint twice as a child, a leg joint outside 1 .. joints - 1, out_dev == positions_dev. */
int mst_retarget_joints(const float* positions_dev, const int32_t* lengths_dev, int32_t batch, int32_t frames, int32_t joints,
                        const int32_t* face_ids_host, const int32_t* chains_host, const int32_t* chain_starts_host, int32_t num_chains,
                        const float* raw_offsets_host, const float* target_offsets_host, const int32_t* leg_ids_host, float* out_dev,
                        void* stream);
/* Longest clip mst_retarget_joints takes (nothing is kept on chip: the bound of mst_bvh_max_frames).  -1 for joints outside 2..24. */
int mst_retarget_max_frames(int32_t joints);

/* -------------------------------------------------------------------------------------------
 * A sample's rotation channels decoded, one launch for a batch, one workgroup per clip: recover_root_rot_pos
 * (data_loaders/humanml/common/bvh_utils.py:1299-1318; the angle an exclusive, root x and z inclusive prefix sums, taken in double by a
 * workgroup scan and rounded to fp32 once per frame) followed by one route.
 * route 0, HML_ROT, feats = 12 * joints - 1 (263 at 22 joints): output_bvh (bvh_utils.py:1382-1441) -- the joints - 1 6D blocks at feature
 * 4 + 3 * (joints - 1) through cont6d2q (common/rotation.py:744-776), world quaternions chain by chain, every chain restarting from
 * r_rot_quat, gathered onto the expanded skeleton and made local, qinv(world[parent]) (x) world[i] -- and recover_from_rot (:1321-1335;
 * Skeleton.forward_kinematics_cont6d, common/skeleton.py:177-198).
 * route 2, POS_IK, the same 12 * joints - 1 row read for its positions: output_bvh_with_pos (:1444-1511) -- recover_from_ric (:1348-1363),
 * Skeleton.inverse_kinematics_np(smooth_forward=True) (common/skeleton.py:55-103; the forward direction smoothed by 161 taps summed in
 * double, as mst_encode_motion does), the IK's root dropped, then route 0's chain products and expanded skeleton; joints_dev receives
 * recover_from_ric's positions.  face_ids_host[4] = r_hip, l_hip, sdr_r, sdr_l and raw_offsets_host[joints][3], the unit bone
 * directions, belong to this route (NULL otherwise).  A zero-length bone divides by zero, here as in the reference.
 * route 1, REAL_ROT, feats = 9 * joints + 1 (181 / 190): output_bvh_from_real_rot (:1538-1563; joints 6D blocks through cont6d2q, the
 * root's multiplied from the left by r_rot_quat), recover_from_real_rot (:1337-1345; forward_kinematics_real_cont6d, skeleton.py:200-222)
 * and process_pos_from_real_rot (:1366-1378; root-relative rows; stated deviation: the reference subtracts the root's x and z in place from the
 * storage it reads, so what it returns depends on how torch splits the loop, and a short clip loses the subtraction altogether).
 * data_dev: element (b, t, f) at data_dev[b * stride_batch + t * stride_frame + f * stride_feat], as mst_fit_joints reads it; mean_dev /
 * std_dev: [feats], both or neither, applied as x * std + mean.  lengths_dev: [batch] int32, 1 <= len <= frames, or NULL; the kernel clamps
 * the values into that range, so no access leaves a clip (the Python handle checks them).  The kinematic chains flattened as in
 * mst_encode_motion; every joint 1 .. joints - 1 is a child of exactly one chain.  offsets_host: [joints][3], the bone offsets of the
 * forward kinematics (row 0 unused).  Routes 0 and 2: out_source_host[out_joints], expanded joint -> the joint whose world quaternion it carries
 * (-1: the identity), and out_parents_host[out_joints] (entry 0 ignored) -- both a pure function of the chains, formed on the host; they
 * are read only when quats_dev is given.  Route 1: out_joints = joints, both NULL.
 * Outputs, each optional (NULL: not written), at least one: quats_dev [batch][frames][out_joints][4] local quaternions (w, x, y, z),
 * root_pos_dev [batch][frames][3], joints_dev [batch][frames][joints][3], local_dev [batch][frames][3 * (joints - 1)] (route 1 only).
 * Rows at or past a clip's length: exact zeros.  Not reproduced: rotm2axangle's SVD branch for an angle that is an exact multiple of pi.
 * Refused here: a route that is none of the three, route 2 without face joints or raw offsets or with a face joint outside the skeleton, joints outside 2 .. mst_rot_decode_max_joints, feats that are not the route's, frames < 1 or above
 * mst_rot_decode_max_frames, batch outside 1..65535, null data or skeleton, one of mean / std without the other, no output, local_dev on
 * route 0, a chain shorter than two joints, starting at a joint not yet placed, or naming a joint outside the skeleton or twice as a
 * child, a joint no chain names, out_joints out of range, a gather map that names a joint >= joints, a parent outside the expanded skeleton.
 * ----------------------------------------------------------------------------------------- */
int mst_rot_decode(const float* data_dev, int64_t stride_batch, int64_t stride_frame, int64_t stride_feat, const float* mean_dev,
                   const float* std_dev, const int32_t* lengths_dev, int32_t batch, int32_t frames, int32_t feats, int32_t joints,
                   int32_t route, const int32_t* chains_host, const int32_t* chain_starts_host, int32_t num_chains,
                   const float* offsets_host, const int32_t* face_ids_host, const float* raw_offsets_host,
                   const int32_t* out_source_host, const int32_t* out_parents_host, int32_t out_joints,
                   float* quats_dev, float* root_pos_dev, float* joints_dev, float* local_dev, void* stream);
/* Most joints mst_rot_decode takes: a lane keeps 16 floats a joint of chain state in scratch memory (24 joints: 1536 bytes a lane). */
int mst_rot_decode_max_joints(void);
/* Longest clip mst_rot_decode takes: LDS holds the scans' wave totals alone (96 bytes), so the bound is time -- 16 rounds of 256 frames
 * at the cap of 4096, what the windowed loops return.  -1 for joints outside 2 .. mst_rot_decode_max_joints. */
int mst_rot_decode_max_frames(int32_t joints);

/* -------------------------------------------------------------------------------------------
 * The T2M evaluators (data_loaders/humanml/networks/modules.py: MovementConvEncoder, MotionEncoderBiGRUCo, TextEncoderBiGRUCo) and the
 * statistics of data_loaders/humanml/utils/metrics.py, as building blocks: mst_amd.data_loaders.evaluator_wrapper and mst_amd.utils.metrics
 * chain them.  Everything is fp32 -- operands, accumulation (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, two chains an output), hidden
 * state, expf / tanhf -- and the covariance double: an evaluator is the instrument the sampler is measured with.  No atomics: every
 * result is a fixed-order sum, so a row does not depend on what else is in the batch.  All pointers are device pointers; every launch
 * goes to `stream`; nothing is allocated and nothing synchronises.
 *
 * mst_eval_gemm: c[m][n] = act(sum_k A[m][k] w[n][k] + bias[n] + add[m][n]); bias and add optional, act LeakyReLU(0.2) when leaky.
 * Any M, N, K >= 1.  mode 0: A[m][k] = a[m * lda + k].  mode 1, Conv1d(channels, N, 4, 2, 1) over rows a[b][frame][0 .. ldx): M =
 * batch * T_out, T_out = (frames_in - 2) / 2 + 1, K = 4 * channels, k = tap * channels + channel (the weight laid out [N][4][channels]),
 * output frame t reads frames 2 t - 1 + tap, frames outside the clip are zero; channels <= ldx drops trailing features.  mode 2: the same
 * over a sample a[b][feature][0][frame] (ldx features).  stride_batch: elements between clips.  scale / shift [channels], both or neither,
 * modes 1 and 2: every value read becomes x * scale + shift (the padding stays zero).
 *
 * mst_eval_gru: torch's bidirectional one-layer GRU over packed sequences, final hidden states only.  xproj [batch][positions][2][3][width]
 * holds W_ih x + b_ih (gates r, z, n); w_hh [2][3 width][width], b_hh [2][3 width], hidden [2][1][width] the initial state, broadcast.
 * Clip b takes part in steps 0 .. steps_dev[b] - 1 (clamped into 0 .. positions); the forward direction reads position s, the backward
 * one steps[b] - 1 - s; a finished clip's state is carried.  max_steps (host): the number of step launches, the largest steps[b].
 * work: 2 * batch * 2 * width floats; out [batch][2][width]: gru_last, forward then backward.  width a multiple of 64.
 *
 * mst_eval_layernorm: y = LeakyReLU?((x - mean) / sqrt(var + eps) * gamma + beta) per row, two-pass, biased variance.
 *
 * mst_eval_dist_rank: dist[i][j] = sqrt(-2 e1[i].e2[j] + |e1[i]|^2 + |e2[j]|^2) in fp32 (the reference's expansion; it yields NaN
 * where rounding makes the radicand negative, this 0).  Only a radicand below zero is clamped: NaN and +inf pass through the root as
 * they do there, so a non-finite row of e1 (e2) gives a non-finite row (column) of dist, never 0.  rank (optional,
 * n1 == n2): per row the number of entries strictly below the diagonal one -- calculate_R_precision's top-k is rank < k; a NaN entry is
 * not below anything, and a row whose diagonal entry is not finite gets rank n2, in no top-k (the reference's argsort puts NaN last and
 * ranks an all-NaN row by position).  d <= 8192.
 *
 * mst_eval_cov: mean[d] and, when cov is given (n >= 2), the (n - 1)-normalised covariance [d][d] of fp32 rows a[n][d], in double, the
 * mean subtracted before the products (np.cov(rowvar=False)).
 *
 * mst_eval_pair_norms: out[k] = |a[ia[k]] - b[ib[k]]|, summed in fp32; an index outside its matrix gives NaN.
 * ----------------------------------------------------------------------------------------- */
int mst_eval_gemm(const float* a_dev, const float* w_dev, const float* bias_dev, const float* add_dev, float* c_dev, int32_t m, int32_t n,
                  int32_t k, int64_t lda, int64_t ldc, int64_t ldadd, int32_t mode, int32_t batch, int32_t frames_in, int32_t channels,
                  int64_t ldx, int64_t stride_batch, const float* scale_dev, const float* shift_dev, int32_t leaky, void* stream);
int mst_eval_gru(const float* xproj_dev, const float* w_hh_dev, const float* b_hh_dev, const float* hidden_dev, const int32_t* steps_dev,
                 int32_t batch, int32_t positions, int32_t width, int32_t max_steps, float* work_dev, float* out_dev, void* stream);
int mst_eval_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* y_dev, int32_t rows, int32_t width,
                       float eps, int32_t leaky, void* stream);
int mst_eval_dist_rank(const float* e1_dev, const float* e2_dev, int32_t n1, int32_t n2, int32_t d, float* dist_dev, int32_t* rank_dev,
                       void* stream);
int mst_eval_cov(const float* a_dev, int32_t n, int32_t d, double* mean_dev, double* cov_dev, void* stream);
int mst_eval_pair_norms(const float* a_dev, const float* b_dev, const int32_t* ia_dev, const int32_t* ib_dev, int32_t pairs, int32_t na,
                        int32_t nb, int32_t d, float* out_dev, void* stream);

/* -----------------------------------------------------------------------------------------
 * CLIP's text tower (csrc/mst_clip.h).  Replaces: clip_model.encode_text of model/mdm_forstyledataset.py's encode_text -- token and
 * positional embedding, `layers` pre-LayerNorm blocks (width 512, 8 heads of 64, causal attention, FFN 2048 with QuickGELU), ln_final on
 * the row of the end-of-text token and `@ text_projection`.  Only the live rows of a prompt (0 .. its end-of-text position) are
 * computed, packed into one row range for the whole batch.  The residual stream is fp32 throughout; GEMM operands are f16
 * (v_mfma_f32_16x16x32_f16, fp32 accumulation); LayerNorm, softmax and QuickGELU are fp32.  No atomics, no split-K: every output is a
 * fixed-order sum that depends neither on the batch nor on where the prompt's rows lie, so a prompt encodes to the same bits alone
 * and in any batch.  All pointers but `layer_host` and the plan's arrays are device pointers; every launch goes to `stream`; nothing
 * is allocated and nothing synchronises.
 *
 * mst_clip_pack_weight: a row-major [n][k] matrix (out features x in features; float32, or f16 when src_is_f16) -> n * k halves in the
 * MFMA fragment order the GEMMs read.  n a multiple of 16, k of 32.  For in_proj_weight [1536][512], out_proj [512][512], c_fc
 * [2048][512] and c_proj [512][2048].
 * mst_clip_plan (host only): lens_host[b] = live rows of prompt b (end-of-text position + 1, 1 .. context) -> offsets_host[b], the
 * first packed row of prompt b, their total and the workspace a call needs.
 * mst_clip_encode: ids [batch][ids_stride] int32 (ids_stride <= context; an id outside 0 .. vocab - 1 is clamped, the caller
 * validates), lens / offsets as planned (device copies; rows a mismatched plan would put outside 0 .. total_rows - 1 are not
 * computed) -> out float32 [batch][512].  The table: tok_emb f16 [vocab][512], pos_emb f16 [context][512], proj f16 [512 in][512 out]
 * (text_projection as stored, applied as x @ P), LayerNorm vectors and biases float32, the four matrices of a layer packed.
 * Width 512, 8 heads and FFN 2048 are the only tower built: anything else is refused by name.
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_clip_layer {
    const float* ln1_g_dev;
    const float* ln1_b_dev;
    const void* wqkv_dev;  /* packed [1536][512], rows q | k | v */
    const float* bqkv_dev;
    const void* wo_dev;    /* packed [512][512] */
    const float* bo_dev;
    const float* ln2_g_dev;
    const float* ln2_b_dev;
    const void* w1_dev;    /* packed [2048][512] */
    const float* b1_dev;
    const void* w2_dev;    /* packed [512][2048] */
    const float* b2_dev;
} mst_clip_layer;

typedef struct mst_clip_weights {
    int32_t layers, vocab, context, width, heads, ffn;
    const void* tok_emb_dev;
    const void* pos_emb_dev;
    const float* lnf_g_dev;
    const float* lnf_b_dev;
    const void* proj_dev;
    const mst_clip_layer* layer_host; /* host array of `layers` entries */
} mst_clip_weights;

int mst_clip_pack_weight(const void* src_dev, int32_t src_is_f16, int32_t n, int32_t k, void* dst_dev, void* stream);
int mst_clip_plan(const int32_t* lens_host, int32_t batch, int32_t context, int32_t* offsets_host, int32_t* total_rows,
                  int64_t* workspace_bytes);
int mst_clip_encode(const mst_clip_weights* w, const int32_t* ids_dev, int32_t batch, int32_t ids_stride, const int32_t* lens_dev,
                    const int32_t* offsets_dev, int32_t total_rows, void* workspace_dev, int64_t workspace_bytes, float* out_dev,
                    void* stream);

/* -----------------------------------------------------------------------------------------
 * The SMPL body (csrc/mst_smpl.h), forward only, fp32.  Replaces: smplx.SMPLLayer's forward (`lbs`) under model/smpl.py:86-97 and the
 * conversions, masking, root subtraction and translation of model/rotation2xyz.py:17-92 (Rotation2xyz.__call__), called by
 * visualize/vis_utils.py:37 and visualize/render_final.py:62.  Stateless: every pointer but the `_host` ones is a device pointer,
 * every launch goes to `stream`, nothing is allocated and nothing synchronises.  No atomics, no split-K: a frame's output is a
 * fixed-order sum of its own operands and depends on neither the batch, its position in it, other clips' lengths nor the stream.
 * Only bodies of 24 joints are built.
 *
 * mst_smpl_packed_bytes / mst_smpl_pack_body: posedirs [207][3 vertices] (row k = 9 (joint - 1) + 3 row + column of R - I, column
 * 3 vertex + axis) and shapedirs [vertices][3][10] -> the operand image mst_smpl_skin streams: per tile of 32 vertices 224 rows
 * (207 pose rows, 10 shape rows, 7 zeros) x 96 columns in MFMA fragment order.  Once per body.
 * mst_smpl_workspace_bytes: what one call chain (pose -> skin -> regress) needs for `live` frames; keep_vertices != 0 adds the
 * [live][vertices][3] vertices mst_smpl_regress reads.  The three entries carve it alike from (live, vertices, keep_vertices).
 * mst_smpl_pose (rotation2xyz.py:38-66 and lbs' joints): element (b, j, f, t) of the sample at x_dev[b * stride_batch + j * stride_joint +
 * f * stride_feat + t * stride_frame], read where it lies.  frame_ids_dev [live]: b * frames + t of every live frame in ascending
 * order (values are clamped into the sample), or NULL when batch = 1 and every frame is live.  pose_rep 0 rot6d (6 features; the
 * reference's own column form, utils/rotation_conversions.py:536-551, no epsilon), 1 rotmat (9), 2 rotquat (4; :38-66), 3 rotvec (3;
 * :448-478 with its branch at 1e-6).  glob != 0: sample row 0 is the global orientation and rows 1 .. 23 the body pose; glob = 0:
 * glob_rot_host[3], one axis-angle for every frame, and sample rows 0 .. 22.  betas_dev [live][10], or NULL for (0, beta, 0, ...).
 * j0_dev [24][3] and jdirs_dev [24][3][10]: J_regressor (v_template + shapedirs beta) split into its constant and its linear part (the
 * host forms them in double).  parents_host[24]: parents[0] = -1, parents[j] < j.  Writes the workspace (the transforms A [live][24][12],
 * the operand rows [live][224], the posed joints [live][24][3]); rotations_dev [live][24][3][3] (optional): the matrices;
 * joints_out_dev [batch][24][3][frames] (optional; jointstype 'smpl'): the posed joints minus joint 0, plus trans[t] - trans[0] when
 * trans_joint >= 0 names the sample row whose features 0 .. 2 are the translation.  Frames that are not live are not written.
 * mst_smpl_skin (lbs' vertices): v_posed = v_template + [R - I, beta] [posedirs; shapedirs], T[v] = sum_j W[v][j] A[j] over all 24
 * joints in ascending order, vertex = T [v_posed; 1], + trans[t] - trans[0] when trans_dev is given (element (b, axis, t) at
 * trans_dev[b * trans_stride_batch + axis * trans_stride_axis + t * trans_stride_frame]).  Element (b, t, v, axis) goes to
 * out_dev[b * out_stride_batch + t * out_stride_frame + v * out_stride_vertex + axis * out_stride_axis]: the reference's
 * [batch][vertices][3][frames] and a [batch][frames][vertices][3] sequence layout are the same store.  out_dev = NULL: into the
 * workspace's vertices, for mst_smpl_regress.  weights_dev [vertices][24], v_template_dev [vertices][3].
 * mst_smpl_regress (smpl.py:89-95): the list of 54 = 24 posed joints | the vertices at vertex_ids_host[21] | extra_dev [9][vertices]
 * times the vertices (summed in double, fixed order); output joint i is entry map_host[i], minus entry map_host[root] (root = -1:
 * nothing subtracted), plus the translation -> out_dev [batch][map_len][3][frames].
 * Refused without touching a device: null pointers, vertices <= 0, live < 1, joints != 24, parents[0] != -1 or a parents entry that is
 * not an earlier joint, a pose_rep outside 0 .. 3, a sample with too few rotation rows, a vertex id outside the body, a map entry outside
 * 0 .. 53, a root outside the list, a missing frame-id list when more than one clip or not every frame is live.
 * ----------------------------------------------------------------------------------------- */
int64_t mst_smpl_packed_bytes(int32_t vertices);
int64_t mst_smpl_workspace_bytes(int32_t live, int32_t vertices, int32_t keep_vertices);
int mst_smpl_pack_body(const float* posedirs_dev, const float* shapedirs_dev, int32_t vertices, float* packed_dev, void* stream);
int mst_smpl_pose(const float* x_dev, int64_t stride_batch, int64_t stride_joint, int64_t stride_feat, int64_t stride_frame,
                  const int32_t* frame_ids_dev, int32_t live, int32_t batch, int32_t frames, int32_t sample_joints, int32_t joints,
                  int32_t vertices, int32_t keep_vertices, int32_t pose_rep, int32_t glob, const float* glob_rot_host,
                  const float* betas_dev, float beta, const float* j0_dev, const float* jdirs_dev, const int32_t* parents_host,
                  int32_t trans_joint, void* workspace_dev, float* rotations_dev, float* joints_out_dev, void* stream);
int mst_smpl_skin(const float* packed_dev, const float* v_template_dev, const float* weights_dev, int32_t vertices, int32_t keep_vertices,
                  const int32_t* frame_ids_dev, int32_t live, int32_t batch, int32_t frames, void* workspace_dev, const float* trans_dev,
                  int64_t trans_stride_batch, int64_t trans_stride_axis, int64_t trans_stride_frame, float* out_dev,
                  int64_t out_stride_batch, int64_t out_stride_frame, int64_t out_stride_vertex, int64_t out_stride_axis, void* stream);
int mst_smpl_regress(void* workspace_dev, const float* extra_dev, const int32_t* vertex_ids_host, int32_t vertices,
                     const int32_t* frame_ids_dev, int32_t live, int32_t batch, int32_t frames, const int32_t* map_host, int32_t map_len,
                     int32_t root, const float* trans_dev, int64_t trans_stride_batch, int64_t trans_stride_axis,
                     int64_t trans_stride_frame, float* out_dev, void* stream);

/* -----------------------------------------------------------------------------------------
 * The SMPLify-3D objective (csrc/mst_smplify.h): value and gradient of one stage of the fit for every frame of a clip, fp32, the
 * reverse pass written by hand.  Replaces, per evaluation of an optimiser's closure: the smplx forward pass, camera_fitting_loss_3d and
 * body_fitting_loss_3d (visualize/joints2smpl/src/customloss.py:6-21, :128-226), MaxMixturePrior.merged_log_likelihood
 * (prior.py:180-195) and `loss.backward()` (smplify.py:168-181, :218-235, :260-272).  No vertex is formed: the posed joints are
 * J0 + Jdirs beta through the rigid chain.  Stateless: every pointer but the `_host` ones is a device pointer, every launch goes to
 * `stream`, nothing is allocated and nothing synchronises; at most two launches.  No atomics, no split-K: a frame's loss and gradients
 * are the same bits alone, anywhere in a batch and on any stream, whatever other frames hold.
 *
 * mst_smplify_packed_prior_bytes / mst_smplify_pack_prior: precisions_dev [8][69][69] -- the SYMMETRIC part 1/2 (P + P^T) of the
 * float32 precisions, formed by the host in double -- means_dev [8][69] and neg_log_weights_dev [8] = -log(nll_weights) -> the operand
 * image of the kernel (precisions in MFMA fragment order, K = 69 padded to 72, five 16-row tiles).  Once per prior.
 * mst_smplify_workspace_bytes: [frames][24][3] floats, 256-byte aligned.  After a call the workspace holds the posed joints (no camera
 * translation) of every frame: what guess_init_3d (smplify.py:19-40) reads.
 * mst_smplify_objective: stage 0 (camera): sum over the joints 2, 1, 17, 16 of |target - (joint + cam)|^2 + depth^2 |cam - cam_est|^2;
 * gradients to global_orient and camera_translation only.  The reference's broadcast adds its depth term once per selected joint
 * (customloss.py:219-226): the caller states that as depth = 2 x 100.  stage 1 (body): joint^2 sum_j conf_j^2 sum_c gmof(joint + cam -
 * target, sigma) + prior^2 min_m [1/2 d_m^T P_m d_m - log nll_weight_m] + angle^2 sum exp(s_i pose[i])^2 over entries 52, 55, 9, 12
 * (signs +, -, -, -) + shape^2 |betas|^2 + keep^2 |body_pose - preserve|^2; the smallest component wins, ties to the lowest index.
 * body_pose_dev [frames][69], global_orient_dev [frames][3], betas_dev [frames][10], camera_translation_dev [frames][3], target_dev
 * [frames][nj][3] with nj = 22 ('AMASS') or 24 ('orig'), conf_dev [nj], preserve_dev [frames][69], camera_estimate_dev [frames][3],
 * j0_dev [24][3], jdirs_dev [24][3][10], parents_host[24].  Rotations are smplx's batch_rodrigues form as recalled (not verified, see
 * csrc/mst_smplify.h): |theta + 1e-8|, K = skew(theta / angle), I + sin K + (1 - cos) K K.  Outputs: per_frame_dev [frames]; loss_dev [1]
 * (optional): their sum in double in ascending frame order, rounded once; grad_*_dev in the operands' layouts, each optional (NULL: not
 * computed and nothing written); rotations_dev [frames][24][3][3] (optional).
 * Refused without touching a device: null operands, frames < 1, nj not 22 or 24, a stage outside 0 .. 1, the stage's own operands
 * missing, a body-pose or betas gradient asked of the camera stage, parents[0] != -1 or a parents entry that is not an earlier joint.
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_smplify_weights {
    float sigma, joint, prior, angle, shape, keep, depth;
} mst_smplify_weights;

int64_t mst_smplify_packed_prior_bytes(void);
int mst_smplify_pack_prior(const float* precisions_dev, const float* means_dev, const float* neg_log_weights_dev, void* packed_dev,
                           void* stream);
int64_t mst_smplify_workspace_bytes(int32_t frames);
int mst_smplify_objective(int32_t stage, int32_t nj, int32_t frames, const float* body_pose_dev, const float* global_orient_dev,
                          const float* betas_dev, const float* camera_translation_dev, const float* target_dev, const float* conf_dev,
                          const float* preserve_dev, const float* camera_estimate_dev, const float* j0_dev, const float* jdirs_dev,
                          const int32_t* parents_host, const void* packed_prior_dev, const mst_smplify_weights* weights_host,
                          void* workspace_dev, float* per_frame_dev, float* loss_dev, float* grad_body_pose_dev,
                          float* grad_global_orient_dev, float* grad_betas_dev, float* grad_camera_translation_dev, float* rotations_dev,
                          void* stream);

/* -----------------------------------------------------------------------------------------
 * Pose tracks (csrc/mst_track.h): a video pose estimator's per-frame output -> joints at the model's frame rate.  Replaces
 * `downsample`, `joints_downsample` and the frame loop of `amass_to_pose` (utils/process_smpl_from_hybrik.py:56-180) and the fractional
 * branch of read_bvh (data_loaders/humanml/common/bvh_utils.py:251-287).  Stateless: one launch on `stream`, nothing allocated,
 * nothing synchronised.  No atomics; a clip's outputs are the same bits alone, anywhere in a batch and on any stream, whatever other
 * clips or the rows behind its length hold.
 *
 * The rate is the rational up / down: a clip of L source frames has the output frames k with k * down < (L - 1) * up -- the reference
 * resamples intervals, so the source's last frame is dropped even at rate 1 -- taken from the interval i = (k * down) / up at
 * t = ((k * down) % up) / up.  Outputs hold ceil((frames - 1) * up / down) rows a clip; rows at and behind a clip's own count are
 * exact zeros.  lengths_dev [batch] int32 or NULL (every clip has `frames`); values are clamped to 1..frames.
 *
 * mst_track_resample: quats_dev [batch][frames][joints][4] (w first) through `qslerp` in float32 -- both ends normalised,
 * qmul(q1, qinv(q0)), qpow with its 10e-10 guard, qmul with q0; shortest != 0 negates the relative quaternion when its w is negative --
 * and points_dev [batch][frames][points][3] through p0 + t (p1 - p0) in double, stored as float32.  Either track may be absent (NULL
 * with a count of 0).
 * mst_track_joints: rotations_dev [batch][frames][rot_joints][4], or with is_matrix [..][3][3] (converted by the closed form of the
 * reference's rotm2q, on the largest of the four diagonal combinations; the shorter arc is then always taken), resampled as above,
 * `q2axangle`, Rodrigues (the form of mst_smplify_objective), J = j0_dev [22][3] + jdirs_dev [22][3][10] betas_dev [batch][10], the
 * rigid chain over parents_host [22] -- only the first 22 joints of a frame are read -- plus the resampled transl_dev
 * [batch][frames][3] under with_trans, re-axed (x and z swapped, y negated) into out_dev [batch][rows][22][3].  est_joints_dev
 * [batch][frames][est_joint_count][3] (optional): the estimator's own joints through the same lerp, translation, re-axing and [:22]
 * into est_out_dev.
 * Refused without touching a device: batch < 1 (mst_track_joints: > 65535), frames outside 2..mst_track_max_frames, up or down outside
 * 1..100000, a joint or point count outside its range, a count that disagrees with its pointer, an output that is its input, null
 * operands, with_trans without transl_dev, parents[0] != -1 or a parents entry that is not an earlier joint.
 * mst_track_max_frames: the longest source clip (16384); -1 for joints outside 1..4096.
 * ----------------------------------------------------------------------------------------- */
int mst_track_resample(const float* quats_dev, const float* points_dev, const int32_t* lengths_dev, int32_t batch, int32_t frames,
                       int32_t joints, int32_t points, int32_t up, int32_t down, int32_t shortest, float* quats_out_dev,
                       float* points_out_dev, void* stream);
int mst_track_joints(const float* rotations_dev, int32_t is_matrix, int32_t rot_joints, const float* transl_dev, const float* betas_dev,
                     const float* est_joints_dev, int32_t est_joint_count, const int32_t* lengths_dev, int32_t batch, int32_t frames,
                     int32_t up, int32_t down, int32_t shortest, int32_t with_trans, const float* j0_dev, const float* jdirs_dev,
                     const int32_t* parents_host, float* out_dev, float* est_out_dev, void* stream);
int mst_track_max_frames(int32_t joints);

/* -----------------------------------------------------------------------------------------
 * Clips to video frames (csrc/mst_render.h): joints -> [batch][frames][height][width][3] uint8 images of the stick figure over its
 * ground plane, with root or joint traces.  Replaces the per-frame matplotlib redraw of `explicit_plot_3d_motion`
 * (data_loaders/humanml/utils/plot_script.py:168-311): its scene, drawn by the rules below, not by matplotlib's rasteriser.
 * Stateless: one launch each on `stream`, nothing allocated, nothing synchronised.  No atomics; a clip's frames are the same bits
 * alone, anywhere in a batch, on any stream and for any frame sub-range, whatever other clips or the frames behind its length hold.
 * Frames at and behind a clip's length are exact zeros.  All arithmetic is float32 without fused multiply-adds.
 *
 * mst_render_scene: joints_dev element (b, t, j, c) lies at b * stride_batch + t * stride_frame + j * stride_joint + c * stride_coord
 * (elements; [B][T][J][3] and [B][J][3][T] are both a choice of strides); joints2_dev (optional) is a second skeleton with the same
 * strides; lengths_dev [batch] int32 or NULL (every clip has `frames`), clamped to 1..frames.
 *
 * mst_render_bounds (:221-225, :243): bounds_dev [batch][8] = MINS xyz, MAXS xyz of scale * joints over the clip's live frames, all
 * joints and both skeletons, then two zeros.  Minimum and maximum pass over NaN (fmin / fmax).
 *
 * mst_render_frames (:257-305), frame t of a clip, everything relative to (traj[t].x, 0, traj[t].z), traj[t] = scale * joints[t, 0]:
 *   W[k, j] = scale * joints[k, j] with y -= MINS.y; a point of frame k seen from frame t is W[k, j] - (traj[t].x, 0, traj[t].z).
 *   Ground quad: (MINS.x, 0, MINS.z), (MINS.x, 0, MAXS.z), (MAXS.x, 0, MAXS.z), (MAXS.x, 0, MINS.z), each minus traj[t] in x and z;
 *     0.5 grey at alpha 0.5; coverage clamp(0.5 + min over the edges of the signed distance, 0, 1) in pixels, the sign from the
 *     quad's area; an edge of no length is passed over; coverage 0 where |area| < 1e-12 px^2 or a corner is not drawn.
 *   Chains: the first mst_render_chains_drawn() (5: the reference's zip with a five-colour palette stops there) of the chains given,
 *     each one polyline of width 4 pt in colour [palette][chain]; with joints2 its chain right after the first skeleton's same chain,
 *     in the same colour.  palette_dev [batch][frames] int32 (0 blue, 1 orange, 2 purple, 3 upper_body; NULL: orange; clamped).
 *   Traces, each one polyline of width 2 pt in colour [palette][0]: kind 0 (root_horizontal) joint 0 at frames k < t with y = 0,
 *     kind 1 (root) joint 0 at k < t, kind 2 joint trace_joints[i] at k <= t.  Fewer than 2 points draw nothing.
 *   Polyline coverage: clamp((w / 2 + 0.5) - d, 0, 1), w = pt * dpi / 72 pixels, d the minimum over the polyline's segments of the
 *     distance from the pixel centre to the segment (parameter clamped to [0, 1], a segment of no length is a point).  A point is not
 *     drawn when a coordinate is not finite or its projective w is not positive and finite; a segment with such an end is skipped.
 *     One polyline is one layer.
 *   Projection: (X, Y, . , w) = proj (x, y, z, 1) (row-major 4 x 4; the depth row is not read), pixels = affine (X / w, Y / w, 1)
 *     (row-major 2 x 3), y up: pixel (row, col) has its centre at (col + 0.5, height - row - 0.5).
 *   Compositing: straight-alpha over, c = c (1 - a) + colour a, on white, in the order quad, chains, traces, then overlay_dev
 *     [overlay_batch = 1 or batch][height][width] uint8 (optional) as coverage / 255 in black.  out_dev = floor(255 c + 0.5);
 *     out_float_dev (optional) is c itself in the same layout.  Frames t0 <= t < t1 are rendered into t1 - t0 output frames; traces
 *     still reach back to frame 0.
 * Refused without touching a device: a null scene, view, joints, bounds or output; batch outside 1..65535; frames outside
 * 1..mst_render_max_frames (4096); joints outside 1..mst_render_max_joints (64); a stride below 1; a scale or dpi that is not finite
 * (dpi: and positive); width or height outside 16..mst_render_max_side (1024); more than 16 chains, or more than 128 points in the
 * chains drawn; a chain or trace joint outside 0..joints-1; a trace kind outside 0..2; more than mst_render_max_traces (8) traces;
 * an overlay batch that is neither 1 nor batch; a range that is not 0 <= t0 < t1 <= frames; an output that is an input or the other
 * output.  mst_render_chunk: the polyline points a workgroup holds on chip at a time (512).
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_render_scene {
    const float* joints_dev;
    const float* joints2_dev;
    int64_t stride_batch, stride_frame, stride_joint, stride_coord;
    const int32_t* lengths_dev;
    int32_t batch, frames, joints;
    float scale;
} mst_render_scene;
typedef struct mst_render_view {
    int32_t n_chains;
    const int32_t* chain_offsets_host;        /* [n_chains + 1], from 0 */
    const int32_t* chain_joints_host;
    int32_t n_traces;
    const int32_t* trace_kinds_host;          /* [n_traces] */
    const int32_t* trace_joints_host;         /* [n_traces]; read for kind 2 */
    const int32_t* palette_dev;
    float proj[16];
    float affine[6];
    int32_t width, height;
    float dpi;
    const uint8_t* overlay_dev;
    int32_t overlay_batch;
    int32_t t0, t1;
} mst_render_view;
int mst_render_bounds(const mst_render_scene* scene_host, float* bounds_dev, void* stream);
int mst_render_frames(const mst_render_scene* scene_host, const float* bounds_dev, const mst_render_view* view_host, uint8_t* out_dev,
                      float* out_float_dev, void* stream);
int mst_render_max_frames(void);
int mst_render_max_joints(void);
int mst_render_chains_drawn(void);
int mst_render_max_traces(void);
int mst_render_max_side(void);
int mst_render_chunk(void);

/* -----------------------------------------------------------------------------------------
 * Meshes to video frames (csrc/mst_mesh.h): posed vertices -> [batch][frames][height][width][4] uint8 RGBA images of the shaded body
 * over a translucent background.  Replaces the per-frame pyrender draw of `render` (visualize/render_final.py:79-89, :169-251): its
 * scene and camera, drawn by the rules below, not by pyrender / OpenGL.  Stateless: one launch each on `stream`, nothing allocated,
 * nothing synchronised.  No atomics; a clip's frames are the same bits alone, anywhere in a batch, on any stream and for any frame
 * sub-range, whatever other clips or the frames behind its length hold.  Frames at and behind a clip's length are exact zeros (the
 * face-index image: -1).  All arithmetic is float32 without fused multiply-adds, division and square root correctly rounded.
 *
 * mst_mesh_scene: vertices_dev element (b, t, v, c) lies at b * stride_batch + t * stride_frame + v * stride_vertex + c * stride_coord
 * (elements; Rotation2xyz's [B][V][3][T] and [B][T][V][3] are both a choice of strides); lengths_dev [batch] int32 or NULL (every clip
 * has `frames`), clamped to 1..frames.  faces [faces][3] int32 and the vertex -> faces adjacency in CSR form (adj_offsets
 * [vertices + 1], adj_faces [3 faces]: the faces naming vertex v, ascending, a face once for each time it names v) are passed twice,
 * a host copy that is checked and a device copy that the kernels read.  mst_mesh_bounds reads neither.
 *
 * mst_mesh_bounds (:79-80): bounds_dev [batch][8] = MINS xyz, MAXS xyz of the vertices over the clip's live frames, then two zeros.
 * Minimum and maximum pass over NaN (fmin / fmax).
 *
 * mst_mesh_vertices, vertex v of frame t0 <= t < t1 of a clip, into workspace_dev (mst_mesh_workspace_bytes(batch, t1 - t0, vertices)):
 *   Normal: n = the sum over the vertex's faces (p0, p1, p2), in adjacency order, of cross(p1 - p0, p2 - p0), each component
 *     a * b - c * d; l = sqrt((nx nx + ny ny) + nz nz); n / l when 0 < l < inf, else n = 0.
 *   Shade: s = ambient + (1 - ambient) max((nx lx + ny ly) + nz lz, 0); `light` is the direction towards the light, used as given.
 *     (The reference's three directional lights (:221-229) are posed by translation only, so all three shine along -z: light (0, 0, 1);
 *     its ambient (:197) is 0.4.)
 *   Projection: (X, Y, Z, w) = proj (x, y, z, 1) (row-major 4 x 4: rows x, y, depth, w; proj_batch = 1 matrix for all clips or one a
 *     clip), each row ((m0 x + m1 y) + m2 z) + m3; pixels = affine (X / w, Y / w, 1) (row-major 2 x 3), y up: pixel (row, col) covers
 *     x in [col, col + 1], y in [height - row - 1, height - row]; depth = Z / w; 1 / w is kept.  A vertex is not drawn (all its
 *     values NaN) when a coordinate is not finite, w is not positive and finite, or a pixel, the depth or 1 / w is not finite.
 *   Also the pixel bounding box of the vertices drawn, one per workgroup of 256 vertices.
 * mst_mesh_frames, from the same scene, view and workspace:
 *   A face is never drawn when a vertex of it is not drawn or its doubled pixel area is zero or not finite.  There is no near-plane
 *     clipping: a face with a vertex behind the camera is dropped whole.
 *   Sample points: `samples` (1..4) a side of a pixel, sub-sample (j, i) of pixel (row, col) at x = col + (i + 0.5) / samples,
 *     y = (height - row) - (j + 0.5) / samples; sub-sample index j * samples + i.
 *   Coverage: the face's vertices in ascending vertex index L < M < H with pixels (xL, yL) ...; at sample (sx, sy)
 *       wH = (xM - xL)(sy - yL) - (yM - yL)(sx - xL),  wM = -((xH - xL)(sy - yL) - (yH - yL)(sx - xL)),
 *       wL = (xH - xM)(sy - yM) - (yH - yM)(sx - xM):
 *     each edge function is formed from its edge's lower-index end, so two faces sharing an edge form the same number: both cover a
 *     sample on the edge and there is no gap.  The doubled area is (xM - xL)(yH - yL) - (yM - yL)(xH - xL).  A sample is covered when
 *     it lies inside the face's pixel bounding box (bounds included), wL, wM, wH are all >= 0 or all <= 0, and sum = (wL + wM) + wH
 *     is not zero.
 *   Depth: ((wL zL + wM zM) + wH zH) / sum, the screen-space barycentric mean of the vertices' depths.  The winner is the minimum of
 *     (depth, face index) over the covering faces with a depth below +inf (NaN never wins); the face index breaks exact ties.
 *   Shade, perspective-correct: a = w / w_clip per vertex (aL = wL (1 / w)L ...), ((aL sL + aM sM) + aH sH) / ((aL + aM) + aH).
 *   Colour: rgb(frame) * shade composited over the background with the frame's alpha a: c = a surf + (1 - a) bg per channel, alpha
 *     a + (1 - a) bg_a; a sample no face covers is the background (bg_r, bg_g, bg_b, bg_a).  Only the nearest surface is composited.
 *     colors_dev [batch][frames][4] float32 RGBA per frame, or NULL: the reference's ramp (:184) for frame n of the clip,
 *     (1, min((145 + 0.8 n) / 255, 1), min((33 + 0.5 n) / 255, 1), 0.9).  The reference's background (:169) is (1, 1, 1, 0.8).
 *   Pixel: the sum of its sub-samples' colours in sub-sample order, divided by samples^2 last, clamped to 0..1 (NaN -> 0).
 *     out_dev = floor(255 c + 0.5), [batch][t1 - t0][height][width][4]; out_float_dev (optional) is c itself in the same layout;
 *     out_ids_dev (optional) int32 [batch][t1 - t0][height][width]: the winning face at sub-sample `ids_sample`, -1 for none.
 * Refused without touching a device: a null scene, view, vertices, workspace or output, null faces, adjacency or matrix (either copy);
 * batch outside 1..65535; frames outside 1..65535; vertices outside 1..mst_mesh_max_vertices (32768); faces outside
 * 1..mst_mesh_max_faces (65536); a stride below 1; a face naming a vertex outside 0..vertices-1; adjacency offsets that do not run
 * from 0 to 3 faces without falling, or an entry outside 0..faces-1; a proj_batch that is neither 1 nor batch; a matrix, affine, light,
 * ambient or background that is not finite; width or height outside 16..mst_mesh_max_side (1024); samples outside
 * 1..mst_mesh_max_samples (4); ids_sample outside 0..samples^2-1; a range that is not 0 <= t0 < t1 <= frames; a workspace smaller
 * than mst_mesh_workspace_bytes says (which returns 0 for counts outside the limits); an image that is not 4-byte aligned (float
 * image: 16); an output that is an input or another output.  mst_mesh_chunk: the faces a workgroup culls at a time (1024).
 * ----------------------------------------------------------------------------------------- */
typedef struct mst_mesh_scene {
    const float* vertices_dev;
    int64_t stride_batch, stride_frame, stride_vertex, stride_coord;
    const int32_t* lengths_dev;
    int32_t batch, frames, vertices, faces;
    const int32_t* faces_host;
    const int32_t* faces_dev;
    const int32_t* adj_offsets_host;
    const int32_t* adj_offsets_dev;
    const int32_t* adj_faces_host;
    const int32_t* adj_faces_dev;
} mst_mesh_scene;
typedef struct mst_mesh_view {
    const float* proj_host;                   /* [proj_batch][16] */
    const float* proj_dev;
    int32_t proj_batch;
    float affine[6];
    int32_t width, height, samples;
    float light[3];
    float ambient;
    const float* colors_dev;
    float background[4];
    int32_t t0, t1;
    int32_t ids_sample;
} mst_mesh_view;
int mst_mesh_bounds(const mst_mesh_scene* scene_host, float* bounds_dev, void* stream);
int mst_mesh_vertices(const mst_mesh_scene* scene_host, const mst_mesh_view* view_host, void* workspace_dev, uint64_t workspace_bytes,
                      void* stream);
int mst_mesh_frames(const mst_mesh_scene* scene_host, const mst_mesh_view* view_host, const void* workspace_dev, uint64_t workspace_bytes,
                    uint8_t* out_dev, float* out_float_dev, int32_t* out_ids_dev, void* stream);
uint64_t mst_mesh_workspace_bytes(int32_t batch, int32_t frames_out, int32_t vertices);
int mst_mesh_max_vertices(void);
int mst_mesh_max_faces(void);
int mst_mesh_max_side(void);
int mst_mesh_max_samples(void);
int mst_mesh_chunk(void);

/* Per-kernel device timing of the most recent mst_sample_loop / mst_forward when profiling is
 * enabled: HIP events recorded around every launch on the caller's stream.  names/ms are arrays
 * of `cap` entries filled with per-kernel-family totals; returns the number of families. */
int mst_profile_enable(mst_engine* e, int32_t on);
float mst_profile_event_overhead_us(const mst_engine* e);   /* what an empty HIP-event pair reports: the fixed part of every event-timed launch */
int mst_profile_read(mst_engine* e, const char** names, float* total_ms, int32_t* launches,
                     int32_t cap);

/* Precise mode (no reference counterpart: the reference computes in fp32, model/mdm_forstyledataset.py:539-546).  on != 0: every
 * layer GEMM of the sampling path (mst_forward, mst_sample_loop) multiplies its activation operand as hi + lo -- f16(x) and
 * f16(x - hi), ~22 significant bits -- instead of f16(x): for checkpoints whose statistics (LayerNorm-gain outlier channels, large
 * FFN / attention weights) put plain f16 operands above the 1e-3 relative-L2 bar.  Takes the small-tile kernels at any batch size
 * (about half the throughput of the default path at 64 clips); default off, also MST_PRECISE=1.
 * The weights' lo halves are written by mst_load_weight only while precise mode is on (a fine-tune iteration re-uploads 96 tensors and
 * never reads them).  Returns 0, or 2 when it was switched on over weights uploaded without them: upload those again (mst_forward /
 * mst_sample_loop fail until then). */
int mst_set_precise(mst_engine* e, int32_t on);

/* Resident-group trunk (no reference counterpart; csrc/mst_trunk.h).  on != 0: a sampling step's encoder stack (the 8 x [fused QKV +
 * attention, fused layer tail] of model/mdm_forstyledataset.py:539-546, 602-625) runs as ONE launch in which the four workgroups of a
 * clip stay resident and hand their phase outputs to each other through a per-clip arrival counter; shapes it does not cover (token
 * counts other than 193 .. 208, precise mode, debug stops, instrumented steps) keep the two launches per layer.  Results are
 * bit-identical either way.  Also MST_TRUNK=1 / 0.  mst_trunk_check: after the caller has synchronised, 0 when every hand-off of every
 * such launch arrived (a bounded wait that gives up sets a host-visible word instead of hanging the device). */
int mst_set_trunk_groups(mst_engine* e, int32_t on);

/* Several fine-tuned styles in one batch (csrc/mst_style.h).  Replaces: one StyleDiffusion per style, each sampled by its own loop
 * (sample/demo_style_transfer.py:74-85, 244-258); two styles differ only in model/mdm_forstyledataset.py:602-625's seqTransEncoder.
 * mst_style_slots: the engine holds n slots (n >= the current count).  Slot 0 is the engine's own weights (mst_load_weight /
 * mst_load_layers, training untouched); slots 1 .. n-1 hold only what sampling reads -- biases and LayerNorm vectors and the packed
 * matrices of the fused QKV + attention, fused tail and small-launch kernels (about 64 MB each at 8 layers). */
int mst_style_slots(mst_engine* e, int32_t n);
/* The 12 x num_layers stack tensors of one slot, in mst_load_layers' order (float32 device pointers), packed on `stream` as slot 0's
 * copies are packed (mst_load_layers for slot 0).  Not in precise mode (the extra slots have no lo halves). */
int mst_load_layers_slot(mst_engine* e, int32_t slot, const float* const* srcs_host_array, void* stream);
/* The slot of every clip of the next mst_forward / mst_sample_loop calls (host int32[batch], any order; under CFG a clip's
 * unconditional twin uses the clip's slot).  styles_host = NULL: back to the single-style behaviour.  With more than one slot the
 * calls refuse (and name) every configuration the style-aware kernels do not cover: precise mode, the resident trunk, MST_FUSE_TAIL=0,
 * MST_FUSE_QKV_ATTN other than 1, MST_SMALL_FAST=0, clips of <= 16 or > 207 frames, debug stops, graph replay, profiling.
 * A clip naming a slot that mst_load_layers_slot never filled (slot 0: weights incomplete) is refused here.  While styles are set,
 * mst_train_forward, mst_train_model_forward and mst_motion_encoder_forward refuse: training runs slot 0 only. */
int mst_set_styles(mst_engine* e, const int32_t* styles_host, int32_t batch, void* stream);
/* Host-only planner (no GPU): split every tile of `tile_rows` token rows of nclips x S rows into maximal runs of one slot.  Writes
 * {row0, row_lo, row_hi, slot} int32 records to out (at most cap of them); returns their count, or -1 (mst_last_error) if cap is
 * too small.  At most tiles + nclips records. */
int32_t mst_plan_style_segments(const int32_t* styles_host, int32_t nclips, int32_t S, int32_t tile_rows, int32_t* out, int32_t cap);
int mst_trunk_check(mst_engine* e);

/* Debug / test hooks (no reference counterpart): stop the encoder stack after (layer, stage) --
 * stage 0 = token stream assembled, 1 = QKV, 2 = attention, 3 = out-proj + LayerNorm1, 4 = FFN1,
 * 5 = FFN2 + LayerNorm2; layer = stage = -1 runs everything -- and copy a workspace buffer
 * ("hs" f32 stream, "hx"/"qkv"/"att"/"hid" f16, "temb"/"textproj" f32) into caller memory. */
int mst_debug_stop_after(mst_engine* e, int32_t layer, int32_t stage);
int mst_debug_copy(mst_engine* e, const char* which, void* dst_dev, uint64_t nbytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MST_ENGINE_H */
