/*
 * dad.h — C ABI of libdad_hip.so: the MI355X (gfx950) reverse-diffusion planning sampler.
 *
 * The reference (darshangm/dynamics-aware-diffusion) is 100 % Python and has no FFI seam;
 * its seam is the Python class API of m_diffuser.models / m_diffuser.guides that
 * scripts/evaluate.py consumes.  This library sits UNDER a Python
 * mirror of that API (dynamics_aware_diffusion_amd/) and is bound with ctypes.  Each entry
 * point names the reference function it replaces (paths under /root/reference/).
 *
 * Conventions
 *  - plain C types only; every function returns 0 on success or a negative DAD_E_* code;
 *    dad_last_error() returns a thread-local message.  Nothing throws or aborts.
 *  - device pointers are fp32, contiguous, owned by the caller (torch-ROCm tensors);
 *    trajectories use the reference's external layout (batch, horizon, transition_dim).
 *  - all work is enqueued asynchronously on the caller's hipStream_t (passed as void*);
 *    step functions never allocate: the caller passes a workspace of dad_workspace_bytes().
 *  - no process-wide mutable state: every knob (precision, debug hooks, caches, graphs) lives on
 *    the dad_model; the only statics are the immutable kernel table and a mutex-guarded set of
 *    devices whose kernels had their LDS limit raised.  One dad_model per device; calls on
 *    different models may run on different threads (thread-compatible: one thread per model).
 *  - ONE STREAM PER MODEL AT A TIME: the split-K arrival tickets, the Philox key cell and the
 *    persistent-step flags are owned by the dad_model, so two calls on the same model must not be in
 *    flight on different streams concurrently (enqueue them on one stream, or synchronise between
 *    streams; concurrent loops need one dad_model each, as bench.py --inflight builds them).
 */
#ifndef DAD_H
#define DAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAD_OK 0
#define DAD_E_INVALID (-1)   /* bad argument / unsupported shape                      */
#define DAD_E_STATE (-2)     /* call order violated (e.g. step before finalize)       */
#define DAD_E_KEY (-3)       /* unknown or duplicate weight key, or shape mismatch    */
#define DAD_E_HIP (-4)       /* a HIP runtime call failed (message has hipGetErrorString) */
#define DAD_E_RANGE (-5)     /* timestep outside the loaded schedule (reference: RuntimeError
                                from gather, m_diffuser/models/diffusion.py:28)       */
#define DAD_E_WORKSPACE (-6) /* workspace too small                                   */

#define DAD_MAX_LEVELS 8

/* How the conv GEMMs multiply (dad_model_set_precision).  Both accumulate in fp32 and meet the same
 * fp32 parity tolerance against the reference (m_diffuser runs F.conv1d in fp32):
 *   FP32   exact fp32 products on v_mfma_f32_32x32x2_f32 (default);
 *   F16X3  every fp32 operand carried as two halves (hi + lo*2^-11, 22 significant bits), three
 *          v_mfma_f32_32x32x16_f16 per product block; activations must stay within +-65504. */
#define DAD_PREC_FP32 0
#define DAD_PREC_F16X3 1

typedef struct dad_model dad_model;
typedef void* dad_stream_t; /* hipStream_t */

/* Architecture of the denoiser + diffusion constants.
 * Mirrors TemporalUnet.__init__ (m_diffuser/models/temporal_unet.py:135-197) and
 * GaussianDiffusion.__init__ (m_diffuser/models/diffusion.py:62-94). */
typedef struct dad_cfg {
    int32_t transition_dim;           /* observation_dim + action_dim                     */
    int32_t dim;                      /* width of the sinusoidal embedding                */
    int32_t time_dim;                 /* time-embedding width (reference: == dim)         */
    int32_t n_levels;                 /* len(dim_mults)                                   */
    int32_t channels[DAD_MAX_LEVELS]; /* dim * dim_mults[i] per level                     */
    int32_t kernel_size;              /* 3, 5 or 7 (temporal_unet.py:139; 5 in every recipe)  */
    int32_t horizon;                  /* planning horizon H: a power of two with
                                         H / 2^(n_levels-1) >= 4 (the deepest level keeps at
                                         least 4 positions; else DAD_E_INVALID)              */
    int32_t n_timesteps;              /* length T of the trained schedule                 */
    int32_t predict_epsilon;          /* diffusion.py:192-197                             */
    int32_t clip_denoised;            /* diffusion.py:199-200                             */
} dad_cfg;

const char* dad_last_error(void);
const char* dad_version(void);

/* Replaces: TemporalUnet(...) / GaussianDiffusion(...) construction + .to(device). */
int dad_model_create(const dad_cfg* cfg, dad_model** out);
void dad_model_destroy(dad_model* m);

/* Replaces: load_state_dict (scripts/evaluate.py:198).  `key` is the reference's
 * state_dict key WITHOUT the leading "model." (SURVEY.md Appendix C); `data` is a HOST
 * fp32 pointer in the reference's layout; the library packs and uploads its own copy.
 * May be called again for the same key before the next finalize (weights updated). */
int dad_model_load_weight(dad_model* m, const char* key, const float* data,
                          const int64_t* shape, int32_t ndim);

/* The five schedule buffers the reverse step reads (diffusion.py:117-128), HOST fp32,
 * each of length cfg.n_timesteps: sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod,
 * posterior_mean_coef1, posterior_mean_coef2, posterior_log_variance_clipped. */
int dad_model_load_schedule(dad_model* m, const float* sqrt_recip, const float* sqrt_recipm1,
                            const float* coef1, const float* coef2, const float* log_var);

/* Optional.  The SinusoidalPosEmb table (temporal_unet.py:19-32) for t = 0 .. n_timesteps-1,
 * HOST fp32 (n_timesteps, dim), computed by the caller: the Python mirror evaluates the
 * reference's own torch expression so the table is bit-identical to what the reference computes
 * on the same host.  Without it dad_model_finalize evaluates the same formula with libm. */
int dad_model_load_time_embedding(dad_model* m, const float* emb, int32_t n_timesteps, int32_t dim);

/* No reference counterpart (the reference computes in whatever dtype the module holds, fp32 in
 * scripts/evaluate.py): selects the conv arithmetic, DAD_PREC_*.  Takes effect at the next
 * dad_model_finalize (weights are re-packed); a finalized model must be finalized again. */
int dad_model_set_precision(dad_model* m, int32_t precision);

/* Widths the reference accepts and the conv-GEMM tiles do not — GroupNorm(8, C) needs only C % 8 == 0
 * (temporal_unet.py:71: `--dim 48`, `--dim 96`), the tiles a multiple of 32 with a power-of-two C / 8: the host
 * language pads every GroupNorm group of such a level with zero channels up to the next power of two >= 4 (weights,
 * biases, gamma / beta of the padding are zero: the padded net computes the same function), gives the PADDED widths
 * in dad_cfg and states the real ones here; the GroupNorm statistics then count the real channels only.  Call
 * between dad_model_create and dad_model_finalize.  Such models run the batch kernels at every batch size; they
 * train as the padded net (dad_unet_backward fills padded gradient tensors: the entries of the padding are garbage
 * the host language drops; the GroupNorm backward counts the real channels). */
int dad_model_set_group_channels(dad_model* m, const int32_t* real_channels, int32_t n_levels);

/* Horizons the reference accepts and the tiles do not: its U-Net takes any length every level can halve
 * (temporal_unet.py:35-54: H % 2^(levels-1) == 0 — 24, 48, 96, 100 ...), the conv-GEMM tiles whole power-of-two
 * samples.  Give the next power of two in dad_cfg.horizon and the real horizon here: every activation keeps the padded
 * layout with ZERO rows behind the real ones (exactly the zero padding a conv sees at the end of a sample), the
 * GroupNorm statistics count the real rows only, and the external tensors (x, noise, guide gradient, outputs) keep
 * the real shape (B, real_horizon, transition_dim).  Call between dad_model_create and dad_model_finalize.  Such models
 * run the batch kernels at every batch size; they train (the data gradients are zero-padded the same way). */
int dad_model_set_horizon(dad_model* m, int32_t real_horizon);
/* Checks every tensor is present, builds the per-timestep time-embedding tables
 * (SinusoidalPosEmb + time_mlp + every block's Mish->Linear, temporal_unet.py:19-32,
 * 97-100,155-160 — batch-invariant during sampling) and the launch plan. */
int dad_model_finalize(dad_model* m, dad_stream_t stream);

/* Bytes of device scratch one call at batch size B needs: the activation buffers of the launch
 * plan plus, for batches small enough to use grid-level split-K, the partial-tile slabs. */
int dad_workspace_bytes(const dad_model* m, int32_t batch, size_t* bytes);

/* Replaces: TemporalUnet.forward(x, t) with one shared timestep t
 * (temporal_unet.py:199-241).  x, out: (B, H, td) device fp32.  out = eps_theta(x, t). */
int dad_unet_forward(dad_model* m, const float* x, int32_t t, float* out, int32_t batch,
                     void* workspace, size_t workspace_bytes, dad_stream_t stream);

/* Replaces: TemporalUnet.forward(x, t) with one timestep PER ROW, as the training objective calls
 * it (GaussianDiffusion.loss, m_diffuser/models/diffusion.py:253-290: t ~ randint per trajectory).
 * t_rows: (B) int32 on the DEVICE, every entry in [0, n_timesteps) (the caller checks the range:
 * the library cannot without a device synchronisation).  Inference form (time embeddings from the
 * per-timestep tables); the differentiable form is dad_unet_forward_train below. */
int dad_unet_forward_rows(dad_model* m, const float* x, const int32_t* t_rows, float* out, int32_t batch,
                          void* workspace, size_t workspace_bytes, dad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training side: replaces loss.backward() through TemporalUnet in the reference's training step
 * (m_diffuser/utils/training.py:144-156; the objective is GaussianDiffusion.loss,
 * m_diffuser/models/diffusion.py:253-290).  The reference relies on torch autograd; here the
 * denoiser's backward pass is explicit:
 *   - data gradients of Conv1d / ConvTranspose1d (temporal_unet.py:35-54,70) run on the forward
 *     conv-GEMM kernels with transposed, tap-flipped weight images packed at dad_model_finalize;
 *   - weight gradients are an MFMA GEMM over the batch rows (csrc/train_bwd.hpp, conv_wgrad);
 *   - GroupNorm(8) + Mish backward (temporal_unet.py:71-72) is one kernel per conv, fed by the
 *     pre-normalisation output and the (mean, rstd) pairs the training forward keeps.
 * The time MLPs (SinusoidalPosEmb -> Linear -> Mish -> Linear and every block's Mish -> Linear,
 * temporal_unet.py:97-100,155-160) come in two forms.  dad_unet_forward_train / dad_unet_backward take their
 * per-row outputs (B, temb_width) — the concatenation, in launch order, of every ResidualTemporalBlock's
 * projection — and return the gradient with respect to them: a caller with an autograd of its own keeps the MLPs
 * there.  dad_train_objective_forward / dad_train_objective_backward (below) run the whole objective in the
 * library: q_sample, the time MLPs forward and backward, the denoiser, the loss.  fp32 only; no optimiser, no EMA.
 *
 * dad_model_set_training(m, 1) must precede dad_model_finalize (the extra weight images are packed
 * there).  dad_train_grad_info enumerates the gradient tensors (reference state_dict key without "model.",
 * element count; `offset` is their position in a packed buffer for callers that want one) — every tensor in
 * the reference's own layout (Conv1d (out, in, k); ConvTranspose1d (in, out, k)).  The time-MLP tensors are
 * not in the list (dad_train_time_grad_info has them). */
int dad_model_set_training(dad_model* m, int32_t on);
/* Replaces: nothing in the reference (its modules ARE the parameters); here the engine holds packed copies,
 * and an optimiser step (utils/training.py:166) changes the parameters every iteration.  Re-derives, ON THE
 * DEVICE, everything the engine keeps of the given tensors — packed conv images (forward and, in training
 * mode, the data-gradient images), biases, GroupNorm affine parameters, the per-timestep time tables — from
 * DEVICE fp32 tensors in the reference's layouts (same keys as dad_model_load_weight).  A conv whose block's
 * 1x1 residual conv rides in its image needs both weights in the same call.  fp32 arithmetic only.
 * Asynchronous on `stream`; captured loops stay valid (the images are updated in place). */
int dad_model_refresh_weights(dad_model* m, int32_t n, const char* const* keys, const float* const* tensors,
                              dad_stream_t stream);
int dad_train_grad_count(const dad_model* m, int32_t* count, int64_t* total_floats);
int dad_train_grad_info(const dad_model* m, int32_t i, const char** key, int64_t* offset, int64_t* numel);
/* saved: every activation of one forward (nothing is overwritten before the backward pass reads it);
 * scratch: gradient tensors and reduction slabs of one backward pass. */
int dad_train_workspace_bytes(const dad_model* m, int32_t batch, size_t* saved_bytes, size_t* scratch_bytes);
/* Replaces: TemporalUnet.forward(x, t) inside GaussianDiffusion.loss (diffusion.py:272) in training mode.
 * row_index: (B) int32 device, row b of temb_rows that sample b uses (normally 0..B-1); temb_rows:
 * (rows, temb_width) device fp32.  out = eps_theta (B, H, td); `saved` is handed to dad_unet_backward. */
int dad_unet_forward_train(dad_model* m, const float* x, const int32_t* row_index, const float* temb_rows,
                           float* out, int32_t batch, void* saved, size_t saved_bytes, dad_stream_t stream);
/* Replaces: autograd's walk from d loss / d eps back through the denoiser.  d_out: (B, H, td);
 * d_x (optional): (B, H, td) gradient w.r.t. the noisy trajectory; d_temb_rows: (B, temb_width), fully
 * overwritten; grad_tensors: one device tensor per entry of dad_train_grad_info, in that order, each of that
 * entry's element count and fully overwritten (separate tensors so that autograd can adopt them as .grad
 * without a copy; each call computes the gradient of ONE batch: accumulation over micro-batches is the
 * caller's add). */
int dad_unet_backward(dad_model* m, const float* x, const float* d_out, float* d_x, float* d_temb_rows,
                      float* const* grad_tensors, int32_t n_grad_tensors, int32_t batch, void* saved,
                      size_t saved_bytes, void* scratch, size_t scratch_bytes, dad_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The whole training objective in the library: GaussianDiffusion.loss (m_diffuser/models/diffusion.py:253-290)
 * and loss.backward() (m_diffuser/utils/training.py:152-156) as two calls.  Only the random draws stay with the
 * caller (t ~ randint, noise ~ randn_like, diffusion.py:265-268).  Needs dad_model_set_training(m, 1), the fp32
 * arithmetic and dad_model_load_train_schedule.  Argument errors — a null pointer, a loss_type other than
 * DAD_LOSS_L1 / DAD_LOSS_L2, training mode off, the split-f16 arithmetic, a wrong tensor count — return
 * DAD_E_INVALID with a message, before the first launch.  Nothing synchronises with the host. */
#define DAD_LOSS_L1 1        /* nn.L1Loss  (diffusion.py:85)  */
#define DAD_LOSS_L2 2        /* nn.MSELoss (diffusion.py:87)  */

/* The two schedule vectors q_sample reads (diffusion.py:113-114, 138-157): sqrt_alphas_cumprod and
 * sqrt_one_minus_alphas_cumprod, HOST fp32, n == cfg.n_timesteps.  Before or after dad_model_finalize; a load after it replaces the device copy and
 * waits for the device first (a step in flight may still read the old one). */
int dad_model_load_train_schedule(dad_model* m, const float* sqrt_ac, const float* sqrt_1m_ac, int32_t n);

/* The time-MLP gradient tensors, a list of its own beside dad_train_grad_info (which is unchanged): time_mlp.1.weight,
 * time_mlp.1.bias, time_mlp.3.weight, time_mlp.3.bias, then every ResidualTemporalBlock's time_mlp.1.weight / .bias in
 * launch order (temporal_unet.py:97-100,155-160); torch layouts, `offset` in floats within a packed buffer of
 * *total_floats. */
int dad_train_time_grad_count(const dad_model* m, int32_t* count, int64_t* total_floats);
int dad_train_time_grad_info(const dad_model* m, int32_t i, const char** key, int64_t* offset, int64_t* numel);

/* saved / scratch of the two calls below: what dad_train_workspace_bytes reports (those results are unchanged) plus
 * the objective's own regions behind them (x_t, the denoiser output, the time chain's activations; d loss / d out,
 * the projections' gradient, the time chain's gradients). */
int dad_train_objective_workspace_bytes(const dad_model* m, int32_t batch, size_t* saved_bytes, size_t* scratch_bytes);

/* Replaces: GaussianDiffusion.loss (diffusion.py:253-290) after its two draws — q_sample (diffusion.py:138-157; x_t
 * bit-identical to torch's two products and one sum), SinusoidalPosEmb lookup + time_mlp + every block's Mish -> Linear
 * per row (temporal_unet.py:19-32,97-100,155-160), TemporalUnet.forward in training mode (diffusion.py:272), the
 * elementwise L1 / L2 against the noise (or x_0: cfg.predict_epsilon), optional weights, mean (diffusion.py:274-290).
 * x0, noise, weights (or NULL): (B, H, td) device fp32; t_rows: (B) int32 device, clamped to [0, n_timesteps - 1]
 * before any table read; loss_out: device scalar.  `saved` is handed to dad_train_objective_backward. */
int dad_train_objective_forward(dad_model* m, const float* x0, const int32_t* t_rows, const float* noise,
                                const float* weights, int32_t loss_type, float* loss_out, int32_t batch, void* saved,
                                size_t saved_bytes, dad_stream_t stream);
/* Replaces: loss.backward() (utils/training.py:152-156): autograd's walk from the scalar through the mean, the
 * elementwise loss (sign(0) = 0 for L1, as torch), the denoiser (dad_unet_backward) and the time MLPs.  d_loss: DEVICE
 * scalar, autograd's incoming gradient, read on the device.  grad_tensors: as dad_unet_backward; time_grad_tensors: one
 * device tensor per entry of dad_train_time_grad_info; all fully overwritten, fixed summation order. */
int dad_train_objective_backward(dad_model* m, const float* x0, const float* noise, const float* weights, int32_t loss_type,
                                 const float* d_loss, float* const* grad_tensors, int32_t n_grad_tensors,
                                 float* const* time_grad_tensors, int32_t n_time_grad_tensors, int32_t batch, void* saved,
                                 size_t saved_bytes, void* scratch, size_t scratch_bytes, dad_stream_t stream);

/* Arguments of one reverse step beyond (x, t). All pointers may be NULL unless noted. */
typedef struct dad_step_args {
    const float* noise;      /* (B,H,td) injected z; NULL => in-kernel Philox            */
    uint64_t seed;           /* Philox key (used when noise == NULL)                     */
    uint64_t row_offset;     /* global index of batch row 0 (multi-GPU shards)           */
    uint64_t draw;           /* Philox draw id of this step (loop uses T - t)            */
    const float* cond0;      /* inpainting value for horizon step 0: (td) or (B,td)      */
    int32_t cond_per_row;    /* 0: cond0 is (td) broadcast; 1: (B,td)                    */
    const float* guide_grad; /* (B,H,td) d guide/d x_t, or NULL                          */
    float guide_weight;      /* policies.py:97                                           */
    float* mean_out;         /* optional (B,H,td): posterior mean incl. guidance         */
    float* eps_out;          /* optional (B,H,td): raw model output                      */
} dad_step_args;

/* Replaces: GaussianDiffusion.p_sample (diffusion.py:205-223) and
 * GuidedPolicy.p_sample_with_guidance (guides/policies.py:65-112): U-Net, x0 prediction,
 * clamp, posterior mean, guidance nudge, noise, inpainting — x updated IN PLACE.
 * With args->mean_out set and x_out_disabled != 0 it is p_mean_variance only
 * (diffusion.py:182-203) and x is left untouched. */
int dad_denoise_step(dad_model* m, float* x, int32_t t, int32_t batch, const dad_step_args* args,
                     int32_t x_out_disabled, void* workspace, size_t workspace_bytes,
                     dad_stream_t stream);

/* Replaces: GaussianDiffusion.p_sample_loop (diffusion.py:225-251) and
 * GuidedPolicy.sample_loop without a guide (guides/policies.py:114-149): runs
 * t = n_steps-1 .. 0 on x (which must already hold x_T, with conditions applied).
 * noise_stack: (n_steps,B,H,td) injected z in loop order, or NULL for in-kernel Philox
 * (draw id of iteration j is j+1; draw 0 is reserved for x_T, see dad_fill_normal).
 * proj: optional projection applied after every step (README semantics; the shipped
 * reference never calls it — SURVEY.md F5), alphas[n_steps] indexed by t on the HOST.
 * use_graph != 0 replays a cached hipGraph of the whole loop: every pointer argument and
 * (n_steps, batch, row_offset) are frozen in the capture, so callers keep them stable (a new
 * combination is captured once; at most 16 graphs are cached).  The Philox seed is NOT frozen:
 * it is written to device memory ahead of each replay. */
typedef struct dad_project_args {
    const float* P;         /* (D,D) device, D = (H+1)*n + H*m, row-major             */
    const float* obs_mean;  /* device (od) */
    const float* obs_std;
    const float* act_mean;  /* device (ad) */
    const float* act_std;
    int32_t state_dim;      /* n */
    int32_t observation_dim;/* od (== n in every reachable reference configuration)  */
    int32_t action_dim;     /* m */
    /* Optional device scratch of at least batch * H * (od + m) floats, owned by the caller.  With it,
     * batches of 32+ trajectories run v @ P as an MFMA GEMM that reads P once per 32 trajectories
     * (required beyond D = 2000, where one trajectory's partial sums no longer fit a CU's LDS);
     * without it every trajectory streams P on its own. */
    float* scratch;
    size_t scratch_bytes;
} dad_project_args;

int dad_sample_loop(dad_model* m, float* x, int32_t n_steps, int32_t batch,
                    const float* noise_stack, uint64_t seed, uint64_t row_offset,
                    const float* cond0, int32_t cond_per_row,
                    const dad_project_args* proj, const float* proj_alphas_host,
                    int32_t use_graph, void* workspace, size_t workspace_bytes,
                    dad_stream_t stream);

/* Replaces: DynamicsAwarePolicy.apply_projection (guides/policies.py:409-485) for one
 * alpha (policies.py:358-383 is evaluated by the caller).  x: (B,H,od+m) IN PLACE. */
int dad_project(const dad_project_args* p, float alpha, float* x, int32_t batch,
                int32_t horizon, dad_stream_t stream);

/* Replaces: the arithmetic of ProjectionLoss.compute (m_diffuser/losses/__init__.py:161-186):
 * violation[b] = sum_d (v_b - v_b P)_d^2 with v the de-normalised concatenated trajectory
 * [s_0..s_{H-1}, s_{H-1}, a_0..a_{H-1}] — the caller divides the sum over rows by B * D.
 * x (B,H,od+m) is read only; violation: (B) device fp32. */
int dad_projection_violation(const dad_project_args* p, const float* x, float* violation, int32_t batch,
                             int32_t horizon, dad_stream_t stream);

/* Replaces: torch.randn(shape) for x_T (diffusion.py:241; policies.py:134) with the
 * library's counter-based generator: element e of global row r gets Philox4x32-10
 * (key = seed, counter = (draw, r*H*td + e)) -> Box-Muller.  Result is independent of how
 * rows are sharded over GPUs. */
int dad_fill_normal(float* x, int32_t batch, int32_t row_elems, uint64_t seed,
                    uint64_t row_offset, uint64_t draw, dad_stream_t stream);

/* Optional kernel timing: when enabled, the run of conv-GEMM launches of every denoiser
 * evaluation is bracketed by one pair of HIP events on the launch stream;
 * dad_profile_read synchronises, returns the summed duration, the number of conv-GEMM
 * launches inside the brackets and their algorithmic FLOPs, and resets the counters. */
int dad_profile_enable(dad_model* m, int32_t on);
int dad_profile_read(dad_model* m, double* conv_ms, int64_t* conv_launches, double* conv_flops);

/* Test / tuning hooks, all per model (two models in one process do not interact).
 * dad_debug_set_tile: force conv tile configuration `cfg` (0..9, see kTiles in csrc/host_plan.hpp)
 * wherever it is valid for a layer; -1 restores the heuristic; 100+cfg (99 = heuristic tile)
 * additionally disables grid-level split-K.
 * dad_debug_set_option: "fuse_residual" (the 1x1 residual conv rides in its block's first conv
 * launch; 0 = always its own launch), "xswz" (LDS slot shifts), "xcd_order" (XCD-aware tile
 * order), "split_target" (blocks a split-K layer aims for), "cc" (small batches take the
 * consumer-combine kernels of csrc/conv_cc.hpp; 0 = always the batch-256 kernels), "cc_max_rows"
 * (largest batch * horizon that does), "ccw_max_rows" (the same bound for nets whose small-batch plan
 * needs the streamed-weight kernels of csrc/conv_ccw.hpp: GroupNorm groups wider than 64 channels),
 * "ccw_min_blocks" (blocks a wide layer keeps when its K slices are fattened), "ccw_prefer16" (two
 * 16-row tiles instead of a 32-row tile whose K slice LDS would halve), "wgrad_blocks" (blocks a
 * weight-gradient launch of the backward pass aims for: tiles x batch splits), "halo8" (5-tap convs of
 * 8-position layers at full-chip batches under the heuristic take csrc/conv_halo8.hpp; 0 = the conv-GEMM kernels),
 * "step_seam" (dad_sample_loop runs the posterior update of a step and the first conv of the next evaluation as one
 * launch, csrc/conv_seam.hpp, where dad_debug_seam_plan says so; 0 = the two launches; same bits either way).
 * Results do not depend on these choices beyond fp32 summation order. */
int dad_debug_set_tile(dad_model* m, int32_t cfg);
int dad_debug_set_option(dad_model* m, const char* name, int32_t value);

/* Test hooks for direct comparison against the reference's intermediates (synchronous).
 * dad_debug_read_table copies row t of a per-timestep table to HOST memory (`capacity` floats
 * available; the row width is returned in *width_out):
 *   DAD_TABLE_SINUSOID  SinusoidalPosEmb(t)                      (dim floats;  temporal_unet.py:19-32)
 *   DAD_TABLE_TIME_MLP  time_mlp(t) = Linear(Mish(Linear(emb)))  (time_dim;    temporal_unet.py:155-160)
 *   DAD_TABLE_BLOCKS    every block's Linear(Mish(time_mlp(t)))  (sum of C_out over residual
 *                       blocks, in launch order;                  temporal_unet.py:97-100)
 * dad_debug_mish applies the conv epilogue's Mish to n device floats. */
#define DAD_TABLE_SINUSOID 0
#define DAD_TABLE_TIME_MLP 1
#define DAD_TABLE_BLOCKS 2
int dad_debug_read_table(dad_model* m, int32_t which, int32_t t, float* host_out, int32_t capacity,
                         int32_t* width_out);
int dad_debug_mish(const float* in, float* out, int64_t n, dad_stream_t stream);
/* Where dad_train_objective_forward keeps x_t and the denoiser's output inside `saved` (byte offsets; host-side
 * query): lets a test compare x_t with q_sample (diffusion.py:138-157) bit for bit. */
int dad_debug_objective_offsets(const dad_model* m, int32_t batch, size_t* xt_offset, size_t* out_offset);
/* 1 when the kernel registry, generated from the planner's statements of which kernels of every family (DAD_FAMILY_*)
 * exist, holds an entry wherever a statement is true over its whole domain, nothing else, and the expected number of
 * kernels per family (no device call) */
int dad_debug_kernel_table_consistent(void);
/* Which kernels a batch takes (host-side query, no device work): launches_out = conv launches of one
 * denoiser evaluation through the small-batch consumer-combine kernels (csrc/conv_cc.hpp), 0 when the
 * batch runs the batch-256 kernels; wide_out = how many of them are the streamed-weight form for
 * wide layers (csrc/conv_ccw.hpp). */
int dad_debug_small_batch_plan(dad_model* m, int32_t batch, int32_t* launches_out, int32_t* wide_out);
/* Which kernels one training step (dad_unet_forward_train + dad_unet_backward) takes at a batch, under the current
 * debug options (host-side query, no device work; needs dad_model_set_training(m, 1) but neither weights nor
 * dad_model_finalize).  Writes min(capacity, *needed_out) int32 values to `out`:
 *   [DAD_BP_WGRADS]         weight-gradient launches (conv_wgrad)
 *   [DAD_BP_MULTI]          ... whose fullest block stages more than one chunk (the double-buffered steady state)
 *   [DAD_BP_MAX_CHUNKS]     most chunks a block stages
 *   [DAD_BP_MAX_KSPLIT]     deepest batch split (slabs sum_slabs_kernel adds)
 *   [DAD_BP_PART]           launches whose last chunk is part filled (samples % chunk samples != 0; the windows of a
 *                           long layer count as samples)
 *   [DAD_BP_PART_MULTI]     ... in a block that stages more than one chunk
 *   [DAD_BP_WINDOWED]       launches of the windowed kernel (layers longer than 128 positions)
 *   [DAD_BP_TILE + tile]    launches per wgrad tile: 0 = 64x64, 1 = 64x32, 2 = 32x32, 3 = 32x32 on rows that are not
 *                           whole aligned float4s (the trajectory's columns)
 *   [DAD_BP_TAPS_TILE + 4 * i + tile]   the same per tap count, i indexing 1, 3, 4, 5, 7 taps
 *   [DAD_BP_FWD + 2 * cfg + s]          conv launches of the training forward on conv tile cfg (0..9) without (s = 0)
 *                                       and with (s = 1) grid-level split-K
 *   [DAD_BP_DGRAD + 2 * cfg + s]        the same for the data-gradient convs
 *   [DAD_BP_RECORD_INTS]    ints per record (DAD_BP_REC_*); one record per weight-gradient launch follows from
 *                           DAD_BP_HEADER on, in launch order:
 *     taps, tile, windowed (0 / 1), samples (windows of a windowed launch), samples per chunk, samples per block
 *     (a whole number of chunks), blocks over the batch (ksplit), chunks the fullest block stages, chunks the last
 *     block stages. */
#define DAD_BP_WGRADS 0
#define DAD_BP_MULTI 1
#define DAD_BP_MAX_CHUNKS 2
#define DAD_BP_MAX_KSPLIT 3
#define DAD_BP_PART 4
#define DAD_BP_PART_MULTI 5
#define DAD_BP_WINDOWED 6
#define DAD_BP_TILE 7
#define DAD_BP_TAPS_TILE 11
#define DAD_BP_FWD 31
#define DAD_BP_DGRAD 51
#define DAD_BP_RECORD_INTS 71
#define DAD_BP_HEADER 72
#define DAD_BP_REC_TAPS 0
#define DAD_BP_REC_TILE 1
#define DAD_BP_REC_WINDOWED 2
#define DAD_BP_REC_SAMPLES 3
#define DAD_BP_REC_SPC 4
#define DAD_BP_REC_SPS 5
#define DAD_BP_REC_KSPLIT 6
#define DAD_BP_REC_CHUNKS 7
#define DAD_BP_REC_LAST_CHUNKS 8
#define DAD_BP_REC_INTS 9
int dad_debug_backward_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* Everything dad_unet_backward replays at a batch, step by step, read from the list of steps and the per-batch geometry
 * the entry point launches from (host-side query, no device work; the conditions of dad_debug_backward_plan).  Writes
 * min(capacity, *needed_out) int32 values to `out`:
 *   [DAD_BS_STEPS]             records that follow from DAD_BS_HEADER on, [DAD_BS_RECORD_INTS] ints each, in launch order
 *   [DAD_BS_BATCH]             the batch
 *   [DAD_BS_COLSUMS_LAUNCHES]  col_sums_many_kernel launches that end the pass ([DAD_BS_COLSUMS_ENTRIES] arrays of
 *                              `batch` rows in all, the widest of [DAD_BS_COLSUMS_WIDEST] columns)
 *   [DAD_BS_PADCOPY]           1: the horizon is zero padded ([DAD_BS_REAL_HORIZON] of [DAD_BS_HORIZON] positions exist):
 *                              pad_rows_kernel copies the trajectory and d out in, slice_rows_cols_kernel copies d x out
 *   [DAD_BS_DX]                1: a gradient reaches the trajectory
 * A record starts with its kind, [DAD_BS_KIND] = DAD_BS_K_*; fields a kind does not name are 0.
 *   DAD_BS_K_BIAS   row_partial_sums_kernel: rows per sample, columns
 *   DAD_BS_K_WGRAD  conv_wgrad<taps, tile, windowed>: M, C0, C1 (the Z operand is the concat [C0 | C1]), stride, pad, Lg and
 *                   Lz (rows per sample of G and Z as the kernel counts them: per window when windowed), grid x / y,
 *                   ragged (rows that are not whole aligned float4s), concat_inside (the boundary C0 falls inside one
 *                   block's staged columns), edge_m / edge_c (the last M / C tile is partly filled), swapped (G is the
 *                   conv's input, Z the gradient: the transposed conv), ksplit, slab_n4 (float4s per slab
 *                   sum_slabs_kernel adds; 0 when ksplit == 1), and samples, spc, sps, chunks, last_chunks as
 *                   DAD_BP_REC_* of dad_debug_backward_plan
 *   DAD_BS_K_DGRAD  a data-gradient conv (its launch: mode 3 of dad_debug_forward_plan): forward conv, sub, write (0 set,
 *                   1 add through the residual operand, 2 staged and added by add_inplace_kernel)
 *   DAD_BS_K_GN     gn_mish_bwd_wave_kernel<nv> (nv = 0: gn_mish_bwd_kernel): channels per group, L, lreal (> 0: positions
 *                   that exist), cpg_real (> 0: channels per group that exist), dtemb (d time projection is written),
 *                   short_pair (a pair has fewer than 64 float4), C
 *   DAD_BS_K_RESID  identity residual: write (0: a copy, 1: add_inplace_kernel), floats per sample, to_x (into d x)
 *   DAD_BS_K_COLS   take_cols_kernel: C columns at `off` of rows of `ld`, rows per sample, write (1: accumulates) */
#define DAD_BS_STEPS 0
#define DAD_BS_RECORD_INTS 1
#define DAD_BS_BATCH 2
#define DAD_BS_COLSUMS_LAUNCHES 3
#define DAD_BS_COLSUMS_ENTRIES 4
#define DAD_BS_COLSUMS_WIDEST 5
#define DAD_BS_PADCOPY 6
#define DAD_BS_HORIZON 7
#define DAD_BS_REAL_HORIZON 8
#define DAD_BS_DX 9
#define DAD_BS_HEADER 12
#define DAD_BS_K_BIAS 0
#define DAD_BS_K_WGRAD 1
#define DAD_BS_K_DGRAD 2
#define DAD_BS_K_GN 3
#define DAD_BS_K_RESID 4
#define DAD_BS_K_COLS 5
#define DAD_BS_KIND 0
#define DAD_BS_BIAS_ROWS 1
#define DAD_BS_BIAS_C 2
#define DAD_BS_WG_TAPS 1
#define DAD_BS_WG_TILE 2
#define DAD_BS_WG_WINDOWED 3
#define DAD_BS_WG_M 4
#define DAD_BS_WG_C0 5
#define DAD_BS_WG_C1 6
#define DAD_BS_WG_STRIDE 7
#define DAD_BS_WG_PAD 8
#define DAD_BS_WG_LG 9
#define DAD_BS_WG_LZ 10
#define DAD_BS_WG_GX 11
#define DAD_BS_WG_GY 12
#define DAD_BS_WG_RAGGED 13
#define DAD_BS_WG_CONCAT_INSIDE 14
#define DAD_BS_WG_EDGE_M 15
#define DAD_BS_WG_EDGE_C 16
#define DAD_BS_WG_SWAPPED 17
#define DAD_BS_WG_KSPLIT 18
#define DAD_BS_WG_SLAB_N4 19
#define DAD_BS_WG_SAMPLES 20
#define DAD_BS_WG_SPC 21
#define DAD_BS_WG_SPS 22
#define DAD_BS_WG_CHUNKS 23
#define DAD_BS_WG_LAST_CHUNKS 24
#define DAD_BS_DG_CONV 1
#define DAD_BS_DG_SUB 2
#define DAD_BS_DG_WRITE 3
#define DAD_BS_GN_NV 1
#define DAD_BS_GN_CPG 2
#define DAD_BS_GN_L 3
#define DAD_BS_GN_LREAL 4
#define DAD_BS_GN_CPG_REAL 5
#define DAD_BS_GN_DTEMB 6
#define DAD_BS_GN_SHORT_PAIR 7
#define DAD_BS_GN_C 8
#define DAD_BS_RS_WRITE 1
#define DAD_BS_RS_N 2
#define DAD_BS_RS_TO_X 3
#define DAD_BS_CL_C 1
#define DAD_BS_CL_OFF 2
#define DAD_BS_CL_LD 3
#define DAD_BS_CL_ROWS 4
#define DAD_BS_CL_WRITE 5
#define DAD_BS_REC_INTS 25
int dad_debug_backward_steps(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* The time chain of one fused objective step (dad_train_objective_forward + dad_train_objective_backward) at a batch:
 * the list of launches the two entry points replay (host-side query, no device work; needs
 * dad_model_set_training(m, 1) but neither weights nor dad_model_finalize; a batch the objective refuses is refused
 * here too).  Writes min(capacity, *needed_out) int32 values to `out`:
 *   [DAD_OP_LOSS_BLOCKS]    blocks of the loss's partial sums (at most 1024)
 *   [DAD_OP_KSLICES]        K slices of d act = d rows . W (slabs time_dtemb_kernel adds in slice order)
 *   [DAD_OP_KSLICE]         k values per slice (a multiple of 128)
 *   [DAD_OP_TEMB_WIDTH]     columns of the time projections (padded widths), the K of that product
 *   [DAD_OP_BLOCKS]         ResidualTemporalBlocks
 *   [DAD_OP_N]              batch x horizon x transition_dim: the elements the loss is a mean of (real ones only)
 *   [DAD_OP_RECORD_INTS]    ints per record (DAD_OP_REC_*)
 *   [DAD_OP_LAUNCHES]       records: 9, one per launch in launch order (3 forward, 6 backward), from DAD_OP_HEADER on:
 *     mode (DAD_OP_TG_*: the eight instantiations of time_gemm_kernel in the order of its TimeGemm enumeration, and
 *     DAD_OP_TG_DTEMB for time_dtemb_kernel: M x N elements, K = slabs added), M, N, K of out[M][N] = sum over K, the
 *     grid x / y / z (32 x 32 output tiles, K slices), 32-wide K chunks in a full slice (the block's four waves take
 *     them round robin) and in the last slice, K % 32, k values per slice; the three chunk / tail fields are 0 for
 *     DAD_OP_TG_DTEMB. */
#define DAD_OP_LOSS_BLOCKS 0
#define DAD_OP_KSLICES 1
#define DAD_OP_KSLICE 2
#define DAD_OP_TEMB_WIDTH 3
#define DAD_OP_BLOCKS 4
#define DAD_OP_N 5
#define DAD_OP_RECORD_INTS 6
#define DAD_OP_LAUNCHES 7
#define DAD_OP_HEADER 8
#define DAD_OP_REC_MODE 0
#define DAD_OP_REC_M 1
#define DAD_OP_REC_N 2
#define DAD_OP_REC_K 3
#define DAD_OP_REC_GRID_X 4
#define DAD_OP_REC_GRID_Y 5
#define DAD_OP_REC_GRID_Z 6
#define DAD_OP_REC_CHUNKS 7
#define DAD_OP_REC_LAST_CHUNKS 8
#define DAD_OP_REC_KTAIL 9
#define DAD_OP_REC_KSLICE 10
#define DAD_OP_REC_INTS 11
#define DAD_OP_TG_FWD_H1 0
#define DAD_OP_TG_FWD_TEMB 1
#define DAD_OP_TG_FWD_ROWS 2
#define DAD_OP_TG_BWD_DWK 3
#define DAD_OP_TG_BWD_DACT 4
#define DAD_OP_TG_BWD_DW3 5
#define DAD_OP_TG_BWD_DH1 6
#define DAD_OP_TG_BWD_DW1 7
#define DAD_OP_TG_DTEMB 8
int dad_debug_objective_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* What one forward evaluation launches at a batch under the current debug options: the description the entry point
 * itself replays (csrc/host_plan.hpp: FwdPlan of plan_forward; mode 3: TrainScratch of train_scratch), written down
 * (host-side query, no device work; needs neither weights nor dad_model_finalize; modes 2 / 3 need
 * dad_model_set_training(m, 1); a batch the call refuses is refused here too).  `mode`:
 *   0  dad_unet_forward / dad_denoise_step with one shared timestep (may take the small-batch kernels)
 *   1  the same evaluation on the batch kernels: dad_unet_forward_rows (per-row timesteps)
 *   2  dad_unet_forward_train (the training plan)
 *   3  the data-gradient conv launches of dad_unet_backward, in launch order
 * Writes min(capacity, *needed_out) int32 values to `out`:
 *   [DAD_FP_MODE] [DAD_FP_BATCH]   as asked
 *   [DAD_FP_SMALL]          1: the small-batch plan is taken (csrc/conv_cc.hpp, conv_ccw.hpp), the records are DAD_FP_CC_*
 *   [DAD_FP_RECORDS]        records that follow from DAD_FP_HEADER on, [DAD_FP_RECORD_INTS] ints each
 *   [DAD_FP_FINAL_GX] [DAD_FP_FINAL_GY]   grid of the final kernel (0 in mode 3)
 *   [DAD_FP_FINAL_KERNEL]   DAD_FP_FINAL_POSTERIOR (final_posterior_kernel), DAD_FP_FINAL_CC (final_cc_kernel) or
 *                           DAD_FP_FINAL_NONE (mode 3)
 * One record per conv-GEMM launch in launch order (a 1x1 residual conv that rides in its carrier's launch has none):
 *   conv index into the plan (mode 3: the forward conv whose data gradient this is, -1 = final_conv[1]), sub (mode 3:
 *   which of that conv's data-gradient launches), tile cfg, taps, stride, flags (bit 0 x3, 1 bdir, 2 ragged, 3 res —
 *   the ride —, 4 padded, 5 windowed: the flag word of kernel_registered_f, so (cfg, taps, stride, flags) names the
 *   instantiation), K chunk, grid-level K slices, npt of the gn_pass_kernel<npt> launch that follows (0: none),
 *   N tiles, M tiles, 1 when the last N tile holds fewer samples than it has room for, kernel family:
 *   DAD_FP_FAMILY_GEMM (conv_gemm_f32, the instantiation named above) or DAD_FP_FAMILY_HALO8 (conv_halo8_f32 of
 *   csrc/conv_halo8.hpp on the same tile, grid and ride: cfg 0 / 1 and flag bit 3 name its instantiation).
 * With [DAD_FP_SMALL] one record per launched small-batch conv instead:
 *   conv index, taps, stride, wide (conv_ccw), ride, big, ride_in, rows per tile (16 / 32), windowed, channels per K
 *   slice, K slices, N tiles, res_kind (how the output's residual reaches its consumer: 0 none, 1 the trajectory,
 *   2 a finished tensor, 3 the ride slabs of a carrier, 4 the slabs of a stand-alone 1x1 conv). */
#define DAD_FP_MODE 0
#define DAD_FP_BATCH 1
#define DAD_FP_SMALL 2
#define DAD_FP_RECORDS 3
#define DAD_FP_RECORD_INTS 4
#define DAD_FP_FINAL_GX 5
#define DAD_FP_FINAL_GY 6
#define DAD_FP_FINAL_KERNEL 7
#define DAD_FP_HEADER 8
#define DAD_FP_FINAL_NONE 0
#define DAD_FP_FINAL_POSTERIOR 1
#define DAD_FP_FINAL_CC 2
#define DAD_FP_REC_CONV 0
#define DAD_FP_REC_SUB 1
#define DAD_FP_REC_CFG 2
#define DAD_FP_REC_TAPS 3
#define DAD_FP_REC_STRIDE 4
#define DAD_FP_REC_FLAGS 5
#define DAD_FP_REC_KC 6
#define DAD_FP_REC_KSLICES 7
#define DAD_FP_REC_GN_NPT 8
#define DAD_FP_REC_NTILES_N 9
#define DAD_FP_REC_MTILES 10
#define DAD_FP_REC_PART_TILE 11
#define DAD_FP_REC_FAMILY 12
#define DAD_FP_REC_INTS 13
#define DAD_FP_FAMILY_GEMM 0
#define DAD_FP_FAMILY_HALO8 1
#define DAD_FP_CC_CONV 0
#define DAD_FP_CC_TAPS 1
#define DAD_FP_CC_STRIDE 2
#define DAD_FP_CC_WIDE 3
#define DAD_FP_CC_RIDE 4
#define DAD_FP_CC_BIG 5
#define DAD_FP_CC_RIDE_IN 6
#define DAD_FP_CC_TILE_ROWS 7
#define DAD_FP_CC_WINDOWED 8
#define DAD_FP_CC_SLICE_CH 9
#define DAD_FP_CC_KSLICES 10
#define DAD_FP_CC_NTILES 11
#define DAD_FP_CC_RES_KIND 12
#define DAD_FP_CC_INTS 13
int dad_debug_forward_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out);
/* The conv_halo8_f32 launches (csrc/conv_halo8.hpp) of the same description, modes 0 and 1 only, with what the kernel
 * makes of its ConvParams: read from the ConvOp / LaunchGeom the launch fills them from (csrc/host_plan.hpp,
 * halo8_plan_encode), nothing decided.  Writes min(capacity, *needed_out) int32 values: [0] the records, [1]
 * DAD_H8_INTS, then per launch in launch order
 *   [DAD_H8_CONV] [DAD_H8_CFG] [DAD_H8_RIDE]   conv index, tile (0 / 1), the riding 1x1 conv: the instantiation
 *   [DAD_H8_CHUNKS]       32-channel K chunks, (cin0 + cin1) / 32
 *   [DAD_H8_SRC1_CHUNK]   the chunk from which the second source is read, -1 without one
 *   [DAD_H8_RES] [DAD_H8_TEMB]   a residual operand / a time embedding is present
 *   [DAD_H8_PER_ROW]      the time embedding is indexed per sample (mode 1, where there is one)
 *   [DAD_H8_GN]           GroupNorm runs in the kernel
 *   [DAD_H8_WPP]          waves one (sample, group) pair spans (0 without GroupNorm; > 1: the cross-wave sum through LDS)
 *   [DAD_H8_XCD_GN]       0: the plain grid (y = M tile, z = N tile), else the XCD-aware tile order
 *   [DAD_H8_MTILES] [DAD_H8_NTILES_N] [DAD_H8_PART_TILE]   as the DAD_FP_REC_* fields of those names */
#define DAD_H8_HEADER 2
#define DAD_H8_CONV 0
#define DAD_H8_CFG 1
#define DAD_H8_RIDE 2
#define DAD_H8_CHUNKS 3
#define DAD_H8_SRC1_CHUNK 4
#define DAD_H8_RES 5
#define DAD_H8_TEMB 6
#define DAD_H8_PER_ROW 7
#define DAD_H8_GN 8
#define DAD_H8_WPP 9
#define DAD_H8_XCD_GN 10
#define DAD_H8_MTILES 11
#define DAD_H8_NTILES_N 12
#define DAD_H8_PART_TILE 13
#define DAD_H8_INTS 14
int dad_debug_halo8_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out);
/* Which kernel one dad_project (violation == 0) or dad_projection_violation (violation != 0) call launches for
 * trajectories (batch, horizon, observation_dim + action_dim) and a dad_project_args.scratch of scratch_bytes (0: none),
 * and on which grid: the plan the two entry points launch from.  Host logic only, no device call.  out[DAD_PP_INTS]:
 *   [DAD_PP_FORM]            DAD_PP_ROW1 (project_kernel<1,16>: one trajectory per block), DAD_PP_ROW4 (project_kernel<4,16>:
 *                            four per block, batches beyond 512 whose four rows fit LDS) or DAD_PP_GEMM (project_gemm_kernel:
 *                            32 trajectories x 32 columns of P per block; never for the violation)
 *   [DAD_PP_ROWS_PER_BLOCK]  1, 4 or 32
 *   [DAD_PP_GX] [DAD_PP_GY]  the grid
 *   [DAD_PP_LDS_BYTES]       dynamic LDS of one block
 *   [DAD_PP_REFUSED]         1: the call fails with DAD_E_INVALID (one trajectory's partial sums exceed LDS and there is
 *                            no scratch, or fewer than 32 trajectories, for the GEMM form); the other fields then describe
 *                            the launch that does not fit */
#define DAD_PP_FORM 0
#define DAD_PP_ROWS_PER_BLOCK 1
#define DAD_PP_GX 2
#define DAD_PP_GY 3
#define DAD_PP_LDS_BYTES 4
#define DAD_PP_REFUSED 5
#define DAD_PP_INTS 6
#define DAD_PP_ROW1 0
#define DAD_PP_ROW4 1
#define DAD_PP_GEMM 2
int dad_debug_project_plan(int32_t state_dim, int32_t observation_dim, int32_t action_dim, int32_t batch, int32_t horizon,
                           size_t scratch_bytes, int32_t violation, int32_t* out);
/* Whether dad_sample_loop at `batch` (projection != 0: called with a projection argument) takes the seam between two
 * denoise steps as one launch (csrc/conv_seam.hpp; the rule: plan_seam in csrc/host_plan.hpp), under the model's current
 * options.  Host logic only, no device call; the model needs no weights.  out[DAD_SEAM_INTS]:
 *   [DAD_SEAM_TAKEN]      1 / 0
 *   [DAD_SEAM_REASON]     0 = taken, else the first condition that refuses it; dad_debug_seam_reason names it
 *   [DAD_SEAM_GRID] [DAD_SEAM_THREADS] [DAD_SEAM_LDS_BYTES]   the launch (0 when refused)
 *   [DAD_SEAM_TILE]       the first conv's tile (0 or 1), whose summation order the launch keeps; -1 when refused
 *   [DAD_SEAM_UNITS]      8-channel units it multiplies (1: transition_dim <= 8, 2)
 *   [DAD_SEAM_SPT]        samples of one 32-row tile (32 / horizon); 0 when refused
 *   [DAD_SEAM_LAST]       samples in the last tile (1 .. DAD_SEAM_SPT); 0 when refused
 *   [DAD_SEAM_BUFFERS]    which allowed relation of seam_buffers_ok holds: DAD_SEAM_BUF_APART (final_act overlaps neither
 *                         buffer the launch writes), DAD_SEAM_BUF_DST (it is the conv's dst), DAD_SEAM_BUF_RDST (it is the
 *                         ride's); -1 when refused
 *   [DAD_SEAM_DIM] [DAD_SEAM_TILE0]   the instantiation conv_seam_f32<dim, tile0>; 0 / -1 when refused */
#define DAD_SEAM_TAKEN 0
#define DAD_SEAM_REASON 1
#define DAD_SEAM_GRID 2
#define DAD_SEAM_THREADS 3
#define DAD_SEAM_LDS_BYTES 4
#define DAD_SEAM_TILE 5
#define DAD_SEAM_UNITS 6
#define DAD_SEAM_SPT 7
#define DAD_SEAM_LAST 8
#define DAD_SEAM_BUFFERS 9
#define DAD_SEAM_DIM 10
#define DAD_SEAM_TILE0 11
#define DAD_SEAM_INTS 12
#define DAD_SEAM_BUF_APART 0
#define DAD_SEAM_BUF_DST 1
#define DAD_SEAM_BUF_RDST 2
int dad_debug_seam_plan(dad_model* m, int32_t batch, int32_t projection, int32_t* out);
const char* dad_debug_seam_reason(int32_t reason);
/* The kernels of one family in the library's own registry: the table every launch looks its kernel up in (no device
 * call).  Writes min(capacity, *needed_out) int32 values to `out`: [0] the number of kernels, [1] the ints of one key,
 * then the keys —
 *   DAD_FAMILY_GEMM   conv_gemm_f32   (tile cfg, taps, stride, flag word as above)
 *   DAD_FAMILY_CC     conv_cc         (taps, stride, riding 1x1 conv, big, rows per tile, windowed)
 *   DAD_FAMILY_CCW    conv_ccw        (taps, stride, riding 1x1 conv, ride_in, rows per tile)
 *   DAD_FAMILY_HALO8  conv_halo8_f32  (tile cfg, riding 1x1 conv)
 *   DAD_FAMILY_SEAM   conv_seam_f32   (dim, the first conv's tile is 0)
 *   DAD_FAMILY_WGRAD  conv_wgrad      (taps, tile as DAD_BP_TILE, windowed) */
#define DAD_FAMILY_GEMM 0
#define DAD_FAMILY_CC 1
#define DAD_FAMILY_CCW 2
#define DAD_FAMILY_HALO8 3
#define DAD_FAMILY_SEAM 4
#define DAD_FAMILY_WGRAD 5
#define DAD_FAMILIES 6
#define DAD_KERNEL_KEY_MAX 6
int dad_debug_kernel_list(int32_t family, int32_t* out, int32_t capacity, int32_t* needed_out);

/* ------------------------------------------------------------------------------------------------
 * The optimiser step.  Replaces what Trainer.train_step does after loss.backward() (utils/training.py:158-189):
 * clip_grad_norm_(parameters, max_norm), torch.optim.Adam.step() and the update_ema loop, as at most two launches
 * over a list of tensors, with no host synchronisation.  A dad_optim is independent of dad_model: it sees pointers.
 *
 * Per tensor (utils/training.py:158-189; torch.optim.Adam's arithmetic in its operation order):
 *   coef = min(1, max_grad_norm / (total_norm + 1e-6)),  total_norm = sqrt(sum of g^2 over every tensor with a grad)
 *          (clip_grad_norm_, utils/training.py:158-163; not special-cased for non-finite values)
 *   g'   = coef g  (+ weight_decay p: L2 weight decay);   with `decoupled`, p *= 1 - lr weight_decay first (AdamW)
 *   m    = m + (g' - m) one_minus_beta1;   v = beta2 v + one_minus_beta2 g'^2
 *   p    = p - step_size m / (sqrt(v) / bc2_sqrt + eps)                        (utils/training.py:165-166)
 *   ema  = ema_decay ema + (1 - ema_decay) p                                    (utils/training.py:180-189)
 * THE GRADIENT IS READ ONLY: after the step `grad` still holds the unclipped gradient, where clip_grad_norm_ scales
 * it in place.  A tensor with grad == NULL only has its EMA updated (update_ema covers every parameter); one with
 * ema == NULL has none.  Tensors are fp32 and contiguous; a tensor whose pointers are all 16-byte aligned is read
 * and written 16 bytes at a time, any other one element at a time.
 * The summation order of total_norm is fixed by the plan (dad_debug_optim_plan): one partial per block, added in
 * block order, no atomics: two runs give the same bits.
 * The descriptor table lives on the device and is uploaded (stream-ordered, from pinned staging buffers that are
 * not rewritten while a copy may be in flight) only when a pointer, size or group index changed since the last
 * step.  ONE STREAM PER dad_optim AT A TIME; device memory is allocated at the first step on the current device.
 * A table that outgrows its device buffer gets a new one of twice the size; the old buffer (a step in flight may
 * still read it) and the staging buffers are kept until dad_optim_destroy.
 * When no tensor of a step has a grad, total_norm is 0: grad_norm_out receives 0 and nothing is clipped. */
typedef struct dad_optim dad_optim;
typedef struct dad_optim_tensor {
    float* param;
    const float* grad;    /* NULL: EMA only                                                        */
    float* exp_avg;       /* m and v: required when grad is set                                    */
    float* exp_avg_sq;
    float* ema;           /* NULL: no EMA                                                          */
    int64_t numel;
    int32_t group;        /* index into dad_optim_args.groups                                      */
} dad_optim_tensor;
/* One set of hyper-parameters: a torch param group at one step count.  step_size = lr / (1 - beta1^step),
 * bc2_sqrt = sqrt(1 - beta2^step), one_minus_beta1 = 1 - beta1 and one_minus_beta2 = 1 - beta2 are computed by the
 * caller in double, as torch does, and rounded once (1 - 0.999f is 1.3e-5 away from 0.001). */
typedef struct dad_optim_group {
    float lr, beta1, beta2, eps, weight_decay, step_size, bc2_sqrt;
    int32_t decoupled;
    float one_minus_beta1, one_minus_beta2;
} dad_optim_group;        /* at most 8 per step */
typedef struct dad_optim_args {
    const dad_optim_group* groups;
    int32_t n_groups;
    float max_grad_norm;  /* <= 0: no clipping (the square-sum pass then runs only if grad_norm_out is set) */
    float ema_decay;
    float* grad_norm_out; /* device scalar that receives the pre-clip total_norm, or NULL         */
} dad_optim_args;
int dad_optim_create(dad_optim** out);             /* no device call */
void dad_optim_destroy(dad_optim* o);
/* Enqueues one step on `s`.  DAD_E_INVALID, with a message and before any device call, for: a null pointer, n <= 0,
 * numel <= 0, a group index out of range, n_groups outside 1 .. 8, grad set but a moment missing, a tensor with
 * neither grad nor ema. */
int dad_optim_step(dad_optim* o, const dad_optim_tensor* tensors, int32_t n, const dad_optim_args* a, dad_stream_t s);
/* The work split dad_optim_step replays for tensors of these sizes (csrc/host_plan.hpp: optim_plan; host-side query,
 * no device call).  Writes min(capacity, *needed_out) int32 values to `out`:
 *   [DAD_OS_CHUNK]        elements per chunk (a multiple of 4)
 *   [DAD_OS_CHUNKS]       chunks = records that follow from DAD_OS_HEADER on
 *   [DAD_OS_GRID]         blocks of each of the two kernels (at most 2048)
 *   [DAD_OS_PARTIALS]     partial square sums (one per block)
 *   [DAD_OS_RECORD_INTS]  ints per record (DAD_OS_REC_*)
 * One record per chunk in chunk order: tensor, first element (its low 31 bits, then the bits above), elements, and
 * the block that owns the chunk (a block walks its chunks in this order). */
#define DAD_OS_CHUNK 0
#define DAD_OS_CHUNKS 1
#define DAD_OS_GRID 2
#define DAD_OS_PARTIALS 3
#define DAD_OS_RECORD_INTS 4
#define DAD_OS_HEADER 5
#define DAD_OS_REC_TENSOR 0
#define DAD_OS_REC_FIRST 1
#define DAD_OS_REC_FIRST_HI 2
#define DAD_OS_REC_COUNT 3
#define DAD_OS_REC_BLOCK 4
#define DAD_OS_REC_INTS 5
int dad_debug_optim_plan(const int64_t* numel, int32_t n, int32_t* out, int32_t capacity, int32_t* needed_out);

#ifdef __cplusplus
}
#endif
#endif /* DAD_H */
