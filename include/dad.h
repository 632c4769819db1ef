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

struct dad_project_args;
/* The dynamics-aware objective: the objective above and the dynamics violation of the plan the model predicts, from ONE
 * evaluation of the denoiser (they share t, the noise, x_t and `out`):
 *   total = diffusion_weight * Ld + projection_weight * Lp
 *   Ld    = the loss of dad_train_objective_forward (same launches, same bits)
 *   Lp    = sum_b tw[t_b] * violation(x0_hat_b) / (B * D),   violation as dad_projection_violation_fwd (physical units)
 *   x0_hat = sqrt_recip_ac[t_b] x_t - sqrt_recipm1_ac[t_b] out  (cfg.predict_epsilon; the two tables of
 *            dad_model_load_schedule; two products and one difference, each rounded, as torch's expression), else `out`;
 *            never clamped.  It is formed inside the violation kernels' gather: no x0_hat tensor is written.
 * `proj`: P (D, D), D = (H + 1) n + H m for the trajectories' horizon H, and the normaliser; `p_dim`: the side of P as
 * the caller holds it (checked against D); observation_dim + action_dim must be the model's transition_dim.  `form`:
 * -1 / 0 / 1 as dad_projection_violation_fwd.  `timestep_weights`: tw, (n_timesteps) device fp32, or NULL for all ones.
 * `parts`: device float[3] = (Ld, projection_weight * Lp, total), written by the forward.
 * The backward pass runs the violation backward of the same form with the per-trajectory factor
 * d_loss * projection_weight * tw[t_b] / (B D) and writes d total / d out ONCE, in its scatter epilogue:
 *   d_out = d_loss * diffusion_weight * u / n  +  s_b * (the scattered, de-normalised projection gradient)
 * (u: the unit gradient of the L1 / L2 term, weights included; s_b = -sqrt_recipm1_ac[t_b], or 1 when the model predicts
 * x_0), then the denoiser's and the time chain's backward exactly as dad_train_objective_backward.  P and x_0 get no
 * gradient.  No atomics; every sum has one order.  Refusals come before the first launch, with a message: those of the
 * objective above, then DAD_E_INVALID for missing projection arguments, a shape that does not fit (p_dim != D, the
 * widths), an unknown form, a forced row form whose row does not fit a CU's LDS; DAD_E_STATE without
 * dad_model_load_schedule; DAD_E_WORKSPACE for buffers smaller than dad_train_dynamics_objective_workspace_bytes reports. */
int dad_train_dynamics_objective_workspace_bytes(const dad_model* m, const struct dad_project_args* proj, int32_t form,
                                                 int32_t batch, size_t* saved_bytes, size_t* scratch_bytes);
int dad_train_dynamics_objective_forward(dad_model* m, const float* x0, const int32_t* t_rows, const float* noise,
                                         const float* weights, int32_t loss_type, const struct dad_project_args* proj,
                                         int32_t p_dim, int32_t form, float diffusion_weight, float projection_weight,
                                         const float* timestep_weights, float* parts, int32_t batch, void* saved,
                                         size_t saved_bytes, dad_stream_t stream);
int dad_train_dynamics_objective_backward(dad_model* m, const float* x0, const float* noise, const float* weights,
                                          int32_t loss_type, const struct dad_project_args* proj, int32_t p_dim, int32_t form,
                                          float diffusion_weight, float projection_weight, const float* timestep_weights,
                                          const float* d_loss, float* const* grad_tensors, int32_t n_grad_tensors,
                                          float* const* time_grad_tensors, int32_t n_time_grad_tensors, int32_t batch,
                                          void* saved, size_t saved_bytes, void* scratch, size_t scratch_bytes,
                                          dad_stream_t stream);

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

/* One reverse step described by its coefficients rather than by a schedule index: what a strided (DDIM) sampler over
 * the trained schedule hands in.  In the tail kernels' operation order, per element:
 *   x0   = c_recip * x_t - c_recipm1 * out          (or x0 = out when the model predicts x0)
 *   x0  += guide_weight * guide_x0 * g              (only with a guide gradient g)
 *   x0   = clamp(x0, -1, 1)                         (cfg.clip_denoised)
 *   mean = coef_x0 * x0 + coef_xt * x_t
 *   mean += guide_weight * guide_mean * g           (only with a guide gradient g)
 *   x    = mean + sigma * z, then the inpainting of horizon step 0.
 * `t` is the row of the time-embedding tables the network is evaluated at.  The ancestral step of dad_denoise_step
 * is {t, sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], 0, posterior_mean_coef1[t],
 * posterior_mean_coef2[t], exp(log_var[t]), t == 0 ? 0 : exp(0.5 log_var[t])} of the loaded schedule. */
typedef struct dad_sampler_coef {
    int32_t t;
    float c_recip, c_recipm1, guide_x0, coef_x0, coef_xt, guide_mean, sigma;
} dad_sampler_coef;

/* dad_denoise_step with the step's coefficients given by the caller.  DAD_E_RANGE for coef->t outside
 * [0, n_timesteps), DAD_E_INVALID for a coefficient that is not finite or a negative sigma: checked before anything
 * else about the model, so an unfinalised model refuses them too. */
int dad_sampler_step(dad_model* m, float* x, const dad_sampler_coef* coef, int32_t batch, const dad_step_args* args,
                     int32_t x_out_disabled, void* workspace, size_t workspace_bytes, dad_stream_t stream);

/* dad_sample_loop over `n_steps` caller-given steps, steps[0] first: iteration j evaluates the network at steps[j].t
 * and uses Philox draw j + 1 (or noise_stack[j]).  proj_alphas_host[n_steps] is in the same (execution) order.
 * Refusals as dad_sampler_step for every step, and DAD_E_INVALID for n_steps < 1.  use_graph: the bytes of `steps`
 * are part of the key of the cached graph, so every sampler is captured once and replayed by value. */
int dad_sampler_loop(dad_model* m, float* x, const dad_sampler_coef* steps, int32_t n_steps, int32_t batch,
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

/* The same violation as a differentiable pair.  Replaces: ProjectionLoss.compute (m_diffuser/losses/__init__.py:161-186)
 * as torch autograd sees it — the reference's expression is plain torch, so loss.backward() differentiates it with
 * respect to whatever trajectory it is handed; here the two passes are explicit.
 *   forward:  r_b = v_b - v_b P,  violation[b] = sum_d r_{b,d}^2;  r (B, D) stays in `workspace`
 *   backward: g_b = 2 d_violation[b] (r_b - r_b P^T)   (P is neither symmetric nor idempotent to this code), then
 *             d_x[b,ts,k]    = obs_std[k] (g_b[ts n + k] + (ts == H-1 ? g_b[H n + k] : 0))      k < n
 *             d_x[b,ts,k]    = 0                                                              n <= k < od
 *             d_x[b,ts,od+k] = act_std[k] g_b[(H+1) n + ts m + k]
 * d_x is fully overwritten; P gets no gradient (the reference keeps it a plain tensor).  `form`: -1 lets the planner
 * choose (plan_violation_grad, csrc/host_plan.hpp), 0 forces the row form (one trajectory per block), 1 the GEMM form
 * (32 trajectories x 32 columns per block on v_mfma_f32_32x32x2_f32; any batch, any D) — a test hook, like
 * dad_debug_set_tile.  The backward pass must be given the workspace, batch, horizon and form of its forward pass.
 * Both calls are asynchronous on `stream` and allocate nothing; no floating-point atomics: the same inputs give the
 * same bits.  Refusals come before any launch, with a message: DAD_E_INVALID for a null pointer, batch or
 * horizon <= 0, state_dim > observation_dim, an unknown form, or a forced row form whose row does not fit LDS;
 * DAD_E_WORKSPACE for fewer than dad_violation_grad_workspace_bytes bytes.  dad_project_args.scratch is not used. */
int dad_violation_grad_workspace_bytes(const dad_project_args* p, int32_t batch, int32_t horizon, int32_t form,
                                       size_t* bytes);
int dad_projection_violation_fwd(const dad_project_args* p, const float* x, float* violation, void* workspace,
                                 size_t workspace_bytes, int32_t batch, int32_t horizon, int32_t form,
                                 dad_stream_t stream);
int dad_projection_violation_bwd(const dad_project_args* p, const float* d_violation /* (B) device */,
                                 float* d_x /* (B,H,od+m), fully overwritten */, void* workspace,
                                 size_t workspace_bytes, int32_t batch, int32_t horizon, int32_t form,
                                 dad_stream_t stream);

/* A value guide the library evaluates itself.  Replaces: ValueGuidedPolicy's guide, sum over the horizon of
 * value_model(observations) (guides/policies.py:243-271), and its gradient at x_t as p_sample_with_guidance takes it
 * (guides/policies.py:87-97), for value models that are a small MLP applied to each horizon step's observation:
 *   h_0 = x[b, l, :in_dim],  a_i = W_i h_{i-1} + b_i,  h_i = act(a_i),  V = w_L . h_{L-1} + b_L        (per row (b, l))
 *   d V / d x[b, l, :in_dim] = W_1^T (act'(a_1) * W_2^T ( ... (act'(a_{L-1}) * w_L))),  0 on the channels from in_dim on.
 * A plain struct, no library-side state.  n_layers Linear layers (2 .. 4, the last with one output), one activation
 * (DAD_GD_ACTS) between them; widths[i] is the output width of layer i, padded[0] the zero-padded in_dim and
 * padded[i + 1] the zero-padded widths[i] of a hidden layer, exactly as dad_debug_guide_plan reports them.  Layer i
 * (0-based) of a hidden layer travels as two zero-padded device images, so that both passes read their MFMA B operand
 * contiguously: w_fwd[i] = W^T as [padded[i]][padded[i + 1]], w_bwd[i] = W as [padded[i + 1]][padded[i]]; bias[i] is
 * [padded[i + 1]] (a missing bias: zeros).  The last layer: w_fwd[L - 1] = its weight row as [padded[L - 1]],
 * w_bwd[L - 1] unused, bias[L - 1] one float.  grad: caller-owned scratch of batch * H * td floats, the gradient
 * dad_guided_loop hands from its guide launch to the step's tail. */
#define DAD_GUIDE_MAX_LAYERS 4
typedef struct dad_guide_args {
    int32_t n_layers, in_dim;
    int32_t widths[DAD_GUIDE_MAX_LAYERS];
    int32_t padded[DAD_GUIDE_MAX_LAYERS];
    int32_t activation;
    const float* w_fwd[DAD_GUIDE_MAX_LAYERS];
    const float* w_bwd[DAD_GUIDE_MAX_LAYERS];
    const float* bias[DAD_GUIDE_MAX_LAYERS];
    float* grad;
    size_t grad_bytes;
} dad_guide_args;

/* The stand-alone gradient of that guide (guides/policies.py:243-271 differentiated as :87-97 does): grad_out
 * (B, H, td) fully overwritten, value_rows_out (B * H) the per-row V, or NULL.  x: (B, H, td) device fp32, read only.
 * One launch of guide_mlp_kernel (csrc/guide_mlp.hpp) on `stream`: asynchronous, allocates nothing, no atomics (the
 * same inputs give the same bits).  dad_guide_args.grad is not used.  Refusals come before any launch, each with a
 * message: DAD_E_INVALID for a null pointer, batch, horizon or transition_dim <= 0, a net plan_guide refuses
 * (DAD_GD_REFUSALS) or `padded` other than the plan's. */
int dad_guide_grad(const dad_guide_args* guide, const float* x, float* grad_out, float* value_rows_out, int32_t batch,
                   int32_t horizon, int32_t transition_dim, dad_stream_t stream);

/* dad_sampler_loop with that guide inside it.  Replaces: GuidedPolicy.sample_loop with a value guide
 * (guides/policies.py:114-149 with :243-271 as the guide and :87-97 as the step), as one library call.  steps == NULL
 * runs the ancestral steps t = n_steps-1 .. 0 of the loaded schedule (dad_sample_loop's); proj_alphas_host[n_steps] is
 * in EXECUTION order either way.  Per iteration the guide launch goes out after the evaluation's first launch — on
 * a seamed loop the seam, which reads the previous step's gradient and writes the x this one is taken at — and before
 * the step's tail, which gets guide->grad and guide_weight (dad_step_args).  Everything stays on the one stream.
 * guide == NULL or guide_weight <= 0 is the unguided loop, launch for launch.  use_graph: the guide's pointers, shape,
 * activation and guide_weight are part of the graph's key; its weights are read at replay, so values changed in place
 * are followed.  Refusals as dad_sampler_loop and dad_guide_grad, and DAD_E_INVALID for a guide whose `grad` is null
 * or holds fewer than batch * H * td floats; all before any launch. */
int dad_guided_loop(dad_model* m, float* x, const dad_sampler_coef* steps, int32_t n_steps, int32_t batch,
                    const float* noise_stack, uint64_t seed, uint64_t row_offset,
                    const float* cond0, int32_t cond_per_row,
                    const dad_guide_args* guide, float guide_weight,
                    const dad_project_args* proj, const float* proj_alphas_host,
                    int32_t use_graph, void* workspace, size_t workspace_bytes,
                    dad_stream_t stream);

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
 * "halo8_wreg" (which of those launches take the register-weight form conv_halo8w_f32: 1 all, 0 none, -1 = the default,
 * the forms measured faster; the same bits either way),
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

/* ------------------------------------------------------------------------------------------------
 * Plan reports: host-side queries (no device work) that carry the planner's decisions out as flat int32 vectors.  A
 * sized report writes min(capacity, *needed_out) values to `out`: its header, then its records in launch order.
 * Every section of a report — header, record, one kind of record — is stated ONCE, as a list LENGTH_LIST(F) of
 *   F(CONSTANT, the name the Python binding gives the field, ints the field spans, "what it holds")
 * named after the constant LENGTH that holds the section's length.  DAD_LAYOUT(LENGTH, first) makes the constants:
 * each field's offset (the spans before it, counted from `first`) and LENGTH, where the section ends.  A field named
 * `_` is reserved: 0, not reported.  The values a field can take are lists of the same form: value = position.
 * dad_debug_report_layout returns the lists as text, all the binding knows of a layout: a new field costs its line
 * here and one named write in the encoder (csrc/plan_report.hpp). */
#define DAD_LAYOUT_ENUM(NAME, name, span, doc) NAME, NAME##_LAST_ = NAME + (span) - 1,
#define DAD_LAYOUT(LENGTH, first) enum { LENGTH##_FIRST_ = (first) - 1, LENGTH##_LIST(DAD_LAYOUT_ENUM) LENGTH }
/* Section `section` of report `report` (both from 0), NULL outside the table: "LENGTH CONSTANT name span CONSTANT name
 * span ...".  Static text; needs neither a model nor a device. */
const char* dad_debug_report_layout(int32_t report, int32_t section);

/* Which kernels one training step (dad_unet_forward_train + dad_unet_backward) takes at a batch, under the current
 * debug options (needs dad_model_set_training(m, 1) but neither weights nor dad_model_finalize): one record per
 * weight-gradient launch. */
#define DAD_BP_HEADER_LIST(F) \
    F(DAD_BP_WGRADS, wgrads, 1, "weight-gradient launches (conv_wgrad)") \
    F(DAD_BP_MULTI, multi, 1, "... whose fullest block stages more than one chunk (the double-buffered steady state)") \
    F(DAD_BP_MAX_CHUNKS, max_chunks, 1, "most chunks a block stages") \
    F(DAD_BP_MAX_KSPLIT, max_ksplit, 1, "deepest batch split (slabs sum_slabs_kernel adds)") \
    F(DAD_BP_PART, part, 1, "launches whose last chunk is part filled (samples % chunk samples != 0; windows count as samples)") \
    F(DAD_BP_PART_MULTI, part_multi, 1, "... in a block that stages more than one chunk") \
    F(DAD_BP_WINDOWED, windowed, 1, "launches of the windowed kernel (layers longer than 128 positions)") \
    F(DAD_BP_TILE, tile, 4, "[+ tile] launches per wgrad tile: 0 = 64x64, 1 = 64x32, 2 = 32x32, 3 = 32x32 on ragged rows (the trajectory's)") \
    F(DAD_BP_TAPS_TILE, taps_tile, 20, "[+ 4 * i + tile] the same per tap count, i indexing 1, 3, 4, 5, 7 taps") \
    F(DAD_BP_FWD, fwd, 20, "[+ 2 * cfg + s] training-forward conv launches on conv tile cfg (0..9) without / with (s) grid split-K") \
    F(DAD_BP_DGRAD, dgrad, 20, "[+ 2 * cfg + s] the same for the data-gradient convs") \
    F(DAD_BP_RECORD_INTS, record_ints, 1, "ints per record")
DAD_LAYOUT(DAD_BP_HEADER, 0);
#define DAD_BP_REC_INTS_LIST(F) \
    F(DAD_BP_REC_TAPS, taps, 1, "taps") \
    F(DAD_BP_REC_TILE, tile, 1, "wgrad tile, as DAD_BP_TILE") \
    F(DAD_BP_REC_WINDOWED, windowed, 1, "0 / 1") \
    F(DAD_BP_REC_SAMPLES, samples, 1, "samples (windows of a windowed launch)") \
    F(DAD_BP_REC_SPC, spc, 1, "samples per chunk") \
    F(DAD_BP_REC_SPS, sps, 1, "samples per block (a whole number of chunks)") \
    F(DAD_BP_REC_KSPLIT, ksplit, 1, "blocks over the batch") \
    F(DAD_BP_REC_CHUNKS, chunks, 1, "chunks the fullest block stages") \
    F(DAD_BP_REC_LAST_CHUNKS, last_chunks, 1, "chunks the last block stages")
DAD_LAYOUT(DAD_BP_REC_INTS, 0);
int dad_debug_backward_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* Everything dad_unet_backward replays at a batch, step by step, read from the list of steps and the per-batch geometry
 * the entry point launches from (the conditions of dad_debug_backward_plan): one record per step. */
#define DAD_BS_HEADER_LIST(F) \
    F(DAD_BS_STEPS, steps, 1, "records") \
    F(DAD_BS_RECORD_INTS, record_ints, 1, "ints per record") \
    F(DAD_BS_BATCH, batch, 1, "the batch") \
    F(DAD_BS_COLSUMS_LAUNCHES, colsums_launches, 1, "col_sums_many_kernel launches that end the pass") \
    F(DAD_BS_COLSUMS_ENTRIES, colsums_entries, 1, "arrays of `batch` rows they sum, in all") \
    F(DAD_BS_COLSUMS_WIDEST, colsums_widest, 1, "columns of the widest") \
    F(DAD_BS_PADCOPY, padcopy, 1, "1: the horizon is zero padded: pad_rows_kernel copies x and d out in, slice_rows_cols_kernel d x out") \
    F(DAD_BS_HORIZON, horizon, 1, "positions of the padded layout") \
    F(DAD_BS_REAL_HORIZON, real_horizon, 1, "positions that exist") \
    F(DAD_BS_DX, dx, 1, "1: a gradient reaches the trajectory") \
    F(DAD_BS_UNUSED, _, 2, "reserved")
DAD_LAYOUT(DAD_BS_HEADER, 0);
#define DAD_BS_KINDS_LIST(F) \
    F(DAD_BS_K_BIAS, bias, 1, "row_partial_sums_kernel") \
    F(DAD_BS_K_WGRAD, wgrad, 1, "conv_wgrad<taps, tile, windowed>") \
    F(DAD_BS_K_DGRAD, dgrad, 1, "a data-gradient conv (its launch: mode 3 of dad_debug_forward_plan)") \
    F(DAD_BS_K_GN, gn, 1, "gn_mish_bwd_wave_kernel<nv> (nv = 0: gn_mish_bwd_kernel)") \
    F(DAD_BS_K_RESID, resid, 1, "identity residual") \
    F(DAD_BS_K_COLS, cols, 1, "take_cols_kernel")
DAD_LAYOUT(DAD_BS_KINDS, 0);
#define DAD_BS_KIND_FIELD(F) F(DAD_BS_KIND, kind, 1, "DAD_BS_K_*: which of the six lists below names the rest")
#define DAD_BS_REC_INTS_LIST(F) DAD_BS_KIND_FIELD(F) F(DAD_BS_REC_REST, _, 24, "as the kind's list says; 0 where it names nothing")
DAD_LAYOUT(DAD_BS_REC_INTS, 0);
#define DAD_BS_BIAS_INTS_LIST(F) \
    F(DAD_BS_BIAS_ROWS, rows, 1, "rows per sample") \
    F(DAD_BS_BIAS_C, C, 1, "columns") \
    F(DAD_BS_BIAS_UNUSED, _, 22, "reserved")
DAD_LAYOUT(DAD_BS_BIAS_INTS, DAD_BS_REC_REST);
#define DAD_BS_WGRAD_INTS_LIST(F) \
    F(DAD_BS_WG_TAPS, taps, 1, "the instantiation: taps") \
    F(DAD_BS_WG_TILE, tile, 1, "... tile, as DAD_BP_TILE") \
    F(DAD_BS_WG_WINDOWED, windowed, 1, "... windowed") \
    F(DAD_BS_WG_M, M, 1, "rows of the gradient") \
    F(DAD_BS_WG_C0, C0, 1, "columns of the first source") \
    F(DAD_BS_WG_C1, C1, 1, "... of the second (the Z operand is the concat [C0 | C1])") \
    F(DAD_BS_WG_STRIDE, stride, 1, "stride") \
    F(DAD_BS_WG_PAD, pad, 1, "pad") \
    F(DAD_BS_WG_LG, Lg, 1, "rows per sample of G as the kernel counts them (per window when windowed)") \
    F(DAD_BS_WG_LZ, Lz, 1, "... of Z") \
    F(DAD_BS_WG_GX, gx, 1, "grid x") \
    F(DAD_BS_WG_GY, gy, 1, "grid y") \
    F(DAD_BS_WG_RAGGED, ragged, 1, "rows that are not whole aligned float4s") \
    F(DAD_BS_WG_CONCAT_INSIDE, concat_inside, 1, "the boundary C0 falls inside one block's staged columns") \
    F(DAD_BS_WG_EDGE_M, edge_m, 1, "the last M tile is partly filled") \
    F(DAD_BS_WG_EDGE_C, edge_c, 1, "the last C tile is partly filled") \
    F(DAD_BS_WG_SWAPPED, swapped, 1, "G is the conv's input, Z the gradient: the transposed conv") \
    F(DAD_BS_WG_KSPLIT, ksplit, 1, "blocks over the batch") \
    F(DAD_BS_WG_SLAB_N4, slab_n4, 1, "float4s per slab sum_slabs_kernel adds; 0 when ksplit == 1") \
    F(DAD_BS_WG_SAMPLES, samples, 1, "as DAD_BP_REC_SAMPLES") \
    F(DAD_BS_WG_SPC, spc, 1, "as DAD_BP_REC_SPC") \
    F(DAD_BS_WG_SPS, sps, 1, "as DAD_BP_REC_SPS") \
    F(DAD_BS_WG_CHUNKS, chunks, 1, "as DAD_BP_REC_CHUNKS") \
    F(DAD_BS_WG_LAST_CHUNKS, last_chunks, 1, "as DAD_BP_REC_LAST_CHUNKS")
DAD_LAYOUT(DAD_BS_WGRAD_INTS, DAD_BS_REC_REST);
#define DAD_BS_DGRAD_INTS_LIST(F) \
    F(DAD_BS_DG_CONV, conv, 1, "the forward conv") \
    F(DAD_BS_DG_SUB, sub, 1, "which of its data-gradient launches") \
    F(DAD_BS_DG_WRITE, write, 1, "0 set, 1 add through the residual operand, 2 staged and added by add_inplace_kernel") \
    F(DAD_BS_DG_UNUSED, _, 21, "reserved")
DAD_LAYOUT(DAD_BS_DGRAD_INTS, DAD_BS_REC_REST);
#define DAD_BS_GN_INTS_LIST(F) \
    F(DAD_BS_GN_NV, nv, 1, "the instantiation") \
    F(DAD_BS_GN_CPG, cpg, 1, "channels per group") \
    F(DAD_BS_GN_L, L, 1, "positions") \
    F(DAD_BS_GN_LREAL, lreal, 1, "> 0: positions that exist") \
    F(DAD_BS_GN_CPG_REAL, cpg_real, 1, "> 0: channels per group that exist") \
    F(DAD_BS_GN_DTEMB, dtemb, 1, "d time projection is written") \
    F(DAD_BS_GN_SHORT_PAIR, short_pair, 1, "a pair has fewer than 64 float4") \
    F(DAD_BS_GN_C, C, 1, "channels") \
    F(DAD_BS_GN_UNUSED, _, 16, "reserved")
DAD_LAYOUT(DAD_BS_GN_INTS, DAD_BS_REC_REST);
#define DAD_BS_RESID_INTS_LIST(F) \
    F(DAD_BS_RS_WRITE, write, 1, "0: a copy, 1: add_inplace_kernel") \
    F(DAD_BS_RS_N, n, 1, "floats per sample") \
    F(DAD_BS_RS_TO_X, to_x, 1, "into d x") \
    F(DAD_BS_RS_UNUSED, _, 21, "reserved")
DAD_LAYOUT(DAD_BS_RESID_INTS, DAD_BS_REC_REST);
#define DAD_BS_COLS_INTS_LIST(F) \
    F(DAD_BS_CL_C, C, 1, "columns taken") \
    F(DAD_BS_CL_OFF, off, 1, "... from this column on") \
    F(DAD_BS_CL_LD, ld, 1, "... of rows this long") \
    F(DAD_BS_CL_ROWS, rows, 1, "rows per sample") \
    F(DAD_BS_CL_WRITE, write, 1, "1: accumulates") \
    F(DAD_BS_CL_UNUSED, _, 19, "reserved")
DAD_LAYOUT(DAD_BS_COLS_INTS, DAD_BS_REC_REST);
int dad_debug_backward_steps(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* The time chain of one fused objective step (dad_train_objective_forward + dad_train_objective_backward) at a batch:
 * the list of launches the two entry points replay (needs dad_model_set_training(m, 1) but neither weights nor
 * dad_model_finalize; a batch the objective refuses is refused here too): one record per launch (3 forward, 6
 * backward), each out[M][N] = sum over K on a grid of 32 x 32 output tiles (x, y) and K slices (z). */
#define DAD_OP_HEADER_LIST(F) \
    F(DAD_OP_LOSS_BLOCKS, loss_blocks, 1, "blocks of the loss's partial sums (at most 1024)") \
    F(DAD_OP_KSLICES, kslices, 1, "K slices of d act = d rows . W (slabs time_dtemb_kernel adds in slice order)") \
    F(DAD_OP_KSLICE, kslice, 1, "k values per slice (a multiple of 128)") \
    F(DAD_OP_TEMB_WIDTH, temb_width, 1, "columns of the time projections (padded widths), the K of that product") \
    F(DAD_OP_BLOCKS, blocks, 1, "ResidualTemporalBlocks") \
    F(DAD_OP_N, n, 1, "batch x horizon x transition_dim: the elements the loss is a mean of (real ones only)") \
    F(DAD_OP_RECORD_INTS, record_ints, 1, "ints per record") \
    F(DAD_OP_LAUNCHES, launches, 1, "records: 9")
DAD_LAYOUT(DAD_OP_HEADER, 0);
#define DAD_OP_REC_INTS_LIST(F) \
    F(DAD_OP_REC_MODE, mode, 1, "DAD_OP_TG_*") \
    F(DAD_OP_REC_M, M, 1, "M") \
    F(DAD_OP_REC_N, N, 1, "N") \
    F(DAD_OP_REC_K, K, 1, "K") \
    F(DAD_OP_REC_GRID_X, gx, 1, "grid x") \
    F(DAD_OP_REC_GRID_Y, gy, 1, "grid y") \
    F(DAD_OP_REC_GRID_Z, gz, 1, "grid z") \
    F(DAD_OP_REC_CHUNKS, chunks, 1, "32-wide K chunks in a full slice (the block's four waves take them round robin); 0 for DTEMB") \
    F(DAD_OP_REC_LAST_CHUNKS, last_chunks, 1, "... in the last slice; 0 for DTEMB") \
    F(DAD_OP_REC_KTAIL, ktail, 1, "K % 32; 0 for DTEMB") \
    F(DAD_OP_REC_KSLICE, kslice, 1, "k values per slice")
DAD_LAYOUT(DAD_OP_REC_INTS, 0);
#define DAD_OP_TG_MODES_LIST(F) \
    F(DAD_OP_TG_FWD_H1, FWD_H1, 1, "(time_gemm_kernel's eight instantiations, in the order of TimeGemm) h1 = emb W1^T + b1") \
    F(DAD_OP_TG_FWD_TEMB, FWD_TEMB, 1, "temb = mish(h1) W3^T + b3, act = mish(temb)") \
    F(DAD_OP_TG_FWD_ROWS, FWD_ROWS, 1, "rows = act Wk^T + bk, all blocks") \
    F(DAD_OP_TG_BWD_DWK, BWD_DWK, 1, "d Wk = d rows^T act, d bk") \
    F(DAD_OP_TG_BWD_DACT, BWD_DACT, 1, "d act = d rows W, K slices in slabs") \
    F(DAD_OP_TG_BWD_DW3, BWD_DW3, 1, "d W3 = d temb^T mish(h1), d b3") \
    F(DAD_OP_TG_BWD_DH1, BWD_DH1, 1, "d h1 = (d temb W3) mish'(h1)") \
    F(DAD_OP_TG_BWD_DW1, BWD_DW1, 1, "d W1 = d h1^T emb, d b1") \
    F(DAD_OP_TG_DTEMB, DTEMB, 1, "time_dtemb_kernel: M x N elements, K = slabs added")
DAD_LAYOUT(DAD_OP_TG_MODES, 0);
int dad_debug_objective_plan(dad_model* m, int32_t batch, int32_t* out, int32_t capacity, int32_t* needed_out);

/* What one dynamics-aware objective step (dad_train_dynamics_objective_forward + _backward) adds to the fused objective
 * step of the report above, for a projector over (state_dim, observation_dim, action_dim) under `form`: the layout of
 * its own parts of `saved` / `scratch` and one record per launch of its own kernels, the forward's first (host logic
 * only; needs what dad_debug_objective_plan needs; a shape the entry points refuse is refused here too, a forced row
 * form that does not fit is reported, DAD_DO_REFUSED).  Sizes are capped at INT32_MAX. */
#define DAD_DO_HEADER_LIST(F) \
    F(DAD_DO_FORM, form, 1, "DAD_VG_ROW / DAD_VG_GEMM: the form both passes take (plan_violation_grad's choice for x0_hat's shape)") \
    F(DAD_DO_D, D, 1, "(H + 1) state_dim + H action_dim") \
    F(DAD_DO_HORIZON, horizon, 1, "H: the trajectories' horizon (the real one of a zero-padded model)") \
    F(DAD_DO_COL_BLOCKS, col_blocks, 1, "gemm: 32-column blocks of P = partial sums per trajectory; row: 0") \
    F(DAD_DO_REFUSED, refused, 1, "1: the calls fail with DAD_E_INVALID (a forced row form beyond one CU's LDS)") \
    F(DAD_DO_SAVED_BASE, saved_base, 1, "bytes of `saved` the fused objective holds (dad_train_objective_workspace_bytes, rounded up to 256)") \
    F(DAD_DO_SAVED_BYTES, saved_bytes, 1, "dad_train_dynamics_objective_workspace_bytes: saved") \
    F(DAD_DO_SCRATCH_BASE, scratch_base, 1, "bytes of `scratch` the fused objective holds") \
    F(DAD_DO_SCRATCH_BYTES, scratch_bytes, 1, "dad_train_dynamics_objective_workspace_bytes: scratch") \
    F(DAD_DO_R_OFFSET, r_offset, 1, "saved, floats behind saved_base: the residual r (B, D)") \
    F(DAD_DO_PART_OFFSET, part_offset, 1, "... gemm: sums of r^2 per (trajectory, column block)") \
    F(DAD_DO_VIOLATION_OFFSET, violation_offset, 1, "... row: the violation per trajectory (B)") \
    F(DAD_DO_G_OFFSET, g_offset, 1, "scratch, floats behind scratch_base: gemm: g (B, D)") \
    F(DAD_DO_OBJECTIVE_LAUNCHES, objective_launches, 1, "launches of the time chain the step shares with the fused objective (dad_debug_objective_plan): 9") \
    F(DAD_DO_FWD_LAUNCHES, fwd_launches, 1, "records that belong to the forward: 2") \
    F(DAD_DO_RECORD_INTS, record_ints, 1, "ints per record") \
    F(DAD_DO_LAUNCHES, launches, 1, "records: 3 (row) or 4 (gemm)")
DAD_LAYOUT(DAD_DO_HEADER, 0);
#define DAD_DO_REC_INTS_LIST(F) \
    F(DAD_DO_REC_KIND, kind, 1, "DAD_DO_K_*") \
    F(DAD_DO_REC_GRID_X, gx, 1, "grid x") \
    F(DAD_DO_REC_GRID_Y, gy, 1, "grid y") \
    F(DAD_DO_REC_THREADS, threads, 1, "threads per block") \
    F(DAD_DO_REC_LDS_BYTES, lds_bytes, 1, "dynamic LDS of one block") \
    F(DAD_DO_REC_ROWS_PER_BLOCK, rows_per_block, 1, "trajectories per block (0: an elementwise launch)")
DAD_LAYOUT(DAD_DO_REC_INTS, 0);
#define DAD_DO_KINDS_LIST(F) \
    F(DAD_DO_K_FWD_ROW, fwd_row, 1, "dynamics_violation_fwd_row_kernel: project_kernel's violation branch with x0_hat formed in the gather, r kept") \
    F(DAD_DO_K_FWD_GEMM, fwd_gemm, 1, "dynamics_violation_fwd_gemm_kernel: violation_fwd_gemm_kernel's body on the same gather") \
    F(DAD_DO_K_FWD_PARTS, fwd_parts, 1, "dynamics_parts_kernel: Lp = sum_b tw violation_b / (B D) in one fixed order, and the total") \
    F(DAD_DO_K_BWD_ROW, bwd_row, 1, "dynamics_violation_bwd_row_kernel: violation_bwd_row_kernel's body; its epilogue writes d total / d out") \
    F(DAD_DO_K_BWD_GEMM, bwd_gemm, 1, "dynamics_violation_bwd_gemm_kernel: violation_bwd_gemm_kernel's body with the per-trajectory factor formed on the device") \
    F(DAD_DO_K_BWD_SCATTER, bwd_scatter, 1, "dynamics_scatter_dout_kernel: d total / d out from g and the diffusion term's unit gradient")
DAD_LAYOUT(DAD_DO_KINDS, 0);
int dad_debug_dynamics_objective_plan(dad_model* m, int32_t batch, int32_t state_dim, int32_t observation_dim,
                                      int32_t action_dim, int32_t form, int32_t* out, int32_t capacity, int32_t* needed_out);

/* What one forward evaluation launches at a batch under the current debug options: the description the entry point
 * itself replays (csrc/host_plan.hpp: FwdPlan of plan_forward; mode 3: TrainScratch of train_scratch), written down
 * (host-side query, no device work; needs neither weights nor dad_model_finalize; modes 2 / 3 need
 * dad_model_set_training(m, 1); a batch the call refuses is refused here too).  `mode`:
 *   0  dad_unet_forward / dad_denoise_step with one shared timestep (may take the small-batch kernels)
 *   1  the same evaluation on the batch kernels: dad_unet_forward_rows (per-row timesteps)
 *   2  dad_unet_forward_train (the training plan)
 *   3  the data-gradient conv launches of dad_unet_backward, in launch order
 * One record per conv-GEMM launch (a 1x1 residual conv that rides in its carrier's launch has none) or, with
 * [DAD_FP_SMALL], one DAD_FP_CC_* record per launched small-batch conv instead. */
#define DAD_FP_HEADER_LIST(F) \
    F(DAD_FP_MODE, mode, 1, "as asked") \
    F(DAD_FP_BATCH, batch, 1, "as asked") \
    F(DAD_FP_SMALL, small, 1, "1: the small-batch plan is taken (csrc/conv_cc.hpp, conv_ccw.hpp)") \
    F(DAD_FP_RECORDS, records, 1, "records") \
    F(DAD_FP_RECORD_INTS, record_ints, 1, "ints per record") \
    F(DAD_FP_FINAL_GX, final_gx, 1, "grid x of the final kernel (0 in mode 3)") \
    F(DAD_FP_FINAL_GY, final_gy, 1, "grid y") \
    F(DAD_FP_FINAL_KERNEL, final_kernel, 1, "DAD_FP_FINAL_*")
DAD_LAYOUT(DAD_FP_HEADER, 0);
#define DAD_FP_FINALS_LIST(F) \
    F(DAD_FP_FINAL_NONE, none, 1, "mode 3") \
    F(DAD_FP_FINAL_POSTERIOR, final_posterior_kernel, 1, "the batch kernels' final kernel") \
    F(DAD_FP_FINAL_CC, final_cc_kernel, 1, "the small-batch plan's")
DAD_LAYOUT(DAD_FP_FINALS, 0);
#define DAD_FP_REC_INTS_LIST(F) \
    F(DAD_FP_REC_CONV, conv, 1, "index into the plan (mode 3: the forward conv whose data gradient this is, -1 = final_conv[1])") \
    F(DAD_FP_REC_SUB, sub, 1, "mode 3: which of that conv's data-gradient launches") \
    F(DAD_FP_REC_CFG, cfg, 1, "tile cfg") \
    F(DAD_FP_REC_TAPS, taps, 1, "taps") \
    F(DAD_FP_REC_STRIDE, stride, 1, "stride") \
    F(DAD_FP_REC_FLAGS, flags, 1, "bit 0 x3, 1 bdir, 2 ragged, 3 res (the ride), 4 padded, 5 windowed: kernel_registered_f's flag word; (cfg, taps, stride, flags) names the conv_gemm_f32 instantiation, cfg 0 / 1 and bit 3 the conv_halo8_f32 one") \
    F(DAD_FP_REC_KC, kc, 1, "K chunk") \
    F(DAD_FP_REC_KSLICES, kslices, 1, "grid-level K slices") \
    F(DAD_FP_REC_GN_NPT, gn_npt, 1, "npt of the gn_pass_kernel<npt> launch that follows (0: none)") \
    F(DAD_FP_REC_NTILES_N, ntiles_n, 1, "N tiles") \
    F(DAD_FP_REC_MTILES, mtiles, 1, "M tiles") \
    F(DAD_FP_REC_PART_TILE, part_tile, 1, "1 when the last N tile holds fewer samples than it has room for") \
    F(DAD_FP_REC_FAMILY, family, 1, "DAD_FP_FAMILY_*")
DAD_LAYOUT(DAD_FP_REC_INTS, 0);
#define DAD_FP_FAMILIES_LIST(F) \
    F(DAD_FP_FAMILY_GEMM, gemm, 1, "conv_gemm_f32") \
    F(DAD_FP_FAMILY_HALO8, halo8, 1, "conv_halo8_f32 of csrc/conv_halo8.hpp on the same tile, grid and ride") \
    F(DAD_FP_FAMILY_HALO8W, halo8w, 1, "its register-weight form conv_halo8w_f32 under the same key (option halo8_wreg)")
DAD_LAYOUT(DAD_FP_FAMILIES, 0);
#define DAD_FP_CC_INTS_LIST(F) \
    F(DAD_FP_CC_CONV, conv, 1, "index into the plan") \
    F(DAD_FP_CC_TAPS, taps, 1, "taps") \
    F(DAD_FP_CC_STRIDE, stride, 1, "stride") \
    F(DAD_FP_CC_WIDE, wide, 1, "conv_ccw") \
    F(DAD_FP_CC_RIDE, ride, 1, "a 1x1 residual conv rides") \
    F(DAD_FP_CC_BIG, big, 1, "the big form") \
    F(DAD_FP_CC_RIDE_IN, ride_in, 1, "consumes ride slabs") \
    F(DAD_FP_CC_TILE_ROWS, tile_rows, 1, "rows per tile (16 / 32)") \
    F(DAD_FP_CC_WINDOWED, windowed, 1, "windowed") \
    F(DAD_FP_CC_SLICE_CH, slice_ch, 1, "channels per K slice") \
    F(DAD_FP_CC_KSLICES, kslices, 1, "K slices") \
    F(DAD_FP_CC_NTILES, ntiles, 1, "N tiles") \
    F(DAD_FP_CC_RES_KIND, res_kind, 1, "how the residual reaches its consumer: 0 none, 1 the trajectory, 2 a finished tensor, 3 a carrier's ride slabs, 4 a stand-alone 1x1 conv's slabs")
DAD_LAYOUT(DAD_FP_CC_INTS, 0);
int dad_debug_forward_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out);
/* The conv_halo8_f32 launches (csrc/conv_halo8.hpp) of the same description, modes 0 and 1 only, with what the kernel
 * makes of its ConvParams: read from the ConvOp / LaunchGeom the launch fills them from (csrc/plan_report.hpp,
 * halo8_plan_encode), nothing decided: one record per launch. */
#define DAD_H8_HEADER_LIST(F) \
    F(DAD_H8_RECORDS, records, 1, "records") \
    F(DAD_H8_RECORD_INTS, record_ints, 1, "ints per record")
DAD_LAYOUT(DAD_H8_HEADER, 0);
#define DAD_H8_INTS_LIST(F) \
    F(DAD_H8_CONV, conv, 1, "conv index") \
    F(DAD_H8_CFG, cfg, 1, "the instantiation: tile (0 / 1)") \
    F(DAD_H8_RIDE, ride, 1, "... the riding 1x1 conv") \
    F(DAD_H8_CHUNKS, chunks, 1, "32-channel K chunks, (cin0 + cin1) / 32") \
    F(DAD_H8_SRC1_CHUNK, src1_chunk, 1, "the chunk from which the second source is read, -1 without one") \
    F(DAD_H8_RES, res, 1, "a residual operand is present") \
    F(DAD_H8_TEMB, temb, 1, "a time embedding is present") \
    F(DAD_H8_PER_ROW, per_row, 1, "the time embedding is indexed per sample (mode 1, where there is one)") \
    F(DAD_H8_GN, gn, 1, "GroupNorm runs in the kernel") \
    F(DAD_H8_WPP, wpp, 1, "waves one (sample, group) pair spans (0 without GroupNorm; > 1: the cross-wave sum through LDS)") \
    F(DAD_H8_XCD_GN, xcd_gn, 1, "0: the plain grid (y = M tile, z = N tile), else the XCD-aware tile order") \
    F(DAD_H8_MTILES, mtiles, 1, "as DAD_FP_REC_MTILES") \
    F(DAD_H8_NTILES_N, ntiles_n, 1, "as DAD_FP_REC_NTILES_N") \
    F(DAD_H8_PART_TILE, part_tile, 1, "as DAD_FP_REC_PART_TILE")
DAD_LAYOUT(DAD_H8_INTS, 0);
int dad_debug_halo8_plan(dad_model* m, int32_t batch, int32_t mode, int32_t* out, int32_t capacity, int32_t* needed_out);
/* Which kernel one dad_project (violation == 0) or dad_projection_violation (violation != 0) call launches for
 * trajectories (batch, horizon, observation_dim + action_dim) and a dad_project_args.scratch of scratch_bytes (0: none),
 * and on which grid: the plan the two entry points launch from.  Host logic only, no device call.  out[DAD_PP_INTS]. */
#define DAD_PP_INTS_LIST(F) \
    F(DAD_PP_FORM, form, 1, "DAD_PP_ROW1 / ROW4 / GEMM") \
    F(DAD_PP_ROWS_PER_BLOCK, rows_per_block, 1, "1, 4 or 32") \
    F(DAD_PP_GX, gx, 1, "grid x") \
    F(DAD_PP_GY, gy, 1, "grid y") \
    F(DAD_PP_LDS_BYTES, lds_bytes, 1, "dynamic LDS of one block") \
    F(DAD_PP_REFUSED, refused, 1, "1: the call fails with DAD_E_INVALID (a trajectory's partial sums exceed LDS and the GEMM form has no scratch or fewer than 32 trajectories); the other fields then describe the launch that does not fit")
DAD_LAYOUT(DAD_PP_INTS, 0);
#define DAD_PP_FORMS_LIST(F) \
    F(DAD_PP_ROW1, row1, 1, "project_kernel<1,16>: one trajectory per block") \
    F(DAD_PP_ROW4, row4, 1, "project_kernel<4,16>: four per block, batches beyond 512 whose four rows fit LDS") \
    F(DAD_PP_GEMM, gemm, 1, "project_gemm_kernel: 32 trajectories x 32 columns of P per block; never for the violation")
DAD_LAYOUT(DAD_PP_FORMS, 0);
int dad_debug_project_plan(int32_t state_dim, int32_t observation_dim, int32_t action_dim, int32_t batch, int32_t horizon,
                           size_t scratch_bytes, int32_t violation, int32_t* out);
/* Which kernels one dad_projection_violation_fwd / _bwd pair launches for trajectories (batch, horizon,
 * observation_dim + action_dim) under `form` (-1, 0, 1 as there), on which grids, and the workspace it needs: the plan
 * the two entry points launch from (plan_violation_grad).  Host logic only, no device call.  out[DAD_VG_INTS].
 * DAD_E_INVALID for batch or horizon <= 0, state_dim > observation_dim or an unknown form; a forced row form that does
 * not fit is reported (DAD_VG_REFUSED), not refused here. */
#define DAD_VG_INTS_LIST(F) \
    F(DAD_VG_FORM, form, 1, "DAD_VG_ROW / DAD_VG_GEMM: the form both passes take") \
    F(DAD_VG_FWD_ROWS_PER_BLOCK, fwd_rows_per_block, 1, "forward: trajectories per block (row: 1 or 4, as dad_projection_violation plans; gemm: 32)") \
    F(DAD_VG_FWD_GX, fwd_gx, 1, "... grid x (blocks over the batch)") \
    F(DAD_VG_FWD_GY, fwd_gy, 1, "... grid y (gemm: 32-column blocks of P; row: 1)") \
    F(DAD_VG_FWD_LDS_BYTES, fwd_lds_bytes, 1, "... dynamic LDS of one block") \
    F(DAD_VG_FWD_SUM_GX, fwd_sum_gx, 1, "... blocks of the launch that adds the column blocks' partial sums per trajectory (gemm; row: 0, no such launch)") \
    F(DAD_VG_BWD_ROWS_PER_BLOCK, bwd_rows_per_block, 1, "backward: trajectories per block (row: 1; gemm: 32)") \
    F(DAD_VG_BWD_GX, bwd_gx, 1, "... grid x") \
    F(DAD_VG_BWD_GY, bwd_gy, 1, "... grid y (gemm: 32-row blocks of P; row: 1)") \
    F(DAD_VG_BWD_LDS_BYTES, bwd_lds_bytes, 1, "... dynamic LDS of one block") \
    F(DAD_VG_BWD_SCATTER_GX, bwd_scatter_gx, 1, "... blocks of the launch that scatters g into d_x (gemm; row: 0, the row kernel scatters itself)") \
    F(DAD_VG_WORKSPACE_BYTES, workspace_bytes, 1, "dad_violation_grad_workspace_bytes (capped at INT32_MAX): r (B, D), and in the gemm form the partial sums (B, column blocks) and g (B, D)") \
    F(DAD_VG_REFUSED, refused, 1, "1: the calls fail with DAD_E_INVALID (a forced row form whose forward LDS, a row and its 16 partial sets, exceeds one CU's); the other fields then describe the launches that do not fit")
DAD_LAYOUT(DAD_VG_INTS, 0);
#define DAD_VG_FORMS_LIST(F) \
    F(DAD_VG_ROW, row, 1, "project_kernel's violation branch keeping r, violation_bwd_row_kernel: one trajectory per block streams P") \
    F(DAD_VG_GEMM, gemm, 1, "violation_fwd_gemm_kernel, violation_bwd_gemm_kernel: 32 trajectories x 32 columns per block, P read once per 32 trajectories")
DAD_LAYOUT(DAD_VG_FORMS, 0);
int dad_debug_violation_grad_plan(int32_t state_dim, int32_t observation_dim, int32_t action_dim, int32_t batch,
                                  int32_t horizon, int32_t form, int32_t* out);
/* What one dad_guide_grad call (and every guide launch of dad_guided_loop) launches for a value net of `n_layers`
 * Linear layers in_dim -> widths[0] -> ... -> widths[n_layers - 1] with `activation` (DAD_GD_ACTS) between them, on
 * trajectories (batch, horizon, transition_dim): plan_guide of csrc/host_plan.hpp, the one statement of the limits
 * on the value models (guides/policies.py:243-271) whose gradient (guides/policies.py:87-97) the library takes itself.
 * Host logic only, no device call.  out[DAD_GD_INTS].  DAD_E_INVALID for a null pointer or batch, horizon or
 * transition_dim <= 0 (or more than 2^31 elements); a net the library does not evaluate is reported
 * (DAD_GD_REFUSED), not refused here. */
#define DAD_GD_INTS_LIST(F) \
    F(DAD_GD_LAYERS, layers, 1, "Linear layers, as given") \
    F(DAD_GD_PADDED_IN, padded_in, 1, "in_dim zero-padded to whole 32-column MFMA tiles: dad_guide_args.padded[0]") \
    F(DAD_GD_PADDED_1, padded_1, 1, "widths[0] padded likewise (padded[1]); 0 where refused before the widths were read") \
    F(DAD_GD_PADDED_2, padded_2, 1, "widths[1] padded, 0 unless it is a hidden layer") \
    F(DAD_GD_PADDED_3, padded_3, 1, "widths[2] padded, 0 unless it is a hidden layer") \
    F(DAD_GD_ROWS_PER_BLOCK, rows_per_block, 1, "rows of batch * horizon one block owns: 32") \
    F(DAD_GD_THREADS, threads, 1, "threads of a block") \
    F(DAD_GD_GX, gx, 1, "grid x: blocks over the rows, each row in exactly one") \
    F(DAD_GD_LDS_BYTES, lds_bytes, 1, "dynamic LDS of one block: 33 floats per kept column (the padded input, every padded hidden width, twice under Mish)") \
    F(DAD_GD_REFUSED, refused, 1, "DAD_GD_REFUSALS: 0, or the first limit the net misses (the calls then fail with DAD_E_INVALID)")
DAD_LAYOUT(DAD_GD_INTS, 0);
#define DAD_GD_ACTS_LIST(F) \
    F(DAD_GD_TANH, tanh, 1, "nn.Tanh") \
    F(DAD_GD_RELU, relu, 1, "nn.ReLU (derivative 0 at 0, as torch)") \
    F(DAD_GD_MISH, mish, 1, "nn.Mish, through the conv epilogue's device function")
DAD_LAYOUT(DAD_GD_ACTS, 0);
#define DAD_GD_REFUSALS_LIST(F) \
    F(DAD_GD_OK, ok, 1, "the net is evaluated") \
    F(DAD_GD_BAD_LAYERS, layers, 1, "fewer than 2 or more than 4 Linear layers") \
    F(DAD_GD_BAD_WIDTH, width, 1, "a width below 1 or above 512") \
    F(DAD_GD_BAD_ACT, activation, 1, "an activation that is none of DAD_GD_ACTS") \
    F(DAD_GD_BAD_IN_DIM, in_dim, 1, "in_dim below 1 or above transition_dim") \
    F(DAD_GD_BAD_LAST, last_width, 1, "the last layer has more than one output") \
    F(DAD_GD_BAD_LDS, lds, 1, "the kept tensors of 32 rows exceed one CU's LDS")
DAD_LAYOUT(DAD_GD_REFUSALS, 0);
int dad_debug_guide_plan(int32_t in_dim, const int32_t* widths, int32_t n_layers, int32_t activation, int32_t batch,
                         int32_t horizon, int32_t transition_dim, int32_t* out);
/* Whether dad_sample_loop at `batch` (projection != 0: called with a projection argument) takes the seam between two
 * denoise steps as one launch (csrc/conv_seam.hpp; the rule: plan_seam in csrc/host_plan.hpp), under the model's current
 * options.  Host logic only, no device call; the model needs no weights.  out[DAD_SEAM_INTS]. */
#define DAD_SEAM_INTS_LIST(F) \
    F(DAD_SEAM_TAKEN, taken, 1, "1 / 0") \
    F(DAD_SEAM_REASON, reason, 1, "0 = taken, else the first condition that refuses it; dad_debug_seam_reason names it") \
    F(DAD_SEAM_GRID, grid, 1, "the launch: blocks (0 when refused)") \
    F(DAD_SEAM_THREADS, threads, 1, "... threads (0 when refused)") \
    F(DAD_SEAM_LDS_BYTES, lds_bytes, 1, "... LDS (0 when refused)") \
    F(DAD_SEAM_TILE, tile, 1, "the first conv's tile (0 or 1), whose summation order the launch keeps; -1 when refused") \
    F(DAD_SEAM_UNITS, units, 1, "8-channel units it multiplies (1: transition_dim <= 8, 2)") \
    F(DAD_SEAM_SPT, spt, 1, "samples of one 32-row tile (32 / horizon); 0 when refused") \
    F(DAD_SEAM_LAST, last, 1, "samples in the last tile (1 .. spt); 0 when refused") \
    F(DAD_SEAM_BUFFERS, buffers, 1, "which allowed relation of seam_buffers_ok holds, DAD_SEAM_BUF_*; -1 when refused") \
    F(DAD_SEAM_DIM, dim, 1, "the instantiation conv_seam_f32<dim, tile0>: dim; 0 when refused") \
    F(DAD_SEAM_TILE0, tile0, 1, "... tile0; -1 when refused")
DAD_LAYOUT(DAD_SEAM_INTS, 0);
#define DAD_SEAM_BUFS_LIST(F) \
    F(DAD_SEAM_BUF_APART, apart, 1, "final_act overlaps neither buffer the launch writes") \
    F(DAD_SEAM_BUF_DST, dst, 1, "it is the conv's dst") \
    F(DAD_SEAM_BUF_RDST, rdst, 1, "it is the ride's")
DAD_LAYOUT(DAD_SEAM_BUFS, 0);
int dad_debug_seam_plan(dad_model* m, int32_t batch, int32_t projection, int32_t* out);
const char* dad_debug_seam_reason(int32_t reason);
/* The kernels of one family in the library's own registry: the table every launch looks its kernel up in (no device
 * call): the header, then the keys. */
#define DAD_KL_HEADER_LIST(F) \
    F(DAD_KL_KERNELS, kernels, 1, "keys that follow") \
    F(DAD_KL_KEY_INTS, key_ints, 1, "ints of one key")
DAD_LAYOUT(DAD_KL_HEADER, 0);
#define DAD_FAMILIES_LIST(F) \
    F(DAD_FAMILY_GEMM, gemm, 1, "conv_gemm_f32   (tile cfg, taps, stride, flag word as DAD_FP_REC_FLAGS)") \
    F(DAD_FAMILY_CC, cc, 1, "conv_cc         (taps, stride, riding 1x1 conv, big, rows per tile, windowed)") \
    F(DAD_FAMILY_CCW, ccw, 1, "conv_ccw        (taps, stride, riding 1x1 conv, ride_in, rows per tile)") \
    F(DAD_FAMILY_HALO8, halo8, 1, "conv_halo8_f32  (tile cfg, riding 1x1 conv)") \
    F(DAD_FAMILY_SEAM, seam, 1, "conv_seam_f32   (dim, the first conv's tile is 0)") \
    F(DAD_FAMILY_WGRAD, wgrad, 1, "conv_wgrad      (taps, tile as DAD_BP_TILE, windowed)")
DAD_LAYOUT(DAD_FAMILIES, 0);
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
 * no device call): one record per chunk in chunk order. */
#define DAD_OS_HEADER_LIST(F) \
    F(DAD_OS_CHUNK, chunk, 1, "elements per chunk (a multiple of 4)") \
    F(DAD_OS_CHUNKS, chunks, 1, "chunks = records") \
    F(DAD_OS_GRID, grid, 1, "blocks of each of the two kernels (at most 2048)") \
    F(DAD_OS_PARTIALS, partials, 1, "partial square sums (one per block)") \
    F(DAD_OS_RECORD_INTS, record_ints, 1, "ints per record")
DAD_LAYOUT(DAD_OS_HEADER, 0);
#define DAD_OS_REC_INTS_LIST(F) \
    F(DAD_OS_REC_TENSOR, tensor, 1, "tensor") \
    F(DAD_OS_REC_FIRST, first, 1, "first element: its low 31 bits") \
    F(DAD_OS_REC_FIRST_HI, first_hi, 1, "... the bits above") \
    F(DAD_OS_REC_COUNT, count, 1, "elements") \
    F(DAD_OS_REC_BLOCK, block, 1, "the block that owns the chunk (a block walks its chunks in this order)")
DAD_LAYOUT(DAD_OS_REC_INTS, 0);
int dad_debug_optim_plan(const int64_t* numel, int32_t n, int32_t* out, int32_t capacity, int32_t* needed_out);

#ifdef __cplusplus
}
#endif
#endif /* DAD_H */
