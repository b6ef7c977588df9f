/*
 * mi355ppo.h -- C ABI of libmi355ppo.so: the MI355X (gfx950 / CDNA4) PPO hot path.
 *
 * The reference (vwxyzjn/cleanrl) has no FFI, plugin or operator boundary: its PPO scripts are
 * executed, never imported, and the hot path is inline tensor code.  This header therefore DEFINES
 * the drop-in boundary at the tensor seams of that inline code; every entry point cites the
 * reference lines (cleanrl/<file>:<lines>) whose op chain it replaces.  A maintainer binds it with
 * ctypes (the reference is Python) -- see INTEGRATION.md for the stub.
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensor .data_ptr()),
 *     contiguous, row-major, never retained past the call;
 *   - no allocation, no hipMalloc/hipFree, no host<->device copy, no device synchronisation inside:
 *     work is only enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream),
 *     so every call is legal inside a hipGraph stream capture;
 *   - scratch memory is caller-provided (`workspace`, sized by the *_workspace_bytes query) and is
 *     written before it is read in every call: it needs no initialisation and may be shared by
 *     calls that are ordered on one stream;
 *   - hyper-parameters are `double` because the reference holds them as Python floats and torch
 *     rounds them to f32 at each scalar-tensor op; the kernels reproduce that rounding;
 *   - return 0 on success, a negative MI355PPO_E* code otherwise; mi355ppo_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - re-entrant and thread-safe: no global mutable state.
 */
#ifndef MI355PPO_H_
#define MI355PPO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355PPO_VERSION 271 /* major*100 + minor*10 + patch.  The minor moves whenever an exported signature changes or an entry
                                  point is added (1.1: adv_mean_den / conv1_variant arguments of round 2; 1.2, 1.3: round 3;
                                  1.4: the *_cpu host-pointer twins; 1.5: mi355ppo_init; 1.6: round 4 -- the fused MLP family K7,
                                  mi355ppo_clip_adam_sched_f32; 1.7: mi355ppo_fc_heads_act_categorical_f32, mi355ppo_nature_packs_f32,
                                  mi355ppo_synth_atari_step_hwc_ctr_u8; 1.8: round 5 -- the *_f16x2 / *_amax entry points and mi355ppo_absmax_f32;
                                  1.9: round 6 -- the kernel queries mi355ppo_fc_packed_kernel_f16x2, mi355ppo_fc_wgrad_kernel_f16x2, mi355ppo_cnn_conv_wgrad_kernel_f16x2;
                                  heads of up to 18 actions, a 4-byte-aligned critic row; 2.0: the peer-memory gradient exchange mi355ppo_dp_*; 2.1: the fused MLP family takes obs_dim <= 512, n_out <= 20;
                                  2.2: the done-masked LSTM sequence scans mi355ppo_lstm_seq_fwd_f32 / _bwd_f32 and their *_cpu twins;
                                  2.3: the TrXL episodic-memory attention mi355ppo_trxl_attn_fwd_f32 / _bwd_f32 and their *_cpu twins;
                                  2.4: the IMPALA-CNN trunk mi355ppo_impala_* (forward, backward, max pool, sizes) and the *_cpu twins;
                                  2.5: PQN -- mi355ppo_pqn_* (e-greedy, Q(lambda), TD loss, the LayerNorm MLP), clip + RAdam, the *_cpu twins;
                                  2.6: the recurrent PQN tail mi355ppo_pqn_lstm_act_f32, mi355ppo_pqn_lstm_td_fwd_bwd_f32 (+ workspace size) and their *_cpu twins);
                                  2.7: DDPG / TD3 -- the device replay ring and mi355ppo_td3_* / mi355ppo_polyak_f32 and their *_cpu twins;
                                  2.7.1: SAC -- mi355ppo_sac_* (policy, target, actor, alpha) and their *_cpu twins.  Entry points were only
                                  added and no existing signature moved, so a 2.7 binding keeps working against this library: the patch
                                  moves, the minor stays;
                                  DQN / C51 -- mi355ppo_dqn_act_f32, mi355ppo_dqn_td_fwd_bwd_f32, mi355ppo_c51_fwd_bwd_f32 (+ workspace sizes) and
                                  their *_cpu twins were added the same way: no existing signature moved, and the number stays at 2.7.1 (a
                                  binding finds out whether they are there by looking the symbols up);
                                  the Atari DQN / C51 heads, Rainbow and discrete SAC on Atari (mi355ppo_replay_add2_u8, mi355ppo_replay_gather2_u8,
                                  mi355ppo_sacd_*) likewise;
                                  RND -- mi355ppo_rnd_* (newest-frame normalisation, exact observation moments, intrinsic reward, the
                                  env-axis reward filter, the distillation / intrinsic-value loss) and their *_cpu twins likewise: only
                                  added, the number stays at 2.7.1;
                                  PPG's auxiliary phase -- mi355ppo_ppg_* (the rollout gather, the old policy's normalised logits, the three
                                  heads with the joint loss and its backward), mi355ppo_clip_adam_split_f32 and their *_cpu twins likewise:
                                  only added, the number stays at 2.7.1;
                                  the LayerNorm NatureCNN of pqn_atari_envpool.py -- mi355ppo_layernorm_relu_* (+ workspace size, *_cpu twins) and the
                                  pre-activation forwards mi355ppo_cnn_conv1q_pre_fwd (+ twin), mi355ppo_cnn_conv_pre_packed_f16x2_f32,
                                  mi355ppo_fc_pre_packed_f16x2_f32 likewise: only added, the number stays at 2.7.1;
                                  the same network on one frame (pqn_atari_envpool_lstm.py) -- mi355ppo_cnn_conv1q1_pack (+ size, twin),
                                  mi355ppo_cnn_conv1q1_pre_fwd (+ twin), mi355ppo_cnn_conv1p1_wgrad_f16x2 (+ workspace size) likewise:
                                  only added, the number stays at 2.7.1;
                                  the plain ReLU network on one frame (ppo_atari_lstm.py) -- mi355ppo_cnn_conv1q1_fwd_bits, _fwd_amax and the
                                  twin mi355ppo_cnn_conv1q1_fwd_cpu likewise: only added, the number stays at 2.7.1;
                                  a binding must check major AND minor (cleanrl_amd/_lib.py does) */

#if defined(__GNUC__)
#define MI355PPO_API __attribute__((visibility("default")))
#else
#define MI355PPO_API
#endif

/* An "amax record": the bit pattern of max |x| of an f32 tensor, kept as 16 uint32 slots 64 bytes apart (1 KiB; the record's value is
 * the maximum over the slots).  The *_f16x2 entry points read the record of every tensor they split into two f16 terms (the tensor's
 * power-of-two scale derives from it) and fold the values they store into the record of the tensor they produce; the caller zeroes
 * records before their producers run (one memset for all records of a pass) -- see mi355ppo_absmax_f32 and csrc/f16split.h. */
#define MI355PPO_AMAX_WORDS 256

#define MI355PPO_OK 0
#define MI355PPO_EINVAL (-1)     /* null pointer, non-positive or unsupported shape            */
#define MI355PPO_EALIGN (-2)     /* a pointer is not aligned to its element size               */
#define MI355PPO_EHIP (-3)       /* a HIP runtime call / kernel launch failed                  */
#define MI355PPO_EWORKSPACE (-4) /* workspace NULL or smaller than *_workspace_bytes()         */
#define MI355PPO_ETIMEOUT (-5)   /* mi355ppo_dp_comm_status: a wait on a peer gave up          */

MI355PPO_API int mi355ppo_version(void);
MI355PPO_API const char* mi355ppo_last_error(void);
/* Capability check: 0 if `device` (a HIP device ordinal) can run this library's kernels (gfx950), MI355PPO_EHIP / EINVAL with a
 * message otherwise (no device, ordinal out of range, another architecture).  Optional -- the library keeps no per-device state
 * and every entry point works without it --; cleanrl_amd/_lib.py calls it once per device, so that a wrong GPU fails at load
 * time with a sentence instead of at the first launch with "invalid device function". */
MI355PPO_API int mi355ppo_init(int device);

/* ---------------------------------------------------------------------------------------------
 * K1  Generalised Advantage Estimation, fused reverse scan.
 * Replaces cleanrl/ppo_atari_multigpu.py:290-301 (== ppo.py:220-231, ppo_atari.py:237-248,
 * ppo_atari_envpool.py:252-263, ppo_continuous_action.py:235-246): ~10 elementwise torch kernels
 * per time step x T steps, plus `returns = advantages + values`.
 *   rewards, dones, values : (T,N) f32, time-major (N contiguous)      [in]
 *   next_done, next_value  : (N)   f32                                  [in]
 *   advantages, returns    : (T,N) f32                                  [out]
 * Bit-exact with the reference's f32 op order: ((g*nv)*nnt), ((r+.)-v), (((g*l)*nnt)*last), where
 * g*l is formed in double and then rounded to f32 (no FMA contraction).
 * `variant`: 0 = auto, 1 / 3 = column-streaming kernels (large N), 6 = staged-scan kernel (small N: off-chain math by all threads, chain
 * out of LDS) (tuning/testing; 2 / 4 / 5 -- round 1's single-scanner tile kernels -- were retired in ABI 2.1: MI355PPO_EINVAL).
 */
MI355PPO_API int mi355ppo_gae_f32(const float* rewards, const float* dones, const float* values,
                     const float* next_done, const float* next_value,
                     float* advantages, float* returns,
                     int T, int N, double gamma, double gae_lambda, void* stream);
MI355PPO_API int mi355ppo_gae_f32_variant(const float* rewards, const float* dones, const float* values,
                             const float* next_done, const float* next_value,
                             float* advantages, float* returns,
                             int T, int N, double gamma, double gae_lambda, int variant, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2  Categorical(logits): sample + log_prob + entropy in one launch.
 * Replaces Agent.get_action_and_value's distribution ops, cleanrl/ppo_atari_multigpu.py:156-159
 * (== ppo.py:122-126, ppo_atari_envpool.py:134-139): logits - logsumexp, softmax,
 * multinomial(probs,1) [= argmax(probs / Exp(1)) in ATen], gather, entropy.
 *   logits      : (B,A) f32                                             [in]
 *   noise_exp1  : (B,A) f32 Exponential(1) draws, or NULL               [in]
 *                 NULL => draws come from an internal Philox4x32-10 stream keyed by (seed, offset);
 *                 counter = row*A + column, so results do not depend on the launch geometry.
 *   action_i64  : (B) int64, may be NULL                                [out]
 *   action_f32  : (B) f32,   may be NULL  (the reference stores Discrete actions in an f32 rollout
 *                 tensor, ppo_atari_multigpu.py:236,265)                [out]
 *   logprob     : (B) f32                                               [out]
 *   entropy     : (B) f32, may be NULL                                  [out]
 */
MI355PPO_API int mi355ppo_categorical_sample_f32(const float* logits, const float* noise_exp1,
                                    uint64_t seed, uint64_t offset,
                                    int64_t* action_i64, float* action_f32,
                                    float* logprob, float* entropy,
                                    int B, int A, void* stream);
/* The same with the Philox stream position in device memory: offset_eff = offset + *offset_base (offset_base may be
 * NULL).  A launch captured into a hipGraph can then be replayed with a new position (the rollout-step graphs of
 * PPOLearner.capture_rollout advance the base once per rollout). */
MI355PPO_API int mi355ppo_categorical_sample_ctr_f32(const float* logits, const float* noise_exp1, uint64_t seed,
                                        uint64_t offset, const uint64_t* offset_base, int64_t* action_i64,
                                        float* action_f32, float* logprob, float* entropy, int B, int A, void* stream);

/* log_prob / entropy of GIVEN actions (the `action is not None` branch, :157-159).
 * Exactly one of action_i64 / action_f32 must be non-NULL. */
MI355PPO_API int mi355ppo_categorical_logprob_entropy_f32(const float* logits,
                                             const int64_t* action_i64, const float* action_f32,
                                             float* logprob, float* entropy,
                                             int B, int A, void* stream);

/* Backward of the two outputs above w.r.t. logits, for code that differentiates
 * Agent.get_action_and_value(x, action) itself (autograd of torch categorical.py log_prob/entropy):
 *   dlogits[b,j] = g_logprob[b]*(1[j==a_b] - p_bj) - g_entropy[b]*p_bj*(logp_bj + H_b).
 * g_logprob / g_entropy (B) may be NULL (= zeros). */
MI355PPO_API int mi355ppo_categorical_logprob_entropy_bwd_f32(const float* logits,
                                             const int64_t* action_i64, const float* action_f32,
                                             const float* g_logprob, const float* g_entropy,
                                             float* dlogits, int B, int A, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2' Normal(mean, exp(logstd)): sample + summed log_prob + summed entropy.
 * Replaces cleanrl/ppo_continuous_action.py:134-141.
 *   mean (B,D), logstd (D), noise_std_normal (B,D) or NULL (=> Philox + Box-Muller),
 *   action (B,D) out, logprob_sum (B) out, entropy_sum (B) out or NULL.
 * action = noise * exp(logstd) + mean (mul then add, as torch.normal); log_prob uses
 * log(exp(logstd)) for log_scale exactly as torch.distributions.Normal does.
 */
MI355PPO_API int mi355ppo_normal_sample_f32(const float* mean, const float* logstd, const float* noise_std_normal,
                               uint64_t seed, uint64_t offset,
                               float* action, float* logprob_sum, float* entropy_sum,
                               int B, int D, void* stream);
MI355PPO_API int mi355ppo_normal_logprob_entropy_f32(const float* mean, const float* logstd, const float* action,
                                        float* logprob_sum, float* entropy_sum,
                                        int B, int D, void* stream);

/* Backward of (logprob_sum, entropy_sum): dmean (B,D) and the per-row contributions to dlogstd
 * (B,D), which the caller sums over rows. */
MI355PPO_API int mi355ppo_normal_logprob_entropy_bwd_f32(const float* mean, const float* logstd, const float* action,
                                        const float* g_logprob, const float* g_entropy,
                                        float* dmean, float* dlogstd_rows, int B, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K3  Minibatch PPO loss, forward + backward fused (clipped surrogate + value loss + entropy).
 * Replaces cleanrl/ppo_atari_multigpu.py:320(b_actions.long()[mb_inds])-355 and the autograd
 * backward of those ops down to the network outputs (== ppo.py:250-285, ppo_atari.py:267-302,
 * ppo_atari_envpool.py:282-317).
 *   new_logits (M,A), new_value (M)        : network outputs for the minibatch rows  [in]
 *   mb_inds (M) int64 or NULL (= identity) : rows of the flat batch                  [in]
 *   b_actions_f32, b_logprobs, b_advantages, b_returns, b_values : (Bflat) f32       [in]
 *   scalars7 : loss, pg_loss, v_loss, entropy, old_approx_kl, approx_kl, clipfrac    [out, 7 f32]
 *   dlogits (M,A), dvalue (M) : d loss / d new_logits, d loss / d new_value          [out]
 *   adv_mean_den : NULL, or 2 f32 = (mean, unbiased std + 1e-8) of b_advantages[mb_inds] from
 *                  mi355ppo_adv_stats_f32 (then no statistics launch happens here)        [in]
 * Reductions are computed in a fixed order (deterministic); advantage mean / unbiased std are
 * accumulated in f64.  Tolerances vs the reference are stated in tests/test_gpu_kernels.py.
 * One row has no unbiased std: norm_adv with M == 1 and adv_mean_den == NULL is refused (MI355PPO_EINVAL, nothing
 * launched) by every loss entry point, the packed and the continuous-action ones and the *_cpu twins included; with a
 * caller-supplied adv_mean_den the call is valid.
 * Launches per call: statistics (only if norm_adv and adv_mean_den == NULL), row pass, scalar fold
 * (only if scalars7 != NULL).  scalars7 == NULL defers the fold: the call's partial sums stay in
 * its workspace, which then must be a slot no other call overwrites until
 * mi355ppo_loss_scalars_f32 has folded it (categorical family only).
 */
MI355PPO_API size_t mi355ppo_loss_workspace_bytes(int M, int D);
MI355PPO_API int mi355ppo_loss_categorical_fwd_bwd_f32(const float* new_logits, const float* new_value,
                                          const int64_t* mb_inds, const float* b_actions_f32,
                                          const float* b_logprobs, const float* b_advantages,
                                          const float* b_returns, const float* b_values,
                                          int M, int A,
                                          double clip_coef, double ent_coef, double vf_coef,
                                          int norm_adv, int clip_vloss, const float* adv_mean_den,
                                          float* scalars7, float* dlogits, float* dvalue,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* Deferred scalar fold: row j of scalars (nslots,7) <- the partial sums that a categorical call
 * with scalars7 == NULL left in the workspace at workspaces + j*slot_stride_bytes.  One launch for
 * all minibatches of an update (the scalars are diagnostics: nothing on the device waits for them). */
MI355PPO_API int mi355ppo_loss_scalars_f32(const void* workspaces, size_t slot_stride_bytes, int nslots,
                                           float* scalars, void* stream);

/* Advantage statistics of ALL minibatches of one epoch in one call / two launches (`mb_advantages.mean()`,
 * `mb_advantages.std() + 1e-8`, cleanrl/ppo_atari_multigpu.py:337-338): they depend only on the
 * epoch's permutation and the GAE output, not on anything the network produces, so the learner
 * computes them when it uploads the permutation and K3 runs without its statistics launch.
 *   inds (total) int64 or NULL (= identity); minibatch j = rows [j*M, min((j+1)*M, total));
 *   mean_den : (ceil(total / M), 2) f32                                                  [out]
 * A minibatch of ONE row (M == 1, or a ragged last minibatch of one row) gets (that row's advantage, NaN): the unbiased
 * variance is 0 / 0, as torch's `std()` of one element is NaN.  The statistics calls do not refuse it (the other rows
 * of the table are valid); a loss call that is handed such a row normalises with NaN. */
MI355PPO_API size_t mi355ppo_adv_stats_workspace_bytes(int64_t total, int M);
MI355PPO_API int mi355ppo_adv_stats_f32(const float* b_advantages, const int64_t* inds, int64_t total, int M,
                                        float* mean_den, void* workspace, size_t workspace_bytes, void* stream);

/* Packed behaviour rows (round 3): the five per-row behaviour scalars the loss gathers through mb_inds --
 * `b_actions.long()[mb_inds]`, `b_logprobs[mb_inds]`, `b_advantages[mb_inds]`, `b_returns[mb_inds]`, `b_values[mb_inds]`
 * (cleanrl/ppo_atari_multigpu.py:320-352) -- stored as ONE 32-byte row per flat batch index,
 *   pack[i] = {action (f32 storage), old log-prob, advantage, return, old value, 0, 0, 0},
 * so that a minibatch row costs one 32-byte gather instead of five 4-byte gathers from five arrays (five 128-byte lines
 * per row once the flat batch outgrows the caches).  mi355ppo_batch_pack_f32 builds the rows once per iteration, after
 * GAE; the *_packed_* entry points are the K3 calls above reading them: same arithmetic, bit-identical results.
 *   pack (B, 8) f32, 32-byte aligned.  The packed loss call takes its advantage statistics from the caller
 *   (adv_mean_den from mi355ppo_adv_stats_packed_f32) whenever norm_adv is set: one launch per minibatch. */
MI355PPO_API int mi355ppo_batch_pack_f32(const float* b_actions_f32, const float* b_logprobs, const float* b_advantages,
                                         const float* b_returns, const float* b_values, float* pack, int64_t B, void* stream);
MI355PPO_API int mi355ppo_adv_stats_packed_f32(const float* pack, const int64_t* inds, int64_t total, int M,
                                               float* mean_den, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_loss_categorical_packed_fwd_bwd_f32(const float* new_logits, const float* new_value,
                                          const int64_t* mb_inds, const float* pack, int M, int A,
                                          double clip_coef, double ent_coef, double vf_coef,
                                          int norm_adv, int clip_vloss, const float* adv_mean_den,
                                          float* scalars7, float* dlogits, float* dvalue,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* Continuous-action variant, cleanrl/ppo_continuous_action.py:265-300:
 *   new_mean (M,D), logstd (D), b_actions (Bflat,D) -> dmean (M,D), dlogstd (D), dvalue (M). */
MI355PPO_API int mi355ppo_loss_normal_fwd_bwd_f32(const float* new_mean, const float* logstd, const float* new_value,
                                     const int64_t* mb_inds, const float* b_actions,
                                     const float* b_logprobs, const float* b_advantages,
                                     const float* b_returns, const float* b_values,
                                     int M, int D,
                                     double clip_coef, double ent_coef, double vf_coef,
                                     int norm_adv, int clip_vloss, const float* adv_mean_den,
                                     float* scalars7, float* dmean, float* dlogstd, float* dvalue,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K5  Observation path: uint8 rollout storage -> f32 network input, gather + convert fused.
 * Replaces `b_obs[mb_inds]` followed by `x / 255.0` (cleanrl/ppo_atari_multigpu.py:320,154) and,
 * with inds == NULL, the per-step `x / 255.0` of :151,154.  The reference stores observations as
 * f32 (:235); uint8 storage is exact because frames are integers 0..255.
 *   src_u8 : (rows_total, row_bytes) u8;  inds : (rows) int64 or NULL;  dst_f32 : (rows, row_bytes)
 *   scale_255 != 0 => dst = (float)src / 255.0f, correctly rounded (bit-equal to torch's division);
 *   scale_255 == 0 => dst = (float)src.
 * row_bytes must be a multiple of 4; src rows must be 4-byte aligned, dst 16-byte aligned.
 */
MI355PPO_API int mi355ppo_obs_u8_to_f32(const uint8_t* src_u8, const int64_t* inds, float* dst_f32,
                           int64_t rows, int64_t row_bytes, int scale_255, void* stream);

/* Store-time relayout of incoming frames: channel-planar (rows, C, HW) uint8 -> pixel-interleaved
 * (rows, HW, C) uint8 ("NHWC").  Replaces nothing in the reference (it stores f32 NCHW, :235,258); it lets
 * the rollout buffer feed the conv stack channels-last so that no layout transposes run on f32 data.
 * C == 4 with HW % 4 == 0 (FrameStack(4) of 84x84) takes the coalesced register-transpose path. */
MI355PPO_API int mi355ppo_obs_nchw_to_nhwc_u8(const uint8_t* src, uint8_t* dst, int64_t rows, int C, int HW,
                                              void* stream);

/* FrameStack(4) delta store: dst_rows[r] = prev_rows[r] with channels 1..3 moved to 0..2 and channel 3 taken from
 * newest_planes[r] (rows, HW) -- the next observation of every env that was not reset, from ONE new plane.  Lets the
 * host send 1/4 of the frame bytes per step (envs flagged done send their full stack through
 * mi355ppo_obs_nchw_to_nhwc_u8).  prev_rows may equal dst_rows. */
MI355PPO_API int mi355ppo_obs_shift_append_u8_c4(const uint8_t* prev_rows, const uint8_t* newest_planes, uint8_t* dst_rows,
                                                 int64_t rows, int HW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * a8/a9  Flat-buffer optimiser step: (grad * grad_scale) -> global-norm clip -> Adam, fused.
 * Replaces the unpack-and-divide of cleanrl/ppo_atari_multigpu.py:368-374 (grad_scale =
 * 1/world_size), nn.utils.clip_grad_norm_ (:376) and optim.Adam(eps=1e-5).step() (:377) on a
 * persistent flat parameter/gradient buffer.
 *   params, grads, exp_avg, exp_avg_sq : (n) f32 ; grads is scaled+clipped in place
 *   step : 1-based Adam step count ; total_norm_out : (1) f32 pre-clip norm, may be NULL
 */
MI355PPO_API size_t mi355ppo_clip_adam_workspace_bytes(int64_t n);
MI355PPO_API int mi355ppo_clip_adam_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                           double grad_scale, double max_grad_norm, double lr,
                           double beta1, double beta2, double eps, int64_t step,
                           float* total_norm_out, void* workspace, size_t workspace_bytes, void* stream);

/* The two schedule-dependent constants of an Adam step, as the kernels consume them (HOST function, host pointer):
 * out2_host = {(float)(-(lr / (1 - beta1^step))), (float)sqrt(1 - beta2^step)}  (torch adam.py: step_size, bias_correction2_sqrt). */
MI355PPO_API int mi355ppo_adam_schedule_f32(double lr, double beta1, double beta2, int64_t step, float* out2_host);
/* mi355ppo_clip_adam_f32 with those two constants read from DEVICE memory (`sched2`, 2 floats the caller copied there): a launch
 * captured into a hipGraph is replayed with the next step's learning rate / bias corrections without re-capturing
 * (PPOLearner.capture_update).  Bit-identical to mi355ppo_clip_adam_f32 for the same (lr, step). */
MI355PPO_API int mi355ppo_clip_adam_sched_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                              double grad_scale, double max_grad_norm, double beta1, double beta2, double eps,
                                              const float* sched2, float* total_norm_out, void* workspace, size_t workspace_bytes,
                                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * a9/e  The data-parallel gradient exchange over peer memory (csrc/dpcomm.hip): all_reduce(SUM) of the persistent flat gradient
 * buffer across the ranks of ONE node without a collective library -- replaces dist.all_reduce(all_grads_list, op=SUM) of
 * cleanrl/ppo_atari_multigpu.py:360-367 (the division by world_size of :368-374 stays grad_scale of mi355ppo_clip_adam_*).
 * Every rank owns one device segment which its peers map through HIP IPC (xGMI between GPUs); a call is five small launches on
 * `stream` -- publish, reduce slice `rank` of every rank's copy in rank order and push it to every rank, collect -- synchronised by
 * flags in the segments.  No host round trip, no second stream: legal inside a hipGraph capture (the round counter lives on the
 * device).  Every element is summed by one rank in one fixed order: all ranks receive the same bits.
 *
 * The communicator is the ONE object of this header that owns memory, so the conventions at the top hold for
 * mi355ppo_dp_allreduce_sum_f32 only; create / handle / connect / destroy are set-up calls (they allocate, synchronise the device
 * and must not run during a capture).  Set-up, on every rank, with the current HIP device = the rank's GPU:
 *   mi355ppo_dp_comm_create(world, rank, max_floats, timeout_ms, &comm)     world <= MI355PPO_DP_MAX_WORLD
 *   mi355ppo_dp_comm_handle(comm, handle)                                    MI355PPO_DP_HANDLE_BYTES bytes to send to every rank
 *   ... the ranks exchange their handles (any host channel: the reference's process group, a file, a pipe) ...
 *   mi355ppo_dp_comm_connect(comm, handles)                                  world x MI355PPO_DP_HANDLE_BYTES, in rank order
 *   ... a host barrier: every rank has connected before the first exchange ...
 * Every rank must then issue the same sequence of mi355ppo_dp_allreduce_sum_f32 calls (same n).  grads: (n) f32, 16-byte aligned,
 * n <= max_floats; summed in place.  A wait on a peer gives up after timeout_ms (the peer died or skipped a call): the round, the
 * peer and the phase (1 = reduce, 2 = collect) are recorded, every later wait of this communicator returns at once, and
 * mi355ppo_dp_comm_status -- a HOST read, no synchronisation -- returns MI355PPO_ETIMEOUT from then on; grads then hold garbage and
 * the communicator must be destroyed.  Ranks are processes: one communicator per process and rank. */
#define MI355PPO_DP_MAX_WORLD 8
#define MI355PPO_DP_HANDLE_BYTES 64
typedef struct mi355ppo_dp_comm mi355ppo_dp_comm;
MI355PPO_API int mi355ppo_dp_comm_create(int world, int rank, int64_t max_floats, double timeout_ms, mi355ppo_dp_comm** comm_out);
MI355PPO_API int mi355ppo_dp_comm_handle(mi355ppo_dp_comm* comm, unsigned char* handle_out);
MI355PPO_API int mi355ppo_dp_comm_connect(mi355ppo_dp_comm* comm, const unsigned char* handles);
MI355PPO_API int mi355ppo_dp_allreduce_sum_f32(mi355ppo_dp_comm* comm, float* grads, int64_t n, void* stream);
MI355PPO_API int mi355ppo_dp_comm_status(mi355ppo_dp_comm* comm, int* round_out, int* peer_out, int* phase_out);   /* outputs may be NULL */
MI355PPO_API int mi355ppo_dp_comm_destroy(mi355ppo_dp_comm* comm);

/* ---------------------------------------------------------------------------------------------
 * K7  The reference's MLP agents (two independent 64-64 tanh networks: actor and critic) as one kernel family (csrc/mlp.hip).
 * Agents: cleanrl/ppo.py:100-126 (Categorical head), cleanrl/ppo_continuous_action.py:112-141 (Normal head with the
 * state-independent actor_logstd).  A network is passed as a HOST array of six DEVICE pointers in torch's own layouts:
 *   {W1 (64, O), b1 (64), W2 (64, 64), b2 (64), W3 (n_out, 64), b3 (n_out)}   (nn.Linear.weight is (out, in))
 * obs_dim O <= 512 and n_out <= 20 (ABI 2.1; CartPole 4 / 2, HalfCheetah 17 / 6, Ant 27 / 8, Humanoid 376 / 17 ...): beyond that the entry points
 * return MI355PPO_EINVAL and the caller keeps the networks on library GEMMs.  Up to O = 32 and n_out = 8 a lane keeps its row of W1 in registers;
 * wider shapes run the WIDE kernels (layer 1 and its weight gradient walk the observation in chunks of 32 columns, blocks of <= 32 rows).
 *
 * mi355ppo_mlp_fwd_f32: both forwards -- actor_out (B, n_out) = logits or mean, value (B) -- e.g. the bootstrap value of
 *   ppo.py:218-219.
 * mi355ppo_mlp_act_*: the rollout step of Agent.get_action_and_value(next_obs) (ppo.py:205-210,
 *   ppo_continuous_action.py:221-226): both forwards + K2 / K2' (same Philox streams as mi355ppo_categorical_sample_ctr_f32 /
 *   mi355ppo_normal_sample_f32: counter = row * ceil(n_out / 4) + column / 4; offset_eff = offset + *offset_base) in ONE launch.
 *   logits_out / mean_out / entropy may be NULL.
 * mi355ppo_mlp_ppo_*_fwd_bwd_f32: one minibatch of the update (ppo.py:250-287 / ppo_continuous_action.py:265-302 up to and
 *   including loss.backward()): gather b_obs[mb_inds], both forwards, the distribution, the PPO loss terms of K3 (same row
 *   function), both backward passes; the parameter gradients are ADDED to `actor_grads` / `critic_grads` (host arrays of six
 *   device pointers, layouts as the parameters; `dlogstd` (D) likewise), the seven scalars of K3 written to scalars7.
 *   norm_adv needs adv_mean_den (mi355ppo_adv_stats_f32).  mean_shift (M, D) or NULL is added to the mean before the loss
 *   (rpo_continuous_action.py:138-142).  rows_per_block: 0 = auto.  Two launches; deterministic (fixed-order f64 folds).
 */
MI355PPO_API int mi355ppo_mlp_fwd_f32(const float* obs, int B, int O, const void* const* actor, const void* const* critic, int n_out,
                                      float* actor_out, float* value, void* stream);
MI355PPO_API int mi355ppo_mlp_act_categorical_f32(const float* obs, int B, int O, const void* const* actor, const void* const* critic,
                                                  int A, const float* noise_exp1, uint64_t seed, uint64_t offset,
                                                  const uint64_t* offset_base, int64_t* action_i64, float* action_f32, float* logprob,
                                                  float* entropy, float* value, float* logits_out, void* stream);
MI355PPO_API int mi355ppo_mlp_act_normal_f32(const float* obs, int B, int O, const void* const* actor_mean, const void* const* critic,
                                             const float* logstd, int D, const float* noise_std_normal, uint64_t seed, uint64_t offset,
                                             const uint64_t* offset_base, float* action, float* logprob_sum, float* entropy_sum,
                                             float* value, float* mean_out, void* stream);
MI355PPO_API size_t mi355ppo_mlp_ppo_workspace_bytes(int M, int O, int n_out, int rows_per_block);
MI355PPO_API int mi355ppo_mlp_ppo_categorical_fwd_bwd_f32(
    const float* b_obs, const int64_t* mb_inds, int M, int O, const void* const* actor, const void* const* critic, int A,
    const float* b_actions_f32, const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values,
    double clip_coef, double ent_coef, double vf_coef, int norm_adv, int clip_vloss, const float* adv_mean_den, void* const* actor_grads,
    void* const* critic_grads, float* scalars7, int rows_per_block, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_mlp_ppo_normal_fwd_bwd_f32(
    const float* b_obs, const int64_t* mb_inds, int M, int O, const void* const* actor_mean, const void* const* critic, const float* logstd,
    int D, const float* mean_shift, const float* b_actions, const float* b_logprobs, const float* b_advantages, const float* b_returns,
    const float* b_values, double clip_coef, double ent_coef, double vf_coef, int norm_adv, int clip_vloss, const float* adv_mean_den,
    void* const* actor_grads, void* const* critic_grads, float* dlogstd, float* scalars7, int rows_per_block, void* workspace,
    size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LSTM  The recurrence of ppo_atari_lstm.py's get_states (cleanrl/ppo_atari_lstm.py:140-158): one layer of nn.LSTM(512, 128)
 * run over T time-major steps of B envs, the state multiplied by keep_t = 1 - done[t] before step t (a multiply: a non-binary
 * done scales the state as the reference's does).  Replaces T x (two masking multiplies + a length-1 nn.LSTM call) and, in the
 * update, the backward through T per-step autograd graphs.  Gate order i, f, g, o; H must be 128.  Math: csrc/lstm_rows.h.
 *   gx        : (T,B,4H) f32  x W_ih^T + b_ih + b_hh, formed by the caller                      [in]
 *   w_hh      : (4H,H)   f32  nn.LSTM's weight_hh_l0 (row-major, any 4-byte offset)             [in]
 *   h0, c0    : (B,H)    f32  state before step 0                                              [in]
 *   done      : (T,B)    f32                                                                   [in]
 *   h         : (T,B,H)  f32  h_t                                                              [out]
 *   hT, cT    : (B,H)    f32  h_{T-1}, c_{T-1} (not masked: the state the reference returns)   [out]
 *   record    : 7 T B H  f32 activation record for the backward, or NULL (inference: the rollout step and the bootstrap
 *               value).  Planes: post-activation gates (T,B,4,H) | c_t (T,B,H) | hk_t = keep_t h_{t-1} (T,B,H) |
 *               ck_t = keep_t c_{t-1} (T,B,H)                                                  [out]
 * One workgroup walks one env's chain in a fixed order: deterministic, and env b's results do not depend on B or on b.
 */
MI355PPO_API int mi355ppo_lstm_seq_fwd_f32(const float* gx, const float* w_hh, const float* h0, const float* c0, const float* done,
                                           float* h, float* hT, float* cT, float* record, int T, int B, int H, void* stream);
/* Backward through the scan (BPTT):
 *   dh        : (T,B,H)  d loss / d h_t from the heads                                         [in]
 *   dhT, dcT  : (B,H)    d loss / d (hT, cT), or NULL (= zeros)                                [in]
 *   record    : as written by the forward of the same inputs                                   [in]
 *   dgx       : (T,B,4H) d loss / d pre-activation gates (= d gx)                               [out]
 *   dh0, dc0  : (B,H)    d loss / d (h0, c0), or NULL                                          [out]
 * The dense products stay with the caller: dW_hh = dgx^T hk (the record's hk plane), dW_ih = dgx^T x, dx = dgx W_ih,
 * d b_ih = d b_hh = column sums of dgx. */
MI355PPO_API int mi355ppo_lstm_seq_bwd_f32(const float* dh, const float* dhT, const float* dcT, const float* record,
                                           const float* w_hh, const float* done, float* dgx, float* dh0, float* dc0, int T, int B,
                                           int H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * TRXL  The episodic-memory attention core of ppo_trxl.py (cleanrl/ppo_trxl/ppo_trxl.py: batched_index_select of the
 * window, Transformer.forward's positional encoding, TransformerLayer.forward's norm_kv, MultiHeadAttention.forward's keys,
 * masked softmax and weighted sum) for one layer, reassociated so that no matrix is applied per row.  Per sample b, window
 * row j < L and head h (d = D / H):
 *   y_j  = LayerNorm(mem[ep[b], rows[b,j], layer, :] + pe[pos[b,j]])   (eps 1e-5, biased variance; no pe term if pe == NULL)
 *   s_j  = (mask[b,j] ? q[b,h] . y_j,h : -1e20) / sqrt(D)             (q = q~ = W_k^T q_h: the caller's `q @ keys.weight`)
 *   u[b,h] = sum_j softmax(s)_j y_j,h                                  (the caller applies `values` and `fc_out` to u)
 * A fully masked window is a uniform softmax over its L rows, as in the reference (the fill precedes the scale).
 *   memory     : (E, T_ep, layers, D) f32, the episode pool                                   [in]
 *   ep         : (B) int64 episode of each sample;  rows, pos : (B, L) int64 window rows / pe rows  [in]
 *   mask       : (B, L) uint8;  pe : (P, D) f32 or NULL;  gamma, beta : (D) f32 of norm_kv   [in]
 *   q          : (B, H, d) f32                                                                [in]
 *   u          : (B, H, d) f32;  stats : (B, H, 2) f32 softmax max and sum, for the backward  [out]
 *   err        : int32 error word or NULL: an index outside [0, E) / [0, T_ep) / [0, P) is clamped (never read out of bounds)
 *                and 1 is stored to *err; the caller zeroes it before and reads it after       [out]
 * Shapes: D % 64 == 0, D <= 512, H divides 64, 1 <= L <= 1024 (else MI355PPO_EINVAL).  One workgroup per sample folds every
 * sum in a fixed order: deterministic, and sample b's bits do not depend on B or on b.  Math: csrc/trxl_rows.h.
 */
MI355PPO_API int mi355ppo_trxl_attn_fwd_f32(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                            const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe, int P,
                                            const float* gamma, const float* beta, const float* q, float* u, float* stats, int* err,
                                            int B, int L, int D, int H, void* stream);
/* Backward, re-streaming the window with the forward's u and stats:
 *   du         : (B, H, d) f32 d loss / d u                                                   [in]
 *   dq         : (B, H, d) f32 d loss / d q                                                   [out]
 *   dln_rows   : (2, B, D) f32 per-sample d gamma and d beta rows (caller scratch, also a result) [out]
 *   dgamma, dbeta : (D) f32 the rows folded over b in a fixed order (no atomics)               [out]
 * No gradient reaches the memory: the reference stores detached layer inputs. */
MI355PPO_API int mi355ppo_trxl_attn_bwd_f32(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                            const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe, int P,
                                            const float* gamma, const float* beta, const float* q, const float* u, const float* stats,
                                            const float* du, float* dq, float* dln_rows, float* dgamma, float* dbeta, int* err, int B,
                                            int L, int D, int H, void* stream);

/* ---------------------------------------------------------------------------------------------
 * IMPALA  The IMPALA-CNN trunk of ppo_procgen.py / ppg_procgen.py (cleanrl/ppo_procgen.py:86-124, cleanrl/ppg_procgen.py:123-165):
 * 3 x [conv3x3 -> max_pool2d(3, 2, 1) -> 2 residual blocks], channels [16, 32, 32], on 64x64x3 frames; the Flatten -> ReLU ->
 * Linear tail stays with the caller.  Activations are channels-last f32 (B, H, W, C): x is the frames as K5
 * (mi355ppo_obs_u8_to_f32) writes them, y the (B, 8, 8, 32) output -- NCHW order is y.permute(0, 3, 1, 2).  Exact f32 on
 * v_mfma_f32_16x16x4_f32; orders, tie rule and layouts: csrc/impala_rows.h.
 *   params    : host array of 30 pointers, the trunk's conv weights (C_out, C_in, 3, 3) and biases in state_dict order
 *               (network.0.conv.weight, network.0.conv.bias, network.0.res_block0.conv0.weight, ...), any 4-byte offset  [in]
 *   saved     : mi355ppo_impala_saved_floats(B) f32, the activations the backward reads (16-byte aligned)      [out / in]
 *   argmax    : mi355ppo_impala_argmax_bytes(B) bytes, the pools' window-relative argmax                        [out / in]
 *   workspace : mi355ppo_impala_workspace_bytes(B, backward) bytes, 256-byte aligned (packed weights, scratch planes,
 *               weight-gradient partials)
 * Only B > 0, H = W = 64, C = 3 and channels (ch0, ch1, ch2) = (16, 32, 32); anything else returns MI355PPO_EINVAL before
 * any launch, with the outputs untouched.  The backward writes all 30 parameter gradients (grads: host array of 30 device
 * pointers, written, not accumulated) and no input gradient.  Deterministic (weight gradients: fixed-order partials and a
 * fixed-order fold, no atomics); forward results of one image do not depend on the batch.  No host synchronisation and no
 * allocation: capturable.
 */
MI355PPO_API int64_t mi355ppo_impala_saved_floats(int B);
MI355PPO_API int64_t mi355ppo_impala_argmax_bytes(int B);
MI355PPO_API size_t mi355ppo_impala_workspace_bytes(int B, int backward);
MI355PPO_API int mi355ppo_impala_fwd_f32(const float* x, const float* const* params, float* y, float* saved, uint8_t* argmax, int B,
                                         int H, int W, int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes,
                                         void* stream);
MI355PPO_API int mi355ppo_impala_bwd_f32(const float* x, const float* const* params, const float* saved, const uint8_t* argmax,
                                         const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1, int ch2,
                                         void* workspace, size_t workspace_bytes, void* stream);
/* The same trunk on Atari frame stacks (the student of qdagger_dqn_atari_impalacnn.py:164-184): x is (B, 84, 84, 4) u8
 * channels-last rows as mi355ppo_replay_gather_u8 writes them, read by layer 0 as byte / 255.0f (no f32 copy of the frames is
 * made, no gradient for them); planes 84 -> 42 -> 21 -> 11 (the pool's (h + 1) / 2), y (B, 11, 11, 32).  Same kernels, orders and
 * tie rule as the 64x64x3 family on ragged bands (csrc/impala_rows.h); sizes from the mi355ppo_impala84_* functions.  Only
 * B > 0, H = W = 84, C = 4 and channels (16, 32, 32); anything else returns MI355PPO_EINVAL before any launch. */
MI355PPO_API int64_t mi355ppo_impala84_saved_floats(int B);
MI355PPO_API int64_t mi355ppo_impala84_argmax_bytes(int B);
MI355PPO_API size_t mi355ppo_impala84_workspace_bytes(int B, int backward);
MI355PPO_API int mi355ppo_impala84_fwd_u8(const uint8_t* x, const float* const* params, float* y, float* saved, uint8_t* argmax, int B,
                                          int H, int W, int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes,
                                          void* stream);
MI355PPO_API int mi355ppo_impala84_bwd_u8(const uint8_t* x, const float* const* params, const float* saved, const uint8_t* argmax,
                                          const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1, int ch2,
                                          void* workspace, size_t workspace_bytes, void* stream);
/* The trunks' max pool alone (channels-last; only their shapes: 64x64x16, 32x32x32, 16x16x32 and 84x84x16, 42x42x32, 21x21x32):
 * y (B, (H+1)/2, (W+1)/2, C) and the argmax byte per output; the backward writes dx (B, H, W, C) from dy and the argmax. */
MI355PPO_API int mi355ppo_impala_maxpool_fwd_f32(const float* x, float* y, uint8_t* argmax, int B, int H, int W, int C, void* stream);
MI355PPO_API int mi355ppo_impala_maxpool_bwd_f32(const float* dy, const uint8_t* argmax, float* dx, int B, int H, int W, int C,
                                                 void* stream);

/* ---------------------------------------------------------------------------------------------
 * Host-pointer twins (csrc/host_twins.hip) of the PPO-path entry points above: the same arguments minus `stream` and
 * `workspace`, every pointer a HOST pointer, the call returns when the result is written.  Same math by construction: the
 * row / element functions (GAE step, Categorical row, loss row terms, advantage statistics fold, Adam element, Philox stream)
 * are the device kernels' own, compiled for the host from the same headers (csrc/ppo_rows.h, catrow.h, common.h) without FMA
 * contraction; results differ from the device's only by libm vs the device math library (expf / logf: a few ulp) and by the
 * order of the f64 reductions (row order here).  Serial.  They serve BASELINE config A -- cleanrl/ppo.py on CPU (`--no-cuda`:
 * CartPole, num_envs = 4) -- and the world_size-2 gloo tests through cleanrl_amd/host_ops.py.  They are NOT a fallback: nothing
 * routes a device pointer here, and a CUDA device without the HIP kernels raises (cleanrl_amd/_lib.py).
 * Reference lines: as for the device entry point of the same name.
 */
MI355PPO_API int mi355ppo_gae_f32_cpu(const float* rewards, const float* dones, const float* values, const float* next_done,
                                      const float* next_value, float* advantages, float* returns, int T, int N, double gamma,
                                      double gae_lambda);
MI355PPO_API int mi355ppo_categorical_sample_f32_cpu(const float* logits, const float* noise_exp1, uint64_t seed, uint64_t offset,
                                                     int64_t* action_i64, float* action_f32, float* logprob, float* entropy,
                                                     int B, int A);
MI355PPO_API int mi355ppo_categorical_logprob_entropy_f32_cpu(const float* logits, const int64_t* action_i64,
                                                              const float* action_f32, float* logprob, float* entropy, int B,
                                                              int A);
MI355PPO_API int mi355ppo_categorical_logprob_entropy_bwd_f32_cpu(const float* logits, const int64_t* action_i64,
                                                                  const float* action_f32, const float* g_logprob,
                                                                  const float* g_entropy, float* dlogits, int B, int A);
MI355PPO_API int mi355ppo_normal_sample_f32_cpu(const float* mean, const float* logstd, const float* noise_std_normal, uint64_t seed,
                                                uint64_t offset, float* action, float* logprob_sum, float* entropy_sum, int B,
                                                int D);
MI355PPO_API int mi355ppo_normal_logprob_entropy_f32_cpu(const float* mean, const float* logstd, const float* action,
                                                         float* logprob_sum, float* entropy_sum, int B, int D);
MI355PPO_API int mi355ppo_normal_logprob_entropy_bwd_f32_cpu(const float* mean, const float* logstd, const float* action,
                                                             const float* g_logprob, const float* g_entropy, float* dmean,
                                                             float* dlogstd_rows, int B, int D);
MI355PPO_API int mi355ppo_loss_categorical_fwd_bwd_f32_cpu(const float* new_logits, const float* new_value, const int64_t* mb_inds,
                                                           const float* b_actions_f32, const float* b_logprobs,
                                                           const float* b_advantages, const float* b_returns, const float* b_values,
                                                           int M, int A, double clip_coef, double ent_coef, double vf_coef,
                                                           int norm_adv, int clip_vloss, const float* adv_mean_den, float* scalars7,
                                                           float* dlogits, float* dvalue);
MI355PPO_API int mi355ppo_loss_normal_fwd_bwd_f32_cpu(const float* new_mean, const float* logstd, const float* new_value,
                                                      const int64_t* mb_inds, const float* b_actions, const float* b_logprobs,
                                                      const float* b_advantages, const float* b_returns, const float* b_values,
                                                      int M, int D, double clip_coef, double ent_coef, double vf_coef, int norm_adv,
                                                      int clip_vloss, const float* adv_mean_den, float* scalars7, float* dmean,
                                                      float* dlogstd, float* dvalue);
MI355PPO_API int mi355ppo_clip_adam_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                            double grad_scale, double max_grad_norm, double lr, double beta1, double beta2,
                                            double eps, int64_t step, float* total_norm_out);
MI355PPO_API int mi355ppo_obs_u8_to_f32_cpu(const uint8_t* src_u8, const int64_t* inds, float* dst_f32, int64_t rows,
                                            int64_t row_bytes, int scale_255);
MI355PPO_API int mi355ppo_lstm_seq_fwd_f32_cpu(const float* gx, const float* w_hh, const float* h0, const float* c0,
                                               const float* done, float* h, float* hT, float* cT, float* record, int T, int B,
                                               int H);
MI355PPO_API int mi355ppo_lstm_seq_bwd_f32_cpu(const float* dh, const float* dhT, const float* dcT, const float* record,
                                               const float* w_hh, const float* done, float* dgx, float* dh0, float* dc0, int T,
                                               int B, int H);
/* The TrXL twins refuse (MI355PPO_EINVAL) an out-of-range ep / rows / pos instead of clamping it. */
MI355PPO_API int mi355ppo_trxl_attn_fwd_f32_cpu(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe, int P,
                                                const float* gamma, const float* beta, const float* q, float* u, float* stats, int B,
                                                int L, int D, int H);
MI355PPO_API int mi355ppo_trxl_attn_bwd_f32_cpu(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe, int P,
                                                const float* gamma, const float* beta, const float* q, const float* u,
                                                const float* stats, const float* du, float* dq, float* dln_rows, float* dgamma,
                                                float* dbeta, int B, int L, int D, int H);
MI355PPO_API int mi355ppo_impala_fwd_f32_cpu(const float* x, const float* const* params, float* y, float* saved, uint8_t* argmax,
                                             int B, int H, int W, int C, int ch0, int ch1, int ch2);
MI355PPO_API int mi355ppo_impala_bwd_f32_cpu(const float* x, const float* const* params, const float* saved, const uint8_t* argmax,
                                             const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1,
                                             int ch2);
MI355PPO_API int mi355ppo_impala84_fwd_u8_cpu(const uint8_t* x, const float* const* params, float* y, float* saved, uint8_t* argmax,
                                              int B, int H, int W, int C, int ch0, int ch1, int ch2);
MI355PPO_API int mi355ppo_impala84_bwd_u8_cpu(const uint8_t* x, const float* const* params, const float* saved, const uint8_t* argmax,
                                              const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1,
                                              int ch2);
MI355PPO_API int mi355ppo_impala_maxpool_fwd_f32_cpu(const float* x, float* y, uint8_t* argmax, int B, int H, int W, int C);
MI355PPO_API int mi355ppo_impala_maxpool_bwd_f32_cpu(const float* dy, const uint8_t* argmax, float* dx, int B, int H, int W, int C);

/* ---------------------------------------------------------------------------------------------
 * FC   Linear(3136, 512) + ReLU of the NatureCNN (cleanrl/ppo_atari_multigpu.py:144-145) on the bf16 matrix pipe
 * (kernel Z, csrc/gemmz.hip): every f32 operand is split into three bf16 terms that sum to it exactly, so products of terms
 * are exact in f32 and bf16 MFMAs with f32 accumulation do the work of f32 MFMAs in a fraction of their matrix-pipe time.
 * The six largest of the nine term pairs are multiplied (MI355PPO_BF16_PAIRS=9: all nine, every f32 product exact); the
 * three dropped pairs are together below the rounding of one f32 multiply.  The weight matrix is split AHEAD (once per
 * optimizer step) into MFMA fragment order (`pack`); the activations are loaded coalesced, transposed through wave-private
 * LDS and split in registers.  (The first generation -- lane = row gathers of both operands, round 2's kernel X -- kept the
 * vector-memory front end 83 % busy and the matrix pipe 37 % busy: profiles/r03_pmc_busy_kernels_x_c.csv.)
 *   pack  : B (N,K) f32 with leading dimension ldb -> mi355ppo_fc_pack_bytes(N, K) bytes, 16-byte aligned
 *   fwd   : h (M,N) = relu(a (M,K; lda) @ B^T + bias)         pack = pack(W  (N = 512,  K = 3136))
 *   dgrad : da (M,N) = (dz (M,K; lddz) @ B^T) * (act_in > 0)  pack = pack(Wt (N = 3136, K = 512)): the ReLU backward of the
 *           layer that produced act_in (conv3) is applied where the gradient is produced
 * All matrices row-major; h / da / act_in dense.  K % 16 == 0; a / dz 16-byte aligned with leading dimensions that are
 * multiples of 4 floats, below 4 GiB in all. */
MI355PPO_API size_t mi355ppo_fc_pack_bytes(int N, int K);
MI355PPO_API int mi355ppo_fc_pack_f32(const float* B, int ldb, int N, int K, void* pack, void* stream);
MI355PPO_API int mi355ppo_fc_fwd_relu_packed_f32(const float* a, int lda, const void* pack, const float* bias, float* h,
                                                 int M, int N, int K, void* stream);
MI355PPO_API int mi355ppo_fc_dgrad_mask_packed_f32(const float* dz, int lddz, const void* pack, const float* act_in, float* da,
                                                   int M, int N, int K, void* stream);
/* Forward for rollout-sized and small minibatches (M < 8192: a rollout step's 1,024 envs, config B's 4,096-row minibatch).  M / 64 x N / 64 wave tiles alone cannot fill the chip,
 * so K is split over the grid: raw f32 partials go to `ws` (mi355ppo_fc_fwd_workspace_bytes(M, N, K) bytes, 16-byte aligned; 0 bytes =
 * no split needed), one more pass adds them in a fixed order, then bias and ReLU -- Agent.network[7:9] of the rollout's policy forward
 * (cleanrl/ppo_atari_multigpu.py:144-145,262-264) without a library GEMM.  With ws = NULL: mi355ppo_fc_fwd_relu_packed_f32. */
MI355PPO_API size_t mi355ppo_fc_fwd_workspace_bytes(int M, int N, int K);
MI355PPO_API int mi355ppo_fc_fwd_relu_packed_ws_f32(const float* a, int lda, const void* pack, const float* bias, float* h,
                                                    int M, int N, int K, void* ws, size_t ws_bytes, void* stream);

/* The same kernel family on the convolutions of layers 2 and 3 (cleanrl/ppo_atari_multigpu.py:139-142): a row of the GEMM is an
 * output pixel (forward) or a pixel of the data gradient's grid, a k-step 64 contiguous bytes of a tap row of its window
 * (channels-last activations; zero padding through the buffer range check).  `pack` = mi355ppo_fc_pack_f32 of the layer's
 * (N, K) f32 matrix from mi355ppo_cnn_repack_weights_f32 -- mode 0 (forward: N = 64, K = 512 / 576), mode 1 (layer-3 data
 * gradient: N = 64, K = 576), mode 2 (layer-2 data gradient: N = 128 = 4 stride-parity classes x 32 channels, K = 256).
 *   fwd  : dst (images, Hout, Hout, 64) = relu(conv(src (images, Hin, Hin, Cin)) + bias)
 *   dgrad: dsrc (images, Hin, Hin, Cin) = conv_transpose(dz (images, Hout, Hout, 64)) * (act_in > 0)
 * Tensors channels-last f32, 16-byte aligned, sources below 4 GiB. */
MI355PPO_API int mi355ppo_cnn_conv_fwd_packed_f32(const float* src, const void* pack, const float* bias, float* dst,
                                                  int64_t images, int layer, void* stream);
MI355PPO_API int mi355ppo_cnn_conv_dgrad_packed_f32(const float* dz, const void* pack, const float* act_in, float* dsrc,
                                                    int64_t images, int layer, void* stream);

/* ReLU masks as bits.  The data gradients read the forward activation of the layer below only for its sign -- the reference's
 * autograd keeps the whole f32 tensor for `threshold_backward` (cleanrl/ppo_atari_multigpu.py:137-145: nn.ReLU after every layer).
 * The *_bits forwards write, beside the f32 activation, ONE BIT per element: word w, bit b <-> element 32 w + b of the flat
 * channels-last tensor, set where the activation is > 0 (numel / 32 uint32 words: 400 / 162 / 98 per image for a1 / a2 / a3);
 * the *_bits / maskbits data gradients take those words instead of `act_in` -- 1/32 of the mask bytes, identical results.
 *   conv1q_fwd_bits            : kernel Q (layer 1), also a1's mask       -> conv_dgrad_packed_bits(layer 2)
 *   conv_fwd_packed_bits(2, 3) : kernel Z forward, also a2's / a3's mask  -> conv_dgrad_packed_bits(layer 3) / fc_dgrad_maskbits
 * dst / dsrc / da must sit on a 128-byte boundary (a 32-element tile of the tensor = one word). */
MI355PPO_API int mi355ppo_cnn_conv1q_fwd_bits(const void* src_u8, const int64_t* inds, const void* pack, const float* bias,
                                              float* dst, uint32_t* mask_bits, int64_t images, void* stream);
MI355PPO_API int mi355ppo_cnn_conv_fwd_packed_bits_f32(const float* src, const void* pack, const float* bias, float* dst,
                                                       uint32_t* mask_bits, int64_t images, int layer, void* stream);
MI355PPO_API int mi355ppo_cnn_conv_dgrad_packed_bits_f32(const float* dz, const void* pack, const uint32_t* mask_bits, float* dsrc,
                                                         int64_t images, int layer, void* stream);
MI355PPO_API int mi355ppo_fc_dgrad_maskbits_packed_f32(const float* dz, int lddz, const void* pack, const uint32_t* mask_bits,
                                                       float* da, int M, int N, int K, void* stream);

/* FC weight gradient (csrc/fcw.hip): dW (N,K) = dz (M,N)^T @ a (M,K), the batch cut into slabs whose partials are added in a
 * fixed order (deterministic).  Kernel W (bf16 pipe, both operands transposed through LDS and split in registers) when
 * N == 512, K % 64 == 0, M % 16 == 0 and M >= 1024; kernel Y (f32 matrix pipe) otherwise.  dz takes a leading dimension (even); a is dense.  N % 64 == 0,
 * K % 224 == 0 (whole 64 x 224 wave tiles: 512 x 3136 = 8 x 14 of them); dz 8-byte, a and the workspace 16-byte aligned.
 * hwc_channels = C > 0: the columns of a are features in (h, w, c) order with C channels (the trunk's layout) and dW is
 * written in the reference's (c, h, w) order, i.e. directly as the gradient of Linear(3136,512).weight; 0: as computed. */
MI355PPO_API size_t mi355ppo_fc_wgrad_workspace_bytes(int M, int N, int K);
MI355PPO_API int mi355ppo_fc_wgrad_kernel(int M, int N, int K);      /* 'W' or 'Y': the kernel a call of this shape runs (profiling aid) */
/* 'H', 'W' or 'Y': the kernel mi355ppo_fc_wgrad_f16x2_f32 runs for this shape with a dense dz (ABI 1.9).  Kernel H (csrc/gemmh.hip, round 6)
 * streams both operands through a workgroup-wide LDS ring, split once, fragments by LDS transpose reads; from 4,096 rows on. */
MI355PPO_API int mi355ppo_fc_wgrad_kernel_f16x2(int M, int N, int K);
MI355PPO_API int mi355ppo_fc_wgrad_f32(const float* dz, int lddz, const float* a, float* dW, int M, int N, int K, int hwc_channels,
                                       void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * CNN  NatureCNN convolution stack (Agent.network convs, cleanrl/ppo_atari_multigpu.py:136-142) as
 * f32-MFMA implicit GEMMs on channels-last tensors: forward with fused uint8 gather + /255 + bias +
 * ReLU, data gradient with the ReLU-backward mask fused, weight + bias gradient.  f32 in, f32
 * accumulate (v_mfma_f32_32x32x2_f32): same precision class as the reference's f32 convolutions;
 * results differ from a CPU/MIOpen convolution only by summation order (tolerance in
 * tests/test_gpu_cnn.py).
 *   layer 1: Conv2d(4,32,8,stride 4)  on (84,84,4)  -> (20,20,32)
 *   layer 2: Conv2d(32,64,4,stride 2) on (20,20,32) -> (9,9,64)
 *   layer 3: Conv2d(64,64,3,stride 1) on (9,9,64)   -> (7,7,64)
 * Activations are (images, H, W, C) row-major ("NHWC").  Weights enter the kernels as repacked
 * matrices Bt (produced by mi355ppo_cnn_repack_weights_f32 from torch's (Cout,Cin,KH,KW) tensor):
 *   mode 0  forward / weight-gradient order  Bt[Cout][(kh,kw,cin)]
 *   mode 1  layer-3 data gradient            Bt[Cin][(r,c,cout)]   (taps flipped)
 *   mode 2  layer-2 data gradient            Bt[4][Cin][(r,c,cout)] (one 2x2-tap matrix per parity class)
 *   mode 3  layer-3 data gradient, per border class: 25 matrices [Cin][(r',c',cout)] for the 5x5 (row class,
 *           column class) tap windows (mi355ppo_cnn_conv_dgrad_f32_variant(..., variant 5)); 81*4096 floats
 *   mode 5  layer-2 data gradient, per border class: 9 matrices [4*Cin][(r',c',cout)] for the 3x3 (row class, column
 *           class) tap windows of the 10x10 class grid (variant 6); 16*128*64 floats
 *   mode 4  layer 1 only: the integer-digit pack of kernel Q (csrc/conv1q.hip): every weight as a 31-bit
 *           fixed-point number on its output channel's scale, four signed radix-256 digits in the operand
 *           layout of v_mfma_i32_32x32x32_i8, + accumulator start values + per-channel scales;
 *           mi355ppo_cnn_conv1q_pack_bytes() = 33,408 bytes.  Consumed by forward variant 6.
 * modes 0-2 have Cout*Cin*KH*KW floats.
 */
MI355PPO_API int mi355ppo_cnn_repack_weights_f32(const float* W, float* Bt, int layer, int mode, void* stream);

/* Kernel Q: layer-1 forward on the integer matrix pipe.  The uint8 frame bytes are exact int8 operands
 * (v - 128), the weights four int8 digits; int32 accumulation is exact, the only roundings are the
 * weight's one-time rounding to 2^-30 of its channel's largest weight and five f32 roundings per output
 * (Horner over the digits, scale, bias) -- closer to the float64 convolution than an f32 fma chain of
 * 256 terms, at 1/8 of its matrix-pipe time.  Same contract as mi355ppo_cnn_conv_fwd_f32(layer 1). */
MI355PPO_API size_t mi355ppo_cnn_conv1q_pack_bytes(void);
MI355PPO_API int mi355ppo_cnn_conv1q_pack(const float* W, void* pack, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q_fwd(const void* src_u8, const int64_t* inds, const void* pack, const float* bias,
                                         float* dst, int64_t images, void* stream);

/* dst = relu(conv(src) + bias).  layer 1: src is the uint8 rollout buffer (rows_total, 84,84,4) and
 * `inds` (images) int64 optionally gathers rows (b_obs[mb_inds]); the /255 is applied in registers,
 * correctly rounded.  layers 2,3: src is f32, inds must be NULL. */
MI355PPO_API int mi355ppo_cnn_conv_fwd_f32(const void* src, const int64_t* inds, const float* Bt, const float* bias,
                                           float* dst, int64_t images, int layer, void* stream);
/* `variant` (tuning/testing): 0 = auto (= 2; 4 for tensors beyond 4 GiB),
 * 2 = fixed-geometry streaming kernel F (weights resident in LDS, A fragments fetched straight into a register ring,
 *     taps as compile-time immediates, buffer loads/stores; tensors must be < 4 GiB), 4 = its run-time-geometry
 *     predecessor S; data gradient only: 3 = one launch per stride-parity class (layer 2), 5 = layer 3 split into
 *     its 25 border classes so that no padding zeros are multiplied (needs the mode-3 repack), 6 = layer 2 split
 *     into the 9 border classes of its class grid (needs the mode-5 repack);
 *     forward of layer 1 only: 6 = kernel Q (Bt = the mode-4 pack). */
MI355PPO_API int mi355ppo_cnn_conv_fwd_f32_variant(const void* src, const int64_t* inds, const float* Bt, const float* bias,
                                                   float* dst, int64_t images, int layer, int variant, void* stream);

/* The three forward layers back to back (a1 (images,20,20,32), a2 (images,9,9,64), a3 (images,7,7,64) out): one call
 * for inference-sized batches, where the host-side cost of a launch matters.  conv1_variant: 0 (bt1 = mode-0 matrix)
 * or 6 (bt1 = mode-4 pack, kernel Q). */
MI355PPO_API int mi355ppo_cnn_trunk_fwd_f32(const void* obs_u8, const int64_t* inds, const float* bt1, const float* b1,
                                            const float* bt2, const float* b2, const float* bt3, const float* b3,
                                            float* a1, float* a2, float* a3, int64_t images, int conv1_variant,
                                            void* stream);

/* dsrc = conv_transpose(dz) * (act_in > 0): gradient w.r.t. the layer's INPUT activation act_in
 * (itself a ReLU output), i.e. the pre-activation gradient of the previous layer.  layer = 2 or 3;
 * Bt in mode 2 / mode 1. */
MI355PPO_API int mi355ppo_cnn_conv_dgrad_f32(const float* dz, const float* Bt, const float* act_in, float* dsrc,
                                             int64_t images, int layer, void* stream);
MI355PPO_API int mi355ppo_cnn_conv_dgrad_f32_variant(const float* dz, const float* Bt, const float* act_in, float* dsrc,
                                                     int64_t images, int layer, int variant, void* stream);

/* dW (torch layout (Cout,Cin,KH,KW)) and db (Cout) from the layer input `src` (layer 1: uint8 + inds
 * as above) and the pre-activation gradient dz (images, Hout, Wout, Cout).  Overwrites dW / db.
 * Deterministic: per-workgroup partials in `workspace`, summed in a fixed order.
 * Layer 1: kernel P (csrc/conv1p.hip; bf16 pipe: the uint8 taps are exact bf16 operands, dz is split into three bf16 terms).
 * Layers 2, 3: kernel V (csrc/convw.hip; bf16 pipe, both operands transposed through LDS and split in registers, the batch
 * cut into slabs) for batches of a multiple of 16 images with every tensor below 4 GiB; kernel T (f32 pipe, csrc/conv.hip)
 * otherwise.  mi355ppo_cnn_conv_wgrad_kernel: 'P', 'V' or 'T', the kernel a call of this size runs (profiling aid). */
MI355PPO_API size_t mi355ppo_cnn_conv_wgrad_workspace_bytes(int64_t images, int layer);
MI355PPO_API int mi355ppo_cnn_conv_wgrad_kernel(int64_t images, int layer);
MI355PPO_API int mi355ppo_cnn_conv_wgrad_f32(const void* src, const int64_t* inds, const float* dz, float* dW, float* db,
                                             int64_t images, int layer, void* workspace, size_t workspace_bytes,
                                             void* stream);

/* ---------------------------------------------------------------------------------------------
 * Heads  actor = Linear(H, A) and critic = Linear(H, 1) of Agent (cleanrl/ppo_atari_multigpu.py:148-149,
 * used at :151,157-159), forward and backward.  Degenerate as GEMMs (A + 1 <= 8 columns); here one
 * bandwidth-bound pass over the hidden activations each.  H must be 512 (NatureCNN), 1 <= A <= 18 (every ALE action set; from A = 8 on the weight rows sit in LDS instead of registers -- round 6).
 *   h (M,H); Wa (A,H), ba (A); Wc (H) [= critic.weight (1,H)], bc (1)   ->   logits (M,A), value (M)
 *   backward: dlogits (M,A), dvalue (M)  ->  dh (M,H), dWa (A,H), dba (A), dWc (H), dbc (1)
 * Weight gradients are summed in a fixed order (deterministic); all outputs are overwritten.
 */
MI355PPO_API int mi355ppo_heads_fwd_f32(const float* h, const float* Wa, const float* ba, const float* Wc, const float* bc,
                                        float* logits, float* value, int M, int A, int H, void* stream);
MI355PPO_API size_t mi355ppo_heads_bwd_workspace_bytes(int M, int A);
MI355PPO_API int mi355ppo_heads_bwd_f32(const float* h, const float* Wa, const float* Wc, const float* dlogits,
                                        const float* dvalue, float* dh, float* dWa, float* dba, float* dWc, float* dbc,
                                        int M, int A, int H, void* workspace, size_t workspace_bytes, void* stream);
/* The same for an h that is the output of a ReLU (the FC layer's, :145): writes dz = dh * (h > 0), the gradient with respect
 * to that layer's pre-activation, and dbh (H) = its column sums (that layer's bias gradient) -- autograd's
 * threshold_backward pass and the bias reduction of the Linear below, done where h and dh are in registers anyway.
 * dz takes a row pitch lddz (floats, a multiple of 4, >= H). */
MI355PPO_API int mi355ppo_heads_bwd_relu_f32(const float* h, const float* Wa, const float* Wc, const float* dlogits,
                                             const float* dvalue, float* dz, int lddz, float* dWa, float* dba, float* dWc,
                                             float* dbc, float* dbh, int M, int A, int H, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* Every weight pack of the NatureCNN agent in one launch, from the parameters in torch's layouts (round 4): W1 (32,4,8,8) -> kernel
 * Q's pack (mi355ppo_cnn_conv1q_pack_bytes()); W2 (64,32,4,4) -> kernel Z's layer-2 forward pack [mi355ppo_fc_pack_bytes(64, 512)] and
 * data-gradient pack [(128, 256)]; W3 (64,64,3,3) -> layer-3 forward and data-gradient packs [(64, 576) each]; Wfc (512, 3136) in the
 * reference's (c, h, w) feature order -> the FC forward pack [(512, 3136), features re-ordered (h, w, c)] and data-gradient pack
 * [(3136, 512)].  Bit-identical to mi355ppo_cnn_repack_weights_f32 (modes 4 / 0 / 1 / 2) + mi355ppo_fc_pack_f32 per matrix -- what the
 * learner re-derives after each optimizer step (cleanrl/ppo_atari_multigpu.py:377).  A null output skips its piece. */
MI355PPO_API int mi355ppo_nature_packs_f32(const float* W1, const float* W2, const float* W3, const float* Wfc, void* qpack,
                                           void* conv2_fwd, void* conv3_fwd, void* conv3_dgrad, void* conv2_dgrad, void* fc_fwd,
                                           void* fc_dgrad, void* stream);

/* Rollout step of the NatureCNN agent, fused behind the trunk (round 4): Linear(3136,512) with K split over the grid (raw partials in
 * `workspace`, mi355ppo_fc_fwd_workspace_bytes(M, 512, 3136) bytes; M < 8192), then ONE kernel for the partial fold + bias + ReLU,
 * the two heads and the Categorical draw -- Agent.get_action_and_value(next_obs) from conv3's output on
 * (cleanrl/ppo_atari_multigpu.py:144-149,155-159) -- writing action / log-prob / value (and optionally the hidden activations) in
 * place.  Bit-identical to mi355ppo_fc_fwd_relu_packed_ws_f32 -> mi355ppo_heads_fwd_f32 -> mi355ppo_categorical_sample_ctr_f32. */
MI355PPO_API int mi355ppo_fc_heads_act_categorical_f32(const float* a3, int lda, const void* fc_pack, const float* fc_bias,
                                                       const float* Wa, const float* ba, const float* Wc, const float* bc, int M, int A,
                                                       int H, int K, const float* noise_exp1, uint64_t seed, uint64_t offset,
                                                       const uint64_t* offset_base, int64_t* action_i64, float* action_f32,
                                                       float* logprob, float* value, float* hidden_out, void* workspace,
                                                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Round 5 -- the NatureCNN GEMMs on a TWO-TERM f16 split (csrc/f16split.h): three v_mfma_f32_32x32x16_f16 per f32 product where the
 * three-term bf16 split of the entry points above needs six, f32 accumulation, products of terms exact.  Every split tensor is scaled
 * by a power of two derived from its amax record (MI355PPO_AMAX_WORDS uint32, 64-byte aligned, see above): an entry point READS the
 * record of each f32 operand it splits (`*_amax` inputs; required) and FOLDS the values it stores into the record of its result
 * (`*_amax` outputs; null = nobody will split the result); the caller zeroes the output records of a pass before its first launch.
 * Weights travel as "f16x2 packs": [64-byte header: max |B|][k-step][32-column tile][hi, lo][64 lanes][8 f16] of s B.
 * The reference arithmetic is the same as for the bf16 entry points they mirror (cleanrl/ppo_atari_multigpu.py:136-148 forward, :358
 * backward: f32 Conv2d / Linear); error against float64 at or below theirs (tools/err_f16x2.py, tests/test_gpu_f16x2.py).
 */
MI355PPO_API int mi355ppo_absmax_f32(const float* x, int64_t n, uint32_t* amax, void* stream);   /* amax = max(amax, max |x|) */
MI355PPO_API size_t mi355ppo_fc_pack_f16x2_bytes(int N, int K);
MI355PPO_API int mi355ppo_fc_pack_f16x2_f32(const float* B, int ldb, int N, int K, const uint32_t* b_amax, void* pack, void* stream);
/* mi355ppo_nature_packs_f32 with the six kernel-Z packs as f16x2 packs [mi355ppo_fc_pack_f16x2_bytes of the same shapes]; `w_amax` =
 * three records (3 * MI355PPO_AMAX_WORDS) that receive max |W2|, |W3|, |Wfc| -- every slot written by this call (no zeroing needed). */
MI355PPO_API int mi355ppo_nature_packs_f16x2_f32(const float* W1, const float* W2, const float* W3, const float* Wfc, void* qpack,
                                                 void* conv2_fwd, void* conv3_fwd, void* conv3_dgrad, void* conv2_dgrad, void* fc_fwd,
                                                 void* fc_dgrad, uint32_t* w_amax, void* stream);
/* mi355ppo_cnn_conv1q_fwd / _bits (mask_bits may be null) that also records max(dst) -- the layer-2 forward's A-operand scale. */
MI355PPO_API int mi355ppo_cnn_conv1q_fwd_amax(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                              uint32_t* mask_bits, int64_t images, uint32_t* dst_amax, void* stream);
/* mi355ppo_cnn_conv_fwd_packed_f32 / _bits_f32 (mask_bits may be null) */
MI355PPO_API int mi355ppo_cnn_conv_fwd_packed_f16x2_f32(const float* src, const void* pack, const float* bias, float* dst, uint32_t* mask_bits,
                                                        int64_t images, int layer, const uint32_t* src_amax, uint32_t* dst_amax, void* stream);
/* mi355ppo_cnn_conv_dgrad_packed_f32 / _bits_f32: the ReLU mask from mask_bits if given, else from act_in */
MI355PPO_API int mi355ppo_cnn_conv_dgrad_packed_f16x2_f32(const float* dz, const void* pack, const float* act_in, const uint32_t* mask_bits,
                                                          float* dsrc, int64_t images, int layer, const uint32_t* dz_amax, uint32_t* dsrc_amax,
                                                          void* stream);
/* 'R', 'B' or 'Z': the kernel a forward (dgrad = 0) / bit-masked data-gradient (dgrad = 1) call of this size and layer runs (profiling aid).
 * Kernel R (csrc/convr.hip) holds the source of a group of images in LDS, split once, and takes both forwards and the layer-3 data
 * gradient at every size and the layer-2 data gradient from 512 images on; its results are kernel Z's bit for bit (same products, same order).
 * 'B' = kernel RB (csrc/convrb.hip): kernel R's layer-2 data gradient from 3,072 images on with three images per group and the rows dealt to
 * tiles by border class (the products with a zero-border operand are not issued: two thirds of the matrix instructions, the same bits). */
MI355PPO_API int mi355ppo_cnn_conv_packed_kernel_f16x2(int64_t images, int layer, int dgrad);
/* 'G' or 'Z': the kernel mi355ppo_fc_fwd_relu_packed_f16x2_f32 without a K split (dgrad = 0) / mi355ppo_fc_dgrad_packed_f16x2_f32 with mask
 * bits (dgrad = 1) runs for this shape (ABI 1.9).  Kernel G (csrc/gemmg.hip, round 6) streams both operands through workgroup-wide LDS
 * rings, A split once per workgroup; its results are kernel Z's bit for bit (same products, same order). */
MI355PPO_API int mi355ppo_fc_packed_kernel_f16x2(int M, int N, int K, int dgrad);
/* mi355ppo_cnn_conv_wgrad_f32 for layers 2 / 3 (kernel V); other batches fall to the f32-pipe kernel and ignore the records */
MI355PPO_API int mi355ppo_cnn_conv_wgrad_f16x2_f32(const float* src, const float* dz, float* dW, float* db, int64_t images, int layer,
                                                   void* workspace, size_t workspace_bytes, const uint32_t* src_amax, const uint32_t* dz_amax,
                                                   void* stream);
/* 'U', 'V', 'P' or 'T': the kernel the two f16x2 weight-gradient entry points run for this batch and layer (1..3) -- kernel U (csrc/convu.hip) while the
 * tensors stay inside the 32-bit buffer range, else kernel V / P, else the f32-pipe kernel T (ABI 1.9; profiling aid: bench.py labels its rows with it). */
MI355PPO_API int mi355ppo_cnn_conv_wgrad_kernel_f16x2(int64_t images, int layer);
/* mi355ppo_cnn_conv_wgrad_f32 for layer 1 (kernel P) with dz in two f16 terms; the uint8 frames are exact f16 operands: only dz's record */
MI355PPO_API int mi355ppo_cnn_conv1_wgrad_f16x2(const void* src_u8, const int64_t* inds, const float* dz, float* dW, float* db, int64_t images,
                                                void* workspace, size_t workspace_bytes, const uint32_t* dz_amax, void* stream);
/* mi355ppo_fc_fwd_relu_packed_ws_f32 (ws may be null / 0: whole-K wave tiles); the K-split route records no h_amax (pass null) */
MI355PPO_API int mi355ppo_fc_fwd_relu_packed_f16x2_f32(const float* a, int lda, const void* pack, const float* bias, float* h, int M, int N,
                                                       int K, void* ws, size_t ws_bytes, const uint32_t* a_amax, uint32_t* h_amax, void* stream);
/* mi355ppo_fc_dgrad_mask_packed_f32 / _maskbits_ */
MI355PPO_API int mi355ppo_fc_dgrad_packed_f16x2_f32(const float* dz, int lddz, const void* pack, const float* act_in, const uint32_t* mask_bits,
                                                    float* da, int M, int N, int K, const uint32_t* dz_amax, uint32_t* da_amax, void* stream);
/* mi355ppo_fc_wgrad_f32 (kernel W; other shapes fall to the f32-pipe kernel Y and ignore the records) */
MI355PPO_API int mi355ppo_fc_wgrad_f16x2_f32(const float* dz, int lddz, const float* a, float* dW, int M, int N, int K, int hwc_channels,
                                             void* workspace, size_t workspace_bytes, const uint32_t* dz_amax, const uint32_t* a_amax,
                                             void* stream);
/* mi355ppo_heads_bwd_relu_f32 that also records max |dz| (the FC layer's data / weight gradients scale dz by it) */
MI355PPO_API int mi355ppo_heads_bwd_relu_amax_f32(const float* h, const float* Wa, const float* Wc, const float* dlogits, const float* dvalue,
                                                  float* dz, int lddz, float* dWa, float* dba, float* dWc, float* dbc, float* dbh, int M, int A,
                                                  int H, void* workspace, size_t workspace_bytes, uint32_t* dz_amax, void* stream);
/* mi355ppo_fc_heads_act_categorical_f32 with an f16x2 `fc_pack` and a3's record */
MI355PPO_API int mi355ppo_fc_heads_act_categorical_f16x2_f32(const float* a3, int lda, const void* fc_pack, const float* fc_bias,
                                                             const float* Wa, const float* ba, const float* Wc, const float* bc, int M, int A,
                                                             int H, int K, const float* noise_exp1, uint64_t seed, uint64_t offset,
                                                             const uint64_t* offset_base, int64_t* action_i64, float* action_f32,
                                                             float* logprob, float* value, float* hidden_out, void* workspace,
                                                             size_t workspace_bytes, const uint32_t* a3_amax, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Test / benchmark support -- NOT part of the reference path.  One step of the device-resident synthetic Atari
 * vector env (cleanrl_amd/envs.py::DeviceSyntheticAtariVecEnv) that stands in for envpool / ALE, which this image
 * does not have: obs[n] = planes[cursor_n .. cursor_n+3] (mod pool) as (N,4,84,84) uint8; with advance != 0 first
 * reward in {-1,0,+1} (P = .05,.9,.05), done ~ Bernoulli(done_p), cursor += 1 or jumps on done (Philox(seed; n, step)).
 */
MI355PPO_API int mi355ppo_synth_atari_step_u8(const uint8_t* planes, int pool, int64_t* cursor, uint64_t seed, uint64_t step,
                                              uint8_t* obs, float* reward, float* done, int N, double done_p, int advance,
                                              void* stream);
MI355PPO_API int mi355ppo_synth_atari_step_ctr_u8(const uint8_t* planes, int pool, int64_t* cursor, uint64_t seed, uint64_t step,
                                                  const uint64_t* step_base, uint8_t* obs, float* reward, float* done, int N,
                                                  double done_p, int advance, void* stream);   /* step_eff = step + *step_base */
/* The same step with obs written pixel-interleaved, (N,84,84,4): the rollout rows' layout (gather + relayout in one launch). */
MI355PPO_API int mi355ppo_synth_atari_step_hwc_ctr_u8(const uint8_t* planes, int pool, int64_t* cursor, uint64_t seed, uint64_t step,
                                                      const uint64_t* step_base, uint8_t* obs, float* reward, float* done, int N,
                                                      double done_p, int advance, void* stream);

/* The continuous-control stand-in (cleanrl_amd/envs.py::DeviceSyntheticContinuousVecEnv; bench.py --config E), one launch per env
 * step: a = clip(action, -1, 1); next = noise[(k + *k_base) % bank][n] + state[n] @ At + a @ Bm; reward = next . w - 0.1 |a|^2;
 * truncation after `horizon` steps (state := reset_state).  state (N, O) is updated in place and copied to obs_out. */
MI355PPO_API int mi355ppo_synth_continuous_step_f32(float* state, const float* reset_state, const float* At, const float* Bm, const float* w,
                                                    const float* noise, int bank, uint64_t k, const uint64_t* k_base, float* steps,
                                                    double horizon, const float* action, float* obs_out, float* reward, float* done, int N,
                                                    int O, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PQN (cleanrl/pqn.py, cleanrl/pqn_atari_envpool.py; csrc/pqn.hip, row math in csrc/pqn_rows.h).  All f32, row-major; every
 * *_cpu twin takes host pointers and returns the device's bits.  No entry point allocates or synchronises (all are capturable).
 *
 * e-greedy (the rollout's action logic): per env n, g = argmax q[n, :] (torch's rule: the first maximum wins, a NaN is the maximum
 * and the first NaN wins), values_out[n] = q[n, g], a = (u[n] < (float)epsilon) ? random_actions[n] : g; actions_out[n] = (float)a
 * and, when non-NULL, action_i64_out[n] = a.  actions_out / values_out point at the storage row of the step. */
MI355PPO_API int mi355ppo_pqn_egreedy_f32(const float* q, const int64_t* random_actions, const float* u, double epsilon, float* actions_out,
                                          float* values_out, int64_t* action_i64_out, int N, int A, void* stream);
MI355PPO_API int mi355ppo_pqn_egreedy_f32_cpu(const float* q, const int64_t* random_actions, const float* u, double epsilon,
                                              float* actions_out, float* values_out, int64_t* action_i64_out, int N, int A);
/* Q(lambda) targets: returns (T, N) from rewards, dones, values (T, N), next_done (N) and next_q (N, A) (the bootstrap is
 * torch.max(next_q, dim=-1), NaN-propagating), in the reference loop's operation order with gamma, q_lambda and 1 - q_lambda (formed
 * in double) rounded to f32: bit-equal to the loop run by torch on the CPU. */
MI355PPO_API int mi355ppo_pqn_qlambda_f32(const float* rewards, const float* dones, const float* values, const float* next_done,
                                          const float* next_q, float* returns, int T, int N, int A, double gamma, double q_lambda, void* stream);
MI355PPO_API int mi355ppo_pqn_qlambda_f32_cpu(const float* rewards, const float* dones, const float* values, const float* next_done,
                                              const float* next_q, float* returns, int T, int N, int A, double gamma, double q_lambda);
/* TD loss of a minibatch: old[r] = q[r, (long)b_actions[i]], loss = F.mse_loss(b_returns[i], old) with i = mb_inds[r] (B = rows of
 * b_actions / b_returns; an index or action out of range is clamped).  dq (M, A) = d loss / d q (non-zero only in the action's
 * column); scalars_out = {loss, mean(old)}, summed in f64 in a fixed order. */
MI355PPO_API int mi355ppo_pqn_td_loss_fwd_bwd_f32(const float* q, const int64_t* mb_inds, const float* b_actions, const float* b_returns,
                                                  float* dq, float* scalars_out, int M, int A, int64_t B, void* stream);
MI355PPO_API int mi355ppo_pqn_td_loss_fwd_bwd_f32_cpu(const float* q, const int64_t* mb_inds, const float* b_actions, const float* b_returns,
                                                      float* dq, float* scalars_out, int M, int A, int64_t B);
/* pqn.py's QNetwork: Linear(O, 120) -> LayerNorm(120) -> ReLU -> Linear(120, 84) -> LayerNorm(84) -> ReLU -> Linear(84, A), its
 * parameters flat in agent.parameters() order (params, mi355ppo_pqn_* count: 120 O + 360 + 10080 + 252 + 85 A).  1 <= O <= 64,
 * 1 <= A <= 18, else MI355PPO_EINVAL.  fwd: q_out (N, A).  act: one rollout step in one launch -- the forward, e-greedy as above and,
 * when non-NULL, obs_row_out[n] = obs[n] and done_row_out[n] = done_in[n] (the step's storage rows). */
MI355PPO_API int mi355ppo_pqn_mlp_fwd_f32(const float* obs, const float* params, float* q_out, int N, int O, int A, void* stream);
MI355PPO_API int mi355ppo_pqn_mlp_fwd_f32_cpu(const float* obs, const float* params, float* q_out, int N, int O, int A);
MI355PPO_API int mi355ppo_pqn_mlp_act_f32(const float* obs, const float* params, const int64_t* random_actions, const float* u, double epsilon,
                                          float* actions_out, float* values_out, int64_t* action_i64_out, float* obs_row_out, const float* done_in,
                                          float* done_row_out, int N, int O, int A, void* stream);
MI355PPO_API int mi355ppo_pqn_mlp_act_f32_cpu(const float* obs, const float* params, const int64_t* random_actions, const float* u,
                                              double epsilon, float* actions_out, float* values_out, int64_t* action_i64_out, float* obs_row_out,
                                              const float* done_in, float* done_row_out, int N, int O, int A);
/* One minibatch of pqn.py: gather b_obs[mb_inds] (B rows), forward, the TD loss as above, backward through both LayerNorm + ReLU
 * layers; grads (flat, agent.parameters() order) is OVERWRITTEN with d loss / d params; scalars_out = {td_loss, mean(old)}.  Two
 * launches: per-workgroup (256 rows) partials, then their fold in a fixed order. */
MI355PPO_API size_t mi355ppo_pqn_mlp_td_workspace_bytes(int M, int O, int A);
MI355PPO_API int mi355ppo_pqn_mlp_td_fwd_bwd_f32(const float* b_obs, int64_t B, const int64_t* mb_inds, const float* params,
                                                 const float* b_actions, const float* b_returns, float* grads, float* scalars_out, int M, int O,
                                                 int A, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_pqn_mlp_td_fwd_bwd_f32_cpu(const float* b_obs, int64_t B, const int64_t* mb_inds, const float* params,
                                                     const float* b_actions, const float* b_returns, float* grads, float* scalars_out, int M,
                                                     int O, int A);
/* clip_grad_norm_(max_grad_norm) + torch.optim.RAdam(lr, (beta1, beta2), eps) step `step` (1-based) on flat buffers, in torch's
 * single-tensor operation order; zeroes grads.  mi355ppo_radam_schedule_f32 writes the step's 8-float slot {1 - beta1^step, lr,
 * (1 - beta2^step)^0.5, rect, rho_t > 5, 0, 0, 0} (double, rounded to f32); the _sched form reads such a slot from DEVICE memory. */
MI355PPO_API int mi355ppo_radam_schedule_f32(double lr, double beta1, double beta2, int64_t step, float* out8_host);
MI355PPO_API size_t mi355ppo_clip_radam_workspace_bytes(int64_t n);
MI355PPO_API int mi355ppo_clip_radam_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double max_grad_norm,
                                         double lr, double beta1, double beta2, double eps, int64_t step, float* total_norm_out, void* workspace,
                                         size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_clip_radam_sched_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double max_grad_norm,
                                               double beta1, double beta2, double eps, const float* sched8, float* total_norm_out,
                                               void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_clip_radam_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double max_grad_norm,
                                             double lr, double beta1, double beta2, double eps, int64_t step, float* total_norm_out);

/* ---------------------------------------------------------------------------------------------
 * The recurrent PQN tail (cleanrl/pqn_atari_envpool_lstm.py; csrc/pqn_lstm.hip, row math in csrc/pqn_lstm_rows.h).  All f32,
 * row-major; H must be 128 and 1 <= A <= 18, else MI355PPO_EINVAL.  No entry point allocates or synchronises (all are capturable).
 *
 * act -- one rollout step after the gx GEMM, in one launch.  gx (N, 4H) = x W_ih^T + b_ih + b_hh, w_hh (4H, H), h_in / c_in (N, H),
 * done_in (N), wq (A, H), bq (A).  keep = 1 - done_in; one LSTM cell on (keep h_in, keep c_in): h_out / c_out (N, H) are bit-equal to
 * mi355ppo_lstm_seq_fwd_f32 at T = 1 on the same device, and may alias h_in / c_in.  q[n, a] = dot(wq[a, :], h_out[n, :]) + bq[a]
 * (four interleaved fmaf chains over k, folded (s0 + s1) + (s2 + s3), then the bias).  Then e-greedy on q exactly as
 * mi355ppo_pqn_egreedy_f32 (first maximum wins, a NaN is the maximum, u < (float)epsilon) into actions_out / values_out (the step's
 * storage rows) and, when non-NULL, action_i64_out; done_row_out[n] = done_in[n] when non-NULL.  q_out (N, A) is written when
 * non-NULL.  h_out and c_out are both given or both NULL (NULL: the state is discarded); actions_out, values_out, random_actions
 * and u go together.  The bootstrap form q(next_obs) passes only q_out.  The *_cpu twin shares every FMA with the device; expf /
 * tanhf come from libm, so it agrees to the last bits, not bit for bit. */
MI355PPO_API int mi355ppo_pqn_lstm_act_f32(const float* gx, const float* w_hh, const float* h_in, const float* c_in, const float* done_in,
                                           const float* wq, const float* bq, const int64_t* random_actions, const float* u, double epsilon,
                                           float* h_out, float* c_out, float* q_out, float* actions_out, float* values_out,
                                           int64_t* action_i64_out, float* done_row_out, int N, int H, int A, void* stream);
MI355PPO_API int mi355ppo_pqn_lstm_act_f32_cpu(const float* gx, const float* w_hh, const float* h_in, const float* c_in, const float* done_in,
                                               const float* wq, const float* bq, const int64_t* random_actions, const float* u,
                                               double epsilon, float* h_out, float* c_out, float* q_out, float* actions_out,
                                               float* values_out, int64_t* action_i64_out, float* done_row_out, int N, int H, int A);
/* td -- q_func + gather + F.mse_loss of one minibatch, forward and backward.  h (M, H): the scan's output rows in minibatch order;
 * i = mb_inds[r] indexes b_actions / b_returns (B rows; an index or action out of range is clamped).  a = (long)b_actions[i],
 * old[r] = dot(wq[a, :], h[r, :]) + bq[a] (the act kernel's q), loss = mean((ret - old)^2), g_r = -((float)(2 / M) * (ret - old)).
 * dh (M, H): dh[r, :] = g_r wq[a, :]; dwq (A, H) and dbq (A) are OVERWRITTEN with sum over the rows of that action of g_r h[r, :]
 * and g_r (rows in ascending order within workgroups of 256 rows, then the workgroups in order; an action that never occurs gets
 * exact zeros); scalars_out = {loss, mean(old)}, summed in f64 in a fixed order.  Two launches.  The *_cpu twin returns the
 * device's bits. */
MI355PPO_API size_t mi355ppo_pqn_lstm_td_workspace_bytes(int M, int A);
MI355PPO_API int mi355ppo_pqn_lstm_td_fwd_bwd_f32(const float* h, const int64_t* mb_inds, const float* b_actions, const float* b_returns,
                                                  const float* wq, const float* bq, float* dh, float* dwq, float* dbq, float* scalars_out,
                                                  int M, int H, int A, int64_t B, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu(const float* h, const int64_t* mb_inds, const float* b_actions, const float* b_returns,
                                                      const float* wq, const float* bq, float* dh, float* dwq, float* dbq,
                                                      float* scalars_out, int M, int H, int A, int64_t B);

/* ---- DDPG / TD3 (ABI 2.7, csrc/offpolicy.hip; reference: cleanrl/ddpg_continuous_action.py, cleanrl/td3_continuous_action.py) ----
 * Actor and QNetwork are Linear(K, 256) - ReLU - Linear(256, 256) - ReLU - Linear(256, J) (K = obs_dim, J = act_dim; K = obs_dim +
 * act_dim, J = 1 on cat(obs, action)); a network is its flat f32 parameters in .parameters() order.  1 <= obs_dim <= 512,
 * 1 <= act_dim <= 20, anything else is MI355PPO_EINVAL.  The replay ring is five f32 arrays (slots, n_envs, .): obs, next_obs,
 * actions, rewards, dones; a batch row m is ring row batch_inds[m] * n_envs + env_inds[m] (int64; an index out of range is
 * clamped).  No entry point allocates or synchronises, none uses atomics, all can be captured.  Every *_cpu twin (host pointers, no
 * workspace, no stream) returns the device's bits: the accumulation orders are those of csrc/offpolicy_rows.h.
 *
 * replay_add: one step's N transitions into slot pos (0 <= pos < slots).  One launch. */
MI355PPO_API int mi355ppo_replay_add_f32(const float* obs, const float* next_obs, const float* actions, const float* rewards,
                                         const float* dones, float* ring_obs, float* ring_next_obs, float* ring_actions,
                                         float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int N, int O, int A,
                                         void* stream);
MI355PPO_API int mi355ppo_replay_add_f32_cpu(const float* obs, const float* next_obs, const float* actions, const float* rewards,
                                             const float* dones, float* ring_obs, float* ring_next_obs, float* ring_actions,
                                             float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int N, int O, int A);
/* act: actions_out (N, A) = clip(tanh(actor(obs)) * action_scale + action_bias + noise_row, low, high); noise_row (A) may be NULL.
 * One launch. */
MI355PPO_API int mi355ppo_ddpg_act_f32(const float* obs, const float* actor_params, const float* action_scale, const float* action_bias,
                                       const float* noise_row, const float* low, const float* high, float* actions_out, int N, int O,
                                       int A, void* stream);
MI355PPO_API int mi355ppo_ddpg_act_f32_cpu(const float* obs, const float* actor_params, const float* action_scale,
                                           const float* action_bias, const float* noise_row, const float* low, const float* high,
                                           float* actions_out, int N, int O, int A);
/* target: next_q_value (M) = rewards + (1 - dones) * gamma * min_c q_c(next_obs, a'), a' = target_actor(next_obs) and, with noise (M, A)
 * non-NULL, + (noise * policy_noise).clamp(+-noise_clip) * action_scale clamped to [low0, high0] (TD3); noise NULL: neither (DDPG).
 * target_critics holds n_critics (1 or 2) networks back to back.  next_actions_out (M, A) may be NULL.  One launch. */
MI355PPO_API int mi355ppo_td3_target_f32(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                         const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                         const float* target_actor, const float* target_critics, int n_critics,
                                         const float* action_scale, const float* action_bias, const float* noise, double policy_noise,
                                         double noise_clip, double low0, double high0, double gamma, float* next_q_value,
                                         float* next_actions_out, int M, int O, int A, void* stream);
MI355PPO_API int mi355ppo_td3_target_f32_cpu(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                             const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                             const float* target_actor, const float* target_critics, int n_critics,
                                             const float* action_scale, const float* action_bias, const float* noise,
                                             double policy_noise, double noise_clip, double low0, double high0, double gamma,
                                             float* next_q_value, float* next_actions_out, int M, int O, int A);
/* critic: q_c = critic_c(obs, actions), loss = sum_c F.mse_loss(q_c, next_q_value); grads (n_critics * critic parameters, the order of
 * list(qf1.parameters()) + list(qf2.parameters())) is OVERWRITTEN; scalars_out (2 * n_critics) = {mean q1, qf1_loss, mean q2, qf2_loss}.
 * Two launches: per-workgroup partials, then the fold in workgroup order. */
MI355PPO_API size_t mi355ppo_td3_critic_workspace_bytes(int M, int O, int A, int n_critics);
MI355PPO_API int mi355ppo_td3_critic_fwd_bwd_f32(const float* ring_obs, const float* ring_actions, const int64_t* batch_inds,
                                                 const int64_t* env_inds, int64_t slots, int n_envs, const float* critics, int n_critics,
                                                 const float* next_q_value, float* grads, float* scalars_out, int M, int O, int A,
                                                 void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_td3_critic_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_actions, const int64_t* batch_inds,
                                                     const int64_t* env_inds, int64_t slots, int n_envs, const float* critics,
                                                     int n_critics, const float* next_q_value, float* grads, float* scalars_out, int M,
                                                     int O, int A);
/* actor: actor_loss = -mean(qf1(obs, actor(obs))); grads (actor parameters) is OVERWRITTEN (qf1 gets no gradient: the backward runs
 * through its first layer to the action columns only); dq_daction_out (M, A), the gradient of the loss w.r.t. the action, may be
 * NULL.  Two launches. */
MI355PPO_API size_t mi355ppo_td3_actor_workspace_bytes(int M, int O, int A);
MI355PPO_API int mi355ppo_td3_actor_fwd_bwd_f32(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                int n_envs, const float* actor, const float* qf1, const float* action_scale,
                                                const float* action_bias, float* grads, float* actor_loss_out, float* dq_daction_out,
                                                int M, int O, int A, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_td3_actor_fwd_bwd_f32_cpu(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds,
                                                    int64_t slots, int n_envs, const float* actor, const float* qf1,
                                                    const float* action_scale, const float* action_bias, float* grads,
                                                    float* actor_loss_out, float* dq_daction_out, int M, int O, int A);
/* polyak: target = (float)tau * param + (float)(1 - tau) * target over flat buffers (1 - tau formed in double, as Python does).
 * One launch; bit-equal to the reference's per-parameter loop.  Adam for these scripts is mi355ppo_clip_adam_f32 with
 * grad_scale = 1 and max_grad_norm = +inf (coefficient min(inf, 1) = exactly 1) and eps = 1e-8. */
MI355PPO_API int mi355ppo_polyak_f32(const float* params, float* target_params, int64_t n, double tau, void* stream);
MI355PPO_API int mi355ppo_polyak_f32_cpu(const float* params, float* target_params, int64_t n, double tau);

/* ---- SAC (ABI 2.7.1, csrc/sac.hip; reference: cleanrl/sac_continuous_action.py) ----
 * The critics are the QNetwork of the section above.  The actor is Linear(obs_dim, 256) - ReLU - Linear(256, 256) - ReLU and two heads
 * Linear(256, act_dim), flat in .parameters() order: fc1.w, fc1.b, fc2.w, fc2.b, fc_mean.w, fc_mean.b, fc_logstd.w, fc_logstd.b.
 * get_action(obs, eps): log_std = -5 + 3.5 * (tanh(u) + 1), x = mean + exp(log_std) * eps, y = tanh(x), action = y * action_scale +
 * action_bias, log_pi = sum_a [Normal(mean, std).log_prob(x) - log(action_scale * (1 - y^2) + 1e-6)]; eps (rows, act_dim) is the
 * caller's standard normal draw.  exp, log and tanh are the library's own (csrc/sac_rows.h), identical on host and device.  alpha is
 * read from one float in device memory (host memory for the twins).  Limits, ring, indices and the twins' bit equality as above.
 *
 * policy: get_action forward.  batch_inds / env_inds both NULL: obs is a dense (rows, obs_dim) array; both given: obs is a ring array
 * gathered through them.  actions_out (rows, act_dim) and log_pi_out (rows) may be NULL, not both.  One launch. */
MI355PPO_API int mi355ppo_sac_policy_f32(const float* obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                         const float* actor, const float* action_scale, const float* action_bias, const float* eps,
                                         float* actions_out, float* log_pi_out, int rows, int O, int A, void* stream);
MI355PPO_API int mi355ppo_sac_policy_f32_cpu(const float* obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                             const float* actor, const float* action_scale, const float* action_bias, const float* eps,
                                             float* actions_out, float* log_pi_out, int rows, int O, int A);
/* target: next_q_value (M) = rewards + (1 - dones) * gamma * (min(q1', q2') - alpha * log_pi'), (a', log_pi') = get_action of the ONLINE
 * actor on next_obs, q_c' the two target critics (back to back) on (next_obs, a').  next_actions_out (M, A) and log_pi_out (M) may be
 * NULL.  One launch. */
MI355PPO_API int mi355ppo_sac_target_f32(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                         const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs, const float* actor,
                                         const float* target_critics, const float* action_scale, const float* action_bias, const float* eps,
                                         const float* alpha, double gamma, float* next_q_value, float* next_actions_out, float* log_pi_out,
                                         int M, int O, int A, void* stream);
MI355PPO_API int mi355ppo_sac_target_f32_cpu(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                             const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                             const float* actor, const float* target_critics, const float* action_scale,
                                             const float* action_bias, const float* eps, const float* alpha, double gamma,
                                             float* next_q_value, float* next_actions_out, float* log_pi_out, int M, int O, int A);
/* actor: actor_loss = mean(alpha * log_pi - min(qf1(obs, pi), qf2(obs, pi))), (pi, log_pi) = get_action(obs, eps); critics holds the two
 * online critics back to back and gets no gradient.  grads (actor parameters) is OVERWRITTEN.  torch.min's backward: 1 to the smaller
 * q, 0.5 to each on a tie.  log_pi_out (M), dmean_out and du_out (M, A: d loss / d fc_mean's and fc_logstd's outputs) may be NULL.
 * Two launches. */
MI355PPO_API size_t mi355ppo_sac_actor_workspace_bytes(int M, int O, int A);
MI355PPO_API int mi355ppo_sac_actor_fwd_bwd_f32(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                int n_envs, const float* actor, const float* critics, const float* action_scale,
                                                const float* action_bias, const float* eps, const float* alpha, float* grads,
                                                float* actor_loss_out, float* log_pi_out, float* dmean_out, float* du_out, int M, int O,
                                                int A, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_sac_actor_fwd_bwd_f32_cpu(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds,
                                                    int64_t slots, int n_envs, const float* actor, const float* critics,
                                                    const float* action_scale, const float* action_bias, const float* eps,
                                                    const float* alpha, float* grads, float* actor_loss_out, float* log_pi_out,
                                                    float* dmean_out, float* du_out, int M, int O, int A);
/* alpha: alpha_loss = mean(-exp(log_alpha) * (log_pi + target_entropy)) (f64 fold), its gradient w.r.t. log_alpha (the same value) and
 * one torch Adam step on that scalar; exp_avg / exp_avg_sq are its one-float moments.  sched2 NULL: the step size and bias correction
 * are mi355ppo_adam_schedule_f32(lr, beta1, beta2, step); otherwise they are read from the two device floats sched2 (capturable) and
 * lr / step are ignored.  Writes log_alpha, alpha_out = exp(log_alpha) and alpha_loss_out.  One launch of one workgroup. */
MI355PPO_API int mi355ppo_sac_alpha_f32(const float* log_pi, int M, double target_entropy, float* log_alpha, float* exp_avg,
                                        float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step,
                                        const float* sched2, float* alpha_out, float* alpha_loss_out, void* stream);
MI355PPO_API int mi355ppo_sac_alpha_f32_cpu(const float* log_pi, int M, double target_entropy, float* log_alpha, float* exp_avg,
                                            float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step,
                                            float* alpha_out, float* alpha_loss_out);
/* the library's exp and log on host arrays (tests): exp_out[i] = exp(x[i]), log_out[i] = log(x[i]); either output may be NULL. */
MI355PPO_API int mi355ppo_sac_exp_log_f32_cpu(const float* x, float* exp_out, float* log_out, int64_t n);

/* ---- DQN / C51 (added under ABI 2.7.1, csrc/dqn.hip; reference: cleanrl/dqn.py, cleanrl/c51.py) ----
 * QNetwork is Linear(obs_dim, 120) - ReLU - Linear(120, 84) - ReLU - Linear(84, n_actions * n_atoms), flat f32 parameters in
 * .parameters() order; n_atoms = 1 is dqn.py's network.  1 <= obs_dim <= 512, 2 <= n_actions <= 18, 1 <= n_atoms <= 101,
 * n_actions * n_atoms <= 512 (the C51 update needs n_atoms >= 2); anything else is MI355PPO_EINVAL before any launch.  The ring is
 * the one of the section above with an action width of 1: the action index stored as f32.  atoms (n_atoms) is the network's own
 * torch.linspace buffer; it is read, never recomputed.  exp and log are the library's own (csrc/sac_rows.h).  No entry point allocates
 * or synchronises, none uses atomics, all can be captured; every *_cpu twin returns the device's bits (csrc/dqn_rows.h).
 *
 * act: actions_out (N, int64) = argmax_a q(obs)[a], a tie to the lowest index.  n_atoms == 1: q = q_network(obs) and atoms may be
 * NULL; n_atoms > 1: C51's get_action -- softmax over each action's atoms, q = (pmfs * atoms).sum in ascending atom order.  q_out
 * (N, n_actions) may be NULL.  One launch. */
MI355PPO_API int mi355ppo_dqn_act_f32(const float* obs, const float* params, const float* atoms, int64_t* actions_out, float* q_out, int N,
                                      int O, int n_actions, int n_atoms, void* stream);
MI355PPO_API int mi355ppo_dqn_act_f32_cpu(const float* obs, const float* params, const float* atoms, int64_t* actions_out, float* q_out, int N,
                                          int O, int n_actions, int n_atoms);
/* dqn.py's update: td_target = rewards + gamma * target(next_obs).max(1) * (1 - dones), old_val = online(obs)[action],
 * loss = F.mse_loss(td_target, old_val).  grads (the online network's parameters) is OVERWRITTEN; scalars_out (2) = {td_loss,
 * mean old_val}; target_q_out (M, n_actions) and td_target_out (M) may be NULL.  Two launches: per-workgroup partials, then the fold
 * in workgroup order. */
MI355PPO_API size_t mi355ppo_dqn_td_workspace_bytes(int M, int O, int n_actions);
MI355PPO_API int mi355ppo_dqn_td_fwd_bwd_f32(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                             const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                             const int64_t* env_inds, int64_t slots, int n_envs, const float* online, const float* target,
                                             double gamma, float* grads, float* scalars_out, float* target_q_out, float* td_target_out, int M,
                                             int O, int n_actions, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_dqn_td_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                                 const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                 const int64_t* env_inds, int64_t slots, int n_envs, const float* online,
                                                 const float* target, double gamma, float* grads, float* scalars_out, float* target_q_out,
                                                 float* td_target_out, int M, int O, int n_actions);
/* c51.py's update: next_pmfs = target.get_action(next_obs), the categorical projection onto atoms (each target atom adds its d_m_l
 * terms and then its d_m_u terms in ascending source order, as the reference's two index_add_ calls per row do), old_pmfs =
 * online.get_action(obs, action), loss = mean(-(target_pmfs * old_pmfs.clamp(1e-5, 1 - 1e-5).log()).sum(-1)); the backward passes no
 * gradient where the clamp is active.  grads is OVERWRITTEN; scalars_out (2) = {loss, mean (old_pmfs * atoms).sum(1)};
 * next_pmfs_out and target_pmfs_out (M, n_atoms) may be NULL.  Two launches. */
MI355PPO_API size_t mi355ppo_c51_workspace_bytes(int M, int O, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_c51_fwd_bwd_f32(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                          const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                          const int64_t* env_inds, int64_t slots, int n_envs, const float* online, const float* target,
                                          const float* atoms, double gamma, double v_min, double v_max, float* grads, float* scalars_out,
                                          float* next_pmfs_out, float* target_pmfs_out, int M, int O, int n_actions, int n_atoms,
                                          void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_c51_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                              const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                              const int64_t* env_inds, int64_t slots, int n_envs, const float* online, const float* target,
                                              const float* atoms, double gamma, double v_min, double v_max, float* grads,
                                              float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M, int O, int n_actions,
                                              int n_atoms);

/* ---- Atari DQN / C51 (added under ABI 2.7.1, csrc/dqn_atari.hip; reference: cleanrl/dqn_atari.py, cleanrl/c51_atari.py and
 * ReplayBuffer(optimize_memory_usage=True) of cleanrl_utils/buffers.py) ----
 * The frame ring is ONE u8 array (slots, n_envs, 84, 84, 4), channels-last and 4-byte aligned, beside ring_actions (slots, n_envs) int64,
 * ring_rewards and ring_dones (slots, n_envs) f32.  Every offset into it is 64-bit.  The head is Linear(512, n_actions * n_atoms) on the
 * post-ReLU output h of Linear(3136, 512): w (n_actions * n_atoms, 512) and b as torch keeps them; n_atoms = 1 is dqn_atari.py's head.
 * hidden == 512, 2 <= n_actions <= 18, 1 <= n_atoms <= 101, n_actions * n_atoms <= 1024, 1 <= rows <= 1024 (the C51 update needs
 * n_atoms >= 2); anything else is MI355PPO_EINVAL before any launch.  td_target, the projection, exp / log and every accumulation order
 * are those of the DQN / C51 section above.  No entry point allocates or synchronises, none uses atomics, all can be captured; every
 * *_cpu twin returns the device's bits (csrc/dqn_atari_rows.h).
 *
 * replay_add: the memory-optimised add.  obs / next_obs (n_envs, 4, 84, 84) u8 as the env gives them -> slot pos and slot
 * (pos + 1) % slots, one 4-byte store per pixel; with slots == 1 next_obs alone is written (it is what the reference leaves).  actions
 * (n_envs) int64, rewards, dones (n_envs) f32 -> slot pos.  One launch. */
MI355PPO_API int mi355ppo_replay_add_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                        const float* dones, uint8_t* ring_frames, int64_t* ring_actions, float* ring_rewards,
                                        float* ring_dones, int64_t pos, int64_t slots, int n_envs, void* stream);
MI355PPO_API int mi355ppo_replay_add_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                            const float* dones, uint8_t* ring_frames, int64_t* ring_actions, float* ring_rewards,
                                            float* ring_dones, int64_t pos, int64_t slots, int n_envs);
/* replay_gather: frames_out (2M, 84, 84, 4) u8, 4-byte aligned: rows m < M the frames (batch_inds[m], env_inds[m]), rows M + m the frames
 * ((batch_inds[m] + 1) % slots, env_inds[m]); actions_out (M) int64, rewards_out, dones_out (M) f32.  Indices are clamped into the
 * ring.  One launch. */
MI355PPO_API int mi355ppo_replay_gather_u8(const uint8_t* ring_frames, const int64_t* ring_actions, const float* ring_rewards,
                                           const float* ring_dones, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                           int n_envs, uint8_t* frames_out, int64_t* actions_out, float* rewards_out, float* dones_out, int M,
                                           void* stream);
MI355PPO_API int mi355ppo_replay_gather_u8_cpu(const uint8_t* ring_frames, const int64_t* ring_actions, const float* ring_rewards,
                                               const float* ring_dones, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                               int n_envs, uint8_t* frames_out, int64_t* actions_out, float* rewards_out, float* dones_out,
                                               int M);
/* head_act: actions_out (N, int64) = argmax_a q(h)[a] with mi355ppo_dqn_act_f32's semantics (a tie to the lowest index, a NaN is the
 * maximum, n_atoms > 1: C51's get_action in ascending atom order); q_out (N, n_actions) may be NULL.  Two launches (the product spread
 * over rows x output tiles, then the argmax). */
MI355PPO_API size_t mi355ppo_dqn_head_act_workspace_bytes(int N, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_dqn_head_act_f32(const float* h, const float* w, const float* b, const float* atoms, int64_t* actions_out,
                                           float* q_out, int N, int hidden, int n_actions, int n_atoms, void* workspace,
                                           size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_dqn_head_act_f32_cpu(const float* h, const float* w, const float* b, const float* atoms, int64_t* actions_out,
                                               float* q_out, int N, int hidden, int n_actions, int n_atoms);
/* The updates given h = online trunk(obs) and h_next = target trunk(next_obs), both (M, 512) post-ReLU, and the gathered actions (int64,
 * clamped into [0, n_actions)), rewards and dones.  dh (M, 512) is d loss / d h; dw (n_actions * n_atoms, 512) and db are OVERWRITTEN:
 * the taken actions' rows summed over the batch rows in ascending order, every other row zero.  scalars_out (2) = {loss, mean q}.
 * The optional outputs are the target side's: target_q_out (M, n_actions) and td_target_out (M), or next_pmfs_out and
 * target_pmfs_out (M, n_atoms).  Three launches; mi355ppo_dqn_head_workspace_bytes serves both (n_atoms = 1 for the TD update). */
MI355PPO_API size_t mi355ppo_dqn_head_workspace_bytes(int M, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_dqn_head_td_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                                                  const float* b_target, const int64_t* actions, const float* rewards, const float* dones,
                                                  double gamma, float* dh, float* dw, float* db, float* scalars_out, float* target_q_out,
                                                  float* td_target_out, int M, int hidden, int n_actions, void* workspace,
                                                  size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_dqn_head_td_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b,
                                                      const float* w_target, const float* b_target, const int64_t* actions,
                                                      const float* rewards, const float* dones, double gamma, float* dh, float* dw, float* db,
                                                      float* scalars_out, float* target_q_out, float* td_target_out, int M, int hidden,
                                                      int n_actions);
MI355PPO_API int mi355ppo_c51_head_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                                               const float* b_target, const float* atoms, const int64_t* actions, const float* rewards,
                                               const float* dones, double gamma, double v_min, double v_max, float* dh, float* dw, float* db,
                                               float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M, int hidden,
                                               int n_actions, int n_atoms, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_c51_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                                                   const float* b_target, const float* atoms, const int64_t* actions, const float* rewards,
                                                   const float* dones, double gamma, double v_min, double v_max, float* dh, float* dw,
                                                   float* db, float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M,
                                                   int hidden, int n_actions, int n_atoms);

/* ---- Rainbow: prioritized n-step replay and noisy layers (added under ABI 2.7.1, csrc/rainbow.hip; reference: cleanrl/rainbow_atari.py's
 * PrioritizedReplayBuffer, SumSegmentTree and NoisyLinear) ----
 * The buffer in device memory: ring_obs and ring_next_obs (slots, 84, 84, 4) u8, channels-last and 4-byte aligned, two separate rings;
 * ring_actions (slots) int64, ring_rewards and ring_dones (slots) f32; tree (2 * slots - 1) f32 in the reference's heap layout (node p has
 * the children 2p + 1 and 2p + 2, leaf i is word slots - 1 + i; an inner node is the f32 sum of its two children); state (2) f32 =
 * {max_priority, beta}; size (1) int64.  The caller initialises state to {1, beta} and zeroes the rest.  Every offset is 64-bit.
 * x ** alpha and x ** -beta are pow((double)x, (double)(float)exponent) rounded once to f32: NumPy raises a float32 to a Python float
 * with powf(x, (float)exponent), and the exact power is within 1 ulp of both.  Everything that does not pass through a power is
 * bit-equal between device, twin and reference.  1 <= rows <= 1024; anything else is MI355PPO_EINVAL before any launch.  No entry point
 * allocates or synchronises, none uses atomics, all can be captured.
 *
 * per_add: one n-step transition into slot pos: obs / next_obs (1, 4, 84, 84) u8 as the env gives them, action (1) int64, reward (1)
 * (the n-step return) and done (1) f32, all in device memory.  Leaf pos becomes max_priority ** alpha, its ancestors are recomputed,
 * size becomes min(size + 1, slots).  One launch. */
MI355PPO_API int mi355ppo_rainbow_per_add_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* action, const float* reward,
                                             const float* done, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                             float* ring_rewards, float* ring_dones, float* tree, float* state, int64_t* size, int64_t pos,
                                             int64_t slots, double alpha, void* stream);
MI355PPO_API int mi355ppo_rainbow_per_add_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* action, const float* reward,
                                                 const float* done, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                                 float* ring_rewards, float* ring_dones, float* tree, float* state, int64_t* size,
                                                 int64_t pos, int64_t slots, double alpha);
/* per_sample: PrioritizedReplayBuffer.sample's indices and weights.  u (B) f64: one np.random.random_sample() per sample, which is what
 * each of the reference's np.random.uniform(a, b) draws.  segment = tree[0] / B, a = segment * i, b = segment * (i + 1) in f32; value =
 * a + (b - a) * u in f64, rounded to f32 (NumPy compares and subtracts a Python float against a float32 in float32); the walk takes
 * the left child while value <= tree[left], else subtracts it and goes right.  weights = (size * p / tree[0]) ** -beta / their maximum
 * (a NaN wins).  indices_out (B) int64, weights_out (B) f32.  One launch of one workgroup. */
MI355PPO_API int mi355ppo_rainbow_per_sample(const double* u, const float* tree, const float* state, const int64_t* size, int64_t slots,
                                             int64_t* indices_out, float* weights_out, int B, void* stream);
MI355PPO_API int mi355ppo_rainbow_per_sample_cpu(const double* u, const float* tree, const float* state, const int64_t* size, int64_t slots,
                                                 int64_t* indices_out, float* weights_out, int B);
/* per_gather: frames_out (2M, 84, 84, 4) u8, 4-byte aligned: rows m < M the obs frames of slots indices[m], rows M + m their next_obs
 * frames; actions_out (M) int64, rewards_out, dones_out (M) f32.  Indices are clamped into the ring.  One launch. */
MI355PPO_API int mi355ppo_rainbow_per_gather_u8(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                const float* ring_rewards, const float* ring_dones, const int64_t* indices, int64_t slots,
                                                uint8_t* frames_out, int64_t* actions_out, float* rewards_out, float* dones_out, int M,
                                                void* stream);
MI355PPO_API int mi355ppo_rainbow_per_gather_u8_cpu(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                    const float* ring_rewards, const float* ring_dones, const int64_t* indices,
                                                    int64_t slots, uint8_t* frames_out, int64_t* actions_out, float* rewards_out,
                                                    float* dones_out, int M);
/* per_update: update_priorities.  p = |loss_per_sample| + (float)eps; max_priority = max(max_priority, max p) (a NaN maximum leaves it);
 * leaf indices[i] (clamped into the ring) becomes p[i] ** alpha, of duplicate indices the highest batch position stays, as the
 * reference's serial loop leaves it; every ancestor of a written leaf is recomputed, level by level from the deepest tree level.  One
 * launch of one workgroup. */
MI355PPO_API int mi355ppo_rainbow_per_update(const int64_t* indices, const float* loss_per_sample, float* tree, float* state, int64_t slots,
                                             double alpha, double eps, int B, void* stream);
MI355PPO_API int mi355ppo_rainbow_per_update_cpu(const int64_t* indices, const float* loss_per_sample, float* tree, float* state,
                                                 int64_t slots, double alpha, double eps, int B);
/* The four NoisyLinear layers of NoisyDuelingDistributionalNetwork in one launch.  params / grads: the head's parameters (gradients) as
 * one flat buffer in torch's registration order: per layer weight_mu, weight_sigma, bias_mu, bias_sigma; layers value_head.0 (512, 3136),
 * value_head.2 (n_atoms, 512), advantage_head.0 (512, 3136), advantage_head.2 (n_actions * n_atoms, 512).  eps: per layer
 * weight_epsilon, bias_epsilon in the same layer order (reset_noise()'s).  effective: W_fc (1024, 3136) | b_fc (1024) |
 * W_out ((n_actions + 1) * n_atoms, 512) | b_out, the value stream's rows first.  noisy_count(which = 0): the elements of eps and of
 * effective; (which = 1): of params; 0 outside 2 <= n_actions <= 18, 2 <= n_atoms <= 101, (n_actions + 1) * n_atoms <= 1024.
 * compose: effective = mu + sigma * eps (an f32 multiply, then an add: torch's bits).  grad: dmu = g, dsigma = g * eps of the effective
 * buffer's gradient g, OVERWRITING grads (autograd's bits). */
MI355PPO_API int64_t mi355ppo_rainbow_noisy_count(int n_actions, int n_atoms, int which);
MI355PPO_API int mi355ppo_rainbow_noisy_compose_f32(const float* params, const float* eps, float* effective, int n_actions, int n_atoms,
                                                    void* stream);
MI355PPO_API int mi355ppo_rainbow_noisy_compose_f32_cpu(const float* params, const float* eps, float* effective, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_rainbow_noisy_grad_f32(const float* effective_grad, const float* eps, float* grads, int n_actions, int n_atoms,
                                                 void* stream);
MI355PPO_API int mi355ppo_rainbow_noisy_grad_f32_cpu(const float* effective_grad, const float* eps, float* grads, int n_actions, int n_atoms);
/* The noisy dueling distributional head behind the trunk.  h (rows, 1024): the post-ReLU output of ONE Linear(3136, 1024) that holds both
 * streams' hidden layers (the effective W_fc / b_fc above), the value stream's 512 columns first.  w_out ((n_actions + 1) * n_atoms, 512)
 * and b_out: the effective output layer, the value stream's n_atoms rows first; they read h[:, :512], the advantage rows h[:, 512:].
 * Every dot product starts at 0.0f and adds in ascending index, then the bias.  q_atoms = (v + adv) - mean_a adv (ascending sum / n), a
 * softmax over each action's atoms, expectations against support, argmax under mi355ppo_dqn_act_f32's tie and NaN rules.
 * 1 <= rows <= 1024, 2 <= n_actions <= 18, 2 <= n_atoms <= 101, (n_actions + 1) * n_atoms <= 1024; anything else is MI355PPO_EINVAL.
 * head_act: actions_out (N) int64; q_out (N, n_actions) may be NULL.  Two launches. */
MI355PPO_API size_t mi355ppo_rainbow_head_act_workspace_bytes(int N, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_rainbow_head_act_f32(const float* h, const float* w_out, const float* b_out, const float* support,
                                               int64_t* actions_out, float* q_out, int N, int n_actions, int n_atoms, void* workspace,
                                               size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_rainbow_head_act_f32_cpu(const float* h, const float* w_out, const float* b_out, const float* support,
                                                   int64_t* actions_out, float* q_out, int N, int n_actions, int n_atoms);
/* head_fwd_bwd: rainbow_atari.py's update behind the trunks in three launches.  Three passes: online on h (obs), online on h_next
 * (next_obs), target on h_next_target (next_obs).  The online expectations on next_obs pick best_actions, next_pmfs is the target's
 * distribution there; the projection is the script's own: next_atoms = r + (gamma_n * support) * (1 - d) with gamma_n =
 * (float)(gamma ** n_step), b = (clamp(next_atoms) - v_min) / (float)((v_max - v_min) / (n_atoms - 1)), d_m_l = (u + (l == b) - b) * p,
 * d_m_u = (b - l) * p, added in index_add_'s serial order.  loss_per_sample (M) = -sum target * log(clamp(pred, 1e-5, 1 - 1e-5));
 * scalars_out (2) = {mean(loss_per_sample * weights), mean sum pred * support}.  dh (M, 1024) is d loss / d h; dw_out and db_out are
 * OVERWRITTEN with the effective output layer's gradient (every row: the advantage mean reaches every action).  The optional outputs:
 * best_actions_out (M) int64, next_pmfs_out and target_pmfs_out (M, n_atoms). */
MI355PPO_API size_t mi355ppo_rainbow_head_workspace_bytes(int M, int n_actions, int n_atoms);
MI355PPO_API int mi355ppo_rainbow_head_fwd_bwd_f32(const float* h, const float* h_next, const float* h_next_target, const float* w_out,
                                                   const float* b_out, const float* w_out_target, const float* b_out_target,
                                                   const float* support, const int64_t* actions, const float* rewards, const float* dones,
                                                   const float* weights, double gamma_n, double v_min, double v_max, float* dh, float* dw_out,
                                                   float* db_out, float* scalars_out, float* loss_per_sample, int64_t* best_actions_out,
                                                   float* next_pmfs_out, float* target_pmfs_out, int M, int n_actions, int n_atoms,
                                                   void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_rainbow_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* h_next_target, const float* w_out,
                                                       const float* b_out, const float* w_out_target, const float* b_out_target,
                                                       const float* support, const int64_t* actions, const float* rewards,
                                                       const float* dones, const float* weights, double gamma_n, double v_min, double v_max,
                                                       float* dh, float* dw_out, float* db_out, float* scalars_out, float* loss_per_sample,
                                                       int64_t* best_actions_out, float* next_pmfs_out, float* target_pmfs_out, int M,
                                                       int n_actions, int n_atoms);

/* ---- Discrete SAC on Atari (added under ABI 2.7.1, csrc/sac_atari.hip; reference: cleanrl/sac_atari.py and the plain ReplayBuffer of
 * cleanrl_utils/buffers.py, which sac_atari.py builds without optimize_memory_usage) ----
 * The buffer is TWO u8 rings ring_obs and ring_next_obs (slots, n_envs, 84, 84, 4), channels-last and 4-byte aligned, beside
 * ring_actions (slots, n_envs) int64, ring_rewards and ring_dones (slots, n_envs) f32.  Every offset into a ring is 64-bit.  Five heads
 * Linear(512, n_actions) sit on the post-ReLU outputs h of five Linear(3136, 512): the actor's fc_logits, fc_q of qf1 / qf2 and of their
 * targets; every w is (n_actions, 512) and every b (n_actions) as torch keeps them.  hidden == 512, 2 <= n_actions <= 18, 1 <= rows <=
 * 1024; anything else is MI355PPO_EINVAL before any launch.  alpha is ONE f32 in the caller's memory (device memory for the device entry
 * points: exp(log_alpha) as mi355ppo_sac_alpha_f32 leaves it, or args.alpha).  Every dot product starts at 0.0f and adds in ascending
 * index, then the bias; the softmax is exp(z - max) / sum and logp = (z - max) - log(sum) with the exp / log of the SAC section, sums in
 * ascending action order.  No entry point allocates or synchronises, none uses atomics, all can be captured; every *_cpu twin returns
 * the device's bits (csrc/sac_atari_rows.h).
 *
 * replay_add2: `rb.add(obs, real_next_obs, actions, rewards, terminations, infos)`.  obs / next_obs (n_envs, 4, 84, 84) u8 as the env
 * gives them -> ring_obs and ring_next_obs at slot pos, one 4-byte store per pixel; actions (n_envs) int64, rewards, dones (n_envs) f32
 * -> slot pos.  One launch. */
MI355PPO_API int mi355ppo_replay_add2_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                         const float* dones, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                         float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int n_envs, void* stream);
MI355PPO_API int mi355ppo_replay_add2_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                             const float* dones, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                             float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int n_envs);
/* replay_gather2: `rb.sample`'s `_get_samples`.  frames_out (2M, 84, 84, 4) u8, 4-byte aligned: rows m < M the ring_obs frames
 * (batch_inds[m], env_inds[m]), rows M + m the ring_next_obs frames at the same place; actions_out (M) int64, rewards_out, dones_out
 * (M) f32.  Indices are clamped into the ring.  One launch. */
MI355PPO_API int mi355ppo_replay_gather2_u8(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                            const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                            const int64_t* env_inds, int64_t slots, int n_envs, uint8_t* frames_out, int64_t* actions_out,
                                            float* rewards_out, float* dones_out, int M, void* stream);
MI355PPO_API int mi355ppo_replay_gather2_u8_cpu(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                const int64_t* env_inds, int64_t slots, int n_envs, uint8_t* frames_out,
                                                int64_t* actions_out, float* rewards_out, float* dones_out, int M);
/* sacd_head_act: `Actor.get_action`'s `policy_dist.sample()` on h (N, 512).  actions_out (N) int64 = argmax_a probs[a] / noise_exp1[a]
 * (noise_exp1 (N, n_actions): the caller's Exp(1) draws; the first maximum wins, a NaN never does): one draw of torch.multinomial's
 * rule, as mi355ppo_categorical_sample_f32 draws it.  probs_out (N, n_actions) may be NULL.  Two launches. */
MI355PPO_API size_t mi355ppo_sacd_head_act_workspace_bytes(int N, int n_actions);
MI355PPO_API int mi355ppo_sacd_head_act_f32(const float* h, const float* w, const float* b, const float* noise_exp1, int64_t* actions_out,
                                            float* probs_out, int N, int hidden, int n_actions, void* workspace, size_t workspace_bytes,
                                            void* stream);
MI355PPO_API int mi355ppo_sacd_head_act_f32_cpu(const float* h, const float* w, const float* b, const float* noise_exp1, int64_t* actions_out,
                                                float* probs_out, int N, int hidden, int n_actions);
/* sacd_critic_fwd_bwd: `# CRITIC training` behind the trunks.  h_q1 / h_q2: qf1 / qf2 on obs; h_pi_next / h_q1t_next / h_q2t_next: the
 * actor and the two target critics on next_obs; all (M, 512).  Per row: p, logp of the actor's next logits; V = sum_a p_a *
 * (min(q1t_a, q2t_a) - alpha * logp_a) (torch.min: a NaN wins); y = rewards + ((1 - dones) * gamma) * V; both critics' q at the taken
 * action (int64, clamped into [0, n_actions)); F.mse_loss rows with the gradient (2 / M) * (q - y).  dh1 / dh2 (M, 512) are d qf_loss /
 * d h_q1, d h_q2; dw1 / db1 / dw2 / db2 are OVERWRITTEN: the taken actions' rows summed over the batch rows in ascending order, every
 * other row zero.  scalars_out (4) = {qf1_loss, qf2_loss, mean qf1_a_values, mean qf2_a_values} (f64 folds).  v_out, y_out (M): V and y,
 * optional.  Four launches (two forwards of three and two heads, the rows, the weight gradients with the scalars). */
MI355PPO_API size_t mi355ppo_sacd_critic_workspace_bytes(int M, int n_actions);
MI355PPO_API int mi355ppo_sacd_critic_fwd_bwd_f32(const float* h_q1, const float* h_q2, const float* h_pi_next, const float* h_q1t_next,
                                                  const float* h_q2t_next, const float* w_q1, const float* b_q1, const float* w_q2,
                                                  const float* b_q2, const float* w_pi, const float* b_pi, const float* w_q1t,
                                                  const float* b_q1t, const float* w_q2t, const float* b_q2t, const int64_t* actions,
                                                  const float* rewards, const float* dones, const float* alpha, double gamma, float* dh1,
                                                  float* dh2, float* dw1, float* db1, float* dw2, float* db2, float* scalars_out, float* v_out,
                                                  float* y_out, int M, int hidden, int n_actions, void* workspace, size_t workspace_bytes,
                                                  void* stream);
MI355PPO_API int mi355ppo_sacd_critic_fwd_bwd_f32_cpu(const float* h_q1, const float* h_q2, const float* h_pi_next, const float* h_q1t_next,
                                                      const float* h_q2t_next, const float* w_q1, const float* b_q1, const float* w_q2,
                                                      const float* b_q2, const float* w_pi, const float* b_pi, const float* w_q1t,
                                                      const float* b_q1t, const float* w_q2t, const float* b_q2t, const int64_t* actions,
                                                      const float* rewards, const float* dones, const float* alpha, double gamma, float* dh1,
                                                      float* dh2, float* dw1, float* db1, float* dw2, float* db2, float* scalars_out,
                                                      float* v_out, float* y_out, int M, int hidden, int n_actions);
/* sacd_actor_fwd_bwd: `# ACTOR training` behind the trunks.  h_pi / h_q1 / h_q2: the actor and the two critics (after their Adam step)
 * on obs.  Per row: t_a = alpha * logp_a - min(q1_a, q2_a), s = sum_a p_a * t_a; actor_loss_out (1) = sum_r s_r / (M n) (an f64 fold);
 * dz_j = p_j * (t_j - s) / (M n); dh (M, 512) = dz w_pi; dw (n_actions, 512) and db are OVERWRITTEN with the dense gradient, batch rows
 * ascending.  entropy_rows_out (M): e_r = sum_a p_a * (logp_a + target_entropy) / n_actions, so that mi355ppo_sac_alpha_f32 on it with
 * target_entropy 0 is the script's alpha_loss, its gradient and its Adam step.  Three launches. */
MI355PPO_API size_t mi355ppo_sacd_actor_workspace_bytes(int M, int n_actions);
MI355PPO_API int mi355ppo_sacd_actor_fwd_bwd_f32(const float* h_pi, const float* h_q1, const float* h_q2, const float* w_pi, const float* b_pi,
                                                 const float* w_q1, const float* b_q1, const float* w_q2, const float* b_q2, const float* alpha,
                                                 double target_entropy, float* dh, float* dw, float* db, float* entropy_rows_out,
                                                 float* actor_loss_out, int M, int hidden, int n_actions, void* workspace,
                                                 size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_sacd_actor_fwd_bwd_f32_cpu(const float* h_pi, const float* h_q1, const float* h_q2, const float* w_pi,
                                                     const float* b_pi, const float* w_q1, const float* b_q1, const float* w_q2,
                                                     const float* b_q2, const float* alpha, double target_entropy, float* dh, float* dw,
                                                     float* db, float* entropy_rows_out, float* actor_loss_out, int M, int hidden,
                                                     int n_actions);

/* ---------------------------------------------------------------------------------------------
 * QDagger head (cleanrl/qdagger_dqn_atari_impalacnn.py:294-306, 403-415; csrc/qdagger.hip, row math csrc/qdagger_rows.h): Linear(256, n)
 * of the IMPALA student behind mi355ppo_impala84_fwd_u8 and the torch Linear(3872, 256).
 *   act      actions_out[r] = argmax_a q[r, a] (ties to the lowest index, NaN is the maximum); q_out (N, n) optional.  Two launches.
 *   fwd_bwd  td_target = r + gamma max_j q_target(h_next)[j] (1 - d);  q_loss = mean (td_target - q[r, a_r])^2;  with t = teacher_q / T,
 *            s = q / T:  distill = SUM over rows and actions of -softmax(t) (log_softmax(s) - log_softmax(t));
 *            loss = q_loss + distill_coeff * distill.  OVERWRITES dh (M, 256), dw (n, 256), db (n) with the gradient of loss
 *            (dq is dense over the actions: dW[j, k] sums all rows in ascending r); scalars_out (4) = {loss, q_loss, distill,
 *            mean q[r, a_r]}; target_q_out (M, n) / td_target_out (M) optional.  Three launches, plain f32, no atomics.
 * Limits: hidden == 256, 2 <= n_actions <= 18, 1 <= rows <= 1024, temperature > 0; anything else returns MI355PPO_EINVAL before any
 * launch.  workspace: the *_workspace_bytes functions' size, 16-byte aligned. */
MI355PPO_API size_t mi355ppo_qdagger_head_act_workspace_bytes(int N, int n_actions);
MI355PPO_API int mi355ppo_qdagger_head_act_f32(const float* h, const float* w, const float* b, int64_t* actions_out, float* q_out, int N,
                                               int hidden, int n_actions, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_qdagger_head_act_f32_cpu(const float* h, const float* w, const float* b, int64_t* actions_out, float* q_out, int N,
                                                   int hidden, int n_actions);
MI355PPO_API size_t mi355ppo_qdagger_head_workspace_bytes(int M, int n_actions);
MI355PPO_API int mi355ppo_qdagger_head_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                                                   const float* b_target, const float* teacher_q, const int64_t* actions, const float* rewards,
                                                   const float* dones, double gamma, double temperature, double distill_coeff, float* dh,
                                                   float* dw, float* db, float* scalars_out, float* target_q_out, float* td_target_out, int M,
                                                   int hidden, int n_actions, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_qdagger_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b,
                                                       const float* w_target, const float* b_target, const float* teacher_q,
                                                       const int64_t* actions, const float* rewards, const float* dones, double gamma,
                                                       double temperature, double distill_coeff, float* dh, float* dw, float* db,
                                                       float* scalars_out, float* target_q_out, float* td_target_out, int M, int hidden,
                                                       int n_actions);

/* ---------------------------------------------------------------------------------------------
 * Random Network Distillation (cleanrl/ppo_rnd_envpool.py; csrc/rnd.hip, row math in csrc/rnd_rows.h): what the learner does around
 * the two RND networks.  Every *_cpu twin takes host pointers and returns the device's bits.  No entry point allocates or synchronises
 * (all are capturable); no atomics: every result is a pure function of the inputs.
 *
 * A FRAME is the 84 x 84 = 7056 newest-frame bytes of an observation row of row_bytes bytes (B rows at src), pixel p at byte
 * byte_offset + pixel_stride * p of the row: pixel_stride 4 (the learner's NHWC rows of 4 stacked frames, byte_offset 3: whole 4-byte
 * pixels are read, src 4-byte aligned, row_bytes a multiple of 4) or 1 (planar NCHW rows, byte_offset 3 * 7056).
 *
 * normalize (ppo_rnd_envpool.py:365-370, :449-454): out (M, 1, 84, 84) f32, out[r, p] = (float)clip(((double)x - mean[p]) / sd[p], -5, 5)
 * with x the frame pixel of row idx[r] (idx NULL: row r; an index out of range is clamped): the reference's float64 arithmetic with
 * one rounding to f32.  mean / sd: float64[7056], sd = sqrt(var) formed once by the caller. */
MI355PPO_API int mi355ppo_rnd_normalize_u8_f32(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                               const int64_t* idx, const double* mean, const double* sd, float* out, int M, void* stream);
MI355PPO_API int mi355ppo_rnd_normalize_u8_f32_cpu(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                                   const int64_t* idx, const double* mean, const double* sd, float* out, int M);
/* Per-pixel batch moments of the frame over all B rows, exact: sums (uint64[2][7056]) is OVERWRITTEN with S1[p] = sum x and
 * S2[p] = sum x^2 (32-bit partials over slabs of 256 rows, 255^2 * 256 < 2^32, folded in 64 bits).  The caller forms mean = S1 / B and
 * var = (B S2 - S1^2) / B^2; the numerator is exact in 64-bit integers for B < 2^24 -- a larger B returns MI355PPO_EINVAL.
 * workspace: mi355ppo_rnd_obs_moments_workspace_bytes(B) bytes, 16-byte aligned.  Two launches. */
MI355PPO_API size_t mi355ppo_rnd_obs_moments_workspace_bytes(int64_t B);
MI355PPO_API int mi355ppo_rnd_obs_moments_u8(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                             uint64_t* sums, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_rnd_obs_moments_u8_cpu(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                                 uint64_t* sums);
/* Intrinsic reward (:373): out[n] = sum_f (target[n, f] - predict[n, f])^2 / 2 over F == 512 features (any other F: MI355PPO_EINVAL), in
 * one fixed order (per lane 8 terms, then a 64-lane butterfly).  Feature rows 16-byte aligned. */
MI355PPO_API int mi355ppo_rnd_intrinsic_reward_f32(const float* target, const float* predict, float* out, int N, int F, void* stream);
MI355PPO_API int mi355ppo_rnd_intrinsic_reward_f32_cpu(const float* target, const float* predict, float* out, int N, int F);
/* Intrinsic-reward scaling (:390-400) in one call.  The reference iterates over curiosity_rewards.T, so its RewardForwardFilter runs
 * ALONG THE ENV AXIS with a T-vector of state that persists across rollouts; reproduced as written: for n = 0 .. N-1,
 * rewems[t] = fl32(fl32(rewems[t] * (float)gamma) + curiosity[t][n]) (T independent scans; an all-zero rewems is the reference's first
 * call).  Over the N x T filtered values: mean and population variance in float64 (per scan in ascending n, the scans in ascending t),
 * RunningMeanStd.update_from_moments(mean, var, N) on stats3 = (mean, var, count) in float64 in the host class's operation order, then
 * curiosity (T, N) is OVERWRITTEN with curiosity / (float)sqrt(var_new).  filtered_out (T, N), optional: the filtered values.
 * 1 <= T <= 1024.  One launch of one workgroup. */
MI355PPO_API int mi355ppo_rnd_reward_filter_f32(float* curiosity, float* rewems, double* stats3, float* filtered_out, int T, int N, double gamma,
                                                void* stream);
MI355PPO_API int mi355ppo_rnd_reward_filter_f32_cpu(float* curiosity, float* rewems, double* stats3, float* filtered_out, int T, int N,
                                                    double gamma);
/* The two loss terms of a minibatch that the fused PPO loss does not cover (:463-472, :512), forward and backward, on predict / target
 * (M, 512), uniform draws u (M), v_int (M) and int_returns (B rows) gathered by mb_inds (M; clamped):
 *   mask_m = u_m < (float)update_proportion, c = max(sum mask, 1)
 *   scalars_out[0] = 0.5 * mean_m (v_int - R)^2                 scalars_out[1] = sum_m mask_m mean_f (predict - target)^2 / c
 *   d_v_int[m] = (v_int - R) * (float)(vf_coef / M)             d_predict[m, f] = mask_m * 2 (predict - target) * (float)(1 / (512 c))
 * (the gradients of vf_coef * scalars_out[0] + scalars_out[1]); the scalars are summed in f64 in a fixed order.  F == 512.
 * workspace: mi355ppo_rnd_loss_workspace_bytes(M) bytes, 16-byte aligned.  Three launches. */
MI355PPO_API size_t mi355ppo_rnd_loss_workspace_bytes(int M);
MI355PPO_API int mi355ppo_rnd_loss_fwd_bwd_f32(const float* predict, const float* target, const float* u, double update_proportion,
                                               const float* v_int, const float* int_returns, const int64_t* mb_inds, int64_t B, double vf_coef,
                                               float* scalars_out, float* d_predict, float* d_v_int, int M, int F, void* workspace,
                                               size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_rnd_loss_fwd_bwd_f32_cpu(const float* predict, const float* target, const float* u, double update_proportion,
                                                   const float* v_int, const float* int_returns, const int64_t* mb_inds, int64_t B,
                                                   double vf_coef, float* scalars_out, float* d_predict, float* d_v_int, int M, int F);

/* ---------------------------------------------------------------------------------------------
 * Phasic Policy Gradient, the auxiliary phase (cleanrl/ppg_procgen.py:421-474; csrc/ppg.hip, row math in csrc/ppg_rows.h).  Every
 * *_cpu twin takes host pointers and returns the device's bits.  No entry point allocates or synchronises (all are capturable); no
 * atomics: every dot product and every sum over rows runs in one fixed order.
 *
 * The auxiliary buffers are aux_obs (T, R, row_bytes) u8, aux_pi (T, R, A) f32 and aux_returns (T, R) f32; a minibatch is the n whole
 * rollouts cols (int64[n], distinct; an entry outside [0, R) is clamped), and its FLAT ROW t * n + i is (t, cols[i]) -- flatten01 over
 * (T, n).  All offsets into the three buffers are 64-bit.  hidden must be 256 and 2 <= A <= 30 (A + 2 outputs fit one 32-output tile):
 * anything else returns MI355PPO_EINVAL before any launch.
 *
 * gather: out (T * n, row_bytes) f32 = byte / 255 (correctly rounded: mi355ppo_obs_u8_to_f32's expression).  row_bytes a multiple of 4,
 * aux_obs 4-byte and out 16-byte aligned.  One launch. */
MI355PPO_API int mi355ppo_ppg_aux_gather_u8_f32(const unsigned char* aux_obs, const int64_t* cols, float* out, int T, int n, int64_t R,
                                                int64_t row_bytes, void* stream);
MI355PPO_API int mi355ppo_ppg_aux_gather_u8_f32_cpu(const unsigned char* aux_obs, const int64_t* cols, float* out, int T, int n, int64_t R,
                                                    int64_t row_bytes);
/* The old policy (:424-433): z = h w^T + b on h (T * n, 256), then (z - max) - log sum exp(z - max), written into aux_pi[t, cols[i], :].
 * T * n <= 65,536.  One launch. */
MI355PPO_API int mi355ppo_ppg_old_logits_f32(const float* h, const float* w, const float* b, const int64_t* cols, float* aux_pi, int T, int n,
                                             int64_t R, int A, int hidden, void* stream);
MI355PPO_API int mi355ppo_ppg_old_logits_f32_cpu(const float* h, const float* w, const float* b, const int64_t* cols, float* aux_pi, int T, int n,
                                                 int64_t R, int A, int hidden);
/* The auxiliary minibatch (:449-462) on the hidden rows h (M = T * n <= 65,536, 256): the actor (wa (A, 256), ba), the critic (wc (256),
 * bc) and the auxiliary critic (wx, bx), forward and backward.  Per row: the old row is renormalised, p_old = exp(logp_old),
 * kl_row = sum_j p_old (logp_old - logp_new) with a term inf where p_new == 0 and then 0 where p_old == 0 (torch's rules),
 * d kl_row / d z_j = softmax(z)_j - p_old[j]; both value losses are 0.5 (v - ret)^2.
 *   scalars_out[3] = {mean kl_row, 0.5 mean (v_aux - ret)^2, 0.5 mean (v - ret)^2}: the un-divided means the reference logs
 *   dh (M, 256)    = the gradient of (aux_value_loss + beta_clone kl + real_value_loss) inv_accum through the actor and the auxiliary
 *                    critic (the critic reads detached features)
 *   dwa .. dbx     = the six head gradients of the same loss; accumulate 0 overwrites, 1 adds the folded value to what is there (one add
 *                    per element)
 * Rows are dealt to tiles of 8 whose partials are added in ascending tile order; the loss sums are f64.
 * workspace: mi355ppo_ppg_aux_workspace_bytes(M, A) bytes, 16-byte aligned.  Two launches. */
MI355PPO_API size_t mi355ppo_ppg_aux_workspace_bytes(int M, int A);
MI355PPO_API int mi355ppo_ppg_aux_fwd_bwd_f32(const float* h, const float* wa, const float* ba, const float* wc, const float* bc, const float* wx,
                                              const float* bx, const float* aux_pi, const float* aux_returns, const int64_t* cols, int T, int n,
                                              int64_t R, int A, int hidden, double beta_clone, double inv_accum, float* scalars_out, float* dh,
                                              float* dwa, float* dba, float* dwc, float* dbc, float* dwx, float* dbx, int accumulate,
                                              void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_ppg_aux_fwd_bwd_f32_cpu(const float* h, const float* wa, const float* ba, const float* wc, const float* bc,
                                                  const float* wx, const float* bx, const float* aux_pi, const float* aux_returns,
                                                  const int64_t* cols, int T, int n, int64_t R, int A, int hidden, double beta_clone,
                                                  double inv_accum, float* scalars_out, float* dh, float* dwa, float* dba, float* dwc, float* dbc,
                                                  float* dwx, float* dbx, int accumulate);
/* The auxiliary phase's optimiser step (:466-468) without a host round trip: mi355ppo_clip_adam_f32 (same norm reduction, clip
 * coefficient and element update) with step_head's bias corrections on [0, n_split) and step_tail's on [n_split, n) -- torch.optim.Adam
 * counts steps per parameter and the auxiliary value head only steps in this phase.  Gradients are zeroed.
 * workspace: mi355ppo_clip_adam_workspace_bytes(n).  Two launches. */
MI355PPO_API int mi355ppo_clip_adam_split_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t n_split,
                                              double grad_scale, double max_grad_norm, double lr, double beta1, double beta2, double eps,
                                              int64_t step_head, int64_t step_tail, float* total_norm_out, void* workspace, size_t workspace_bytes,
                                              void* stream);
MI355PPO_API int mi355ppo_clip_adam_split_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t n_split,
                                                  double grad_scale, double max_grad_norm, double lr, double beta1, double beta2, double eps,
                                                  int64_t step_head, int64_t step_tail, float* total_norm_out);

/* ---- ppo_pettingzoo_ma_atari.py on the NatureCNN trunk kernels (added under ABI 2.7.1; csrc/ma_atari.hip, csrc/conv1q.hip) -------------
 * The script's observations are (84, 84, 6) u8, pixel-interleaved: four stacked frames and two agent-indicator planes that are constant
 * over an observation and are NOT divided by 255 (:104).  A constant plane of value v adds v * sum_taps W1[n][c] to every output pixel of
 * conv1's channel n -- a bias per observation -- and its weight gradient is one number for all 64 taps.  So the rollout keeps the four
 * frame channels as (84, 84, 4) rows (what kernels Q and P read) and two indicator bytes per row.
 *
 * split: `frames` incoming (84, 84, 6) frames -> rows4 (frames, 84, 84, 4) and ind (frames, 2) = planes 4 / 5 at pixel (0, 0).  *flag gets
 * bit 0 OR-ed in when any byte of plane 4 / 5 differs from that plane's pixel (0, 0); it is never cleared here.  frames6 8-byte, rows4
 * 16-byte aligned.  One launch. */
MI355PPO_API int mi355ppo_ma_atari_split_u8(const uint8_t* frames6, uint8_t* rows4, uint8_t* ind, uint32_t* flag, int64_t frames, void* stream);
MI355PPO_API int mi355ppo_ma_atari_split_u8_cpu(const uint8_t* frames6, uint8_t* rows4, uint8_t* ind, uint32_t* flag, int64_t frames);
/* pack: W6 (32, 6, 8, 8) read in place -> kernel Q's pack of its channels 0 - 3 (mi355ppo_cnn_conv1q_pack_bytes(); the bytes of
 * mi355ppo_cnn_conv1q_pack on the contiguous [:, :4] slice) and tapsum (32, 2): S[n][j] = sum_{kh,kw} W6[n][4 + j][kh][kw], added in
 * double in tap order, rounded once.  One launch.  mi355ppo_cnn_conv1q_pack_cpu: the twin of mi355ppo_cnn_conv1q_pack. */
MI355PPO_API int mi355ppo_ma_atari_conv1_pack_f32(const float* W6, void* pack, float* tapsum, void* stream);
MI355PPO_API int mi355ppo_ma_atari_conv1_pack_f32_cpu(const float* W6, void* pack, float* tapsum);
MI355PPO_API int mi355ppo_cnn_conv1q_pack_cpu(const float* W, void* pack);
/* forward: mi355ppo_cnn_conv1q_fwd_bits / _amax on the (84, 84, 4) rows with the bias of image i and channel n
 *   fmaf(v5, S[n][1], fmaf(v4, S[n][0], bias[n])),  (v4, v5) = ind[2 s], ind[2 s + 1] as f32,  s = inds ? inds[i] : i
 * (all indicator bytes 0: the bits of the plain entry points).  ind: 2-byte aligned.  The twin serves both forms (mask_bits may be null;
 * it keeps no amax record); mi355ppo_cnn_conv1q_fwd_cpu is the twin of the plain kernel Q forward. */
MI355PPO_API int mi355ppo_ma_atari_conv1_fwd_bits(const void* src_u8, const int64_t* inds, const uint8_t* ind, const void* pack,
                                                  const float* tapsum, const float* bias, float* dst, uint32_t* mask_bits, int64_t images,
                                                  void* stream);
MI355PPO_API int mi355ppo_ma_atari_conv1_fwd_amax(const void* src_u8, const int64_t* inds, const uint8_t* ind, const void* pack,
                                                  const float* tapsum, const float* bias, float* dst, uint32_t* mask_bits, int64_t images,
                                                  uint32_t* dst_amax, void* stream);
MI355PPO_API int mi355ppo_ma_atari_conv1_fwd_cpu(const void* src_u8, const int64_t* inds, const uint8_t* ind, const void* pack,
                                                 const float* tapsum, const float* bias, float* dst, uint32_t* mask_bits, int64_t images);
MI355PPO_API int mi355ppo_cnn_conv1q_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                             uint32_t* mask_bits, int64_t images);
/* weight-gradient fold: dW6 (32, 6, 8, 8) is OVERWRITTEN: channels 0 - 3 = dW4 (32, 4, 8, 8), the layer-1 weight gradient of the rows
 * (mi355ppo_cnn_conv1_wgrad_f16x2 / mi355ppo_cnn_conv_wgrad_f32), every tap of channel 4 + j of output channel n =
 *   sum_i v_j(i) * sum_p dz1[i][p][n]
 * over dz1 (images, 20, 20, 32), accumulated in double in one fixed order (four images per partial, the partials in four interleaved
 * chains; no floating-point atomics: the same input gives the same bits; the twin follows the same order).
 * workspace: mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(images) bytes, 8-byte aligned.  Two launches. */
MI355PPO_API size_t mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(int64_t images);
MI355PPO_API int mi355ppo_ma_atari_conv1_wgrad_fold_f32(const float* dz1, const int64_t* inds, const uint8_t* ind, const float* dW4, float* dW6,
                                                        int64_t images, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(const float* dz1, const int64_t* inds, const uint8_t* ind, const float* dW4,
                                                            float* dW6, int64_t images);

/* ---- The LayerNorm NatureCNN of pqn_atari_envpool.py (added under ABI 2.7.1; csrc/layernorm.hip, csrc/conv1q.hip, csrc/gemmz.hip) ------
 * The network is Conv -> LayerNorm -> ReLU three times, then Linear(3136, 512) -> LayerNorm(512) -> ReLU -> Linear(512, A)
 * (cleanrl/pqn_atari_envpool.py, QNetwork).  Every forward kernel above fuses bias + ReLU; these are the same kernels WITHOUT the ReLU,
 * a LayerNorm + ReLU kernel pair for what sits between, and nothing else: the data- and weight-gradient kernels above are used unchanged
 * (with a = relu(LN(z)), "the gradient under the mask a > 0" is the gradient at the LayerNorm's output).
 *
 * pre-activation forwards: the accumulation, tile shapes and (FC) K split of the ReLU forward of the same size, so relu(z) equals that
 * forward's result bit for bit; no mask bits, no amax record for z (only the LayerNorm reads it).
 *   conv1q_pre_fwd: src_u8 (rows, 84, 84, 4) u8 + optional int64 gather -> dst (images, 20, 20, 32); kernel Q, pack =
 *     mi355ppo_cnn_conv1q_pack.  Alignments of mi355ppo_cnn_conv1q_fwd.
 *   conv_pre_packed_f16x2: layer 2 / 3, src (images, 20, 20, 32) / (images, 9, 9, 64) with its amax record -> dst (images, 9, 9, 64) /
 *     (images, 7, 7, 64); always kernel Z; pack = the layer's f16x2 forward pack.
 *   fc_pre_packed_f16x2: a (M, K) pitch lda with its amax record -> h (M, N) dense; workspace: mi355ppo_fc_fwd_workspace_bytes(M, N, K)
 *     bytes, 16-byte aligned (below 8,192 rows the K split of mi355ppo_fc_fwd_relu_packed_f16x2_f32; two launches). */
MI355PPO_API int mi355ppo_cnn_conv1q_pre_fwd(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                             int64_t images, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q_pre_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                 int64_t images);
MI355PPO_API int mi355ppo_cnn_conv_pre_packed_f16x2_f32(const float* src, const void* pack, const float* bias, float* dst, int64_t images,
                                                        int layer, const uint32_t* src_amax, void* stream);
MI355PPO_API int mi355ppo_fc_pre_packed_f16x2_f32(const float* a, int lda, const void* pack, const float* bias, float* h, int M, int N, int K,
                                                  void* workspace, size_t workspace_bytes, const uint32_t* a_amax, void* stream);
/* LayerNorm + ReLU over rows of D = C * HW floats in (H, W, C) order; gamma / beta / dgamma / dbeta (D) in torch's (C, H, W) order
 * (element p * C + c of a row <-> parameter c * HW + p; the FC layer: C = 512, HW = 1).  C % 4 == 0, D <= 16,384.
 * forward:  mean = sum z / D, var = sum (z - mean)^2 / D (biased, two passes, double partials in an order that depends on D alone),
 *   rstd = 1 / sqrt(var + eps), a = max((z - mean) * rstd * gamma + beta, 0).  z, a (rows, D) 16-byte aligned (may not alias); mean, rstd
 *   (rows).  mask_bits (optional, D % 32 == 0): rows * D / 32 words, word w bit b <-> flat element 32 w + b of a -- the layout of the
 *   *_bits forwards.  a_amax (optional): a's amax record (MI355PPO_AMAX_WORDS uint32, 64-byte aligned, zeroed by the caller).  One launch.
 * backward: dy (rows, D) the gradient at a -- already under the mask a > 0 (what the *_dgrad_* kernels write), or, with act != NULL,
 *   masked here by act > 0 (the FC layer, whose dh comes from the head).  With g = dy * gamma, xh = (z - mean) * rstd:
 *     dz = rstd * ((g - mean_j g) - xh * mean_j (g * xh)),  dgamma[j] = sum_r dy * xh,  dbeta[j] = sum_r dy  (both OVERWRITTEN).
 *   dz_amax (optional): dz's amax record.  No atomics on floats: slabs of rows write partial column sums into the workspace
 *   (mi355ppo_layernorm_bwd_workspace_bytes(rows, C, HW) bytes, 16-byte aligned), a second launch adds them in slab order in double; the
 *   order depends on (rows, D) alone, so the same input gives the same bits, eager or replayed from a graph.  Two launches.
 * The twins follow the same orders and return the device's bits; they fold an amax record's value into its word 0. */
MI355PPO_API int mi355ppo_layernorm_relu_fwd_f32(const float* z, const float* gamma, const float* beta, float* a, float* mean, float* rstd,
                                                 uint32_t* mask_bits, uint32_t* a_amax, int64_t rows, int C, int HW, double eps, void* stream);
MI355PPO_API int mi355ppo_layernorm_relu_fwd_f32_cpu(const float* z, const float* gamma, const float* beta, float* a, float* mean, float* rstd,
                                                     uint32_t* mask_bits, uint32_t* a_amax, int64_t rows, int C, int HW, double eps);
MI355PPO_API size_t mi355ppo_layernorm_bwd_workspace_bytes(int64_t rows, int C, int HW);
MI355PPO_API int mi355ppo_layernorm_relu_bwd_f32(const float* dy, const float* act, const float* z, const float* mean, const float* rstd,
                                                 const float* gamma, float* dz, float* dgamma, float* dbeta, uint32_t* dz_amax, int64_t rows,
                                                 int C, int HW, void* workspace, size_t workspace_bytes, void* stream);
MI355PPO_API int mi355ppo_layernorm_relu_bwd_f32_cpu(const float* dy, const float* act, const float* z, const float* mean, const float* rstd,
                                                     const float* gamma, float* dz, float* dgamma, float* dbeta, uint32_t* dz_amax,
                                                     int64_t rows, int C, int HW);

/* ---- The same network on ONE frame: pqn_atari_envpool_lstm.py (added under ABI 2.7.1; csrc/conv1q1.hip, csrc/conv1p1.hip) ---------------
 * Conv2d(1, 32, 8, stride=4) on uint8 frames (rows, 84, 84): (N, 1, 84, 84) and (N, 84, 84, 1) are the same bytes.  Everything behind
 * conv1 -- layers 2 / 3, the FC layer, the LayerNorm pair, every data and weight gradient -- is the four-frame network's, unchanged.
 *   conv1q1_pack: W (32, 1, 8, 8) -> kernel Q1's pack, mi355ppo_cnn_conv1q1_pack_bytes() = 8,832 bytes, 16-byte aligned.  Kernel Q's
 *     arithmetic (31-bit fixed point per output channel, four signed radix-256 digits) in this kernel's own layout.  One launch.
 *   conv1q1_pre_fwd: conv1(src[inds] / 255) + bias -> dst (images, 20, 20, 32) f32, 128-byte aligned; src 4-byte aligned, every load inside
 *     [src, src + rows * 7,056); inds int64 or NULL; images in 1 .. 1 << 22, the destination inside the 32-bit buffer range.  Exact int32
 *     accumulation and kernel Q's epilogue: the twin returns the device's bits.  One launch.
 *   conv1p1_wgrad_f16x2: dW (32, 1, 8, 8) and db (32), OVERWRITTEN, from the frames (through inds) and dz (images, 20, 20, 32) with its amax
 *     record: dz in two f16 terms under the record's scale, the bytes as exact f16 operands, f32 accumulation, one partial per wave folded in a
 *     fixed order (no atomics on floats: the same input gives the same bits).  workspace: mi355ppo_cnn_conv1p1_wgrad_workspace_bytes(images)
 *     bytes, 16-byte aligned.  Two or three launches. */
MI355PPO_API size_t mi355ppo_cnn_conv1q1_pack_bytes(void);
MI355PPO_API int mi355ppo_cnn_conv1q1_pack(const float* W, void* pack, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q1_pack_cpu(const float* W, void* pack);
MI355PPO_API int mi355ppo_cnn_conv1q1_pre_fwd(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                              int64_t images, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q1_pre_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                  int64_t images);
MI355PPO_API size_t mi355ppo_cnn_conv1p1_wgrad_workspace_bytes(int64_t images);
MI355PPO_API int mi355ppo_cnn_conv1p1_wgrad_f16x2(const void* src_u8, const int64_t* inds, const float* dz, float* dW, float* db,
                                                  int64_t images, void* workspace, size_t workspace_bytes, const uint32_t* dz_amax,
                                                  void* stream);

/* ---- Kernel Q1's ReLU instances: conv1 of ppo_atari_lstm.py's plain NatureCNN on one frame (added under ABI 2.7.1; csrc/conv1q1.hip) -------
 * relu(conv1(src[inds] / 255) + bias) -> dst (images, 20, 20, 32) f32: mi355ppo_cnn_conv1q_fwd_bits / _fwd_amax on (rows, 84, 84) frames, with
 * the pack, the pointer and range checks of mi355ppo_cnn_conv1q1_pre_fwd.  relu() of that entry point's result is this one's, bit for bit.
 *   mask_bits: images * 400 uint32, word p = (dst > 0) of the 32 channels of pixel p (bit b of word w <-> flat element 32 w + b); required by
 *     _fwd_bits, may be NULL in _fwd_amax and the twin.
 *   dst_amax: dst's amax record (zeroed by the caller), 64-byte aligned; the twin folds its maximum into slot 0 and takes NULL.
 * One launch each. */
MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_bits(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                               uint32_t* mask_bits, int64_t images, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_amax(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                               uint32_t* mask_bits, int64_t images, uint32_t* dst_amax, void* stream);
MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                              uint32_t* mask_bits, uint32_t* dst_amax, int64_t images);

/* ---- LeakyReLU over a flat f32 tensor (added under ABI 2.7.1; csrc/leaky.hip, element math in csrc/leaky_rows.h) --------------------------
 * The activation of RNDModel's predictor / target stacks (cleanrl/ppo_rnd_envpool.py:188-233), behind a pre-activation forward and behind a
 * data gradient called with an all-ones mask.  n > 0 elements, any n; z / a / da / dz 16-byte aligned, each pair may be the same buffer.
 *   forward:  a = z > 0 ? z : z * (float)slope, as torch.nn.functional.leaky_relu in f32 (-0 stays -0).  mask_bits (optional): (n + 31) / 32
 *     words, word w bit b <-> (z > 0) of flat element 32 w + b, the bits past n zero.  a_amax (optional): a's amax record (max |a|;
 *     MI355PPO_AMAX_WORDS uint32, 64-byte aligned, zeroed by the caller).
 *   backward: dz = bit ? da : da * (float)slope with the forward's mask_bits (required).  dz_amax (optional): dz's amax record.
 * One launch each; no atomics on floats (a record takes integer maxima): the same input gives the same bits.  The twins return the device's
 * bits and fold an amax record's value into its word 0. */
MI355PPO_API int mi355ppo_leaky_relu_fwd_f32(const float* z, float* a, uint32_t* mask_bits, uint32_t* a_amax, int64_t n, double slope,
                                             void* stream);
MI355PPO_API int mi355ppo_leaky_relu_fwd_f32_cpu(const float* z, float* a, uint32_t* mask_bits, uint32_t* a_amax, int64_t n, double slope);
MI355PPO_API int mi355ppo_leaky_relu_bwd_f32(const float* da, const uint32_t* mask_bits, float* dz, uint32_t* dz_amax, int64_t n, double slope,
                                             void* stream);
MI355PPO_API int mi355ppo_leaky_relu_bwd_f32_cpu(const float* da, const uint32_t* mask_bits, float* dz, uint32_t* dz_amax, int64_t n,
                                                 double slope);

/* ---- The normalising one-frame conv1 of RNDModel's predictor / target (added under ABI 2.7.1; csrc/rnd_conv1.hip) ------------------------
 * Conv2d(1, 32, 8, stride=4) on x[r, p] = the value of mi355ppo_rnd_normalize_u8_f32 (the same row function), straight from the u8
 * observation rows: FRAME addressing, idx (clamped) and mean / sd as there; x never goes to global memory and nothing outside the frames is
 * read.  Arithmetic: the two-term f16 split, x under the static scale 2^12 (|x| <= 5: no amax record, a row's bits do not depend on the
 * rest of its batch), the products hi hi, hi lo, lo hi with f32 accumulation.  Device only; capturable, no allocation, no float atomics.
 *   forward: dst (M, 20, 20, 32) f32 = leaky(conv(x, W1) + bias), leaky(z) = z > 0 ? z : z * (float)slope.  pack: W1 viewed as a (32, 64)
 *     matrix through mi355ppo_fc_pack_f16x2_f32 (mi355ppo_fc_pack_f16x2_bytes(32, 64) bytes, 16-byte aligned).  mask_bits (optional): M * 400
 *     words, word p = (z > 0) of the 32 channels of pixel p (bit b of word w <-> flat element 32 w + b).  dst_amax (optional): dst's amax
 *     record (max |dst|; zeroed by the caller, 64-byte aligned).  M in 1 .. 1 << 22.  One launch.
 *   gradient: dW (32, 1, 8, 8) and db (32), OVERWRITTEN: dW[n][kh][kw] = sum dz[p][n] * x[4 oy + kh][4 ox + kw], db[n] = sum dz[p][n], from
 *     dz (images, 20, 20, 32; 16-byte aligned) in two f16 terms under its amax record (required).  One partial per wave, folded in a fixed
 *     order: the same input gives the same bits.  workspace: mi355ppo_rnd_conv1_wgrad_workspace_bytes(images) bytes, 16-byte aligned.  Two or
 *     three launches. */
MI355PPO_API int mi355ppo_rnd_conv1_fwd_f16x2(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                              const int64_t* idx, const double* mean, const double* sd, const void* pack, const float* bias,
                                              float* dst, uint32_t* mask_bits, uint32_t* dst_amax, int M, double slope, void* stream);
MI355PPO_API size_t mi355ppo_rnd_conv1_wgrad_workspace_bytes(int64_t images);
MI355PPO_API int mi355ppo_rnd_conv1_wgrad_f16x2(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset,
                                                const int64_t* idx, const double* mean, const double* sd, const float* dz, float* dW, float* db,
                                                int64_t images, void* workspace, size_t workspace_bytes, const uint32_t* dz_amax, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355PPO_H_ */
