// Host-pointer twins of the PPO-path entry points ("every entry point has a *_cpu twin with host pointers,
// same math, plain C++, for config A and for tests").
//
// What they are for: BASELINE config A (`cleanrl/ppo.py` CartPole, num_envs = 4, on CPU -- plumbing, no GPU) and the
// world_size-2 gloo tests of the data-parallel logic run the reference's loop on CPU tensors; with the twins that loop calls
// the SAME seams of this library as the GPU path (GAE, sampling, fused loss forward + backward, clip + Adam) instead of a
// second restatement in torch ops.  What they are NOT: a fallback.  Nothing in the library or in cleanrl_amd/ routes a device
// pointer here; a CUDA device always runs the HIP kernels and raises when they are missing (cleanrl_amd/_lib.py).
//
// Same math by construction: the row / element functions (gae_step, categorical_row, ppo_row_terms, mean_den_from_sums,
// adam_elem, the Philox stream, the LSTM cell and its 128-column products) are the device kernels' own, compiled for the host
// from the same headers (ppo_rows.h, catrow.h, lstm_rows.h, trxl_rows.h, impala_rows.h, common.h), without FMA contraction.  Differences to the device results can come only from libm vs the device
// math library (expf / logf / sincosf: a few ulp) and from the order of the f64 reductions (row order here, fixed tree there).
// Serial, single-threaded: sizes of config A are a few hundred rows.
#include "common.h"
#include "catrow.h"
#include "ppo_rows.h"
#include "lstm_rows.h"
#include "trxl_rows.h"
#include "impala_rows.h"
#include "qdagger_rows.h"
#include "pqn_rows.h"
#include "pqn_lstm_rows.h"
#include "offpolicy_rows.h"
#include "dqn_rows.h"
#include "dqn_atari_rows.h"
#include "sac_rows.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

#include <vector>

#pragma clang fp contract(off)

using namespace mi355ppo;

#define TWIN_LOG_SQRT_2PI 0.91893853320467274178f     /* as in distributions.hip / loss.hip */
#define TWIN_HALF_LOG_2PIE 1.4189385332046727418f

namespace {

constexpr int kAMax = 64;

inline void load_host_row(float (&x)[kAMax], const float* row, int A) {
    for (int j = 0; j < kAMax; ++j) x[j] = (j < A) ? row[j] : -INFINITY;
}

inline int action_of(const int64_t* a_i64, const float* a_f32, int64_t row) {
    return a_i64 ? (int)a_i64[row] : (int)a_f32[row];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ K1
extern "C" MI355PPO_API int mi355ppo_gae_f32_cpu(const float* rewards, const float* dones, const float* values,
                                                 const float* next_done, const float* next_value, float* advantages,
                                                 float* returns, int T, int N, double gamma, double gae_lambda) {
    const char* fn = "mi355ppo_gae_f32_cpu";
    MI355_REQUIRE(rewards && dones && values && next_done && next_value && advantages && returns, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE(T > 0 && N > 0, MI355PPO_EINVAL, "%s: T=%d N=%d must be positive", fn, T, N);
    const float g = (float)gamma, gl = (float)(gamma * gae_lambda);      // g*l formed in double, rounded once (gae.hip)
    for (int n = 0; n < N; ++n) {
        float last = 0.0f, nextv = next_value[n], nextd = next_done[n];
        for (int t = T - 1; t >= 0; --t) {
            const size_t i = (size_t)t * N + n;
            float ret;
            last = gae_step(rewards[i], values[i], nextv, nextd, last, g, gl, &ret);
            advantages[i] = last;
            returns[i] = ret;
            nextv = values[i];
            nextd = dones[i];
        }
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ K2
extern "C" MI355PPO_API int mi355ppo_categorical_sample_f32_cpu(const float* logits, const float* noise_exp1, uint64_t seed,
                                                                uint64_t offset, int64_t* action_i64, float* action_f32,
                                                                float* logprob, float* entropy, int B, int A) {
    const char* fn = "mi355ppo_categorical_sample_f32_cpu";
    MI355_REQUIRE(logits && logprob, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(action_i64 || action_f32, MI355PPO_EINVAL, "%s: no action output", fn);
    MI355_REQUIRE(B > 0 && A > 0 && A <= kAMax, MI355PPO_EINVAL, "%s: B=%d must be >0 and A=%d in 1..64", fn, B, A);
    const Philox rng(seed);
    const int nblk = (A + 3) / 4;
    for (int row = 0; row < B; ++row) {
        float x[kAMax], q[kAMax];
        load_host_row(x, logits + (size_t)row * A, A);
        CatRow<kAMax> c;
        categorical_row<kAMax>(x, A, c);
        if (noise_exp1) {
            for (int j = 0; j < A; ++j) q[j] = noise_exp1[(size_t)row * A + j];
        } else {                                   // the device kernel's stream: counter = row * nblk + group, key = seed
            for (int g = 0; g * 4 < A; ++g) {
                const uint4 r = rng((uint64_t)row * nblk + g, offset);
                const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
                for (int k = 0; k < 4 && g * 4 + k < kAMax; ++k) q[g * 4 + k] = -logf(u32_to_unit_open(rr[k]));
            }
        }
        int best = 0;                              // multinomial(probs, 1) == argmax_j probs_j / q_j (first maximum wins)
        float bestv = -INFINITY, best_lp = 0.0f;
        for (int j = 0; j < A; ++j) {
            const float v = c.p[j] / q[j];
            if (v > bestv) { bestv = v; best = j; best_lp = c.lp[j]; }
        }
        if (action_i64) action_i64[row] = best;
        if (action_f32) action_f32[row] = (float)best;
        logprob[row] = best_lp;
        if (entropy) entropy[row] = c.H;
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_categorical_logprob_entropy_f32_cpu(const float* logits, const int64_t* action_i64,
                                                                         const float* action_f32, float* logprob,
                                                                         float* entropy, int B, int A) {
    const char* fn = "mi355ppo_categorical_logprob_entropy_f32_cpu";
    MI355_REQUIRE(logits && logprob, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE((action_i64 != nullptr) != (action_f32 != nullptr), MI355PPO_EINVAL,
                  "%s: exactly one of action_i64/action_f32 must be given", fn);
    MI355_REQUIRE(B > 0 && A > 0 && A <= kAMax, MI355PPO_EINVAL, "%s: B=%d must be >0 and A=%d in 1..64", fn, B, A);
    for (int row = 0; row < B; ++row) {
        float x[kAMax];
        load_host_row(x, logits + (size_t)row * A, A);
        CatRow<kAMax> c;
        categorical_row<kAMax>(x, A, c);
        const int a = action_of(action_i64, action_f32, row);
        logprob[row] = (a >= 0 && a < A) ? c.lp[a] : 0.0f;
        if (entropy) entropy[row] = c.H;
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_categorical_logprob_entropy_bwd_f32_cpu(const float* logits, const int64_t* action_i64,
                                                                             const float* action_f32, const float* g_logprob,
                                                                             const float* g_entropy, float* dlogits, int B,
                                                                             int A) {
    const char* fn = "mi355ppo_categorical_logprob_entropy_bwd_f32_cpu";
    MI355_REQUIRE(logits && dlogits, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE((action_i64 != nullptr) != (action_f32 != nullptr), MI355PPO_EINVAL,
                  "%s: exactly one of action_i64/action_f32 must be given", fn);
    MI355_REQUIRE(B > 0 && A > 0 && A <= kAMax, MI355PPO_EINVAL, "%s: B=%d must be >0 and A=%d in 1..64", fn, B, A);
    for (int row = 0; row < B; ++row) {
        float x[kAMax];
        load_host_row(x, logits + (size_t)row * A, A);
        CatRow<kAMax> c;
        categorical_row<kAMax>(x, A, c);
        const int a = action_of(action_i64, action_f32, row);
        const float gl = g_logprob ? g_logprob[row] : 0.0f, ge = g_entropy ? g_entropy[row] : 0.0f;
        for (int j = 0; j < A; ++j) {
            const float onehot = (j == a) ? 1.0f : 0.0f;
            dlogits[(size_t)row * A + j] = gl * (onehot - c.p[j]) - ge * (c.p[j] * (fmaxf(c.lp[j], -FLT_MAX) + c.H));
        }
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ K2'
namespace {
// One row of Normal(mean, exp(logstd)): log_prob and entropy summed over D (torch normal.py op order, distributions.hip).
template <bool SAMPLE>
inline void normal_row(const float* mean, const float* logstd, const float* noise, const Philox& rng, uint64_t offset, int64_t row,
                       float* action_out, const float* action_in, float* lp_out, float* ent_out, int D) {
    const int nblk = (D + 3) / 4;
    float lp = 0.0f, ent = 0.0f;
    float z4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int d = 0; d < D; ++d) {
        const float mu = mean[(size_t)row * D + d];
        const float sd = expf(logstd[d]);
        float a;
        if (SAMPLE) {
            float z;
            if (noise) {
                z = noise[(size_t)row * D + d];
            } else {
                if ((d & 3) == 0) {   // Box-Muller: 4 uint32 -> 2 (u1,u2) pairs -> 4 standard normals
                    const uint4 r = rng((uint64_t)row * nblk + (d >> 2), offset);
                    const float r0 = sqrtf(-2.0f * logf(u32_to_unit_open(r.x)));
                    const float r1 = sqrtf(-2.0f * logf(u32_to_unit_open(r.z)));
                    float s0, c0, s1, c1;
                    sincosf(6.283185307179586f * u32_to_unit_open(r.y), &s0, &c0);
                    sincosf(6.283185307179586f * u32_to_unit_open(r.w), &s1, &c1);
                    z4[0] = r0 * c0; z4[1] = r0 * s0; z4[2] = r1 * c1; z4[3] = r1 * s1;
                }
                z = z4[d & 3];
            }
            a = z * sd;          // torch.normal(mean, std): normal_(0,1).mul_(std).add_(mean)
            a = a + mu;
            action_out[(size_t)row * D + d] = a;
        } else {
            a = action_in[(size_t)row * D + d];
        }
        const float diff = a - mu;
        const float var = sd * sd;
        const float log_scale = logf(sd);
        float t = -(diff * diff);
        t = t / (2.0f * var);
        t = t - log_scale;
        t = t - TWIN_LOG_SQRT_2PI;
        lp += t;
        ent += TWIN_HALF_LOG_2PIE + log_scale;
    }
    *lp_out = lp;
    *ent_out = ent;
}
}  // namespace

extern "C" MI355PPO_API int mi355ppo_normal_sample_f32_cpu(const float* mean, const float* logstd, const float* noise_std_normal,
                                                           uint64_t seed, uint64_t offset, float* action, float* logprob_sum,
                                                           float* entropy_sum, int B, int D) {
    const char* fn = "mi355ppo_normal_sample_f32_cpu";
    MI355_REQUIRE(mean && logstd && action && logprob_sum, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0 && D > 0, MI355PPO_EINVAL, "%s: B=%d D=%d must be positive", fn, B, D);
    const Philox rng(seed);
    for (int row = 0; row < B; ++row) {
        float lp, ent;
        normal_row<true>(mean, logstd, noise_std_normal, rng, offset, row, action, nullptr, &lp, &ent, D);
        logprob_sum[row] = lp;
        if (entropy_sum) entropy_sum[row] = ent;
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_normal_logprob_entropy_f32_cpu(const float* mean, const float* logstd, const float* action,
                                                                    float* logprob_sum, float* entropy_sum, int B, int D) {
    const char* fn = "mi355ppo_normal_logprob_entropy_f32_cpu";
    MI355_REQUIRE(mean && logstd && action && logprob_sum, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0 && D > 0, MI355PPO_EINVAL, "%s: B=%d D=%d must be positive", fn, B, D);
    const Philox rng(0);
    for (int row = 0; row < B; ++row) {
        float lp, ent;
        normal_row<false>(mean, logstd, nullptr, rng, 0, row, nullptr, action, &lp, &ent, D);
        logprob_sum[row] = lp;
        if (entropy_sum) entropy_sum[row] = ent;
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_normal_logprob_entropy_bwd_f32_cpu(const float* mean, const float* logstd,
                                                                        const float* action, const float* g_logprob,
                                                                        const float* g_entropy, float* dmean,
                                                                        float* dlogstd_rows, int B, int D) {
    const char* fn = "mi355ppo_normal_logprob_entropy_bwd_f32_cpu";
    MI355_REQUIRE(mean && logstd && action && dmean && dlogstd_rows, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0 && D > 0, MI355PPO_EINVAL, "%s: B=%d D=%d must be positive", fn, B, D);
    for (int row = 0; row < B; ++row) {
        const float gl = g_logprob ? g_logprob[row] : 0.0f, ge = g_entropy ? g_entropy[row] : 0.0f;
        for (int d = 0; d < D; ++d) {
            const float sd = expf(logstd[d]);
            const float var = sd * sd;
            const float diff = action[(size_t)row * D + d] - mean[(size_t)row * D + d];
            dmean[(size_t)row * D + d] = gl * (diff / var);
            dlogstd_rows[(size_t)row * D + d] = gl * ((diff * diff) / var - 1.0f) + ge;
        }
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ K3
namespace {

int loss_params(const char* fn, int M, double clip_coef, double ent_coef, double vf_coef, int norm_adv, int clip_vloss,
                const float* adv_mean_den, LossParams* P) {
    MI355_REQUIRE(M > 0, MI355PPO_EINVAL, "%s: M=%d must be positive", fn, M);
    MI355_REQUIRE(!norm_adv || adv_mean_den || M > 1, MI355PPO_EINVAL, "%s: norm_adv needs M > 1 (unbiased std)", fn);
    P->lo = (float)(1.0 - clip_coef);
    P->hi = (float)(1.0 + clip_coef);
    P->clip = (float)clip_coef;
    P->ent_coef = (float)ent_coef;
    P->vf_coef = (float)vf_coef;
    P->norm_adv = norm_adv;
    P->clip_vloss = clip_vloss;
    P->M = M;
    P->stats_blocks = 0;
    return MI355PPO_OK;
}

// (mean, unbiased std + 1e-8) of b_adv[mb_inds]: f64 sums in row order, then the device kernels' own fold.
void adv_mean_den_host(const float* b_adv, const int64_t* inds, int M, const float* given, float* mean, float* den) {
    if (given) { *mean = given[0]; *den = given[1]; return; }
    double s = 0.0, ss = 0.0;
    for (int m = 0; m < M; ++m) {
        const double a = (double)b_adv[inds ? inds[m] : m];
        s += a;
        ss += a * a;
    }
    mean_den_from_sums(s, ss, (double)M, mean, den);
}

// the seven scalars from the six f64 sums: loss_finalize's arithmetic (loss.hip)
void fold_scalars7(const double (&tot)[kNumSums], const LossParams& P, float* scalars7) {
    const double n = (double)P.M;
    const float pg_loss = (float)(tot[0] / n);
    const float v_loss = 0.5f * (float)(tot[1] / n);
    const float entropy = (float)(tot[2] / n);
    float loss = pg_loss - P.ent_coef * entropy;     // :355  pg_loss - ent_coef*entropy + v_loss*vf_coef
    loss = loss + v_loss * P.vf_coef;
    scalars7[0] = loss;
    scalars7[1] = pg_loss;
    scalars7[2] = v_loss;
    scalars7[3] = entropy;
    scalars7[4] = (float)(tot[3] / n);
    scalars7[5] = (float)(tot[4] / n);
    scalars7[6] = (float)(tot[5] / n);
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_loss_categorical_fwd_bwd_f32_cpu(
    const float* new_logits, const float* new_value, const int64_t* mb_inds, const float* b_actions_f32, const float* b_logprobs,
    const float* b_advantages, const float* b_returns, const float* b_values, int M, int A, double clip_coef, double ent_coef,
    double vf_coef, int norm_adv, int clip_vloss, const float* adv_mean_den, float* scalars7, float* dlogits, float* dvalue) {
    const char* fn = "mi355ppo_loss_categorical_fwd_bwd_f32_cpu";
    MI355_REQUIRE(new_logits && new_value && b_actions_f32 && b_logprobs && b_advantages && b_returns && b_values && scalars7 &&
                      dlogits && dvalue,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(A > 0 && A <= kAMax, MI355PPO_EINVAL, "%s: A=%d must be in 1..64", fn, A);
    LossParams P;
    if (int rc = loss_params(fn, M, clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss, adv_mean_den, &P)) return rc;
    float mean = 0.0f, den = 1.0f;
    if (norm_adv) adv_mean_den_host(b_advantages, mb_inds, M, adv_mean_den, &mean, &den);
    double tot[kNumSums] = {0, 0, 0, 0, 0, 0};
    const float ge = P.ent_coef / (float)P.M;
    for (int m = 0; m < M; ++m) {
        const int64_t i = mb_inds ? mb_inds[m] : m;
        float x[kAMax];
        load_host_row(x, new_logits + (size_t)m * A, A);
        CatRow<kAMax> c;
        categorical_row<kAMax>(x, A, c);
        const int a = (int)b_actions_f32[i];
        const float newlp = (a >= 0 && a < A) ? c.lp[a] : 0.0f;
        const RowTerms t = ppo_row_terms(newlp, c.H, new_value[m], b_logprobs[i], b_advantages[i], b_returns[i], b_values[i], mean,
                                         den, P);
        for (int k = 0; k < kNumSums; ++k) tot[k] += (double)t.sums[k];
        dvalue[m] = t.dvalue;
        for (int j = 0; j < A; ++j) {       // d loss/d logits_j = g_lp*(1[j==a] - p_j) + (ent_coef/M) * p_j * (lp_j + H)
            const float onehot = (j == a) ? 1.0f : 0.0f;
            const float lpj = fmaxf(c.lp[j], -FLT_MAX);
            dlogits[(size_t)m * A + j] = t.g_lp * (onehot - c.p[j]) + ge * (c.p[j] * (lpj + c.H));
        }
    }
    fold_scalars7(tot, P, scalars7);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_loss_normal_fwd_bwd_f32_cpu(
    const float* new_mean, const float* logstd, const float* new_value, const int64_t* mb_inds, const float* b_actions,
    const float* b_logprobs, const float* b_advantages, const float* b_returns, const float* b_values, int M, int D,
    double clip_coef, double ent_coef, double vf_coef, int norm_adv, int clip_vloss, const float* adv_mean_den, float* scalars7,
    float* dmean, float* dlogstd, float* dvalue) {
    const char* fn = "mi355ppo_loss_normal_fwd_bwd_f32_cpu";
    MI355_REQUIRE(new_mean && logstd && new_value && b_actions && b_logprobs && b_advantages && b_returns && b_values && scalars7 &&
                      dmean && dlogstd && dvalue,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(D > 0 && D <= 64, MI355PPO_EINVAL, "%s: D=%d must be in 1..64", fn, D);
    LossParams P;
    if (int rc = loss_params(fn, M, clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss, adv_mean_den, &P)) return rc;
    float amean = 0.0f, den = 1.0f;
    if (norm_adv) adv_mean_den_host(b_advantages, mb_inds, M, adv_mean_den, &amean, &den);
    double tot[kNumSums] = {0, 0, 0, 0, 0, 0};
    double dls[64];
    for (int d = 0; d < D; ++d) dls[d] = 0.0;
    const float g_ent = -(P.ent_coef / (float)P.M);   // d loss / d entropy_row ; d entropy_row / d logstd_d = 1
    const Philox unused(0);
    for (int m = 0; m < M; ++m) {
        const int64_t i = mb_inds ? mb_inds[m] : m;
        float lp, ent;
        normal_row<false>(new_mean, logstd, nullptr, unused, 0, m, nullptr, b_actions + ((ptrdiff_t)i - (ptrdiff_t)m) * D, &lp, &ent, D);   // (row m of new_mean, row i of b_actions)
        const RowTerms t = ppo_row_terms(lp, ent, new_value[m], b_logprobs[i], b_advantages[i], b_returns[i], b_values[i], amean,
                                         den, P);
        for (int k = 0; k < kNumSums; ++k) tot[k] += (double)t.sums[k];
        dvalue[m] = t.dvalue;
        for (int d = 0; d < D; ++d) {
            const float mu = new_mean[(size_t)m * D + d];
            const float sd = expf(logstd[d]);
            const float diff = b_actions[(size_t)i * D + d] - mu;
            const float var = sd * sd;
            dmean[(size_t)m * D + d] = t.g_lp * (diff / var);
            dls[d] += (double)(t.g_lp * ((diff * diff) / var - 1.0f) + g_ent);
        }
    }
    fold_scalars7(tot, P, scalars7);
    for (int d = 0; d < D; ++d) dlogstd[d] = (float)dls[d];
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ a8
extern "C" MI355PPO_API int mi355ppo_clip_adam_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                                       double grad_scale, double max_grad_norm, double lr, double beta1,
                                                       double beta2, double eps, int64_t step, float* total_norm_out) {
    const char* fn = "mi355ppo_clip_adam_f32_cpu";
    MI355_REQUIRE(params && grads && exp_avg && exp_avg_sq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0 && step >= 1, MI355PPO_EINVAL, "%s: n=%lld must be >0 and step=%lld >= 1", fn, (long long)n,
                  (long long)step);
    AdamParams A;                                   // as mi355ppo_clip_adam_f32 forms them (optim.hip)
    A.scale = (float)grad_scale;
    A.max_norm = (float)max_grad_norm;
    A.w1 = (float)(1.0 - beta1);
    A.beta2 = (float)beta2;
    A.w2 = (float)(1.0 - beta2);
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    A.bc2_sqrt = (float)sqrt(bc2);
    A.eps = (float)eps;
    A.neg_step = (float)(-(lr / bc1));
    A.nblocks = 1;
    A.zero_grads = 1;
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const float a = grads[i] * A.scale;
        s += (double)a * a;
    }
    const float total = (float)sqrt(s);
    float coef = A.max_norm / (total + 1e-6f);      // clip_grad.py: max_norm / (total_norm + 1e-6)
    coef = fminf(coef, 1.0f);                        //               clamp(max=1.0)
    if (total_norm_out) *total_norm_out = total;
    for (int64_t i = 0; i < n; ++i) adam_elem(params[i], grads[i], exp_avg[i], exp_avg_sq[i], coef, A);
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ K5
extern "C" MI355PPO_API int mi355ppo_obs_u8_to_f32_cpu(const uint8_t* src_u8, const int64_t* inds, float* dst_f32, int64_t rows,
                                                       int64_t row_bytes, int scale_255) {
    const char* fn = "mi355ppo_obs_u8_to_f32_cpu";
    MI355_REQUIRE(src_u8 && dst_f32, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(rows > 0 && row_bytes > 0, MI355PPO_EINVAL, "%s: rows=%lld row_bytes=%lld must be positive", fn, (long long)rows,
                  (long long)row_bytes);
    for (int64_t r = 0; r < rows; ++r) {
        const uint8_t* s = src_u8 + (size_t)(inds ? inds[r] : r) * row_bytes;
        float* d = dst_f32 + (size_t)r * row_bytes;
        for (int64_t k = 0; k < row_bytes; ++k) d[k] = scale_255 ? (float)s[k] / 255.0f : (float)s[k];
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ LSTM
namespace {

// Column k of gate block q of W_hh (512, 128): the backward's operand, read in the device thread (q, k)'s order.
struct LstmColumn {
    const float* p;
    MI355_HD float operator[](int r) const { return p[(size_t)r * kLstmH]; }
};

}  // namespace

extern "C" MI355PPO_API int mi355ppo_lstm_seq_fwd_f32_cpu(const float* gx, const float* w_hh, const float* h0, const float* c0,
                                                          const float* done, float* h, float* hT, float* cT, float* record, int T,
                                                          int B, int H) {
    const char* fn = "mi355ppo_lstm_seq_fwd_f32_cpu";
    MI355_REQUIRE(gx && w_hh && h0 && c0 && done && h && hT && cT, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(T > 0 && B > 0, MI355PPO_EINVAL, "%s: T=%d B=%d must be positive", fn, T, B);
    const size_t TB = (size_t)T * B;
    for (int b = 0; b < B; ++b) {
        float hk[kLstmH], ck[kLstmH], a[kLstmG];
        const float keep0 = 1.0f - done[b];
        for (int u = 0; u < kLstmH; ++u) {
            hk[u] = keep0 * h0[(size_t)b * kLstmH + u];
            ck[u] = keep0 * c0[(size_t)b * kLstmH + u];
        }
        for (int t = 0; t < T; ++t) {
            const size_t row = (size_t)t * B + b;
            for (int j = 0; j < kLstmG; ++j) a[j] = gx[row * kLstmG + j] + lstm_dot128(w_hh + (size_t)j * kLstmH, hk);
            const float keep = t + 1 < T ? 1.0f - done[row + B] : 0.0f;
            for (int u = 0; u < kLstmH; ++u) {
                const LstmCell s = lstm_cell_fwd(a[u], a[kLstmH + u], a[2 * kLstmH + u], a[3 * kLstmH + u], ck[u]);
                h[row * kLstmH + u] = s.h;
                if (record) {
                    float* g = record + row * kLstmG + u;
                    g[0] = s.i;
                    g[kLstmH] = s.f;
                    g[2 * kLstmH] = s.g;
                    g[3 * kLstmH] = s.o;
                    record[TB * 4 * kLstmH + row * kLstmH + u] = s.c;
                    record[TB * 5 * kLstmH + row * kLstmH + u] = hk[u];
                    record[TB * 6 * kLstmH + row * kLstmH + u] = ck[u];
                }
                if (t + 1 == T) {
                    hT[(size_t)b * kLstmH + u] = s.h;
                    cT[(size_t)b * kLstmH + u] = s.c;
                }
                hk[u] = keep * s.h;
                ck[u] = keep * s.c;
            }
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_lstm_seq_bwd_f32_cpu(const float* dh, const float* dhT, const float* dcT, const float* record,
                                                          const float* w_hh, const float* done, float* dgx, float* dh0, float* dc0,
                                                          int T, int B, int H) {
    const char* fn = "mi355ppo_lstm_seq_bwd_f32_cpu";
    MI355_REQUIRE(dh && record && w_hh && done && dgx, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(T > 0 && B > 0, MI355PPO_EINVAL, "%s: T=%d B=%d must be positive", fn, T, B);
    const size_t TB = (size_t)T * B;
    for (int b = 0; b < B; ++b) {
        float dhk[kLstmH], dc[kLstmH], part[4][kLstmH], dg[kLstmG];
        float keep_next = 0.0f;
        for (int u = 0; u < kLstmH; ++u) {
            dhk[u] = dhT ? dhT[(size_t)b * kLstmH + u] : 0.0f;
            dc[u] = dcT ? dcT[(size_t)b * kLstmH + u] : 0.0f;
        }
        for (int t = T - 1; t >= 0; --t) {
            const size_t row = (size_t)t * B + b;
            const float keep = 1.0f - done[row];
            for (int u = 0; u < kLstmH; ++u) {
                const float carry = t == T - 1 ? dhk[u] : keep_next * lstm_fold4(part[0][u], part[1][u], part[2][u], part[3][u]);
                const float* g = record + row * kLstmG + u;
                const LstmCellGrad d = lstm_cell_bwd(g[0], g[kLstmH], g[2 * kLstmH], g[3 * kLstmH], record[TB * 4 * kLstmH + row * kLstmH + u],
                                                     record[TB * 6 * kLstmH + row * kLstmH + u], dh[row * kLstmH + u] + carry, dc[u]);
                dg[u] = d.dai;
                dg[kLstmH + u] = d.daf;
                dg[2 * kLstmH + u] = d.dag;
                dg[3 * kLstmH + u] = d.dao;
                dc[u] = keep * d.dck;
            }
            for (int j = 0; j < kLstmG; ++j) dgx[row * kLstmG + j] = dg[j];
            for (int q = 0; q < 4; ++q)
                for (int k = 0; k < kLstmH; ++k)
                    part[q][k] = lstm_dot128(LstmColumn{w_hh + (size_t)q * kLstmH * kLstmH + k}, dg + q * kLstmH);
            keep_next = keep;
        }
        for (int u = 0; u < kLstmH; ++u) {
            if (dh0) dh0[(size_t)b * kLstmH + u] = keep_next * lstm_fold4(part[0][u], part[1][u], part[2][u], part[3][u]);
            if (dc0) dc0[(size_t)b * kLstmH + u] = dc[u];
        }
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ TrXL
// The episodic-memory attention core (trxl_attn.hip): the 64 lanes and 4 waves of the device layout emulated in order, so the
// sums are folded exactly as the kernels fold them (trxl_rows.h).  Out-of-range indices are refused (the device clamps them and
// raises its error word).
namespace {

struct TwinTrxl {
    const float* mem;
    const int64_t* ep;
    const int64_t* rows;
    const int64_t* pos;
    const uint8_t* mask;
    const float* pe;
    const float* gamma;
    const float* beta;
    const float* q;
    int E, T, layers, layer, P, B, L, D, H;
};

constexpr int kLanes = MI355_WAVE;

// v[i] += v[i ^ off] for off = n/2 .. 1 within groups of n lanes: __shfl_xor's butterfly.
void twin_butterfly(float (&v)[kLanes], int n) {
    for (int off = n >> 1; off >= 1; off >>= 1) {
        float t[kLanes];
        for (int i = 0; i < kLanes; ++i) t[i] = v[i] + v[i ^ off];
        for (int i = 0; i < kLanes; ++i) v[i] = t[i];
    }
}

float twin_wave_sum(const float* x, int C) {
    float v[kLanes];
    for (int l = 0; l < kLanes; ++l) {
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s = s + x[l * C + c];
        v[l] = s;
    }
    twin_butterfly(v, kLanes);
    return v[0];
}

// Per-head dots a . b over the row: out[h] for every head.
void twin_head_dots(const float* a, const float* b, int C, int H, float* out) {
    float v[kLanes];
    for (int l = 0; l < kLanes; ++l) {
        float s = 0.0f;
        for (int c = 0; c < C; ++c) s = s + a[l * C + c] * b[l * C + c];
        v[l] = s;
    }
    const int G = kLanes / H;
    twin_butterfly(v, G);
    for (int h = 0; h < H; ++h) out[h] = v[h * G];
}

// Window row j of sample b -> xhat, y.
void twin_norm_row(const TwinTrxl& a, int b, int j, float* xh, float* y) {
    const int C = a.D / kLanes;
    const int64_t r = a.rows[(size_t)b * a.L + j];
    const float* src = a.mem + (((size_t)a.ep[b] * a.T + (size_t)r) * a.layers + a.layer) * a.D;
    float x[kTrxlMaxD];
    for (int k = 0; k < a.D; ++k) x[k] = a.pe ? src[k] + a.pe[(size_t)a.pos[(size_t)b * a.L + j] * a.D + k] : src[k];
    const float mean = twin_wave_sum(x, C) / (float)a.D;
    for (int k = 0; k < a.D; ++k) xh[k] = x[k] - mean;
    float sq[kTrxlMaxD];
    for (int k = 0; k < a.D; ++k) sq[k] = xh[k] * xh[k];
    const float rstd = trxl_rstd(twin_wave_sum(sq, C) / (float)a.D);
    for (int k = 0; k < a.D; ++k) {
        xh[k] = xh[k] * rstd;
        y[k] = xh[k] * a.gamma[k] + a.beta[k];
    }
}

int twin_trxl_check(const char* fn, const TwinTrxl& a) {
    MI355_REQUIRE(a.mem && a.ep && a.rows && a.mask && a.gamma && a.beta && a.q, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(trxl_shape_ok(a.D, a.H, a.L), MI355PPO_EINVAL,
                  "%s: D=%d H=%d L=%d (need D %% 64 == 0, D <= 512, H dividing 64, 1 <= L <= 1024)", fn, a.D, a.H, a.L);
    MI355_REQUIRE(a.B > 0 && a.E > 0 && a.T > 0 && a.layers > 0 && a.layer >= 0 && a.layer < a.layers, MI355PPO_EINVAL,
                  "%s: B=%d E=%d T_ep=%d layers=%d layer=%d", fn, a.B, a.E, a.T, a.layers, a.layer);
    MI355_REQUIRE(!a.pe || (a.pos && a.P > 0), MI355PPO_EINVAL, "%s: pe needs pos and P > 0 (P=%d)", fn, a.P);
    for (int b = 0; b < a.B; ++b) {
        MI355_REQUIRE(a.ep[b] >= 0 && a.ep[b] < a.E, MI355PPO_EINVAL, "%s: ep[%d]=%lld outside [0, %d)", fn, b, (long long)a.ep[b], a.E);
        for (int j = 0; j < a.L; ++j) {
            const size_t i = (size_t)b * a.L + j;
            MI355_REQUIRE(a.rows[i] >= 0 && a.rows[i] < a.T, MI355PPO_EINVAL, "%s: rows[%d, %d]=%lld outside [0, %d)", fn, b, j,
                          (long long)a.rows[i], a.T);
            MI355_REQUIRE(!a.pe || (a.pos[i] >= 0 && a.pos[i] < a.P), MI355PPO_EINVAL, "%s: pos[%d, %d]=%lld outside [0, %d)", fn, b,
                          j, (long long)a.pos[i], a.P);
        }
    }
    return MI355PPO_OK;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_trxl_attn_fwd_f32_cpu(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                           const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe,
                                                           int P, const float* gamma, const float* beta, const float* q, float* u,
                                                           float* stats, int B, int L, int D, int H) {
    const char* fn = "mi355ppo_trxl_attn_fwd_f32_cpu";
    const TwinTrxl a{memory, ep, rows, pos, mask, pe, gamma, beta, q, E, T_ep, layers, layer, pe ? P : 0, B, L, D, H};
    if (int r = twin_trxl_check(fn, a)) return r;
    MI355_REQUIRE(u && stats, MI355PPO_EINVAL, "%s: null pointer", fn);
    const float sqrt_d = trxl_sqrt_d(D);
    const int d = D / H;
    float xh[kTrxlMaxD], y[kTrxlMaxD], acc[kTrxlWaves][kTrxlMaxD], e[64];
    TrxlOnline st[kTrxlWaves][64];
    for (int b = 0; b < B; ++b) {
        const float* qb = q + (size_t)b * D;
        for (int w = 0; w < kTrxlWaves; ++w) {
            for (int h = 0; h < H; ++h) st[w][h] = TrxlOnline{-INFINITY, 0.0f};
            for (int k = 0; k < D; ++k) acc[w][k] = 0.0f;
            for (int j = w; j < L; j += kTrxlWaves) {
                twin_norm_row(a, b, j, xh, y);
                twin_head_dots(qb, y, D / kLanes, H, e);
                const bool keep = mask[(size_t)b * L + j] != 0;
                for (int h = 0; h < H; ++h) {
                    float p;
                    const float f = trxl_online_step(st[w][h], trxl_score(keep, e[h], sqrt_d), p);
                    for (int k = h * d; k < (h + 1) * d; ++k) acc[w][k] = acc[w][k] * f + p * y[k];
                }
            }
        }
        for (int h = 0; h < H; ++h) {
            float m[kTrxlWaves], f[kTrxlWaves], l[kTrxlWaves], v[kTrxlWaves];
            for (int w = 0; w < kTrxlWaves; ++w) m[w] = st[w][h].m;
            const float M = trxl_merge_max(m);
            for (int w = 0; w < kTrxlWaves; ++w) {
                f[w] = expf(m[w] - M);
                l[w] = st[w][h].l;
            }
            const float lsum = trxl_merge_sum(l, f);
            for (int k = h * d; k < (h + 1) * d; ++k) {
                for (int w = 0; w < kTrxlWaves; ++w) v[w] = acc[w][k];
                u[(size_t)b * D + k] = trxl_merge_sum(v, f) / lsum;
            }
            stats[((size_t)b * H + h) * 2] = M;
            stats[((size_t)b * H + h) * 2 + 1] = lsum;
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_trxl_attn_bwd_f32_cpu(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                           const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe,
                                                           int P, const float* gamma, const float* beta, const float* q, const float* u,
                                                           const float* stats, const float* du, float* dq, float* dln_rows,
                                                           float* dgamma, float* dbeta, int B, int L, int D, int H) {
    const char* fn = "mi355ppo_trxl_attn_bwd_f32_cpu";
    const TwinTrxl a{memory, ep, rows, pos, mask, pe, gamma, beta, q, E, T_ep, layers, layer, pe ? P : 0, B, L, D, H};
    if (int r = twin_trxl_check(fn, a)) return r;
    MI355_REQUIRE(u && stats && du && dq && dln_rows && dgamma && dbeta, MI355PPO_EINVAL, "%s: null pointer", fn);
    const float sqrt_d = trxl_sqrt_d(D);
    const int d = D / H, C = D / kLanes;
    const size_t BD = (size_t)B * D;
    float xh[kTrxlMaxD], y[kTrxlMaxD], e[64], dyu[64], duu[64];
    static thread_local float z[kTrxlWaves][kTrxlMaxD], dg[kTrxlWaves][kTrxlMaxD], db[kTrxlWaves][kTrxlMaxD];
    for (int b = 0; b < B; ++b) {
        const float *qb = q + (size_t)b * D, *dub = du + (size_t)b * D;
        twin_head_dots(dub, u + (size_t)b * D, C, H, duu);
        for (int w = 0; w < kTrxlWaves; ++w) {
            for (int k = 0; k < D; ++k) z[w][k] = dg[w][k] = db[w][k] = 0.0f;
            for (int j = w; j < L; j += kTrxlWaves) {
                twin_norm_row(a, b, j, xh, y);
                twin_head_dots(qb, y, C, H, e);
                twin_head_dots(dub, y, C, H, dyu);
                const bool keep = mask[(size_t)b * L + j] != 0;
                for (int h = 0; h < H; ++h) {
                    const float s = trxl_score(keep, e[h], sqrt_d);
                    const float att = trxl_att(s, stats[((size_t)b * H + h) * 2], stats[((size_t)b * H + h) * 2 + 1]);
                    const float ds = att * (dyu[h] - duu[h]);
                    const float gs = keep ? ds / sqrt_d : 0.0f;
                    for (int k = h * d; k < (h + 1) * d; ++k) {
                        z[w][k] = z[w][k] + gs * y[k];
                        const float dyk = gs * qb[k] + att * dub[k];
                        dg[w][k] = dg[w][k] + dyk * xh[k];
                        db[w][k] = db[w][k] + dyk;
                    }
                }
            }
        }
        for (int k = 0; k < D; ++k) {
            const size_t o = (size_t)b * D + k;
            dq[o] = ((z[0][k] + z[1][k]) + z[2][k]) + z[3][k];
            dln_rows[o] = ((dg[0][k] + dg[1][k]) + dg[2][k]) + dg[3][k];
            dln_rows[BD + o] = ((db[0][k] + db[1][k]) + db[2][k]) + db[3][k];
        }
    }
    for (int k = 0; k < D; ++k) {                            // trxl_ln_fold_kernel's order: wave w sums b = w, w + 4, ...
        float sg[kTrxlWaves], sb[kTrxlWaves];
        for (int w = 0; w < kTrxlWaves; ++w) {
            sg[w] = sb[w] = 0.0f;
            for (int b = w; b < B; b += kTrxlWaves) {
                sg[w] = sg[w] + dln_rows[(size_t)b * D + k];
                sb[w] = sb[w] + dln_rows[BD + (size_t)b * D + k];
            }
        }
        dgamma[k] = ((sg[0] + sg[1]) + sg[2]) + sg[3];
        dbeta[k] = ((sb[0] + sb[1]) + sb[2]) + sb[3];
    }
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------ IMPALA-CNN trunk twins
// The device launches of impala.hip restated serially: every conv output an fmaf chain in the kernel's k order, every weight
// gradient one chain per part in pixel order plus the fold in part order, the max pool through the same window functions
// (impala_rows.h).  The hot loops are compiled twice, with the x86 FMA instructions and without (libm's fmaf); both round
// each fused multiply-add once, so the bits are the same, and the first only runs where the CPU has the instructions.
namespace {

struct ImpConvHost {
    const float* in;
    int ci, co, h;
    bool relu;
    const float* wt;            // Wt[k][n], k < 9 cp (forward: cp = ci rounded up to 4), n < co
    const float* bias;          // forward: bias (+ res); data gradient (bias NULL): mask / res epilogue
    const float* mask;
    const float* res;
    float* out;
    int B;
    const uint8_t* in8 = nullptr;   // the 84 family's layer 0: the frames as bytes (in NULL), read through imp_u8
};

template <int V>
__attribute__((always_inline)) inline void imp_conv_host_impl(const ImpConvHost& a) {
    const int cp = imp_cpad(a.ci), hp = a.h + 2, kp = 9 * cp;
    std::vector<float> pad((size_t)hp * hp * cp);
    float acc[32];
    for (int img = 0; img < a.B; ++img) {
        for (int y = 0; y < hp; ++y)
            for (int x = 0; x < hp; ++x)
                for (int c = 0; c < cp; ++c) {
                    const int yy = y - 1, xx = x - 1;
                    float v = 0.0f;
                    if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.h && c < a.ci) {
                        const size_t e = (((size_t)img * a.h + yy) * a.h + xx) * a.ci + c;
                        v = a.in8 ? imp_u8(a.in8[e]) : a.in[e];
                        if (a.relu) v = imp_relu(v);
                    }
                    pad[((size_t)y * hp + x) * cp + c] = v;
                }
        for (int y = 0; y < a.h; ++y)
            for (int x = 0; x < a.h; ++x) {
                for (int n = 0; n < a.co; ++n) acc[n] = 0.0f;
                for (int k = 0; k < kp; ++k) {
                    const int tap = k / cp;
                    const float v = pad[((size_t)(y + tap / 3) * hp + x + tap % 3) * cp + k % cp];
                    const float* w = a.wt + (size_t)k * a.co;
                    for (int n = 0; n < a.co; ++n) acc[n] = fmaf(v, w[n], acc[n]);
                }
                const size_t o = (((size_t)img * a.h + y) * a.h + x) * a.co;
                for (int n = 0; n < a.co; ++n)
                    a.out[o + n] = a.bias ? imp_epi_fwd(acc[n], a.bias[n], a.res ? a.res + o + n : nullptr)
                                          : imp_epi_dgrad(acc[n], a.mask ? a.mask + o + n : nullptr, a.res ? a.res + o + n : nullptr);
            }
    }
}

struct ImpWgradHost {
    const float* in;
    int ci, co, h;
    bool relu;
    const float* dy;
    float* gw;
    float* gb;
    int B;
    const uint8_t* in8 = nullptr;   // as in ImpConvHost
};

template <int V>
__attribute__((always_inline)) inline void imp_wgrad_host_impl(const ImpWgradHost& a) {
    const ImpGeom g = imp_geom(a.ci, a.co, a.h);
    const int64_t bands = imp_bands(g, a.h, a.B);
    const int parts = imp_parts(bands), jp = g.JP;
    std::vector<float> part((size_t)parts * a.co * jp), row(jp);
    for (int q = 0; q < parts; ++q) {
        float* acc = part.data() + (size_t)q * a.co * jp;
        for (int i = 0; i < a.co * jp; ++i) acc[i] = 0.0f;
        int64_t b0, b1;
        imp_part_range(bands, parts, q, &b0, &b1);
        for (int64_t b = b0; b < b1; ++b) {
            int64_t img0;
            int y0;
            imp_band(g, a.h, b, &img0, &y0);
            for (int64_t img = img0; img < img0 + g.NI && img < a.B; ++img)
                for (int y = y0; y < y0 + g.R && y < a.h; ++y)
                    for (int x = 0; x < a.h; ++x) {
                        for (int j = 0; j < jp; ++j) {
                            float v = j == g.KP ? 1.0f : 0.0f;
                            if (j < g.KP) {
                                const int tap = j / g.CP, c = j % g.CP, yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
                                if (yy >= 0 && yy < a.h && xx >= 0 && xx < a.h && c < a.ci) {
                                    const size_t e = (((size_t)img * a.h + yy) * a.h + xx) * a.ci + c;
                                    v = a.in8 ? imp_u8(a.in8[e]) : a.in[e];
                                    if (a.relu) v = imp_relu(v);
                                }
                            }
                            row[j] = v;
                        }
                        const float* d = a.dy + (((size_t)img * a.h + y) * a.h + x) * a.co;
                        for (int n = 0; n < a.co; ++n) {
                            float* r = acc + (size_t)n * jp;
                            for (int j = 0; j < jp; ++j) r[j] = fmaf(d[n], row[j], r[j]);
                        }
                    }
            // the dead steps that complete the band's last MFMA (impala_rows.h): 0 * 0 into every chain
            for (int dead = (4 - imp_band_pixels(g, a.h, img0, y0, a.B) % 4) % 4; dead > 0; --dead)
                for (int i = 0; i < a.co * jp; ++i) acc[i] = fmaf(0.0f, 0.0f, acc[i]);
        }
    }
    for (int n = 0; n < a.co; ++n)
        for (int j = 0; j <= g.KP; ++j) {
            if (j < g.KP && j % g.CP >= a.ci) continue;
            float s = 0.0f;
            for (int f = 0; f < kImpFoldGroups; ++f) {                 // imp_fold_kernel's order
                int q0, q1;
                imp_fold_range(parts, f, &q0, &q1);
                float r = 0.0f;
                for (int q = q0; q < q1; ++q) r = r + part[((size_t)q * a.co + n) * jp + j];
                s = s + r;
            }
            if (j == g.KP)
                a.gb[n] = s;
            else
                a.gw[((size_t)n * a.ci + j % g.CP) * 9 + j / g.CP] = s;
        }
}

__attribute__((target("avx2,fma"))) void imp_conv_host_fma(const ImpConvHost& a) { imp_conv_host_impl<1>(a); }
void imp_conv_host_plain(const ImpConvHost& a) { imp_conv_host_impl<0>(a); }
__attribute__((target("avx2,fma"))) void imp_wgrad_host_fma(const ImpWgradHost& a) { imp_wgrad_host_impl<1>(a); }
void imp_wgrad_host_plain(const ImpWgradHost& a) { imp_wgrad_host_impl<0>(a); }

bool imp_host_has_fma() {
    static const bool has = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    return has;
}
void imp_conv_host(const ImpConvHost& a) { imp_host_has_fma() ? imp_conv_host_fma(a) : imp_conv_host_plain(a); }
void imp_wgrad_host(const ImpWgradHost& a) { imp_host_has_fma() ? imp_wgrad_host_fma(a) : imp_wgrad_host_plain(a); }

// Dense Wt[k][n] of layer l: the forward's (dgrad = false) or the data gradient's.
std::vector<float> imp_wt_host(int f, const float* w, int l, bool dgrad) {
    const int ci = imp_layer_cin(f, l), co = imp_layer_cout(l);
    const int kp = dgrad ? 9 * co : 9 * imp_cpad(ci), nn = dgrad ? ci : co;
    std::vector<float> wt((size_t)kp * nn);
    for (int k = 0; k < kp; ++k)
        for (int n = 0; n < nn; ++n) wt[(size_t)k * nn + n] = dgrad ? imp_wt_dgrad(w, ci, co, k, n) : imp_wt_fwd(w, ci, k, n);
    return wt;
}

void imp_pool_fwd_host(const float* x, float* y, uint8_t* arg, int B, int h, int c) {
    const int ho = imp_half(h);
    for (int64_t img = 0; img < B; ++img)
        for (int oy = 0; oy < ho; ++oy)
            for (int ox = 0; ox < ho; ++ox)
                for (int ch = 0; ch < c; ++ch) {
                    const int64_t i = ((img * ho + oy) * ho + ox) * c + ch;
                    y[i] = imp_pool_window(x + img * h * h * c + ch, h, c, oy, ox, arg + i);
                }
}

void imp_pool_bwd_host(const float* g, const uint8_t* arg, float* dx, int B, int h, int c) {
    const int ho = imp_half(h);
    for (int64_t img = 0; img < B; ++img)
        for (int iy = 0; iy < h; ++iy)
            for (int ix = 0; ix < h; ++ix)
                for (int ch = 0; ch < c; ++ch) {
                    const int64_t base = img * ho * ho * c + ch;
                    dx[((img * h + iy) * h + ix) * c + ch] = imp_pool_grad(g + base, arg + base, ho, c, iy, ix);
                }
}

int imp_check_host(int f, const char* fn, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%d must be positive", fn, B);
    MI355_REQUIRE(H == imp_fam_h(f) && W == imp_fam_h(f) && C == imp_fam_c(f), MI355PPO_EINVAL, "%s: frames %dx%dx%d (only %dx%dx%d)", fn,
                  H, W, C, imp_fam_h(f), imp_fam_h(f), imp_fam_c(f));
    MI355_REQUIRE(ch0 == 16 && ch1 == 32 && ch2 == 32, MI355PPO_EINVAL, "%s: channels [%d, %d, %d] (only [16, 32, 32])", fn, ch0, ch1,
                  ch2);
    return MI355PPO_OK;
}

bool imp_pool_shape_ok(int B, int H, int W, int C) {
    for (int f : {kImpFam64, kImpFam84})
        for (int s = 0; s < kImpSeqs; ++s)
            if (B > 0 && H == W && H == imp_seq_h(f, s) && C == imp_seq_cout(s)) return true;
    return false;
}

// Family f's forward / backward; the frames are x (f32, the 64 family) or x8 (bytes, the 84 family).
int imp_fwd_host(int f, const char* fn, const float* x, const uint8_t* x8, const float* const* params, float* y, float* saved,
                 uint8_t* argmax, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    MI355_REQUIRE((x || x8) && params && y && saved && argmax, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int st = imp_check_host(f, fn, B, H, W, C, ch0, ch1, ch2)) return st;
    for (int i = 0; i < kImpParams; ++i) MI355_REQUIRE(params[i], MI355PPO_EINVAL, "%s: null pointer (params[%d])", fn, i);
    std::vector<float> big((size_t)B * imp_fam_h(f) * imp_fam_h(f) * 16);
    const float* xin = x;
    for (int s = 0; s < kImpSeqs; ++s) {
        const int ci = imp_seq_cin(f, s), c = imp_seq_cout(s), h = imp_seq_h(f, s), hp = imp_half(h), L = 5 * s;
        float* P = saved + imp_saved_offset(f, B, s, 0);
        float* h0 = saved + imp_saved_offset(f, B, s, 1);
        float* x1 = saved + imp_saved_offset(f, B, s, 2);
        float* h1 = saved + imp_saved_offset(f, B, s, 3);
        float* yo = s < 2 ? saved + imp_saved_offset(f, B, s, 4) : y;
        std::vector<float> wt = imp_wt_host(f, params[2 * L], L, false);
        imp_conv_host({xin, ci, c, h, false, wt.data(), params[2 * L + 1], nullptr, nullptr, big.data(), B, s == 0 ? x8 : nullptr});
        imp_pool_fwd_host(big.data(), P, argmax + imp_argmax_offset(f, B, s), B, h, c);
        const float* ins[4] = {P, h0, x1, h1};
        float* outs[4] = {h0, x1, h1, yo};
        const float* ress[4] = {nullptr, P, nullptr, x1};
        for (int i = 0; i < 4; ++i) {
            wt = imp_wt_host(f, params[2 * (L + 1 + i)], L + 1 + i, false);
            imp_conv_host({ins[i], c, c, hp, true, wt.data(), params[2 * (L + 1 + i) + 1], nullptr, ress[i], outs[i], B});
        }
        xin = yo;
    }
    return MI355PPO_OK;
}

int imp_bwd_host(int f, const char* fn, const float* x, const uint8_t* x8, const float* const* params, const float* saved,
                 const uint8_t* argmax, const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    MI355_REQUIRE((x || x8) && params && saved && argmax && dy && grads, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int st = imp_check_host(f, fn, B, H, W, C, ch0, ch1, ch2)) return st;
    for (int i = 0; i < kImpParams; ++i)
        MI355_REQUIRE(params[i] && grads[i], MI355PPO_EINVAL, "%s: null pointer (params / grads[%d])", fn, i);
    const size_t plane = (size_t)B * imp_plane(f, 0);
    std::vector<float> ga(plane), gb(plane), t(plane), big((size_t)B * imp_fam_h(f) * imp_fam_h(f) * 16);
    const float* g_in = dy;
    for (int s = kImpSeqs - 1; s >= 0; --s) {
        const int ci = imp_seq_cin(f, s), c = imp_seq_cout(s), h = imp_seq_h(f, s), hp = imp_half(h), L = 5 * s;
        const float* P = saved + imp_saved_offset(f, B, s, 0);
        const float* h0 = saved + imp_saved_offset(f, B, s, 1);
        const float* x1 = saved + imp_saved_offset(f, B, s, 2);
        const float* h1 = saved + imp_saved_offset(f, B, s, 3);
        const float* xin = s == 0 ? x : saved + imp_saved_offset(f, B, s - 1, 4);
        auto other = [&](const float* g) { return g == ga.data() ? gb.data() : ga.data(); };
        float* g1 = other(g_in);
        float* g2 = other(g1);
        std::vector<float> wt;
        // res_block1, then res_block0 (the order of bwd_seq in impala.hip)
        imp_wgrad_host({h1, c, c, hp, true, g_in, grads[2 * L + 8], grads[2 * L + 9], B});
        wt = imp_wt_host(f, params[2 * (L + 4)], L + 4, true);
        imp_conv_host({g_in, c, c, hp, false, wt.data(), nullptr, h1, nullptr, t.data(), B});
        imp_wgrad_host({x1, c, c, hp, true, t.data(), grads[2 * L + 6], grads[2 * L + 7], B});
        wt = imp_wt_host(f, params[2 * (L + 3)], L + 3, true);
        imp_conv_host({t.data(), c, c, hp, false, wt.data(), nullptr, x1, g_in, g1, B});
        imp_wgrad_host({h0, c, c, hp, true, g1, grads[2 * L + 4], grads[2 * L + 5], B});
        wt = imp_wt_host(f, params[2 * (L + 2)], L + 2, true);
        imp_conv_host({g1, c, c, hp, false, wt.data(), nullptr, h0, nullptr, t.data(), B});
        imp_wgrad_host({P, c, c, hp, true, t.data(), grads[2 * L + 2], grads[2 * L + 3], B});
        wt = imp_wt_host(f, params[2 * (L + 1)], L + 1, true);
        imp_conv_host({t.data(), c, c, hp, false, wt.data(), nullptr, P, g1, g2, B});
        imp_pool_bwd_host(g2, argmax + imp_argmax_offset(f, B, s), big.data(), B, h, c);
        imp_wgrad_host({xin, ci, c, h, false, big.data(), grads[2 * L], grads[2 * L + 1], B, s == 0 ? x8 : nullptr});
        if (s > 0) {
            float* gx = other(g2);
            wt = imp_wt_host(f, params[2 * L], L, true);
            imp_conv_host({big.data(), c, ci, h, false, wt.data(), nullptr, nullptr, nullptr, gx, B});
            g_in = gx;
        }
    }
    return MI355PPO_OK;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_impala_fwd_f32_cpu(const float* x, const float* const* params, float* y, float* saved,
                                                        uint8_t* argmax, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    return imp_fwd_host(kImpFam64, "mi355ppo_impala_fwd_f32_cpu", x, nullptr, params, y, saved, argmax, B, H, W, C, ch0, ch1, ch2);
}

extern "C" MI355PPO_API int mi355ppo_impala_bwd_f32_cpu(const float* x, const float* const* params, const float* saved,
                                                        const uint8_t* argmax, const float* dy, float* const* grads, int B, int H, int W,
                                                        int C, int ch0, int ch1, int ch2) {
    return imp_bwd_host(kImpFam64, "mi355ppo_impala_bwd_f32_cpu", x, nullptr, params, saved, argmax, dy, grads, B, H, W, C, ch0, ch1,
                        ch2);
}

extern "C" MI355PPO_API int mi355ppo_impala84_fwd_u8_cpu(const uint8_t* x, const float* const* params, float* y, float* saved,
                                                         uint8_t* argmax, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    return imp_fwd_host(kImpFam84, "mi355ppo_impala84_fwd_u8_cpu", nullptr, x, params, y, saved, argmax, B, H, W, C, ch0, ch1, ch2);
}

extern "C" MI355PPO_API int mi355ppo_impala84_bwd_u8_cpu(const uint8_t* x, const float* const* params, const float* saved,
                                                         const uint8_t* argmax, const float* dy, float* const* grads, int B, int H,
                                                         int W, int C, int ch0, int ch1, int ch2) {
    return imp_bwd_host(kImpFam84, "mi355ppo_impala84_bwd_u8_cpu", nullptr, x, params, saved, argmax, dy, grads, B, H, W, C, ch0, ch1,
                        ch2);
}

extern "C" MI355PPO_API int mi355ppo_impala_maxpool_fwd_f32_cpu(const float* x, float* y, uint8_t* argmax, int B, int H, int W, int C) {
    const char* fn = "mi355ppo_impala_maxpool_fwd_f32_cpu";
    MI355_REQUIRE(x && y && argmax, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(imp_pool_shape_ok(B, H, W, C), MI355PPO_EINVAL, "%s: B=%d %dx%dx%d (only the trunks' 64x64x16, 32x32x32, 16x16x32, 84x84x16, 42x42x32, 21x21x32)",
                  fn, B, H, W, C);
    imp_pool_fwd_host(x, y, argmax, B, H, C);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_impala_maxpool_bwd_f32_cpu(const float* dy, const uint8_t* argmax, float* dx, int B, int H, int W,
                                                                int C) {
    const char* fn = "mi355ppo_impala_maxpool_bwd_f32_cpu";
    MI355_REQUIRE(dy && argmax && dx, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(imp_pool_shape_ok(B, H, W, C), MI355PPO_EINVAL, "%s: B=%d %dx%dx%d (only the trunks' 64x64x16, 32x32x32, 16x16x32, 84x84x16, 42x42x32, 21x21x32)",
                  fn, B, H, W, C);
    imp_pool_bwd_host(dy, argmax, dx, B, H, C);
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------------------------ PQN (pqn.hip)
// The device's row functions (pqn_rows.h) and its fold orders (kPqnFold slots, kPqnRows-row partials, the sum-of-squares
// workgroups), run serially: every output equals the device's bit for bit.
namespace {

void pqn_td_scalars_cpu(const std::vector<float>& old, const std::vector<float>& sq, int M, float* scalars) {
    double to = 0.0, ts = 0.0;
    for (int t = 0; t < kPqnFold; ++t) {
        double so = 0.0, ss = 0.0;
        for (int k = t; k < M; k += kPqnFold) {
            so += (double)old[k];
            ss += (double)sq[k];
        }
        to += so;
        ts += ss;
    }
    scalars[0] = (float)(ts / (double)M);
    scalars[1] = (float)(to / (double)M);
}

inline int64_t pqn_clamp_index_cpu(int64_t i, int64_t B) { return i < 0 ? 0 : (i >= B ? B - 1 : i); }

}  // namespace

extern "C" MI355PPO_API int mi355ppo_pqn_egreedy_f32_cpu(const float* q, const int64_t* random_actions, const float* u, double epsilon,
                                                        float* actions_out, float* values_out, int64_t* action_i64_out, int N, int A) {
    const char* fn = "mi355ppo_pqn_egreedy_f32_cpu";
    MI355_REQUIRE(q && random_actions && u && actions_out && values_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(N > 0 && A > 0, MI355PPO_EINVAL, "%s: N=%d A=%d must be positive", fn, N, A);
    const float eps = (float)epsilon;
    for (int r = 0; r < N; ++r) {
        float v;
        const int64_t a = pqn_egreedy(q + (int64_t)r * A, 1, A, random_actions[r], u[r], eps, &v);
        actions_out[r] = (float)a;
        values_out[r] = v;
        if (action_i64_out) action_i64_out[r] = a;
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_qlambda_f32_cpu(const float* rewards, const float* dones, const float* values, const float* next_done,
                                                        const float* next_q, float* returns, int T, int N, int A, double gamma, double q_lambda) {
    const char* fn = "mi355ppo_pqn_qlambda_f32_cpu";
    MI355_REQUIRE(rewards && dones && values && next_done && next_q && returns, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(T > 0 && N > 0 && A > 0, MI355PPO_EINVAL, "%s: T=%d N=%d A=%d must be positive", fn, T, N, A);
    const float g = (float)gamma, lam = (float)q_lambda, oml = (float)(1.0 - q_lambda);
    for (int n = 0; n < N; ++n) {
        const float* nq = next_q + (int64_t)n * A;
        int64_t off = (int64_t)(T - 1) * N + n;
        float ret = pqn_qlambda_last(rewards[off], nq[pqn_argmax(nq, 1, A)], next_done[n], g);
        returns[off] = ret;
        for (int t = T - 2; t >= 0; --t) {
            const int64_t o1 = off;
            off -= N;
            ret = pqn_qlambda_step(rewards[off], ret, values[o1], dones[o1], g, lam, oml);
            returns[off] = ret;
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_td_loss_fwd_bwd_f32_cpu(const float* q, const int64_t* mb_inds, const float* b_actions,
                                                                const float* b_returns, float* dq, float* scalars_out, int M, int A, int64_t B) {
    const char* fn = "mi355ppo_pqn_td_loss_fwd_bwd_f32_cpu";
    MI355_REQUIRE(q && mb_inds && b_actions && b_returns && dq && scalars_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && A > 0 && B > 0, MI355PPO_EINVAL, "%s: M=%d A=%d B=%lld must be positive", fn, M, A, (long long)B);
    const float norm = (float)(2.0 / (double)M);
    std::vector<float> old(M), sq(M);
    for (int r = 0; r < M; ++r) {
        const int64_t i = pqn_clamp_index_cpu(mb_inds[r], B);
        old[r] = pqn_td_row(q + (int64_t)r * A, 1, A, b_actions[i], b_returns[i], norm, dq + (int64_t)r * A, 1, &sq[r]);
    }
    pqn_td_scalars_cpu(old, sq, M, scalars_out);
    return MI355PPO_OK;
}

static int pqn_mlp_shape_cpu(const char* fn, int N, int O, int A) {
    MI355_REQUIRE(N > 0 && O > 0 && O <= kPqnMaxObs && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL,
                  "%s: rows=%d obs_dim=%d n_actions=%d: the PQN MLP takes 1 <= obs_dim <= %d, 1 <= n_actions <= %d", fn, N, O, A, kPqnMaxObs,
                  kPqnMaxA);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_fwd_f32_cpu(const float* obs, const float* params, float* q_out, int N, int O, int A) {
    const char* fn = "mi355ppo_pqn_mlp_fwd_f32_cpu";
    MI355_REQUIRE(obs && params && q_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = pqn_mlp_shape_cpu(fn, N, O, A)) return rc;
    const PqnNet net = pqn_net(params, O, A);
    float h1[kPqnH1], h2[kPqnH2], rstd[2];
    for (int r = 0; r < N; ++r) pqn_row_forward(net, obs + (int64_t)r * O, 1, h1, h1, h2, h2, 1, q_out + (int64_t)r * A, 1, rstd);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_act_f32_cpu(const float* obs, const float* params, const int64_t* random_actions, const float* u,
                                                        double epsilon, float* actions_out, float* values_out, int64_t* action_i64_out,
                                                        float* obs_row_out, const float* done_in, float* done_row_out, int N, int O, int A) {
    const char* fn = "mi355ppo_pqn_mlp_act_f32_cpu";
    MI355_REQUIRE(obs && params && random_actions && u && actions_out && values_out && (!done_row_out || done_in), MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = pqn_mlp_shape_cpu(fn, N, O, A)) return rc;
    const PqnNet net = pqn_net(params, O, A);
    const float eps = (float)epsilon;
    float h1[kPqnH1], h2[kPqnH2], q[kPqnMaxA], rstd[2];
    for (int r = 0; r < N; ++r) {
        const float* x = obs + (int64_t)r * O;
        pqn_row_forward(net, x, 1, h1, h1, h2, h2, 1, q, 1, rstd);
        float v;
        const int64_t a = pqn_egreedy(q, 1, A, random_actions[r], u[r], eps, &v);
        actions_out[r] = (float)a;
        values_out[r] = v;
        if (action_i64_out) action_i64_out[r] = a;
        if (obs_row_out) memcpy(obs_row_out + (int64_t)r * O, x, sizeof(float) * O);
        if (done_row_out) done_row_out[r] = done_in[r];
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_td_fwd_bwd_f32_cpu(const float* b_obs, int64_t B, const int64_t* mb_inds, const float* params,
                                                               const float* b_actions, const float* b_returns, float* grads, float* scalars_out,
                                                               int M, int O, int A) {
    const char* fn = "mi355ppo_pqn_mlp_td_fwd_bwd_f32_cpu";
    MI355_REQUIRE(b_obs && mb_inds && params && b_actions && b_returns && grads && scalars_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%lld must be positive", fn, (long long)B);
    if (int rc = pqn_mlp_shape_cpu(fn, M, O, A)) return rc;
    const PqnNet net = pqn_net(params, O, A);
    const PqnUnits U = pqn_units(O, A);
    const int64_t P = pqn_param_count(O, A);
    const float norm = (float)(2.0 / (double)M);
    // the device's row-interleaved workspace, unit-major with stride M (the layout does not change any value)
    std::vector<float> ws((size_t)U.total * M);
    std::vector<float> old(M), sq(M);
    for (int r = 0; r < M; ++r) {
        const int64_t i = pqn_clamp_index_cpu(mb_inds[r], B);
        float* w = ws.data() + r;
        for (int k = 0; k < O; ++k) w[(int64_t)(U.x + k) * M] = b_obs[i * O + k];
        float rstd[2];
        float* xh1 = w + (int64_t)U.xh1 * M;
        float* a1 = w + (int64_t)U.a1 * M;
        float* xh2 = w + (int64_t)U.xh2 * M;
        float* a2 = w + (int64_t)U.a2 * M;
        float* dq = w + (int64_t)U.dq * M;
        pqn_row_forward(net, w + (int64_t)U.x * M, M, xh1, a1, xh2, a2, M, dq, M, rstd);
        old[r] = pqn_td_row(dq, M, A, b_actions[i], b_returns[i], norm, dq, M, &sq[r]);
        pqn_row_backward(net, dq, M, xh1, a1, xh2, a2, rstd, w + (int64_t)U.dy1 * M, w + (int64_t)U.dz1 * M, w + (int64_t)U.dy2 * M,
                         w + (int64_t)U.dz2 * M, M);
    }
    const int nblk = (M + kPqnRows - 1) / kPqnRows;
    for (int64_t e = 0; e < P; ++e) {
        int u1, u2;
        pqn_grad_units(e, O, A, &u1, &u2);
        const float* p1 = ws.data() + (int64_t)u1 * M;
        const float* p2 = u2 < 0 ? nullptr : ws.data() + (int64_t)u2 * M;
        float g = 0.0f;
        for (int b = 0; b < nblk; ++b) {
            const int r0 = b * kPqnRows, r1 = (r0 + kPqnRows < M) ? r0 + kPqnRows : M;
            float acc = 0.0f;
            if (p2)
                for (int k = r0; k < r1; ++k) acc = acc + p1[k] * p2[k];
            else
                for (int k = r0; k < r1; ++k) acc = acc + p1[k];
            g = g + acc;
        }
        grads[e] = g;
    }
    pqn_td_scalars_cpu(old, sq, M, scalars_out);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_clip_radam_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                                       double max_grad_norm, double lr, double beta1, double beta2, double eps, int64_t step,
                                                       float* total_norm_out) {
    const char* fn = "mi355ppo_clip_radam_f32_cpu";
    MI355_REQUIRE(params && grads && exp_avg && exp_avg_sq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld must be > 0", fn, (long long)n);
    float c[kPqnSched];
    if (int rc = mi355ppo_radam_schedule_f32(lr, beta1, beta2, step, c)) return rc;
    const int G = pqn_sumsq_blocks(n);
    double s = 0.0;
    for (int b = 0; b < G; ++b) {
        double part = 0.0;
        for (int t = 0; t < kPqnFold; ++t) {
            double slot = 0.0;
            for (int64_t i = (int64_t)b * 256 + t; i < n; i += (int64_t)G * 256) {
                const double a = (double)grads[i];
                slot += a * a;
            }
            part += slot;
        }
        s += part;
    }
    if (total_norm_out) *total_norm_out = (float)sqrt(s);
    RAdamParams R;
    R.max_norm = (float)max_grad_norm;
    R.w1 = (float)(1.0 - beta1);
    R.beta2 = (float)beta2;
    R.w2 = (float)(1.0 - beta2);
    R.eps = (float)eps;
    R.nblocks = G;
    const float coef = pqn_clip_coef(s, R.max_norm);
    for (int64_t i = 0; i < n; ++i) pqn_radam_elem(params[i], grads[i], exp_avg[i], exp_avg_sq[i], coef, R, c);
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------ recurrent PQN (pqn_lstm.hip)
// act: every FMA is the device's (lstm_dot128, the cell's products, pqn_lstm_q), expf / tanhf are libm's -- as for the scans, the
// state and q agree with the device to the last bits, not bit for bit.  h_out / c_out of env b are bit-equal to
// mi355ppo_lstm_seq_fwd_f32_cpu at T = 1.
extern "C" MI355PPO_API int mi355ppo_pqn_lstm_act_f32_cpu(const float* gx, const float* w_hh, const float* h_in, const float* c_in,
                                                         const float* done_in, const float* wq, const float* bq,
                                                         const int64_t* random_actions, const float* u, double epsilon, float* h_out,
                                                         float* c_out, float* q_out, float* actions_out, float* values_out,
                                                         int64_t* action_i64_out, float* done_row_out, int N, int H, int A) {
    const char* fn = "mi355ppo_pqn_lstm_act_f32_cpu";
    MI355_REQUIRE(gx && w_hh && h_in && c_in && done_in && wq && bq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(!h_out == !c_out, MI355PPO_EINVAL, "%s: h_out and c_out are both given or both NULL", fn);
    MI355_REQUIRE(!actions_out == !values_out && (!actions_out || (random_actions && u)) && (actions_out || !action_i64_out),
                  MI355PPO_EINVAL, "%s: actions_out, values_out, random_actions and u go together (all NULL: the bootstrap form)", fn);
    MI355_REQUIRE(h_out || q_out || actions_out, MI355PPO_EINVAL, "%s: null pointer (no output)", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(N > 0 && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL, "%s: N=%d A=%d: N must be positive, 1 <= A <= %d", fn, N, A, kPqnMaxA);
    const float eps = (float)epsilon;
    for (int b = 0; b < N; ++b) {
        float hk[kLstmH], ck[kLstmH], a[kLstmG], hn[kLstmH], q[kPqnMaxA];
        const float keep = 1.0f - done_in[b];
        for (int k = 0; k < kLstmH; ++k) {
            hk[k] = keep * h_in[(size_t)b * kLstmH + k];
            ck[k] = keep * c_in[(size_t)b * kLstmH + k];
        }
        for (int j = 0; j < kLstmG; ++j) a[j] = gx[(size_t)b * kLstmG + j] + lstm_dot128(w_hh + (size_t)j * kLstmH, hk);
        for (int k = 0; k < kLstmH; ++k) {
            const LstmCell s = lstm_cell_fwd(a[k], a[kLstmH + k], a[2 * kLstmH + k], a[3 * kLstmH + k], ck[k]);
            hn[k] = s.h;
            if (h_out) {
                h_out[(size_t)b * kLstmH + k] = s.h;
                c_out[(size_t)b * kLstmH + k] = s.c;
            }
        }
        for (int c = 0; c < A; ++c) {
            q[c] = pqn_lstm_q(wq + (size_t)c * kLstmH, hn, bq[c]);
            if (q_out) q_out[(size_t)b * A + c] = q[c];
        }
        if (actions_out) {
            float v;
            const int64_t act = pqn_egreedy(q, 1, A, random_actions[b], u[b], eps, &v);
            actions_out[b] = (float)act;
            values_out[b] = v;
            if (action_i64_out) action_i64_out[b] = act;
        }
        if (done_row_out) done_row_out[b] = done_in[b];
    }
    return MI355PPO_OK;
}

// td: the device's row function, its kPqnRows-row partials and their fold, run serially: every output equals the device's bits.
extern "C" MI355PPO_API int mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu(const float* h, const int64_t* mb_inds, const float* b_actions,
                                                                const float* b_returns, const float* wq, const float* bq, float* dh,
                                                                float* dwq, float* dbq, float* scalars_out, int M, int H, int A,
                                                                int64_t B) {
    const char* fn = "mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h && mb_inds && b_actions && b_returns && wq && bq && dh && dwq && dbq && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(M > 0 && B > 0 && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL, "%s: M=%d B=%lld A=%d: M, B must be positive, 1 <= A <= %d",
                  fn, M, (long long)B, A, kPqnMaxA);
    const float norm = (float)(2.0 / (double)M);
    std::vector<float> old(M), sq(M), g(M);
    std::vector<int> act(M);
    for (int r = 0; r < M; ++r) {
        const int64_t i = pqn_clamp_index(mb_inds[r], B);
        const PqnLstmTd t = pqn_lstm_td_row(h + (size_t)r * kLstmH, wq, bq, A, b_actions[i], b_returns[i], norm);
        old[r] = t.old;
        sq[r] = t.sq;
        g[r] = t.g;
        act[r] = t.a;
        for (int k = 0; k < kLstmH; ++k) dh[(size_t)r * kLstmH + k] = t.g * wq[(size_t)t.a * kLstmH + k];
    }
    const int nblk = (M + kPqnRows - 1) / kPqnRows;
    const int AH = A * kLstmH;
    for (int e = 0; e < AH + A; ++e) {
        float acc = 0.0f;
        for (int b = 0; b < nblk; ++b) {
            const int r0 = b * kPqnRows, r1 = (r0 + kPqnRows < M) ? r0 + kPqnRows : M;
            const float part = e < AH ? pqn_lstm_grad_partial(e, h, g.data() + r0, act.data() + r0, r0, r1)
                                      : pqn_lstm_bias_partial(e - AH, g.data() + r0, act.data() + r0, r1 - r0);
            acc = acc + part;
        }
        if (e < AH)
            dwq[e] = acc;
        else
            dbq[e - AH] = acc;
    }
    pqn_td_scalars_cpu(old, sq, M, scalars_out);
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------ DDPG / TD3 (offpolicy.hip)
// The device's element functions (offpolicy_rows.h) in the device's orders: dot products ascending from 0.0f, weight gradients per
// tile of kOpRows rows, tiles into their group's partial, groups ascending into the flat gradient, f64 slot folds for the scalars.
// Every output equals the device's bit for bit (op_tanh uses no libm function).  The tile helpers up to tile_backward_host serve
// the SAC and DQN / C51 twins below as well: the three families run the same three-layer network at different widths.
namespace {

constexpr int kOpXSh = kOpMaxObs + kOpMaxAct;

// out[r, j] = act(b[j] + sum_k xin[r, k] * W[j, k]) for the tile's kOpRows rows and j < J
template <bool RELU>
void tile_layer_host(const float* xin, int xs, int K, const float* W, const float* b, int J, float* out, int os) {
    for (int r = 0; r < kOpRows; ++r)
        for (int j = 0; j < J; ++j) {
            float acc = 0.0f;
            for (int k = 0; k < K; ++k) acc = op_mac(acc, xin[r * xs + k], W[(int64_t)j * K + k]);
            const float v = acc + b[j];
            out[r * os + j] = RELU ? op_relu(v) : v;
        }
}

// io[r, k] = relu'(io[r, k]) * sum_{j < J} dz[r * ds + j] * W[j * K + k] for k < K (in place over the layer's ReLU output)
void tile_dgrad_host(const float* dz, int ds, int J, const float* W, int K, float* io, int ios) {
    for (int r = 0; r < kOpRows; ++r)
        for (int k = 0; k < K; ++k) {
            float acc = 0.0f;
            for (int j = 0; j < J; ++j) acc = op_mac(acc, dz[r * ds + j], W[(int64_t)j * K + k]);
            io[r * ios + k] = op_relu_bwd(io[r * ios + k], acc);
        }
}

void op_wgrad_host(const float* dz, int ds, const float* in, int is, int J, int K, float* part_w, float* part_b, bool first, int nr) {
    for (int j = 0; j < J; ++j) {
        for (int k = 0; k < K; ++k) {
            float acc = 0.0f;
            for (int r = 0; r < nr; ++r) acc = op_mac(acc, dz[r * ds + j], in[r * is + k]);
            float& p = part_w[(int64_t)j * K + k];
            p = first ? acc : p + acc;
        }
        float acc = 0.0f;
        for (int r = 0; r < nr; ++r) acc = acc + dz[r * ds + j];
        part_b[j] = first ? acc : part_b[j] + acc;
    }
}

void op_fold_host(const float* part, int G, int64_t P, float* grads) {
    for (int64_t e = 0; e < P; ++e) {
        float acc = 0.0f;
        for (int b = 0; b < G; ++b) acc = acc + part[(int64_t)b * P + e];
        grads[e] = acc;
    }
}

// The batch's rows: the ring's (batch_inds[m], env_inds[m]), both clamped into range as the kernels' ring_row clamps them
// (offpolicy_wg.h), or, without indices (the rollout's observations), m itself.
struct TileRows {
    const int64_t *bi, *ei;
    int64_t slots;
    int N;
    int64_t operator()(int m) const { return bi ? op_clamp(bi[m], slots) * N + op_clamp(ei[m], N) : (int64_t)m; }
};

// x[r, k] = src[row(r0 + r), k] for k < O and the tile's kOpRows rows, zero past the batch's `rows`
void tile_gather_host(const float* src, const TileRows& row, int r0, int rows, int O, float* x, int xs) {
    for (int r = 0; r < kOpRows; ++r) {
        const bool in = r0 + r < rows;
        const float* s = src + (in ? row(r0 + r) : 0) * O;
        for (int k = 0; k < O; ++k) x[r * xs + k] = in ? s[k] : 0.0f;
    }
}

// One tile of a three-layer network: the input rows (stride xs) and the two hidden layers' outputs (widths H1 / H2, their strides).
struct TileNet {
    float* x;
    int xs;
    float* h1;
    int H1;
    float* h2;
    int H2;
};

// Linear(K, H1) - ReLU - Linear(H1, H2) - ReLU: what every network of the three families starts with
template <class Net>
void tile_hidden_host(const Net& n, int K, const TileNet& B) {
    tile_layer_host<true>(B.x, B.xs, K, n.w1, n.b1, B.H1, B.h1, B.H1);
    tile_layer_host<true>(B.h1, B.H1, B.H1, n.w2, n.b2, B.H2, B.h2, B.H2);
}

// ... - Linear(H2, n.J) into out (row stride os): the whole forward of an OpNet or a DqNet
template <class Net>
void tile_forward_host(const Net& n, int K, const TileNet& B, float* out, int os) {
    tile_hidden_host(n, K, B);
    tile_layer_host<false>(B.h2, B.H2, B.H2, n.w3, n.b3, n.J, out, os);
}

// The backward below h2, which holds d loss / d (layer 2's output), masked: layer 2's weight gradient, the masked data gradient
// into h1, layer 1's weight gradient -- into the group's partial p at the offsets off.
template <class Net, class Off>
void tile_backward_lower_host(const Net& n, const Off& off, int K, const TileNet& B, float* p, bool first, int nr) {
    op_wgrad_host(B.h2, B.H2, B.h1, B.H1, B.H2, B.H1, p + off.w2, p + off.b2, first, nr);
    tile_dgrad_host(B.h2, B.H2, B.H2, n.w2, B.H1, B.h1, B.H1);
    op_wgrad_host(B.h1, B.H1, B.x, B.xs, B.H1, K, p + off.w1, p + off.b1, first, nr);
}

// The whole chain from dz = d loss / d (layer 3's output), row stride ds: wgrad, dgrad, wgrad, dgrad, wgrad.
template <class Net, class Off>
void tile_backward_host(const Net& n, const Off& off, int K, const float* dz, int ds, const TileNet& B, float* p, bool first, int nr) {
    op_wgrad_host(dz, ds, B.h2, B.H2, n.J, B.H2, p + off.w3, p + off.b3, first, nr);
    tile_dgrad_host(dz, ds, n.J, n.w3, B.H2, B.h2, B.H2);
    tile_backward_lower_host(n, off, K, B, p, first, nr);
}

struct OpTile {
    std::vector<float> x, a1, a2, c1, c2;
    float mu[kOpRows * kOpMaxAct], tv[kOpRows * kOpMaxAct], qv[2 * kOpRows], dq[kOpRows];
    OpTile() : x(kOpRows * kOpXSh), a1(kOpRows * kOpH), a2(kOpRows * kOpH), c1(kOpRows * kOpH), c2(kOpRows * kOpH) {}
    TileNet a() { return TileNet{x.data(), kOpXSh, a1.data(), kOpH, a2.data(), kOpH}; }       // the actor's hidden layers (or a lone critic's)
    TileNet c() { return TileNet{x.data(), kOpXSh, c1.data(), kOpH, c2.data(), kOpH}; }       // a critic's next to the actor's
};

void op_actor_host(const OpNet& an, const float* scale, const float* bias, OpTile& T) {
    tile_forward_host(an, an.K, T.a(), T.mu, an.J);
    for (int r = 0; r < kOpRows; ++r)
        for (int a = 0; a < an.J; ++a) {
            const float th = op_tanh(T.mu[r * an.J + a]);
            T.tv[r * an.J + a] = th;
            T.x[r * kOpXSh + an.K + a] = op_action(th, scale[a], bias[a]);
        }
}

// q of the tile's (obs | action) rows through the n_critics target critics into T.qv (critic c at c * kOpRows)
void op_target_q_host(const float* target_critics, int n_critics, int O, int A, OpTile& T) {
    for (int c = 0; c < n_critics; ++c) {
        const OpNet qn = op_net(target_critics + c * op_critic_count(O, A), O + A, 1);
        tile_forward_host(qn, qn.K, T.a(), T.qv + c * kOpRows, 1);
    }
}

// One critic over the tile's (obs | action) rows, forward into q and back to the action: out[r * A + a] = dq[r] * d q / d action[r, a].
void op_critic_daction_host(const OpNet& qn, const float* dq, int O, int A, OpTile& T, float* q, float* out) {
    const TileNet B = T.c();
    tile_forward_host(qn, qn.K, B, q, 1);
    tile_dgrad_host(dq, 1, 1, qn.w3, kOpH, B.h2, kOpH);
    tile_dgrad_host(B.h2, kOpH, kOpH, qn.w2, kOpH, B.h1, kOpH);
    for (int r = 0; r < kOpRows; ++r)
        for (int a = 0; a < A; ++a) {
            float acc = 0.0f;
            for (int j = 0; j < kOpH; ++j) acc = op_mac(acc, B.h1[r * kOpH + j], qn.w1[(int64_t)j * qn.K + O + a]);
            out[r * A + a] = acc;
        }
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_replay_add_f32_cpu(const float* obs, const float* next_obs, const float* actions, const float* rewards,
                                                       const float* dones, float* ring_obs, float* ring_next_obs, float* ring_actions,
                                                       float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int N, int O, int A) {
    const char* fn = "mi355ppo_replay_add_f32_cpu";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(N > 0 && O > 0 && A > 0 && slots > 0 && pos >= 0 && pos < slots, MI355PPO_EINVAL,
                  "%s: N=%d O=%d A=%d slots=%lld pos=%lld: sizes must be positive and 0 <= pos < slots", fn, N, O, A, (long long)slots,
                  (long long)pos);
    const size_t no = (size_t)N * O, na = (size_t)N * A;
    memcpy(ring_obs + pos * no, obs, no * sizeof(float));
    memcpy(ring_next_obs + pos * no, next_obs, no * sizeof(float));
    memcpy(ring_actions + pos * na, actions, na * sizeof(float));
    memcpy(ring_rewards + pos * N, rewards, (size_t)N * sizeof(float));
    memcpy(ring_dones + pos * N, dones, (size_t)N * sizeof(float));
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_ddpg_act_f32_cpu(const float* obs, const float* actor_params, const float* action_scale,
                                                     const float* action_bias, const float* noise_row, const float* low, const float* high,
                                                     float* actions_out, int N, int O, int A) {
    const char* fn = "mi355ppo_ddpg_act_f32_cpu";
    MI355_REQUIRE(obs && actor_params && action_scale && action_bias && low && high && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = op_shape(fn, N, O, A)) return rc;
    const OpNet an = op_net(actor_params, O, A);
    const TileRows plain{nullptr, nullptr, 0, 0};
    OpTile T;
    for (int r0 = 0; r0 < N; r0 += kOpRows) {
        tile_gather_host(obs, plain, r0, N, O, T.x.data(), kOpXSh);
        op_actor_host(an, action_scale, action_bias, T);
        for (int r = 0; r < kOpRows && r0 + r < N; ++r)
            for (int a = 0; a < A; ++a)
                actions_out[(int64_t)(r0 + r) * A + a] = op_explore(T.x[r * kOpXSh + O + a], noise_row ? noise_row[a] : 0.0f, low[a], high[a]);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_td3_target_f32_cpu(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                                       const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                                       const float* target_actor, const float* target_critics, int n_critics,
                                                       const float* action_scale, const float* action_bias, const float* noise,
                                                       double policy_noise, double noise_clip, double low0, double high0, double gamma,
                                                       float* next_q_value, float* next_actions_out, int M, int O, int A) {
    const char* fn = "mi355ppo_td3_target_f32_cpu";
    MI355_REQUIRE(ring_next_obs && ring_rewards && ring_dones && target_actor && target_critics && action_scale && action_bias && next_q_value &&
                      batch_inds && env_inds,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE((n_critics == 1 || n_critics == 2) && slots > 0 && n_envs > 0, MI355PPO_EINVAL,
                  "%s: n_critics=%d must be 1 or 2, slots=%lld and n_envs=%d positive", fn, n_critics, (long long)slots, n_envs);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    const OpNet an = op_net(target_actor, O, A);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    const float pn = (float)policy_noise, nc = (float)noise_clip, lo0 = (float)low0, hi0 = (float)high0, g = (float)gamma;
    OpTile T;
    for (int r0 = 0; r0 < M; r0 += kOpRows) {
        tile_gather_host(ring_next_obs, ring, r0, M, O, T.x.data(), kOpXSh);
        op_actor_host(an, action_scale, action_bias, T);
        for (int r = 0; r < kOpRows && r0 + r < M; ++r)
            for (int a = 0; a < A; ++a) {
                float& v = T.x[r * kOpXSh + O + a];
                if (noise) v = op_smooth(v, noise[(int64_t)(r0 + r) * A + a], pn, nc, action_scale[a], lo0, hi0);
                if (next_actions_out) next_actions_out[(int64_t)(r0 + r) * A + a] = v;
            }
        op_target_q_host(target_critics, n_critics, O, A, T);
        for (int r = 0; r < kOpRows && r0 + r < M; ++r) {
            const int64_t row = ring(r0 + r);
            const float q = (n_critics == 2) ? op_min(T.qv[r], T.qv[kOpRows + r]) : T.qv[r];
            next_q_value[r0 + r] = op_td_target(ring_rewards[row], ring_dones[row], g, q);
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_td3_critic_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_actions, const int64_t* batch_inds,
                                                               const int64_t* env_inds, int64_t slots, int n_envs, const float* critics,
                                                               int n_critics, const float* next_q_value, float* grads, float* scalars_out, int M,
                                                               int O, int A) {
    const char* fn = "mi355ppo_td3_critic_fwd_bwd_f32_cpu";
    MI355_REQUIRE(ring_obs && ring_actions && critics && next_q_value && grads && scalars_out && batch_inds && env_inds, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE((n_critics == 1 || n_critics == 2) && slots > 0 && n_envs > 0, MI355PPO_EINVAL,
                  "%s: n_critics=%d must be 1 or 2, slots=%lld and n_envs=%d positive", fn, n_critics, (long long)slots, n_envs);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    const int K = O + A, G = op_groups(M), ntiles = op_tiles(M);
    const int64_t Pq = op_critic_count(O, A), P = n_critics * Pq;
    const OpOff off = op_off(K, 1);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    const float norm = (float)(2.0 / (double)M);
    std::vector<float> part((size_t)G * P), rows((size_t)4 * M);
    OpTile T;
    for (int c = 0; c < n_critics; ++c) {
        const OpNet qn = op_net(critics + c * Pq, K, 1);
        for (int tl = 0; tl < ntiles; ++tl) {
            const int g = tl % G, r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
            const bool first = tl == g;
            float* p = part.data() + ((int64_t)g * n_critics + c) * Pq;
            tile_gather_host(ring_obs, ring, r0, M, O, T.x.data(), kOpXSh);
            tile_gather_host(ring_actions, ring, r0, M, A, T.x.data() + O, kOpXSh);
            tile_forward_host(qn, K, T.a(), T.qv, 1);
            for (int r = 0; r < kOpRows; ++r) {
                float d = 0.0f;
                if (r < nr) {
                    float sq;
                    d = op_mse_row(T.qv[r], next_q_value[r0 + r], norm, &sq);
                    rows[(size_t)(2 * c) * M + r0 + r] = T.qv[r];
                    rows[(size_t)(2 * c + 1) * M + r0 + r] = sq;
                }
                T.dq[r] = d;
            }
            tile_backward_host(qn, off, K, T.dq, 1, T.a(), p, first, nr);
        }
    }
    op_fold_host(part.data(), G, P, grads);
    for (int s = 0; s < 2 * n_critics; ++s) scalars_out[s] = 1.0f * op_fold_mean_host(rows.data() + (size_t)s * M, M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_td3_actor_fwd_bwd_f32_cpu(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds,
                                                              int64_t slots, int n_envs, const float* actor, const float* qf1,
                                                              const float* action_scale, const float* action_bias, float* grads,
                                                              float* actor_loss_out, float* dq_daction_out, int M, int O, int A) {
    const char* fn = "mi355ppo_td3_actor_fwd_bwd_f32_cpu";
    MI355_REQUIRE(ring_obs && actor && qf1 && action_scale && action_bias && grads && actor_loss_out && batch_inds && env_inds, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE(slots > 0 && n_envs > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, n_envs);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    const int G = op_groups(M), ntiles = op_tiles(M);
    const int64_t Pa = op_actor_count(O, A);
    const OpNet an = op_net(actor, O, A), qn = op_net(qf1, O + A, 1);
    const OpOff off = op_off(O, A);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    const float dqv = (float)(-1.0 / (double)M);
    std::vector<float> part((size_t)G * Pa), rows(M);
    OpTile T;
    for (int tl = 0; tl < ntiles; ++tl) {
        const int g = tl % G, r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        float* p = part.data() + (int64_t)g * Pa;
        tile_gather_host(ring_obs, ring, r0, M, O, T.x.data(), kOpXSh);
        op_actor_host(an, action_scale, action_bias, T);
        for (int r = 0; r < kOpRows; ++r) T.dq[r] = r < nr ? dqv : 0.0f;
        op_critic_daction_host(qn, T.dq, O, A, T, T.qv, T.mu);
        for (int r = 0; r < kOpRows; ++r) {
            if (r < nr) rows[r0 + r] = T.qv[r];
            for (int a = 0; a < A; ++a) {
                float& v = T.mu[r * A + a];
                if (dq_daction_out && r < nr) dq_daction_out[(int64_t)(r0 + r) * A + a] = v;
                v = op_dmu(v, action_scale[a], T.tv[r * A + a]);
            }
        }
        tile_backward_host(an, off, O, T.mu, A, T.a(), p, first, nr);
    }
    op_fold_host(part.data(), G, Pa, grads);
    *actor_loss_out = -1.0f * op_fold_mean_host(rows.data(), M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_polyak_f32_cpu(const float* params, float* target_params, int64_t n, double tau) {
    const char* fn = "mi355ppo_polyak_f32_cpu";
    MI355_REQUIRE(params && target_params, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld must be > 0", fn, (long long)n);
    const float t = (float)tau, omt = (float)(1.0 - tau);
    for (int64_t i = 0; i < n; ++i) target_params[i] = op_polyak(params[i], target_params[i], t, omt);
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------ SAC (sac.hip)
// The device's element functions (sac_rows.h over offpolicy_rows.h) in the device's orders; every output equals the device's bit for
// bit (op_exp / op_log / op_tanh use no libm function).  The tile helpers are the DDPG / TD3 section's.
namespace {

struct SacTileH {
    float mu[kOpRows * kOpMaxAct], us[kOpRows * kOpMaxAct], y[kOpRows * kOpMaxAct], std[kOpRows * kOpMaxAct], th[kOpRows * kOpMaxAct],
        arg[kOpRows * kOpMaxAct], g1[kOpRows * kOpMaxAct], g2[kOpRows * kOpMaxAct], lpr[kOpRows];
};

// get_action of one tile (wg_sac_policy): T.x's rows hold the observations
void sac_policy_host(const SacNet& an, const float* scale, const float* bias, const float* eps, int r0, int rows, OpTile& T, SacTileH& S) {
    const int A = an.A;
    tile_hidden_host(an, an.K, T.a());
    tile_layer_host<false>(T.a2.data(), kOpH, kOpH, an.wm, an.bm, A, S.mu, A);
    tile_layer_host<false>(T.a2.data(), kOpH, kOpH, an.ws, an.bs, A, S.us, A);
    for (int r = 0; r < kOpRows; ++r) {
        float acc = 0.0f;
        for (int a = 0; a < A; ++a) {
            const int t = r * A + a;
            const float ev = (r0 + r < rows) ? eps[(int64_t)(r0 + r) * A + a] : 0.0f;
            const SacElem e = sac_elem(S.mu[t], S.us[t], ev, scale[a], bias[a]);
            S.y[t] = e.y;
            S.std[t] = e.std;
            S.th[t] = e.th;
            S.arg[t] = e.arg;
            T.x[r * kOpXSh + an.K + a] = e.action;
            acc = acc + e.lp;
        }
        S.lpr[r] = acc;
    }
}

void sac_dgrad2_host(const float* dza, const float* Wa, const float* dzb, const float* Wb, int J, float* io) {
    for (int k = 0; k < kOpH; ++k)
        for (int r = 0; r < kOpRows; ++r) {
            float acc = 0.0f;
            for (int j = 0; j < J; ++j) acc = op_mac(acc, dza[r * J + j], Wa[j * kOpH + k]);
            for (int j = 0; j < J; ++j) acc = op_mac(acc, dzb[r * J + j], Wb[j * kOpH + k]);
            io[r * kOpH + k] = op_relu_bwd(io[r * kOpH + k], acc);
        }
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_sac_exp_log_f32_cpu(const float* x, float* exp_out, float* log_out, int64_t n) {
    const char* fn = "mi355ppo_sac_exp_log_f32_cpu";
    MI355_REQUIRE(x && (exp_out || log_out), MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld must be > 0", fn, (long long)n);
    for (int64_t i = 0; i < n; ++i) {
        if (exp_out) exp_out[i] = op_exp(x[i]);
        if (log_out) log_out[i] = op_log(x[i]);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sac_policy_f32_cpu(const float* obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                       int n_envs, const float* actor, const float* action_scale, const float* action_bias,
                                                       const float* eps, float* actions_out, float* log_pi_out, int rows, int O, int A) {
    const char* fn = "mi355ppo_sac_policy_f32_cpu";
    MI355_REQUIRE(obs && actor && action_scale && action_bias && eps && (actions_out || log_pi_out), MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE((batch_inds == nullptr) == (env_inds == nullptr), MI355PPO_EINVAL, "%s: batch_inds and env_inds come together", fn);
    MI355_REQUIRE(!batch_inds || (slots > 0 && n_envs > 0), MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots,
                  n_envs);
    if (int rc = op_shape(fn, rows, O, A)) return rc;
    const SacNet an = sac_net(actor, O, A);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    OpTile T;
    SacTileH S;
    for (int r0 = 0; r0 < rows; r0 += kOpRows) {
        tile_gather_host(obs, ring, r0, rows, O, T.x.data(), kOpXSh);
        sac_policy_host(an, action_scale, action_bias, eps, r0, rows, T, S);
        for (int r = 0; r < kOpRows && r0 + r < rows; ++r) {
            if (actions_out)
                for (int a = 0; a < A; ++a) actions_out[(int64_t)(r0 + r) * A + a] = T.x[r * kOpXSh + O + a];
            if (log_pi_out) log_pi_out[r0 + r] = S.lpr[r];
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sac_target_f32_cpu(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                                       const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                                       const float* actor, const float* target_critics, const float* action_scale,
                                                       const float* action_bias, const float* eps, const float* alpha, double gamma,
                                                       float* next_q_value, float* next_actions_out, float* log_pi_out, int M, int O, int A) {
    const char* fn = "mi355ppo_sac_target_f32_cpu";
    MI355_REQUIRE(ring_next_obs && ring_rewards && ring_dones && actor && target_critics && action_scale && action_bias && eps && alpha &&
                      next_q_value && batch_inds && env_inds,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(slots > 0 && n_envs > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, n_envs);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    const SacNet an = sac_net(actor, O, A);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    const float g = (float)gamma;
    OpTile T;
    SacTileH S;
    for (int r0 = 0; r0 < M; r0 += kOpRows) {
        tile_gather_host(ring_next_obs, ring, r0, M, O, T.x.data(), kOpXSh);
        sac_policy_host(an, action_scale, action_bias, eps, r0, M, T, S);
        if (next_actions_out)
            for (int r = 0; r < kOpRows && r0 + r < M; ++r)
                for (int a = 0; a < A; ++a) next_actions_out[(int64_t)(r0 + r) * A + a] = T.x[r * kOpXSh + O + a];
        op_target_q_host(target_critics, 2, O, A, T);
        for (int r = 0; r < kOpRows && r0 + r < M; ++r) {
            const int64_t row = ring(r0 + r);
            next_q_value[r0 + r] = op_td_target(ring_rewards[row], ring_dones[row], g, sac_soft_q(T.qv[r], T.qv[kOpRows + r], alpha[0], S.lpr[r]));
            if (log_pi_out) log_pi_out[r0 + r] = S.lpr[r];
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sac_actor_fwd_bwd_f32_cpu(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds,
                                                              int64_t slots, int n_envs, const float* actor, const float* critics,
                                                              const float* action_scale, const float* action_bias, const float* eps,
                                                              const float* alpha, float* grads, float* actor_loss_out, float* log_pi_out,
                                                              float* dmean_out, float* du_out, int M, int O, int A) {
    const char* fn = "mi355ppo_sac_actor_fwd_bwd_f32_cpu";
    MI355_REQUIRE(ring_obs && actor && critics && action_scale && action_bias && eps && alpha && grads && actor_loss_out && batch_inds && env_inds,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(slots > 0 && n_envs > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, n_envs);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    const int K = O + A, G = op_groups(M), ntiles = op_tiles(M);
    const int64_t Pa = sac_actor_count(O, A), Pq = op_critic_count(O, A);
    const SacNet an = sac_net(actor, O, A);
    const SacOff off = sac_off(O, A);
    const TileRows ring{batch_inds, env_inds, slots, n_envs};
    const float inv_m = (float)(1.0 / (double)M), al = alpha[0];
    const float one[kOpRows] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    std::vector<float> part((size_t)G * Pa), rows(M);
    OpTile T;
    SacTileH S;
    for (int tl = 0; tl < ntiles; ++tl) {
        const int g = tl % G, r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        float* p = part.data() + (int64_t)g * Pa;
        tile_gather_host(ring_obs, ring, r0, M, O, T.x.data(), kOpXSh);
        sac_policy_host(an, action_scale, action_bias, eps, r0, M, T, S);
        for (int c = 0; c < 2; ++c)
            op_critic_daction_host(op_net(critics + c * Pq, K, 1), one, O, A, T, T.qv + c * kOpRows, c == 0 ? S.g1 : S.g2);
        for (int r = 0; r < kOpRows; ++r) {
            const float q1 = T.qv[r], q2 = T.qv[kOpRows + r];
            if (r < nr) {
                rows[r0 + r] = sac_actor_row(al, S.lpr[r], q1, q2);
                if (log_pi_out) log_pi_out[r0 + r] = S.lpr[r];
            }
            for (int a = 0; a < A; ++a) {
                const int t = r * A + a;
                float dm = 0.0f, du = 0.0f;
                if (r < nr) {
                    const float dact = (-inv_m) * (sac_min_w(q1, q2) * S.g1[t] + sac_min_w(q2, q1) * S.g2[t]);
                    SacElem e;
                    e.y = S.y[t];
                    e.std = S.std[t];
                    e.th = S.th[t];
                    e.arg = S.arg[t];
                    e.action = 0.0f;
                    e.lp = 0.0f;
                    sac_elem_bwd(e, eps[(int64_t)(r0 + r) * A + a], action_scale[a], dact, al * inv_m, &dm, &du);
                    if (dmean_out) dmean_out[(int64_t)(r0 + r) * A + a] = dm;
                    if (du_out) du_out[(int64_t)(r0 + r) * A + a] = du;
                }
                S.mu[t] = dm;
                S.us[t] = du;
            }
        }
        op_wgrad_host(S.mu, A, T.a2.data(), kOpH, A, kOpH, p + off.wm, p + off.bm, first, nr);
        op_wgrad_host(S.us, A, T.a2.data(), kOpH, A, kOpH, p + off.ws, p + off.bs, first, nr);
        sac_dgrad2_host(S.mu, an.wm, S.us, an.ws, A, T.a2.data());
        tile_backward_lower_host(an, off, O, T.a(), p, first, nr);
    }
    op_fold_host(part.data(), G, Pa, grads);
    *actor_loss_out = 1.0f * op_fold_mean_host(rows.data(), M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sac_alpha_f32_cpu(const float* log_pi, int M, double target_entropy, float* log_alpha, float* exp_avg,
                                                      float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step,
                                                      float* alpha_out, float* alpha_loss_out) {
    const char* fn = "mi355ppo_sac_alpha_f32_cpu";
    MI355_REQUIRE(log_pi && log_alpha && exp_avg && exp_avg_sq && alpha_out && alpha_loss_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && step >= 1, MI355PPO_EINVAL, "%s: rows=%d must be > 0 and step=%lld >= 1", fn, M, (long long)step);
    AdamParams P;
    P.scale = 1.0f;
    P.max_norm = 0.0f;
    P.w1 = (float)(1.0 - beta1);
    P.beta2 = (float)beta2;
    P.w2 = (float)(1.0 - beta2);
    float sc[2];
    mi355ppo_adam_schedule_f32(lr, beta1, beta2, step, sc);
    P.neg_step = sc[0];
    P.bc2_sqrt = sc[1];
    P.eps = (float)eps;
    P.nblocks = 0;
    P.zero_grads = 1;
    const float te = (float)target_entropy;
    double tot = 0.0;
    for (int t = 0; t < kOpFold; ++t) {
        double s = 0.0;
        for (int k = t; k < M; k += kOpFold) s += (double)(log_pi[k] + te);
        tot += s;
    }
    float la = log_alpha[0], m = exp_avg[0], v = exp_avg_sq[0];
    const float loss = sac_alpha_loss(op_exp(la), tot / (double)M);
    float gr = loss;
    adam_elem(la, gr, m, v, 1.0f, P);
    log_alpha[0] = la;
    exp_avg[0] = m;
    exp_avg_sq[0] = v;
    alpha_out[0] = op_exp(la);
    alpha_loss_out[0] = loss;
    return MI355PPO_OK;
}

// ------------------------------------------------------------------------------------------------ DQN / C51 (dqn.hip)
// The device's element functions (dqn_rows.h over sac_rows.h / offpolicy_rows.h) in the device's orders: tiles of kOpRows rows, dot
// products ascending from 0.0f, the softmax and the projection per atom in ascending order, weight gradients per tile into their
// group's partial, groups ascending into the flat gradient, f64 slot folds for the scalars.  Every output equals the device's bit
// for bit.  The tile helpers are the DDPG / TD3 section's, at QNetwork's widths.
namespace {

struct DqTile {
    std::vector<float> x, h1, h2, z, pl, pu, pdl, pdu, tp;
    float qv[kOpRows * kDqMaxAct], yv[kOpRows], dq[kOpRows];
    int act[kOpRows];
    DqTile()
        : x(kOpRows * kDqMaxObs), h1(kOpRows * kDqH1), h2(kOpRows * kDqH2), z(kOpRows * kDqMaxOut), pl(kOpRows * kDqMaxAtoms),
          pu(kOpRows * kDqMaxAtoms), pdl(kOpRows * kDqMaxAtoms), pdu(kOpRows * kDqMaxAtoms), tp(kOpRows * kDqMaxAtoms) {}
    TileNet net() { return TileNet{x.data(), kDqMaxObs, h1.data(), kDqH1, h2.data(), kDqH2}; }
};

// the network over the tile's rows into T.z, then per action the Q value (C51: the softmax in place and its expectation) into T.qv
void dq_qvalues_host(const DqNet& net, DqTile& T, int n, int na, const float* atoms) {
    tile_forward_host(net, net.O, T.net(), T.z.data(), kDqMaxOut);
    for (int r = 0; r < kOpRows; ++r)
        for (int a = 0; a < n; ++a) {
            float* za = T.z.data() + r * kDqMaxOut + a * na;
            T.qv[r * kDqMaxAct + a] = (na > 1) ? dq_softmax_q(za, na, atoms, za) : za[0];
        }
}

// dq_update_kernel<C51> on the host
template <bool C51>
int dq_update_cpu(const float* ring_obs, const float* ring_next_obs, const float* ring_actions, const float* ring_rewards,
                  const float* ring_dones, const TileRows& ring, const float* online, const float* target, const float* atoms, float gamma,
                  float vmin, float vmax, float norm, float* grads, float* scalars_out, float* aux_a, float* aux_b, int M, int O, int n, int na) {
    const int J = n * na, G = op_groups(M), ntiles = op_tiles(M);
    const int64_t P = dq_count(O, J);
    const DqNet tn = dq_net(target, O, J), qn = dq_net(online, O, J);
    const DqOff off = dq_off(O, J);
    std::vector<float> part((size_t)G * P), rows((size_t)2 * M);
    DqTile T;
    const int PS = kDqMaxAtoms, ZS = kDqMaxOut;
    for (int tl = 0; tl < ntiles; ++tl) {
        const int g = tl % G, r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        float* p = part.data() + (int64_t)g * P;
        tile_gather_host(ring_next_obs, ring, r0, M, O, T.x.data(), kDqMaxObs);
        dq_qvalues_host(tn, T, n, na, atoms);
        if constexpr (C51) {
            const float delta_z = atoms[1] - atoms[0];
            for (int r = 0; r < kOpRows; ++r) {
                const int a = dq_argmax(T.qv + r * kDqMaxAct, n);
                for (int j = 0; j < na; ++j) {
                    C51Proj e;
                    e.l = e.u = -1.0f;
                    e.dml = e.dmu = 0.0f;
                    if (r < nr) {
                        const int64_t row = ring(r0 + r);
                        const float pj = T.z[r * ZS + a * na + j];
                        e = c51_proj_elem(ring_rewards[row], ring_dones[row], gamma, atoms[j], vmin, vmax, delta_z, na, pj, false);
                        if (aux_a) aux_a[(int64_t)(r0 + r) * na + j] = pj;
                    }
                    T.pl[r * PS + j] = e.l;
                    T.pu[r * PS + j] = e.u;
                    T.pdl[r * PS + j] = e.dml;
                    T.pdu[r * PS + j] = e.dmu;
                }
                for (int k = 0; k < na; ++k) {
                    const float v = c51_proj_atom(k, &T.pl[r * PS], &T.pu[r * PS], &T.pdl[r * PS], &T.pdu[r * PS], na);
                    T.tp[r * PS + k] = v;
                    if (aux_b && r < nr) aux_b[(int64_t)(r0 + r) * na + k] = v;
                }
            }
        } else {
            for (int r = 0; r < kOpRows; ++r) {
                float y = 0.0f;
                if (r < nr) {
                    const int64_t row = ring(r0 + r);
                    if (aux_a)
                        for (int a = 0; a < n; ++a) aux_a[(int64_t)(r0 + r) * n + a] = T.qv[r * kDqMaxAct + a];
                    y = dq_td_target(ring_rewards[row], ring_dones[row], gamma, T.qv[r * kDqMaxAct + dq_argmax(T.qv + r * kDqMaxAct, n)]);
                    if (aux_b) aux_b[r0 + r] = y;
                }
                T.yv[r] = y;
            }
        }
        for (int r = 0; r < kOpRows; ++r) T.act[r] = r < nr ? dq_action_index(ring_actions[ring(r0 + r)], n) : 0;
        tile_gather_host(ring_obs, ring, r0, M, O, T.x.data(), kDqMaxObs);
        dq_qvalues_host(qn, T, n, na, atoms);
        if constexpr (C51) {
            for (int r = 0; r < kOpRows; ++r) {
                float s = 0.0f, dot = 0.0f;
                for (int k = 0; k < na; ++k) {
                    const C51Loss e = c51_loss_elem(T.tp[r * PS + k], T.z[r * ZS + T.act[r] * na + k], norm);
                    T.pdl[r * PS + k] = e.g;
                    s = s + e.term;
                    dot = dot + e.gp;
                }
                if (r < nr) {
                    rows[r0 + r] = -s;
                    rows[(size_t)M + r0 + r] = T.qv[r * kDqMaxAct + T.act[r]];
                }
                for (int j = 0; j < J; ++j) {
                    const int a = j / na, k = j - a * na;
                    T.z[r * ZS + j] = (r < nr && a == T.act[r]) ? c51_dlogit(T.z[r * ZS + j], T.pdl[r * PS + k], dot) : 0.0f;
                }
            }
        } else {
            for (int r = 0; r < kOpRows; ++r) {
                float d = 0.0f;
                if (r < nr) {
                    float sq;
                    const float q = T.qv[r * kDqMaxAct + T.act[r]];
                    d = op_mse_row(q, T.yv[r], norm, &sq);
                    rows[r0 + r] = sq;
                    rows[(size_t)M + r0 + r] = q;
                }
                for (int j = 0; j < J; ++j) T.z[r * ZS + j] = (j == T.act[r]) ? d : 0.0f;
            }
        }
        tile_backward_host(qn, off, O, T.z.data(), ZS, T.net(), p, first, nr);
    }
    op_fold_host(part.data(), G, P, grads);
    for (int s = 0; s < 2; ++s) scalars_out[s] = 1.0f * op_fold_mean_host(rows.data() + (size_t)s * M, M);
    return MI355PPO_OK;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_dqn_act_f32_cpu(const float* obs, const float* params, const float* atoms, int64_t* actions_out,
                                                    float* q_out, int N, int O, int n_actions, int n_atoms) {
    const char* fn = "mi355ppo_dqn_act_f32_cpu";
    MI355_REQUIRE(obs && params && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = dq_shape(fn, N, O, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms == 1 || atoms, MI355PPO_EINVAL, "%s: n_atoms=%d needs the atoms", fn, n_atoms);
    const DqNet qn = dq_net(params, O, n_actions * n_atoms);
    const TileRows plain{nullptr, nullptr, 0, 0};
    DqTile T;
    for (int r0 = 0; r0 < N; r0 += kOpRows) {
        tile_gather_host(obs, plain, r0, N, O, T.x.data(), kDqMaxObs);
        dq_qvalues_host(qn, T, n_actions, n_atoms, atoms);
        for (int r = 0; r < kOpRows && r0 + r < N; ++r) {
            if (q_out)
                for (int a = 0; a < n_actions; ++a) q_out[(int64_t)(r0 + r) * n_actions + a] = T.qv[r * kDqMaxAct + a];
            actions_out[r0 + r] = (int64_t)dq_argmax(T.qv + r * kDqMaxAct, n_actions);
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_dqn_td_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                                           const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                           const int64_t* env_inds, int64_t slots, int n_envs, const float* online,
                                                           const float* target, double gamma, float* grads, float* scalars_out,
                                                           float* target_q_out, float* td_target_out, int M, int O, int n_actions) {
    const char* fn = "mi355ppo_dqn_td_fwd_bwd_f32_cpu";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && online && target && grads && scalars_out &&
                      batch_inds && env_inds, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(slots > 0 && n_envs > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, n_envs);
    if (int rc = dq_shape(fn, M, O, n_actions, 1)) return rc;
    return dq_update_cpu<false>(ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, TileRows{batch_inds, env_inds, slots, n_envs},
                                online, target, nullptr, (float)gamma, 0.0f, 0.0f, (float)(2.0 / (double)M), grads, scalars_out, target_q_out,
                                td_target_out, M, O, n_actions, 1);
}

extern "C" MI355PPO_API int mi355ppo_c51_fwd_bwd_f32_cpu(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                                        const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                        const int64_t* env_inds, int64_t slots, int n_envs, const float* online,
                                                        const float* target, const float* atoms, double gamma, double v_min, double v_max,
                                                        float* grads, float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M,
                                                        int O, int n_actions, int n_atoms) {
    const char* fn = "mi355ppo_c51_fwd_bwd_f32_cpu";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && online && target && atoms && grads &&
                      scalars_out && batch_inds && env_inds, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(slots > 0 && n_envs > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, n_envs);
    if (int rc = dq_shape(fn, M, O, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms >= 2, MI355PPO_EINVAL, "%s: n_atoms=%d: the projection needs two atoms (delta_z = atoms[1] - atoms[0])", fn, n_atoms);
    return dq_update_cpu<true>(ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, TileRows{batch_inds, env_inds, slots, n_envs},
                               online, target, atoms, (float)gamma, (float)v_min, (float)v_max, (float)(1.0 / (double)M), grads, scalars_out,
                               next_pmfs_out, target_pmfs_out, M, O, n_actions, n_atoms);
}

// ------------------------------------------------------------------------------------------------ Atari DQN / C51 (dqn_atari.hip)
// The frame ring's two copies and the wide heads, from dqn_atari_rows.h / dqn_rows.h in the device's orders: dot products ascending
// from 0.0f, the softmax, the projection and the loss sums per atom in ascending order, dh over the taken action's atoms, dW / db over
// the rows that took the action, the scalars through the f64 slot fold.  Every output equals the device's bit for bit.
namespace {

// z (N, J) = h W^T + b
void da_forward_host(const float* h, const float* w, const float* b, int N, int J, float* z) {
    for (int r = 0; r < N; ++r)
        for (int j = 0; j < J; ++j) z[(int64_t)r * J + j] = da_dot(h + (int64_t)r * kDaH, w + (int64_t)j * kDaH, b[j]);
}

// q[a] of one row; with atoms, the pmfs replace the logits
void da_qvalues_host(float* z, int n, int na, const float* atoms, float* q) {
    for (int a = 0; a < n; ++a) q[a] = (na > 1) ? dq_softmax_q(z + a * na, na, atoms, z + a * na) : z[a];
}

// qh_fwd_kernel<kDaH>, da_row_kernel<C51> and da_wgrad_kernel on the host
template <bool C51>
int da_update_cpu(const float* h, const float* h_next, const float* w, const float* b, const float* w_target, const float* b_target,
                  const float* atoms, const int64_t* actions, const float* rewards, const float* dones, float gamma, float vmin, float vmax,
                  float norm, float* dh, float* dw, float* db, float* scalars_out, float* aux_a, float* aux_b, int M, int n, int na) {
    const int J = n * na;
    std::vector<float> zo((size_t)M * J), zt((size_t)M * J), dz((size_t)M * na), rows((size_t)2 * M), tmp((size_t)5 * na);
    std::vector<int> act(M);
    float qt[kDqMaxAct], qo[kDqMaxAct];
    da_forward_host(h, w, b, M, J, zo.data());
    da_forward_host(h_next, w_target, b_target, M, J, zt.data());
    for (int r = 0; r < M; ++r) {
        float *t = zt.data() + (size_t)r * J, *o = zo.data() + (size_t)r * J, *d = dz.data() + (size_t)r * na;
        da_qvalues_host(t, n, na, atoms, qt);
        da_qvalues_host(o, n, na, atoms, qo);
        const int best = dq_argmax(qt, n), a = (int)op_clamp(actions[r], n);
        act[r] = a;
        if constexpr (C51) {
            rows[r] = c51_row_host(t + best * na, o + a * na, atoms, rewards[r], dones[r], gamma, vmin, vmax, atoms[1] - atoms[0], na, norm, false,
                                   aux_a ? aux_a + (int64_t)r * na : nullptr, aux_b ? aux_b + (int64_t)r * na : nullptr, tmp.data(), d);
        } else {
            if (aux_a)
                for (int k = 0; k < n; ++k) aux_a[(int64_t)r * n + k] = qt[k];
            const float y = dq_td_target(rewards[r], dones[r], gamma, qt[best]);
            if (aux_b) aux_b[r] = y;
            float sq;
            d[0] = op_mse_row(qo[a], y, norm, &sq);
            rows[r] = sq;
        }
        rows[(size_t)M + r] = qo[a];
        for (int k = 0; k < kDaH; ++k) dh[(int64_t)r * kDaH + k] = da_dh(d, na, w + (int64_t)a * na * kDaH, k);
    }
    for (int j = 0; j < J; ++j) {
        const int a = j / na, k0 = j - a * na;
        for (int k = 0; k < kDaH; ++k) dw[(int64_t)j * kDaH + k] = da_wgrad(act.data(), dz.data(), na, M, a, k0, h, k);
        db[j] = da_wgrad(act.data(), dz.data(), na, M, a, k0, nullptr, 0);
    }
    for (int s = 0; s < 2; ++s) scalars_out[s] = op_fold_mean_host(rows.data() + (size_t)s * M, M);
    return MI355PPO_OK;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_replay_add_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                                      const float* dones, uint8_t* ring_frames, int64_t* ring_actions, float* ring_rewards,
                                                      float* ring_dones, int64_t pos, int64_t slots, int n_envs) {
    const char* fn = "mi355ppo_replay_add_u8_cpu";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_frames && ring_actions && ring_rewards && ring_dones, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(pos >= 0 && pos < slots && n_envs <= (1 << 16), MI355PPO_EINVAL, "%s: pos=%lld slots=%lld n_envs=%d: 0 <= pos < slots, n_envs <= 65536",
                  fn, (long long)pos, (long long)slots, n_envs);
    for (int which = (slots == 1 ? 1 : 0); which < 2; ++which)
        for (int e = 0; e < n_envs; ++e) {
            const uint8_t* stack = (which ? next_obs : obs) + (int64_t)e * (kDaPlanes * kDaPix);
            uint8_t* dst = ring_frames + 4 * da_frame(which ? da_next_slot(pos, slots) : pos, e, n_envs);
            for (int p = 0; p < kDaPix; ++p) {
                const uint32_t v = da_pack(stack, p);
                memcpy(dst + 4 * (int64_t)p, &v, 4);
            }
        }
    for (int e = 0; e < n_envs; ++e) {
        ring_actions[pos * n_envs + e] = actions[e];
        ring_rewards[pos * n_envs + e] = rewards[e];
        ring_dones[pos * n_envs + e] = dones[e];
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_replay_gather_u8_cpu(const uint8_t* ring_frames, const int64_t* ring_actions, const float* ring_rewards,
                                                         const float* ring_dones, const int64_t* batch_inds, const int64_t* env_inds,
                                                         int64_t slots, int n_envs, uint8_t* frames_out, int64_t* actions_out, float* rewards_out,
                                                         float* dones_out, int M) {
    const char* fn = "mi355ppo_replay_gather_u8_cpu";
    MI355_REQUIRE(ring_frames && ring_actions && ring_rewards && ring_dones && batch_inds && env_inds && frames_out && actions_out && rewards_out &&
                      dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(M >= 1 && M <= kDaMaxRows, MI355PPO_EINVAL, "%s: rows=%d: 1 <= rows <= %d", fn, M, kDaMaxRows);
    da_gather_host(ring_frames, nullptr, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs, true, frames_out, actions_out,
                   rewards_out, dones_out, M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_dqn_head_act_f32_cpu(const float* h, const float* w, const float* b, const float* atoms, int64_t* actions_out,
                                                         float* q_out, int N, int hidden, int n_actions, int n_atoms) {
    const char* fn = "mi355ppo_dqn_head_act_f32_cpu";
    MI355_REQUIRE(h && w && b && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, N, hidden, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms == 1 || atoms, MI355PPO_EINVAL, "%s: n_atoms=%d needs the atoms", fn, n_atoms);
    const int J = n_actions * n_atoms;
    std::vector<float> z((size_t)N * J);
    da_forward_host(h, w, b, N, J, z.data());
    float q[kDqMaxAct];
    for (int r = 0; r < N; ++r) {
        da_qvalues_host(z.data() + (size_t)r * J, n_actions, n_atoms, atoms, q);
        if (q_out)
            for (int a = 0; a < n_actions; ++a) q_out[(int64_t)r * n_actions + a] = q[a];
        actions_out[r] = (int64_t)dq_argmax(q, n_actions);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_dqn_head_td_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b,
                                                                const float* w_target, const float* b_target, const int64_t* actions,
                                                                const float* rewards, const float* dones, double gamma, float* dh, float* dw,
                                                                float* db, float* scalars_out, float* target_q_out, float* td_target_out, int M,
                                                                int hidden, int n_actions) {
    const char* fn = "mi355ppo_dqn_head_td_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h && h_next && w && b && w_target && b_target && actions && rewards && dones && dh && dw && db && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, 1)) return rc;
    return da_update_cpu<false>(h, h_next, w, b, w_target, b_target, nullptr, actions, rewards, dones, (float)gamma, 0.0f, 0.0f,
                                (float)(2.0 / (double)M), dh, dw, db, scalars_out, target_q_out, td_target_out, M, n_actions, 1);
}

extern "C" MI355PPO_API int mi355ppo_c51_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b,
                                                             const float* w_target, const float* b_target, const float* atoms,
                                                             const int64_t* actions, const float* rewards, const float* dones, double gamma,
                                                             double v_min, double v_max, float* dh, float* dw, float* db, float* scalars_out,
                                                             float* next_pmfs_out, float* target_pmfs_out, int M, int hidden, int n_actions,
                                                             int n_atoms) {
    const char* fn = "mi355ppo_c51_head_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h && h_next && w && b && w_target && b_target && actions && rewards && dones && dh && dw && db && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms >= 2 && atoms, MI355PPO_EINVAL, "%s: n_atoms=%d: the projection needs the atoms, at least two (delta_z = atoms[1] - atoms[0])",
                  fn, n_atoms);
    return da_update_cpu<true>(h, h_next, w, b, w_target, b_target, atoms, actions, rewards, dones, (float)gamma, (float)v_min, (float)v_max,
                               (float)(1.0 / (double)M), dh, dw, db, scalars_out, next_pmfs_out, target_pmfs_out, M, n_actions, n_atoms);
}

// ------------------------------------------------------------------------------------------------ QDagger head (qdagger.hip)
// qh_fwd_kernel<256, 256>, qd_row_kernel and qd_wgrad_kernel on the host, from qdagger_rows.h in the device's orders.
extern "C" MI355PPO_API int mi355ppo_qdagger_head_act_f32_cpu(const float* h, const float* w, const float* b, int64_t* actions_out, float* q_out,
                                                             int N, int hidden, int n_actions) {
    const char* fn = "mi355ppo_qdagger_head_act_f32_cpu";
    MI355_REQUIRE(h && w && b && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = qd_shape(fn, N, hidden, n_actions)) return rc;
    float q[kDqMaxAct];
    for (int r = 0; r < N; ++r) {
        for (int j = 0; j < n_actions; ++j) {
            q[j] = qd_dot(h + (int64_t)r * kQdH, w + (int64_t)j * kQdH, b[j]);
            if (q_out) q_out[(int64_t)r * n_actions + j] = q[j];
        }
        actions_out[r] = (int64_t)dq_argmax(q, n_actions);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_qdagger_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* w, const float* b,
                                                                 const float* w_target, const float* b_target, const float* teacher_q,
                                                                 const int64_t* actions, const float* rewards, const float* dones, double gamma,
                                                                 double temperature, double distill_coeff, float* dh, float* dw, float* db,
                                                                 float* scalars_out, float* target_q_out, float* td_target_out, int M,
                                                                 int hidden, int n_actions) {
    const char* fn = "mi355ppo_qdagger_head_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h && h_next && w && b && w_target && b_target && teacher_q && actions && rewards && dones && dh && dw && db && scalars_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = qd_shape(fn, M, hidden, n_actions)) return rc;
    MI355_REQUIRE(temperature > 0.0, MI355PPO_EINVAL, "%s: temperature=%g must be positive", fn, temperature);
    const int n = n_actions;
    const float norm = (float)(2.0 / (double)M), ck = (float)(distill_coeff / temperature);
    std::vector<float> dq((size_t)M * n), rows((size_t)3 * M);
    float qo[kDqMaxAct], qt[kDqMaxAct];
    for (int r = 0; r < M; ++r) {
        for (int j = 0; j < n; ++j) {
            qo[j] = qd_dot(h + (int64_t)r * kQdH, w + (int64_t)j * kQdH, b[j]);
            qt[j] = qd_dot(h_next + (int64_t)r * kQdH, w_target + (int64_t)j * kQdH, b_target[j]);
            if (target_q_out) target_q_out[(int64_t)r * n + j] = qt[j];
        }
        float* d = dq.data() + (size_t)r * n;
        const QdRow R = qd_row(qo, qt, teacher_q + (int64_t)r * n, n, (int)op_clamp(actions[r], n), rewards[r], dones[r], (float)gamma,
                               (float)temperature, norm, ck, d);
        if (td_target_out) td_target_out[r] = R.y;
        rows[r] = R.sq;
        rows[(size_t)M + r] = R.qa;
        rows[(size_t)2 * M + r] = R.kl;
        for (int k = 0; k < kQdH; ++k) dh[(int64_t)r * kQdH + k] = qd_dh(d, n, w, k);
    }
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < kQdH; ++k) dw[(int64_t)j * kQdH + k] = qd_wgrad(dq.data() + j, n, M, h, k);
        db[j] = qd_wgrad(dq.data() + j, n, M, nullptr, 0);
    }
    const float q_loss = op_fold_mean_host(rows.data(), M), distill = qd_fold_sum_host(rows.data() + (size_t)2 * M, M);
    scalars_out[0] = qd_loss(q_loss, (float)distill_coeff, distill);
    scalars_out[1] = q_loss;
    scalars_out[2] = distill;
    scalars_out[3] = op_fold_mean_host(rows.data() + (size_t)M, M);
    return MI355PPO_OK;
}
