// SAC (cleanrl/sac_continuous_action.py): the stochastic tanh-Gaussian policy (get_action), the soft TD target, the policy update
// (forward + hand-derived backward + flat gradient) and the entropy coefficient's step (gfx950).
//
// The mapping is offpolicy.hip's (its header comment; helpers in offpolicy_wg.h): a workgroup of 256 threads takes a tile of kOpRows
// rows through a whole network, plain f32 VALU, fixed-order folds, no atomics.  What is new here:
//
//   heads     fc_mean and fc_logstd are two wg_head passes (8 * 2A exceeds 256 threads at A = 20, and fc_mean's bias sits between
//             the two matrices); thread (row, a) then runs get_action on its element (sac_elem) and thread `row` adds the row's
//             log_pi in ascending a.
//   critics   the policy update runs the two online critics one after the other through the same two hidden-row buffers: forward,
//             then backward with dq = 1 down to the action columns of the first layer (the critics get no gradient).  The loss is
//             linear in the two d q_c / d action, so they are combined per row with torch.min's backward weights afterwards.
//   backward  thread (row, a) maps d loss / d action and d loss / d log_pi to the gradients at mean and at fc_logstd's output
//             (sac_elem_bwd); the two heads' data gradients are added in one pass over both matrices.
//   alpha     one workgroup: f64 slot fold of log_pi + target_entropy, the loss, its gradient and one Adam step on the scalar.
//
// A network's pointers are formed per phase behind op_here (three networks live across the tile loop would not fit the SGPRs).
// No entry point allocates or synchronises; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "ppo_rows.h"
#include "sac_rows.h"
#include "offpolicy_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kSacE = kOpRows * kOpMaxAct;          // (row, action) elements of a tile

// the per-element state get_action leaves for the backward
struct SacTile {
    float *mu, *us, *y, *std, *th, *arg, *lp, *lpr;
};

// The actor's pointers formed where one layer uses them (op_here: offpolicy_wg.h), so that they die with that layer.
__device__ __forceinline__ SacNet sac_net_here(const float* actor, int O, int A) { return sac_net(actor, op_here(O), op_here(A)); }
// ring_row with the ring's bounds formed at the gather (the clamps' `slots - 1` / `N - 1` would otherwise live across the tile loop)
__device__ __forceinline__ int64_t ring_row_here(const OpRing& R, int m) {
    int64_t slots = R.slots;
    asm volatile("" : "+s"(slots));
    const int N = op_here(R.N);
    return op_clamp(R.bi[m], slots) * N + op_clamp(R.ei[m], (int64_t)N);
}
// The same for an optional output: its null test is made where it is used instead of being carried across the tile loop.
__device__ __forceinline__ float* ptr_here(float* p) {
    asm volatile("" : "+s"(p));
    return p;
}

// get_action of one tile: x's rows hold the observations; the action goes to x[r, K + a], the row's log_pi to S.lpr[r].
// eps (rows, A) is read for rows r0 + r < rows, 0 beyond.  a1 / a2 keep the hidden rows.  Ends with a barrier.
__device__ void wg_sac_policy(const float* __restrict__ actor, int O, int A, const float* __restrict__ scale, const float* __restrict__ bias,
                              const float* __restrict__ eps, int r0, int rows, float* x, float* a1, float* a2, const SacTile& S,
                              float* tile) {
    {
        const SacNet an = sac_net_here(actor, O, A);
        wg_forward<true>(x, kOpXS, an.K, an.w1, an.b1, a1, kOpH, tile);
    }
    {
        const SacNet an = sac_net_here(actor, O, A);
        wg_forward<true>(a1, kOpH, kOpH, an.w2, an.b2, a2, kOpH, tile);
    }
    {
        const SacNet an = sac_net_here(actor, O, A);
        wg_head(a2, kOpH, an.wm, an.bm, A, S.mu);
    }
    {
        const SacNet an = sac_net_here(actor, O, A);
        wg_head(a2, kOpH, an.ws, an.bs, A, S.us);
    }
    const int t = threadIdx.x;
    A = op_here(A);
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        const float ev = (r0 + r < rows) ? eps[(int64_t)(r0 + r) * A + a] : 0.0f;
        const SacElem e = sac_elem(S.mu[t], S.us[t], ev, scale[a], bias[a]);
        S.y[t] = e.y;
        S.std[t] = e.std;
        S.th[t] = e.th;
        S.arg[t] = e.arg;
        S.lp[t] = e.lp;
        x[r * kOpXS + O + a] = e.action;
    }
    __syncthreads();
    if (t < kOpRows) {
        float acc = 0.0f;
#pragma unroll 1
        for (int a = 0; a < A; ++a) acc = acc + S.lp[t * A + a];
        S.lpr[t] = acc;
    }
    __syncthreads();
}

// io[r, k] = relu'(io[r, k]) * (sum_j dza[r * J + j] * Wa[j, k] + sum_j dzb[r * J + j] * Wb[j, k]), head a first, j ascending.
__device__ void wg_dgrad2_masked(const float* dza, const float* __restrict__ Wa, const float* dzb, const float* __restrict__ Wb, int J,
                                 float* io) {
    const int t = threadIdx.x;
    float acc[kOpRows];
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) acc[r] = 0.0f;
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
        const float w = Wa[j * kOpH + t];
#pragma unroll
        for (int r = 0; r < kOpRows; ++r) acc[r] = op_mac(acc[r], dza[r * J + j], w);
    }
#pragma unroll 1
    for (int j = 0; j < J; ++j) {
        const float w = Wb[j * kOpH + t];
#pragma unroll
        for (int r = 0; r < kOpRows; ++r) acc[r] = op_mac(acc[r], dzb[r * J + j], w);
    }
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) io[r * kOpH + t] = op_relu_bwd(io[r * kOpH + t], acc[r]);
    __syncthreads();
}

#define SAC_TILE_LDS                                                                                                              \
    __shared__ float x[kOpRows * kOpXS], a1[kOpRows * kOpH], a2[kOpRows * kOpH], tile[kOpKT * kOpTileLd], s_mu[kSacE], s_us[kSacE], \
        s_y[kSacE], s_std[kSacE], s_th[kSacE], s_arg[kSacE], s_lp[kSacE], s_lpr[kOpRows];                                          \
    const SacTile S = {s_mu, s_us, s_y, s_std, s_th, s_arg, s_lp, s_lpr}

// ---------------------------------------------------------------------------------------------------------------- kernels
// bi == nullptr: obs is a dense (rows, O) array; otherwise a ring array gathered through (bi, ei)
__global__ __launch_bounds__(256) void sac_policy_kernel(const float* __restrict__ obs, const int64_t* __restrict__ bi,
                                                         const int64_t* __restrict__ ei, int64_t slots, int N, const float* __restrict__ actor,
                                                         const float* __restrict__ scale, const float* __restrict__ bias,
                                                         const float* __restrict__ eps, float* __restrict__ actions_out,
                                                         float* __restrict__ log_pi_out, int rows, int O, int A) {
    SAC_TILE_LDS;
    const int t = threadIdx.x, r0 = blockIdx.x * kOpRows;
    for (int i = t; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        float v = 0.0f;
        if (r0 + r < rows) {
            const int64_t row = bi ? op_clamp(bi[r0 + r], slots) * N + op_clamp(ei[r0 + r], N) : (int64_t)(r0 + r);
            v = obs[row * O + k];
        }
        x[r * kOpXS + k] = v;
    }
    __syncthreads();
    wg_sac_policy(actor, O, A, scale, bias, eps, r0, rows, x, a1, a2, S, tile);
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        if (actions_out && r0 + r < rows) actions_out[(int64_t)(r0 + r) * A + a] = x[r * kOpXS + O + a];
    }
    if (log_pi_out && t < kOpRows && r0 + t < rows) log_pi_out[r0 + t] = s_lpr[t];
}

__global__ __launch_bounds__(256) void sac_target_kernel(OpRing R, const float* __restrict__ actor, const float* __restrict__ critics_t,
                                                         const float* __restrict__ scale, const float* __restrict__ bias,
                                                         const float* __restrict__ eps, const float* __restrict__ alpha, float gamma,
                                                         float* __restrict__ y, float* __restrict__ next_act_out,
                                                         float* __restrict__ log_pi_out, int M, int O, int A) {
    SAC_TILE_LDS;
    __shared__ float qv[2 * kOpRows];
    const int t = threadIdx.x, r0 = blockIdx.x * kOpRows;
    for (int i = t; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        x[r * kOpXS + k] = (r0 + r < M) ? R.next_obs[ring_row(R, r0 + r) * O + k] : 0.0f;
    }
    __syncthreads();
    wg_sac_policy(actor, O, A, scale, bias, eps, r0, M, x, a1, a2, S, tile);
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        if (next_act_out && r0 + r < M) next_act_out[(int64_t)(r0 + r) * A + a] = x[r * kOpXS + O + a];
    }
    const int64_t Pq = op_critic_count(O, A);
    for (int c = 0; c < 2; ++c) {
        const OpNet qn = op_net(critics_t + c * Pq, O + A, 1);
        wg_forward<true>(x, kOpXS, O + A, qn.w1, qn.b1, a1, kOpH, tile);
        wg_forward<true>(a1, kOpH, kOpH, qn.w2, qn.b2, a2, kOpH, tile);
        wg_head(a2, kOpH, qn.w3, qn.b3, 1, qv + c * kOpRows);
    }
    if (t < kOpRows && r0 + t < M) {
        const int64_t row = ring_row(R, r0 + t);
        y[r0 + t] = op_td_target(R.rewards[row], R.dones[row], gamma, sac_soft_q(qv[t], qv[kOpRows + t], alpha[0], s_lpr[t]));
        if (log_pi_out) log_pi_out[r0 + t] = s_lpr[t];
    }
}

// ws: rowvals (Mp: alpha * log_pi - min_q), then partials [G][Pa]
__global__ __launch_bounds__(256) void sac_actor_kernel(OpRing R, const float* __restrict__ actor, const float* __restrict__ critics,
                                                        const float* __restrict__ scale, const float* __restrict__ bias,
                                                        const float* __restrict__ eps, const float* __restrict__ alpha,
                                                        float* __restrict__ ws, float* __restrict__ log_pi_out, float* __restrict__ dmean_out,
                                                        float* __restrict__ du_out, int M, int Mp, int O, int A, int G, float inv_m) {
    SAC_TILE_LDS;
    __shared__ float c1[kOpRows * kOpH], c2[kOpRows * kOpH], g2[kSacE], qv[2 * kOpRows], one[kOpRows];
    float* g1 = s_lp;                                   // the elements' log_prob terms are dead once the rows' sums are formed
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t Pa = sac_actor_count(O, A);
    float* part = ws + Mp + (int64_t)g * Pa;
    const int ntiles = op_tiles(M);
    if (t < kOpRows) one[t] = 1.0f;
    for (int tl = g; tl < ntiles; tl += G) {
        const int r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        {
            const int Oh = op_here(O);
            for (int i = t; i < kOpRows * Oh; i += kOpT) {
                const int r = i / Oh, k = i - r * Oh;
                x[r * kOpXS + k] = (r < nr) ? R.obs[ring_row_here(R, r0 + r) * Oh + k] : 0.0f;
            }
            __syncthreads();
        }
        wg_sac_policy(actor, O, A, scale, bias, eps, r0, M, x, a1, a2, S, tile);
        for (int c = 0; c < 2; ++c) {
            const int K = op_here(O) + A;
            const OpNet qn = op_net(critics + c * op_critic_count(K - A, A), K, 1);
            wg_forward<true>(x, kOpXS, K, qn.w1, qn.b1, c1, kOpH, tile);
            wg_forward<true>(c1, kOpH, kOpH, qn.w2, qn.b2, c2, kOpH, tile);
            wg_head(c2, kOpH, qn.w3, qn.b3, 1, qv + c * kOpRows);
            wg_dgrad_masked(one, 1, 1, qn.w3, kOpH, c2, kOpH);
            wg_dgrad_masked(c2, kOpH, kOpH, qn.w2, kOpH, c1, kOpH);
            // the action columns of the critic's first layer only: d q_c / d action
            const int Ah = op_here(A);
            if (t < kOpRows * Ah) {
                const int r = t / Ah, a = t % Ah;
                float acc = 0.0f;
                for (int j = 0; j < kOpH; ++j) acc = op_mac(acc, c1[r * kOpH + j], qn.w1[(int64_t)j * K + (K - A) + a]);
                (c == 0 ? g1 : g2)[t] = acc;
            }
            __syncthreads();
        }
        {
            const float al = alpha[0];
            if (t < kOpRows && t < nr) {
                ws[r0 + t] = sac_actor_row(al, s_lpr[t], qv[t], qv[kOpRows + t]);
                float* lpo = ptr_here(log_pi_out);
                if (lpo) lpo[r0 + t] = s_lpr[t];
            }
            float dm = 0.0f, du = 0.0f;
            const int Ah = op_here(A);
            if (t < kOpRows * Ah) {
                const int r = t / Ah, a = t % Ah;
                if (r < nr) {
                    const float q1 = qv[r], q2 = qv[kOpRows + r];
                    const float dact = (-inv_m) * (sac_min_w(q1, q2) * g1[t] + sac_min_w(q2, q1) * g2[t]);
                    SacElem e;
                    e.y = s_y[t];
                    e.std = s_std[t];
                    e.th = s_th[t];
                    e.arg = s_arg[t];
                    e.action = 0.0f;
                    e.lp = 0.0f;
                    sac_elem_bwd(e, eps[(int64_t)(r0 + r) * Ah + a], scale[a], dact, al * inv_m, &dm, &du);
                    float *dmo = ptr_here(dmean_out), *duo = ptr_here(du_out);
                    if (dmo) dmo[(int64_t)(r0 + r) * Ah + a] = dm;
                    if (duo) duo[(int64_t)(r0 + r) * Ah + a] = du;
                }
            }
            if (t < kOpRows * Ah) {                      // the heads' outputs are dead: their slots take the gradients (0 in padded rows)
                s_mu[t] = dm;
                s_us[t] = du;
            }
            __syncthreads();
        }
        {
            const SacOff off = sac_off(op_here(O), op_here(A));
            wg_wgrad(s_mu, A, a2, kOpH, A, kOpH, part + off.wm, part + off.bm, first, nr);
        }
        {
            const SacOff off = sac_off(op_here(O), op_here(A));
            wg_wgrad(s_us, A, a2, kOpH, A, kOpH, part + off.ws, part + off.bs, first, nr);
        }
        {
            const SacNet an = sac_net_here(actor, O, A);
            wg_dgrad2_masked(s_mu, an.wm, s_us, an.ws, A, a2);
        }
        {
            const SacOff off = sac_off(op_here(O), op_here(A));
            wg_wgrad(a2, kOpH, a1, kOpH, kOpH, kOpH, part + off.w2, part + off.b2, first, nr);
        }
        {
            const SacNet an = sac_net_here(actor, O, A);
            wg_dgrad_masked(a2, kOpH, kOpH, an.w2, kOpH, a1, kOpH);
        }
        {
            const int Oh = op_here(O);
            const SacOff off = sac_off(Oh, op_here(A));
            wg_wgrad(a1, kOpH, x, kOpXS, kOpH, Oh, part + off.w1, part + off.b1, first, nr);
        }
    }
}

// One workgroup.  mean = fold of log_pi + target_entropy (slot t adds rows t, t + 256, ... in f64, thread 0 adds the slots in order);
// alpha_loss = -exp(log_alpha) * mean, which is also d alpha_loss / d log_alpha; one Adam step on log_alpha.
__global__ __launch_bounds__(256) void sac_alpha_kernel(const float* __restrict__ log_pi, int M, float target_entropy, float* __restrict__ log_alpha,
                                                        float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, AdamParams P,
                                                        const float* __restrict__ sched2, float* __restrict__ alpha_out,
                                                        float* __restrict__ alpha_loss_out) {
    __shared__ double red[kOpFold];
    double s = 0.0;
    for (int k = threadIdx.x; k < M; k += kOpFold) s += (double)(log_pi[k] + target_entropy);
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int t = 0; t < kOpFold; ++t) tot += red[t];
    if (sched2) {
        P.neg_step = sched2[0];
        P.bc2_sqrt = sched2[1];
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
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_sac_policy_f32(const float* obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                   int n_envs, const float* actor, const float* action_scale, const float* action_bias,
                                                   const float* eps, float* actions_out, float* log_pi_out, int rows, int O, int A,
                                                   void* stream) {
    const char* fn = "mi355ppo_sac_policy_f32";
    MI355_REQUIRE(obs && actor && action_scale && action_bias && eps && (actions_out || log_pi_out), MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE((batch_inds == nullptr) == (env_inds == nullptr), MI355PPO_EINVAL, "%s: batch_inds and env_inds come together", fn);
    MI355_REQUIRE(!batch_inds || (slots > 0 && n_envs > 0), MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots,
                  n_envs);
    if (int rc = op_shape(fn, rows, O, A)) return rc;
    hipLaunchKernelGGL(sac_policy_kernel, dim3(op_tiles(rows)), dim3(256), 0, as_stream(stream), obs, batch_inds, env_inds, slots, n_envs, actor,
                       action_scale, action_bias, eps, actions_out, log_pi_out, rows, O, A);
    return check_launch("sac_policy_kernel");
}

extern "C" MI355PPO_API int mi355ppo_sac_target_f32(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                                   const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                                   const float* actor, const float* target_critics, const float* action_scale,
                                                   const float* action_bias, const float* eps, const float* alpha, double gamma,
                                                   float* next_q_value, float* next_actions_out, float* log_pi_out, int M, int O, int A,
                                                   void* stream) {
    const char* fn = "mi355ppo_sac_target_f32";
    MI355_REQUIRE(ring_next_obs && ring_rewards && ring_dones && actor && target_critics && action_scale && action_bias && eps && alpha &&
                      next_q_value,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, nullptr, ring_next_obs, nullptr, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs)) return rc;
    hipLaunchKernelGGL(sac_target_kernel, dim3(op_tiles(M)), dim3(256), 0, as_stream(stream), R, actor, target_critics, action_scale, action_bias,
                       eps, alpha, (float)gamma, next_q_value, next_actions_out, log_pi_out, M, O, A);
    return check_launch("sac_target_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_sac_actor_workspace_bytes(int M, int O, int A) {
    if (M <= 0 || O <= 0 || A <= 0) return 0;
    return (size_t)(op_mp(M) + (int64_t)op_groups(M) * sac_actor_count(O, A)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_sac_actor_fwd_bwd_f32(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                          int n_envs, const float* actor, const float* critics, const float* action_scale,
                                                          const float* action_bias, const float* eps, const float* alpha, float* grads,
                                                          float* actor_loss_out, float* log_pi_out, float* dmean_out, float* du_out, int M,
                                                          int O, int A, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_sac_actor_fwd_bwd_f32";
    MI355_REQUIRE(ring_obs && actor && critics && action_scale && action_bias && eps && alpha && grads && actor_loss_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, ring_obs, nullptr, nullptr, nullptr, nullptr, batch_inds, env_inds, slots, n_envs)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_sac_actor_workspace_bytes(M, O, A))) return rc;
    hipStream_t s = as_stream(stream);
    const int Mp = (int)op_mp(M), G = op_groups(M);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(sac_actor_kernel, dim3(G), dim3(256), 0, s, R, actor, critics, action_scale, action_bias, eps, alpha, ws, log_pi_out,
                       dmean_out, du_out, M, Mp, O, A, G, (float)(1.0 / (double)M));
    if (int rc = check_launch("sac_actor_kernel")) return rc;
    return op_fold_launch(s, ws + Mp, G, sac_actor_count(O, A), grads, ws, Mp, M, 1, 1.0f, actor_loss_out);
}

extern "C" MI355PPO_API int mi355ppo_sac_alpha_f32(const float* log_pi, int M, double target_entropy, float* log_alpha, float* exp_avg,
                                                  float* exp_avg_sq, double lr, double beta1, double beta2, double eps, int64_t step,
                                                  const float* sched2, float* alpha_out, float* alpha_loss_out, void* stream) {
    const char* fn = "mi355ppo_sac_alpha_f32";
    MI355_REQUIRE(log_pi && log_alpha && exp_avg && exp_avg_sq && alpha_out && alpha_loss_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && (sched2 || step >= 1), MI355PPO_EINVAL, "%s: rows=%d must be > 0 and step=%lld >= 1", fn, M, (long long)step);
    AdamParams P;
    P.scale = 1.0f;
    P.max_norm = 0.0f;
    P.w1 = (float)(1.0 - beta1);
    P.beta2 = (float)beta2;
    P.w2 = (float)(1.0 - beta2);
    float sc[2] = {0.0f, 1.0f};
    if (!sched2) mi355ppo_adam_schedule_f32(lr, beta1, beta2, step, sc);
    P.neg_step = sc[0];
    P.bc2_sqrt = sc[1];
    P.eps = (float)eps;
    P.nblocks = 0;
    P.zero_grads = 1;
    hipLaunchKernelGGL(sac_alpha_kernel, dim3(1), dim3(256), 0, as_stream(stream), log_pi, M, (float)target_entropy, log_alpha, exp_avg,
                       exp_avg_sq, P, sched2, alpha_out, alpha_loss_out);
    return check_launch("sac_alpha_kernel");
}
