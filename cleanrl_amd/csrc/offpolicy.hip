// DDPG / TD3 (cleanrl/ddpg_continuous_action.py, cleanrl/td3_continuous_action.py): the device replay ring, the rollout's action,
// the TD target, the critic and actor updates (forward + backward + flat gradient) and the Polyak average (gfx950).
//
// At batch 256 and width 256 every launch is latency-bound, so the mapping is plain f32 VALU.  A workgroup of 256 threads takes a
// tile of kOpRows rows through a whole network; the rows' vectors live in LDS:
//
//   forward   thread j owns hidden unit j for all rows of the tile.  W[j, k0 .. k0+8) of all 256 units is staged through an LDS
//             tile (coalesced 32-byte row pieces in; the next tile's loads are in flight while this one is multiplied), the rows'
//             inputs are LDS broadcasts.  The tile's row is padded to 264 floats: a wave's 64 stores go to banks
//             8 * (t % 8) + t / 8 (each of the 32 banks twice, the floor for 64 lanes) and its column reads to consecutive banks.  One 256 x 256 matrix is 256 KiB: it is streamed from
//             L2 by every workgroup, never held.
//   heads     (J = act_dim or 1 outputs) thread (row, j) runs one 256-long dot product.
//   backward  thread k owns input unit k: sum_j dz[j] * W[j, k] reads W coalesced; the ReLU mask is applied in place.
//   gradient  thread e owns weight elements e, e + 256, ...: the tile's rows are added in ascending order and then into the
//             workgroup's partial (tiles ascending); a second launch adds the partials in workgroup order into the flat gradient
//             and folds the loss / q scalars in f64 slots.  No atomics anywhere.
//
// No entry point allocates or synchronises; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "offpolicy_rows.h"
#include "offpolicy_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {


// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void op_replay_add_kernel(const float* __restrict__ obs, const float* __restrict__ next_obs,
                                                            const float* __restrict__ act, const float* __restrict__ rew,
                                                            const float* __restrict__ done, float* __restrict__ r_obs,
                                                            float* __restrict__ r_next, float* __restrict__ r_act, float* __restrict__ r_rew,
                                                            float* __restrict__ r_done, int64_t pos, int N, int O, int A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t no = (int64_t)N * O, na = (int64_t)N * A;
    if (i < no) {
        r_obs[pos * no + i] = obs[i];
        r_next[pos * no + i] = next_obs[i];
    }
    if (i < na) r_act[pos * na + i] = act[i];
    if (i < N) {
        r_rew[pos * N + i] = rew[i];
        r_done[pos * N + i] = done[i];
    }
}

// Actor.forward of one tile into xrow[r, O + a] (the action) and tv[r * A + a] (tanh); a1 / a2 keep the hidden rows.
__device__ void wg_actor(const OpNet& an, const float* scale, const float* bias, float* x, float* a1, float* a2, float* mu, float* tv,
                         float* tile) {
    wg_forward<true>(x, kOpXS, an.K, an.w1, an.b1, a1, kOpH, tile);
    wg_forward<true>(a1, kOpH, kOpH, an.w2, an.b2, a2, kOpH, tile);
    wg_head(a2, kOpH, an.w3, an.b3, an.J, mu);
    const int t = threadIdx.x, A = an.J;
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        const float th = op_tanh(mu[t]);
        tv[t] = th;
        x[r * kOpXS + an.K + a] = op_action(th, scale[a], bias[a]);
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void op_act_kernel(const float* __restrict__ obs, const float* __restrict__ actor, const float* __restrict__ scale,
                                                     const float* __restrict__ bias, const float* __restrict__ noise, const float* __restrict__ low,
                                                     const float* __restrict__ high, float* __restrict__ out, int N, int O, int A) {
    __shared__ float x[kOpRows * kOpXS], a1[kOpRows * kOpH], a2[kOpRows * kOpH], tile[kOpKT * kOpTileLd], mu[kOpRows * kOpMaxAct],
        tv[kOpRows * kOpMaxAct];
    const int t = threadIdx.x, r0 = blockIdx.x * kOpRows;
    for (int i = t; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        x[r * kOpXS + k] = (r0 + r < N) ? obs[(int64_t)(r0 + r) * O + k] : 0.0f;
    }
    __syncthreads();
    wg_actor(op_net(actor, O, A), scale, bias, x, a1, a2, mu, tv, tile);
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        if (r0 + r < N) out[(int64_t)(r0 + r) * A + a] = op_explore(x[r * kOpXS + O + a], noise ? noise[a] : 0.0f, low[a], high[a]);
    }
}

__global__ __launch_bounds__(256) void op_target_kernel(OpRing R, const float* __restrict__ actor_t, const float* __restrict__ critics_t, int ncrit,
                                                        const float* __restrict__ scale, const float* __restrict__ bias,
                                                        const float* __restrict__ noise, float pn, float nc, float lo0, float hi0, float gamma,
                                                        float* __restrict__ y, float* __restrict__ next_act_out, int M, int O, int A) {
    __shared__ float x[kOpRows * kOpXS], a1[kOpRows * kOpH], a2[kOpRows * kOpH], tile[kOpKT * kOpTileLd], mu[kOpRows * kOpMaxAct],
        tv[kOpRows * kOpMaxAct], qv[2 * kOpRows];
    const int t = threadIdx.x, r0 = blockIdx.x * kOpRows;
    for (int i = t; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        x[r * kOpXS + k] = (r0 + r < M) ? R.next_obs[ring_row(R, r0 + r) * O + k] : 0.0f;
    }
    __syncthreads();
    wg_actor(op_net(actor_t, O, A), scale, bias, x, a1, a2, mu, tv, tile);
    if (t < kOpRows * A) {
        const int r = t / A, a = t % A;
        if (noise && r0 + r < M)
            x[r * kOpXS + O + a] = op_smooth(x[r * kOpXS + O + a], noise[(int64_t)(r0 + r) * A + a], pn, nc, scale[a], lo0, hi0);
        if (next_act_out && r0 + r < M) next_act_out[(int64_t)(r0 + r) * A + a] = x[r * kOpXS + O + a];
    }
    __syncthreads();
    const int64_t Pq = op_critic_count(O, A);
    for (int c = 0; c < ncrit; ++c) {
        const OpNet qn = op_net(critics_t + c * Pq, O + A, 1);
        wg_forward<true>(x, kOpXS, O + A, qn.w1, qn.b1, a1, kOpH, tile);
        wg_forward<true>(a1, kOpH, kOpH, qn.w2, qn.b2, a2, kOpH, tile);
        wg_head(a2, kOpH, qn.w3, qn.b3, 1, qv + c * kOpRows);
    }
    if (t < kOpRows && r0 + t < M) {
        const int64_t row = ring_row(R, r0 + t);
        const float q = (ncrit == 2) ? op_min(qv[t], qv[kOpRows + t]) : qv[t];
        y[r0 + t] = op_td_target(R.rewards[row], R.dones[row], gamma, q);
    }
}

// ws: rowvals (4 x Mp: q1 | sq1 | q2 | sq2), then partials [G][ncrit * Pq]
__global__ __launch_bounds__(256) void op_critic_kernel(OpRing R, const float* __restrict__ critics, const float* __restrict__ y, float* __restrict__ ws,
                                                        int M, int Mp, int O, int A, int G, int ncrit, float norm) {
    __shared__ float x[kOpRows * kOpXS], h1[kOpRows * kOpH], h2[kOpRows * kOpH], tile[kOpKT * kOpTileLd], qv[kOpRows], dq[kOpRows];
    const int t = threadIdx.x, g = blockIdx.x, c = blockIdx.y;
    const int64_t Pq = op_critic_count(O, A);
    const float* qp = critics + c * Pq;
    float* part = ws + (int64_t)4 * Mp + ((int64_t)g * ncrit + c) * Pq;
    float* rowq = ws + (int64_t)(2 * c) * Mp;
    float* rowsq = rowq + Mp;
    const int ntiles = op_tiles(M);
    for (int tl = g; tl < ntiles; tl += G) {
        const int r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        {
            const int K = O + A;
            for (int i = t; i < kOpRows * K; i += kOpT) {
                const int r = i / K, k = i - r * K;
                float v = 0.0f;
                if (r < nr) {
                    const int64_t row = ring_row(R, r0 + r);
                    v = (k < O) ? R.obs[row * O + k] : R.actions[row * A + (k - O)];
                }
                x[r * kOpXS + k] = v;
            }
            __syncthreads();
        }
        {
            const int K = op_here(O) + A;
            const OpNet qn = op_net(qp, K, 1);
            wg_forward<true>(x, kOpXS, K, qn.w1, qn.b1, h1, kOpH, tile);
            wg_forward<true>(h1, kOpH, kOpH, qn.w2, qn.b2, h2, kOpH, tile);
            wg_head(h2, kOpH, qn.w3, qn.b3, 1, qv);
        }
        if (t < kOpRows) {
            float d = 0.0f;
            if (t < nr) {
                float sq;
                d = op_mse_row(qv[t], y[r0 + t], norm, &sq);
                rowq[r0 + t] = qv[t];
                rowsq[r0 + t] = sq;
            }
            dq[t] = d;
        }
        __syncthreads();
        {
            const int K = op_here(O) + A;
            const OpNet qn = op_net(qp, K, 1);
            const OpOff off = op_off(K, 1);
            wg_wgrad(dq, 1, h2, kOpH, 1, kOpH, part + off.w3, part + off.b3, first, nr);
            wg_dgrad_masked(dq, 1, 1, qn.w3, kOpH, h2, kOpH);
            wg_wgrad(h2, kOpH, h1, kOpH, kOpH, kOpH, part + off.w2, part + off.b2, first, nr);
            wg_dgrad_masked(h2, kOpH, kOpH, qn.w2, kOpH, h1, kOpH);
            wg_wgrad(h1, kOpH, x, kOpXS, kOpH, K, part + off.w1, part + off.b1, first, nr);
        }
    }
}

// grads[i] = sum of the G partials in ascending order; workgroup 0 also folds `nsc` row arrays into means (scalars[s] = mean(rows s)).
__global__ __launch_bounds__(256) void op_fold_kernel(const float* __restrict__ part, int G, int64_t P, float* __restrict__ grads,
                                                      const float* __restrict__ rows, int Mp, int M, int nsc, float sign,
                                                      float* __restrict__ scalars) {
    __shared__ double red[kOpFold];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < P) {
        float acc = 0.0f;
        for (int b = 0; b < G; ++b) acc = acc + part[(int64_t)b * P + e];
        grads[e] = acc;
    }
    if (blockIdx.x != 0) return;
    for (int s = 0; s < nsc; ++s) {
        const float m = wg_fold_mean(rows + (int64_t)s * Mp, M, red);
        if (threadIdx.x == 0) scalars[s] = sign * m;
    }
}

// ws: rowvals (Mp: q), then partials [G][Pa]
__global__ __launch_bounds__(256) void op_actor_kernel(OpRing R, const float* __restrict__ actor, const float* __restrict__ qf1,
                                                       const float* __restrict__ scale, const float* __restrict__ bias, float* __restrict__ ws,
                                                       float* __restrict__ dact_out, int M, int Mp, int O, int A, int G, float dqv) {
    __shared__ float x[kOpRows * kOpXS], a1[kOpRows * kOpH], a2[kOpRows * kOpH], c1[kOpRows * kOpH], c2[kOpRows * kOpH],
        tile[kOpKT * kOpTileLd], mu[kOpRows * kOpMaxAct], tv[kOpRows * kOpMaxAct], qv[kOpRows], dq[kOpRows];
    const int t = threadIdx.x, g = blockIdx.x;
    const int64_t Pa = op_actor_count(O, A);
    float* part = ws + Mp + (int64_t)g * Pa;
    const int ntiles = op_tiles(M);
    for (int tl = g; tl < ntiles; tl += G) {
        const int r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        for (int i = t; i < kOpRows * O; i += kOpT) {
            const int r = i / O, k = i - r * O;
            x[r * kOpXS + k] = (r < nr) ? R.obs[ring_row(R, r0 + r) * O + k] : 0.0f;
        }
        __syncthreads();
        wg_actor(op_net(actor, op_here(O), A), scale, bias, x, a1, a2, mu, tv, tile);
        {
            const int K = op_here(O) + A;
            const OpNet qn = op_net(qf1, K, 1);
            wg_forward<true>(x, kOpXS, K, qn.w1, qn.b1, c1, kOpH, tile);
            wg_forward<true>(c1, kOpH, kOpH, qn.w2, qn.b2, c2, kOpH, tile);
            wg_head(c2, kOpH, qn.w3, qn.b3, 1, qv);
        }
        if (t < kOpRows) {
            if (t < nr) ws[r0 + t] = qv[t];
            dq[t] = (t < nr) ? dqv : 0.0f;
        }
        __syncthreads();
        {
            const int K = op_here(O) + A;
            const OpNet qn = op_net(qf1, K, 1);
            wg_dgrad_masked(dq, 1, 1, qn.w3, kOpH, c2, kOpH);
            wg_dgrad_masked(c2, kOpH, kOpH, qn.w2, kOpH, c1, kOpH);
            // the action columns of qf1's first layer only: d q / d action, then through `* action_scale` and tanh into mu
            if (t < kOpRows * A) {
                const int r = t / A, a = t % A;
                float acc = 0.0f;
                for (int j = 0; j < kOpH; ++j) acc = op_mac(acc, c1[r * kOpH + j], qn.w1[(int64_t)j * K + (K - A) + a]);
                if (dact_out && r < nr) dact_out[(int64_t)(r0 + r) * A + a] = acc;
                mu[t] = op_dmu(acc, scale[a], tv[t]);
            }
            __syncthreads();
        }
        {
            const int Oh = op_here(O);
            const OpNet an = op_net(actor, Oh, A);
            const OpOff off = op_off(Oh, A);
            wg_wgrad(mu, A, a2, kOpH, A, kOpH, part + off.w3, part + off.b3, first, nr);
            wg_dgrad_masked(mu, A, A, an.w3, kOpH, a2, kOpH);
            wg_wgrad(a2, kOpH, a1, kOpH, kOpH, kOpH, part + off.w2, part + off.b2, first, nr);
            wg_dgrad_masked(a2, kOpH, kOpH, an.w2, kOpH, a1, kOpH);
            wg_wgrad(a1, kOpH, x, kOpXS, kOpH, Oh, part + off.w1, part + off.b1, first, nr);
        }
    }
}

int op_fold_launch(hipStream_t s, const float* part, int G, int64_t P, float* grads, const float* rows, int Mp, int M, int nsc, float sign,
                   float* scalars) {
    hipLaunchKernelGGL(op_fold_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, part, G, P, grads, rows, Mp, M, nsc, sign, scalars);
    return check_launch("op_fold_kernel");
}

__global__ __launch_bounds__(256) void op_polyak_kernel(const float* __restrict__ p, float* __restrict__ tg, int64_t n, float tau, float omt) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) tg[i] = op_polyak(p[i], tg[i], tau, omt);
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_replay_add_f32(const float* obs, const float* next_obs, const float* actions, const float* rewards,
                                                   const float* dones, float* ring_obs, float* ring_next_obs, float* ring_actions,
                                                   float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int N, int O, int A,
                                                   void* stream) {
    const char* fn = "mi355ppo_replay_add_f32";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(N > 0 && O > 0 && A > 0 && slots > 0 && pos >= 0 && pos < slots, MI355PPO_EINVAL,
                  "%s: N=%d O=%d A=%d slots=%lld pos=%lld: sizes must be positive and 0 <= pos < slots", fn, N, O, A, (long long)slots,
                  (long long)pos);
    const int64_t n = (int64_t)N * (O > A ? O : A);
    hipLaunchKernelGGL(op_replay_add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), obs, next_obs, actions, rewards,
                       dones, ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, pos, N, O, A);
    return check_launch("op_replay_add_kernel");
}

extern "C" MI355PPO_API int mi355ppo_ddpg_act_f32(const float* obs, const float* actor_params, const float* action_scale, const float* action_bias,
                                                 const float* noise_row, const float* low, const float* high, float* actions_out, int N, int O,
                                                 int A, void* stream) {
    const char* fn = "mi355ppo_ddpg_act_f32";
    MI355_REQUIRE(obs && actor_params && action_scale && action_bias && low && high && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = op_shape(fn, N, O, A)) return rc;
    hipLaunchKernelGGL(op_act_kernel, dim3(op_tiles(N)), dim3(256), 0, as_stream(stream), obs, actor_params, action_scale, action_bias, noise_row,
                       low, high, actions_out, N, O, A);
    return check_launch("op_act_kernel");
}

extern "C" MI355PPO_API int mi355ppo_td3_target_f32(const float* ring_next_obs, const float* ring_rewards, const float* ring_dones,
                                                   const int64_t* batch_inds, const int64_t* env_inds, int64_t slots, int n_envs,
                                                   const float* target_actor, const float* target_critics, int n_critics,
                                                   const float* action_scale, const float* action_bias, const float* noise, double policy_noise,
                                                   double noise_clip, double low0, double high0, double gamma, float* next_q_value,
                                                   float* next_actions_out, int M, int O, int A, void* stream) {
    const char* fn = "mi355ppo_td3_target_f32";
    MI355_REQUIRE(ring_next_obs && ring_rewards && ring_dones && target_actor && target_critics && action_scale && action_bias && next_q_value,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n_critics == 1 || n_critics == 2, MI355PPO_EINVAL, "%s: n_critics=%d must be 1 or 2", fn, n_critics);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, nullptr, ring_next_obs, nullptr, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs)) return rc;
    hipLaunchKernelGGL(op_target_kernel, dim3(op_tiles(M)), dim3(256), 0, as_stream(stream), R, target_actor, target_critics, n_critics,
                       action_scale, action_bias, noise, (float)policy_noise, (float)noise_clip, (float)low0, (float)high0, (float)gamma,
                       next_q_value, next_actions_out, M, O, A);
    return check_launch("op_target_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_td3_critic_workspace_bytes(int M, int O, int A, int n_critics) {
    if (M <= 0 || O <= 0 || A <= 0 || n_critics <= 0) return 0;
    return (size_t)(4 * op_mp(M) + (int64_t)op_groups(M) * n_critics * op_critic_count(O, A)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_td3_critic_fwd_bwd_f32(const float* ring_obs, const float* ring_actions, const int64_t* batch_inds,
                                                           const int64_t* env_inds, int64_t slots, int n_envs, const float* critics, int n_critics,
                                                           const float* next_q_value, float* grads, float* scalars_out, int M, int O, int A,
                                                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_td3_critic_fwd_bwd_f32";
    MI355_REQUIRE(ring_obs && ring_actions && critics && next_q_value && grads && scalars_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n_critics == 1 || n_critics == 2, MI355PPO_EINVAL, "%s: n_critics=%d must be 1 or 2", fn, n_critics);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, ring_obs, nullptr, ring_actions, nullptr, nullptr, batch_inds, env_inds, slots, n_envs)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_td3_critic_workspace_bytes(M, O, A, n_critics))) return rc;
    hipStream_t s = as_stream(stream);
    const int Mp = (int)op_mp(M), G = op_groups(M);
    const int64_t P = (int64_t)n_critics * op_critic_count(O, A);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(op_critic_kernel, dim3(G, n_critics), dim3(256), 0, s, R, critics, next_q_value, ws, M, Mp, O, A, G, n_critics,
                       (float)(2.0 / (double)M));
    if (int rc = check_launch("op_critic_kernel")) return rc;
    // rows: q1 | sq1 | q2 | sq2 -> scalars {mean q1, qf1_loss, mean q2, qf2_loss}
    return op_fold_launch(s, ws + (int64_t)4 * Mp, G, P, grads, ws, Mp, M, 2 * n_critics, 1.0f, scalars_out);
}

extern "C" MI355PPO_API size_t mi355ppo_td3_actor_workspace_bytes(int M, int O, int A) {
    if (M <= 0 || O <= 0 || A <= 0) return 0;
    return (size_t)(op_mp(M) + (int64_t)op_groups(M) * op_actor_count(O, A)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_td3_actor_fwd_bwd_f32(const float* ring_obs, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                          int n_envs, const float* actor, const float* qf1, const float* action_scale,
                                                          const float* action_bias, float* grads, float* actor_loss_out, float* dq_daction_out,
                                                          int M, int O, int A, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_td3_actor_fwd_bwd_f32";
    MI355_REQUIRE(ring_obs && actor && qf1 && action_scale && action_bias && grads && actor_loss_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = op_shape(fn, M, O, A)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, ring_obs, nullptr, nullptr, nullptr, nullptr, batch_inds, env_inds, slots, n_envs)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_td3_actor_workspace_bytes(M, O, A))) return rc;
    hipStream_t s = as_stream(stream);
    const int Mp = (int)op_mp(M), G = op_groups(M);
    const int64_t P = op_actor_count(O, A);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(op_actor_kernel, dim3(G), dim3(256), 0, s, R, actor, qf1, action_scale, action_bias, ws, dq_daction_out, M, Mp, O, A, G,
                       (float)(-1.0 / (double)M));
    if (int rc = check_launch("op_actor_kernel")) return rc;
    return op_fold_launch(s, ws + Mp, G, P, grads, ws, Mp, M, 1, -1.0f, actor_loss_out);
}

extern "C" MI355PPO_API int mi355ppo_polyak_f32(const float* params, float* target_params, int64_t n, double tau, void* stream) {
    const char* fn = "mi355ppo_polyak_f32";
    MI355_REQUIRE(params && target_params, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld must be > 0", fn, (long long)n);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(op_polyak_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), params, target_params, n, (float)tau,
                       (float)(1.0 - tau));
    return check_launch("op_polyak_kernel");
}
