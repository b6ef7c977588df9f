// Discrete SAC on Atari (cleanrl/sac_atari.py): the two u8 frame rings of the reference's plain ReplayBuffer in device memory, and the
// five heads Linear(512, n_actions) -- the actor's logits, qf1 / qf2 and their targets -- with the soft state value, both critics'
// TD loss, the dense policy gradient and their backward (gfx950).  The NatureCNN trunks and Linear(3136, 512) in front of the heads
// are the matrix-pipe kernels of conv*.hip / gemm*.hip; they run on the gathered batch.
//
//   add      one thread per pixel word: obs goes to ring A at slot pos, next_obs to ring B at the same slot (da_pack).
//   gather   qh_gather_kernel<false> (qhead_wg.h): frames (batch_inds, env_inds) of ring A, then of ring B, into (2M, 84, 84, 4).
//   forward  qh_fwd_kernel<512> (qhead_wg.h), three passes a launch: the critic update's five heads are two launches, the actor
//            update's three heads one.
//   critic   row: one workgroup per batch row -- thread 0 runs the row (softmax, V, y, both MSE rows: n <= 18, serial), then
//            every thread two columns of dh1 and dh2 from the taken action's row of W.  wgrad: one workgroup per (critic, action):
//            dW[j, :] and db[j] over the rows that took j, ascending; one more workgroup folds the four scalars in f64 slots.
//   actor    row: thread 0 runs the row (softmax, t, s, dz, e_r), then every thread two columns of dh = dz W.  wgrad: one workgroup
//            per action: the dense dW[j, :] = sum_r dz[r, j] h[r, :] and db[j], ascending r; one more folds actor_loss.
//   act      the actor's logits through the forward, then one thread per row: softmax and argmax p / q with the caller's Exp(1) draws.
//
// Everything is plain f32 VALU: at batch 64 and n <= 18 the step is latency-bound.  No entry point allocates
// or synchronises, none uses atomics; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "sac_atari_rows.h"
#include "qhead_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// ---------------------------------------------------------------------------------------------------------------- the rings
// grid (ceil(N * 7056 / 256), 2): y selects obs -> ring A (0) / next_obs -> ring B (1)
__global__ __launch_bounds__(256) void sd_add2_kernel(const uint8_t* __restrict__ obs, const uint8_t* __restrict__ next_obs,
                                                      const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                      const float* __restrict__ dones, uint32_t* __restrict__ ring_a, uint32_t* __restrict__ ring_b,
                                                      int64_t* __restrict__ ring_actions, float* __restrict__ ring_rewards,
                                                      float* __restrict__ ring_dones, int64_t pos, int N) {
    const int which = (int)blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N * kDaPix) {
        const int e = i / kDaPix, p = i - e * kDaPix;
        const uint8_t* stack = (which ? next_obs : obs) + (int64_t)e * (kDaPlanes * kDaPix);
        (which ? ring_b : ring_a)[da_frame(pos, e, N) + p] = da_pack(stack, p);
    }
    if (which == 1 && i < N) {
        ring_actions[pos * N + i] = actions[i];
        ring_rewards[pos * N + i] = rewards[i];
        ring_dones[pos * N + i] = dones[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- shared pieces
// sum(v[0 .. M)) / denom: slot t adds rows t, t + 256, ... in f64, thread 0 adds the slots in order.  Valid in thread 0; ends with a barrier.
__device__ float sd_fold(const float* __restrict__ v, int M, double denom, double* red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < M; k += kOpFold) s += (double)v[k];
    red[threadIdx.x] = s;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int t = 0; t < kOpFold; ++t) tot += red[t];
    __syncthreads();
    return (float)(tot / denom);
}

// ---------------------------------------------------------------------------------------------------------------- the critic update
// ws layout (floats): z (5 x M x n: q1, q2 on obs | pi, q1t, q2t on next_obs) | rows (4 x Mp: sq1 | sq2 | q1a | q2a) | dz (2 x M) | act (M ints)
struct SdCriticWs {
    float *z, *rows, *dz;
    int* act;
};
static __host__ __device__ SdCriticWs sd_critic_ws(void* ws, int M, int n) {
    SdCriticWs w;
    w.z = static_cast<float*>(ws);
    w.rows = w.z + (int64_t)5 * M * n;
    w.dz = w.rows + 4 * ((M + 63) / 64 * 64);
    w.act = reinterpret_cast<int*>(w.dz + 2 * M);
    return w;
}

__global__ __launch_bounds__(256) void sd_critic_row_kernel(SdCriticWs S, const float* __restrict__ w1, const float* __restrict__ w2,
                                                            const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                            const float* __restrict__ dones, const float* __restrict__ alpha,
                                                            float* __restrict__ dh1, float* __restrict__ dh2, float* __restrict__ v_out,
                                                            float* __restrict__ y_out, int M, int Mp, int n, float gamma, float norm) {
    __shared__ float d[2];
    __shared__ int act_s;
    const int t = threadIdx.x, r = blockIdx.x;
    if (t == 0) {
        const int64_t mn = (int64_t)M * n;
        const float* z = S.z + (int64_t)r * n;
        const SdCritic c = sd_critic_row(z, z + mn, z + 2 * mn, z + 3 * mn, z + 4 * mn, n, actions[r], rewards[r], dones[r], alpha[0], gamma, norm);
        S.rows[r] = c.sq1;
        S.rows[Mp + r] = c.sq2;
        S.rows[2 * Mp + r] = c.q1a;
        S.rows[3 * Mp + r] = c.q2a;
        S.dz[r] = c.d1;
        S.dz[M + r] = c.d2;
        S.act[r] = c.act;
        if (v_out) v_out[r] = c.V;
        if (y_out) y_out[r] = c.y;
        d[0] = c.d1;
        d[1] = c.d2;
        act_s = c.act;
    }
    __syncthreads();
    const float* wa1 = w1 + (int64_t)act_s * kDaH;
    const float* wa2 = w2 + (int64_t)act_s * kDaH;
    for (int k = t; k < kDaH; k += 256) {
        dh1[(int64_t)r * kDaH + k] = da_dh(d, 1, wa1, k);
        dh2[(int64_t)r * kDaH + k] = da_dh(d + 1, 1, wa2, k);
    }
}

// Workgroup j < 2n: critic j / n, action j % n: dW[a, :] and db[a].  Workgroup 2n: scalars {qf1_loss, qf2_loss, mean qf1_a, mean qf2_a}.
__global__ __launch_bounds__(256) void sd_critic_wgrad_kernel(SdCriticWs S, const float* __restrict__ h1, const float* __restrict__ h2,
                                                              float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                              float* __restrict__ db2, float* __restrict__ scalars, int M, int Mp, int n) {
    __shared__ double red[kOpFold];
    __shared__ int acts[kDaMaxRows];
    __shared__ float dzj[kDaMaxRows];
    const int t = threadIdx.x, j = blockIdx.x;
    if (j == 2 * n) {
        for (int s = 0; s < 4; ++s) {
            const float m = sd_fold(S.rows + (int64_t)s * Mp, M, (double)M, red);
            if (t == 0) scalars[s] = m;
        }
        return;
    }
    const int c = j / n, a = j - c * n;
    for (int r = t; r < M; r += 256) {
        acts[r] = S.act[r];
        dzj[r] = S.dz[c * M + r];
    }
    __syncthreads();
    const float* h = c ? h2 : h1;
    float* dw = c ? dw2 : dw1;
    float* db = c ? db2 : db1;
    for (int k = t; k < kDaH; k += 256) dw[(int64_t)a * kDaH + k] = da_wgrad(acts, dzj, 1, M, a, 0, h, k);
    if (t == 0) db[a] = da_wgrad(acts, dzj, 1, M, a, 0, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------------- the actor update
// ws layout (floats): z (3 x M x n: pi, q1, q2 on obs) | rows (Mp: s) | dz (M x n)
struct SdActorWs {
    float *z, *rows, *dz;
};
static __host__ __device__ SdActorWs sd_actor_ws(void* ws, int M, int n) {
    SdActorWs w;
    w.z = static_cast<float*>(ws);
    w.rows = w.z + (int64_t)3 * M * n;
    w.dz = w.rows + (M + 63) / 64 * 64;
    return w;
}

__global__ __launch_bounds__(256) void sd_actor_row_kernel(SdActorWs S, const float* __restrict__ w, const float* __restrict__ alpha,
                                                           float* __restrict__ dh, float* __restrict__ e_out, int M, int n, float te, float inv_mn) {
    __shared__ float dzs[kDqMaxAct];
    const int t = threadIdx.x, r = blockIdx.x;
    if (t == 0) {
        const int64_t mn = (int64_t)M * n;
        const float* z = S.z + (int64_t)r * n;
        const SdActor a = sd_actor_row(z, z + mn, z + 2 * mn, n, alpha[0], te, inv_mn, dzs);
        S.rows[r] = a.s;
        e_out[r] = a.e;
        for (int j = 0; j < n; ++j) S.dz[(int64_t)r * n + j] = dzs[j];
    }
    __syncthreads();
    for (int k = t; k < kDaH; k += 256) dh[(int64_t)r * kDaH + k] = da_dh(dzs, n, w, k);
}

// Workgroup j < n: dW[j, :] and db[j], dense over the batch rows.  Workgroup n: actor_loss = sum_r s_r / (M n).
__global__ __launch_bounds__(256) void sd_actor_wgrad_kernel(SdActorWs S, const float* __restrict__ h, float* __restrict__ dw, float* __restrict__ db,
                                                             float* __restrict__ loss, int M, int n) {
    __shared__ double red[kOpFold];
    __shared__ float dzj[kDaMaxRows];
    const int t = threadIdx.x, j = blockIdx.x;
    if (j == n) {
        const float m = sd_fold(S.rows, M, (double)M * (double)n, red);
        if (t == 0) loss[0] = m;
        return;
    }
    for (int r = t; r < M; r += 256) dzj[r] = S.dz[(int64_t)r * n + j];
    __syncthreads();
    for (int k = t; k < kDaH; k += 256) dw[(int64_t)j * kDaH + k] = sd_wgrad_dense(dzj, 1, M, h, k);
    if (t == 0) db[j] = sd_wgrad_dense(dzj, 1, M, nullptr, 0);
}

// ---------------------------------------------------------------------------------------------------------------- act
// one thread per row: z (N, n) from qh_fwd_kernel
__global__ __launch_bounds__(64) void sd_act_kernel(const float* __restrict__ z, const float* __restrict__ noise, int64_t* __restrict__ actions,
                                                    float* __restrict__ probs, int N, int n) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= N) return;
    float zr[kDqMaxAct], q[kDqMaxAct], p[kDqMaxAct], lp[kDqMaxAct];
    for (int a = 0; a < n; ++a) {
        zr[a] = z[(int64_t)r * n + a];
        q[a] = noise[(int64_t)r * n + a];
    }
    sd_softmax(zr, n, p, lp);
    if (probs)
        for (int a = 0; a < n; ++a) probs[(int64_t)r * n + a] = p[a];
    actions[r] = (int64_t)sd_sample(p, q, n);
}

static size_t sd_critic_workspace(int M, int n) {
    if (M < 1 || M > kDaMaxRows || !da_limits(kDaH, n, 1)) return 0;
    return (size_t)((int64_t)5 * M * n + 4 * op_mp(M) + 2 * M + M) * sizeof(float);
}
static size_t sd_actor_workspace(int M, int n) {
    if (M < 1 || M > kDaMaxRows || !da_limits(kDaH, n, 1)) return 0;
    return (size_t)((int64_t)3 * M * n + op_mp(M) + (int64_t)M * n) * sizeof(float);
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_replay_add2_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                                   const float* dones, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                                   float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int n_envs, void* stream) {
    const char* fn = "mi355ppo_replay_add2_u8";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = sd_ring_shape(fn, slots, n_envs, pos)) return rc;
    MI355_REQUIRE(aligned(ring_obs, 4) && aligned(ring_next_obs, 4), MI355PPO_EALIGN, "%s: the rings must be 4-byte aligned", fn);
    const unsigned gx = (unsigned)(((int64_t)n_envs * kDaPix + 255) / 256);
    hipLaunchKernelGGL(sd_add2_kernel, dim3(gx, 2), dim3(256), 0, as_stream(stream), obs, next_obs, actions, rewards, dones,
                       reinterpret_cast<uint32_t*>(ring_obs), reinterpret_cast<uint32_t*>(ring_next_obs), ring_actions, ring_rewards, ring_dones, pos,
                       n_envs);
    return check_launch("sd_add2_kernel");
}

extern "C" MI355PPO_API int mi355ppo_replay_gather2_u8(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                      const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                      const int64_t* env_inds, int64_t slots, int n_envs, uint8_t* frames_out,
                                                      int64_t* actions_out, float* rewards_out, float* dones_out, int M, void* stream) {
    const char* fn = "mi355ppo_replay_gather2_u8";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && batch_inds && env_inds && frames_out && actions_out &&
                      rewards_out && dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(M >= 1 && M <= kDaMaxRows, MI355PPO_EINVAL, "%s: rows=%d: 1 <= rows <= %d", fn, M, kDaMaxRows);
    MI355_REQUIRE(aligned(ring_obs, 4) && aligned(ring_next_obs, 4) && aligned(frames_out, 4), MI355PPO_EALIGN,
                  "%s: the rings and the batch must be 4-byte aligned", fn);
    return qh_gather_launch<false>(as_stream(stream), ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots,
                                   n_envs, frames_out, actions_out, rewards_out, dones_out, M);
}

extern "C" MI355PPO_API size_t mi355ppo_sacd_head_act_workspace_bytes(int N, int n_actions) {
    if (N < 1 || N > kDaMaxRows || !da_limits(kDaH, n_actions, 1)) return 0;
    return (size_t)N * n_actions * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_sacd_head_act_f32(const float* h, const float* w, const float* b, const float* noise_exp1, int64_t* actions_out,
                                                      float* probs_out, int N, int hidden, int n_actions, void* workspace, size_t workspace_bytes,
                                                      void* stream) {
    const char* fn = "mi355ppo_sacd_head_act_f32";
    MI355_REQUIRE(h && w && b && noise_exp1 && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, N, hidden, n_actions, 1)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_sacd_head_act_workspace_bytes(N, n_actions))) return rc;
    hipStream_t s = as_stream(stream);
    float* z = static_cast<float*>(workspace);
    if (int rc = qh_fwd_launch<kDaH>(s, QhPasses{{h}, {w}, {b}}, 1, z, N, n_actions, 1)) return rc;
    hipLaunchKernelGGL(sd_act_kernel, dim3((N + 63) / 64), dim3(64), 0, s, z, noise_exp1, actions_out, probs_out, N, n_actions);
    return check_launch("sd_act_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_sacd_critic_workspace_bytes(int M, int n_actions) { return sd_critic_workspace(M, n_actions); }

extern "C" MI355PPO_API int mi355ppo_sacd_critic_fwd_bwd_f32(const float* h_q1, const float* h_q2, const float* h_pi_next, const float* h_q1t_next,
                                                            const float* h_q2t_next, const float* w_q1, const float* b_q1, const float* w_q2,
                                                            const float* b_q2, const float* w_pi, const float* b_pi, const float* w_q1t,
                                                            const float* b_q1t, const float* w_q2t, const float* b_q2t, const int64_t* actions,
                                                            const float* rewards, const float* dones, const float* alpha, double gamma, float* dh1,
                                                            float* dh2, float* dw1, float* db1, float* dw2, float* db2, float* scalars_out,
                                                            float* v_out, float* y_out, int M, int hidden, int n_actions, void* workspace,
                                                            size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_sacd_critic_fwd_bwd_f32";
    MI355_REQUIRE(h_q1 && h_q2 && h_pi_next && h_q1t_next && h_q2t_next && w_q1 && b_q1 && w_q2 && b_q2 && w_pi && b_pi && w_q1t && b_q1t && w_q2t &&
                      b_q2t && actions && rewards && dones && alpha && dh1 && dh2 && dw1 && db1 && dw2 && db2 && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, 1)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, sd_critic_workspace(M, n_actions))) return rc;
    hipStream_t s = as_stream(stream);
    const int n = n_actions, Mp = (int)op_mp(M);
    const SdCriticWs S = sd_critic_ws(workspace, M, n);
    const QhPasses A{{h_q1, h_q2, h_pi_next}, {w_q1, w_q2, w_pi}, {b_q1, b_q2, b_pi}};
    if (int rc = qh_fwd_launch<kDaH>(s, A, 3, S.z, M, n, 1)) return rc;
    const QhPasses B{{h_q1t_next, h_q2t_next}, {w_q1t, w_q2t}, {b_q1t, b_q2t}};
    if (int rc = qh_fwd_launch<kDaH>(s, B, 2, S.z + (int64_t)3 * M * n, M, n, 1)) return rc;
    hipLaunchKernelGGL(sd_critic_row_kernel, dim3(M), dim3(256), 0, s, S, w_q1, w_q2, actions, rewards, dones, alpha, dh1, dh2, v_out, y_out, M, Mp, n,
                       (float)gamma, (float)(2.0 / (double)M));
    if (int rc = check_launch("sd_critic_row_kernel")) return rc;
    hipLaunchKernelGGL(sd_critic_wgrad_kernel, dim3(2 * n + 1), dim3(256), 0, s, S, h_q1, h_q2, dw1, db1, dw2, db2, scalars_out, M, Mp, n);
    return check_launch("sd_critic_wgrad_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_sacd_actor_workspace_bytes(int M, int n_actions) { return sd_actor_workspace(M, n_actions); }

extern "C" MI355PPO_API int mi355ppo_sacd_actor_fwd_bwd_f32(const float* h_pi, const float* h_q1, const float* h_q2, const float* w_pi,
                                                           const float* b_pi, const float* w_q1, const float* b_q1, const float* w_q2,
                                                           const float* b_q2, const float* alpha, double target_entropy, float* dh, float* dw,
                                                           float* db, float* entropy_rows_out, float* actor_loss_out, int M, int hidden,
                                                           int n_actions, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_sacd_actor_fwd_bwd_f32";
    MI355_REQUIRE(h_pi && h_q1 && h_q2 && w_pi && b_pi && w_q1 && b_q1 && w_q2 && b_q2 && alpha && dh && dw && db && entropy_rows_out && actor_loss_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, 1)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, sd_actor_workspace(M, n_actions))) return rc;
    hipStream_t s = as_stream(stream);
    const int n = n_actions;
    const SdActorWs S = sd_actor_ws(workspace, M, n);
    const QhPasses H{{h_pi, h_q1, h_q2}, {w_pi, w_q1, w_q2}, {b_pi, b_q1, b_q2}};
    if (int rc = qh_fwd_launch<kDaH>(s, H, 3, S.z, M, n, 1)) return rc;
    hipLaunchKernelGGL(sd_actor_row_kernel, dim3(M), dim3(256), 0, s, S, w_pi, alpha, dh, entropy_rows_out, M, n, (float)target_entropy,
                       (float)(1.0 / ((double)M * (double)n)));
    if (int rc = check_launch("sd_actor_row_kernel")) return rc;
    hipLaunchKernelGGL(sd_actor_wgrad_kernel, dim3(n + 1), dim3(256), 0, s, S, h_pi, dw, db, actor_loss_out, M, n);
    return check_launch("sd_actor_wgrad_kernel");
}
