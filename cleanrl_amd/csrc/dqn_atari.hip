// Atari DQN / C51 (cleanrl/dqn_atari.py, cleanrl/c51_atari.py): the u8 frame ring of the reference's memory-optimised ReplayBuffer in
// device memory, and the wide Q head Linear(512, n_actions * n_atoms) with its loss, projection and backward (gfx950).  The NatureCNN
// trunk and Linear(3136, 512) in front of the head are the matrix-pipe kernels of conv*.hip / gemm*.hip; they run on the gathered batch.
//
//   add      one thread per pixel: the four planes of an (4, 84, 84) stack become one 4-byte store into the channels-last ring.  obs goes
//            to slot pos, next_obs to (pos + 1) % slots; with one slot only next_obs is written (it would win), so no two threads share a word.
//   gather   one thread per pixel word: frames (batch_inds, env_inds) and ((batch_inds + 1) % slots, env_inds) into (2M, 84, 84, 4)
//            (qh_gather_kernel<true>, qhead_wg.h).
//   forward  both heads in one launch, spread over 8-row tiles x 32-output tiles x {online, target}: h's rows sit in LDS, W streams from
//            L2 through a 32 x 64 LDS tile; thread (row, output) runs its dot product in ascending k (qh_fwd_kernel<kDaH>, qhead_wg.h).
//   row      one workgroup per batch row: the softmax of each action's atoms (one thread per action and network), the target's argmax,
//            td_target or the categorical row (wg_c51_row, qhead_wg.h: one thread per atom), dz of the taken action's atoms and dh (two
//            columns a thread).
//   wgrad    one workgroup per output row j: dW[j, :] and db[j] over the batch rows that took j's action, ascending; zeros elsewhere.  One
//            more workgroup folds the two row scalars in f64 slots (wg_fold_mean).
//
// Everything is plain f32 VALU: at batch 32 the step is latency-bound.  No entry point allocates or synchronises,
// none uses atomics; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "dqn_atari_rows.h"
#include "qhead_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// ---------------------------------------------------------------------------------------------------------------- the ring
// grid (ceil(N * 7056 / 256), 2 or 1): y + first selects obs (0) / next_obs (1)
__global__ __launch_bounds__(256) void da_add_kernel(const uint8_t* __restrict__ obs, const uint8_t* __restrict__ next_obs,
                                                     const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                     const float* __restrict__ dones, uint32_t* __restrict__ ring, int64_t* __restrict__ ring_actions,
                                                     float* __restrict__ ring_rewards, float* __restrict__ ring_dones, int64_t pos, int64_t slots,
                                                     int N, int first) {
    const int which = (int)blockIdx.y + first;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N * kDaPix) {
        const int e = i / kDaPix, p = i - e * kDaPix;
        const uint8_t* stack = (which ? next_obs : obs) + (int64_t)e * (kDaPlanes * kDaPix);
        const int64_t slot = which ? da_next_slot(pos, slots) : pos;
        ring[da_frame(slot, e, N) + p] = da_pack(stack, p);
    }
    if (which == 1 && i < N) {
        ring_actions[pos * N + i] = actions[i];
        ring_rewards[pos * N + i] = rewards[i];
        ring_dones[pos * N + i] = dones[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the heads
// ws layout (floats): z (2 x M x J) | rows (2 x Mp: loss term | q) | dz (M x na) | act (M ints)
struct DaWs {
    float *z, *rows, *dz;
    int* act;
};
static __host__ __device__ DaWs da_ws(void* ws, int M, int J, int na) {
    DaWs w;
    w.z = static_cast<float*>(ws);
    w.rows = w.z + (int64_t)2 * M * J;
    w.dz = w.rows + 2 * ((M + 63) / 64 * 64);
    w.act = reinterpret_cast<int*>(w.dz + (int64_t)M * na);
    return w;
}

// One workgroup per batch row.  aux_a / aux_b (optional): DQN  target q (M, n) and td_target (M);  C51  next_pmfs and target_pmfs (M, na).
template <bool C51>
__global__ __launch_bounds__(256) void da_row_kernel(DaWs S, const float* __restrict__ w_online, const float* __restrict__ atoms,
                                                     const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                     const float* __restrict__ dones, float* __restrict__ dh, float* __restrict__ aux_a,
                                                     float* __restrict__ aux_b, int M, int Mp, int n, int na, float gamma, float vmin, float vmax,
                                                     float norm) {
    constexpr int kP = C51 ? kDqMaxAtoms : 1;
    __shared__ float zt[kDaMaxOut], zo[kDaMaxOut], qt[kDqMaxAct], qo[kDqMaxAct], pl[kP], pu[kP], pdl[kP], pdu[kP], tp[kP], dzs[kDqMaxAtoms], dotv;
    const int t = threadIdx.x, r = blockIdx.x, J = n * na;
    for (int j = t; j < J; j += 256) {
        zo[j] = S.z[(int64_t)r * J + j];
        zt[j] = S.z[((int64_t)M + r) * J + j];
    }
    __syncthreads();
    // Q values: wave 0 takes the target's actions, wave 1 the online network's
    if (t < n) qt[t] = (na > 1) ? dq_softmax_q(zt + t * na, na, atoms, zt + t * na) : zt[t];
    if (t >= 64 && t - 64 < n) qo[t - 64] = (na > 1) ? dq_softmax_q(zo + (t - 64) * na, na, atoms, zo + (t - 64) * na) : zo[t - 64];
    __syncthreads();
    const int best = dq_argmax(qt, n);
    const int act = (int)op_clamp(actions[r], n);
    const float rew = rewards[r], done = dones[r];
    if constexpr (C51) {
        const float ns = wg_c51_row({pl, pu, pdl, pdu, tp, dzs, &dotv}, zt + best * na, zo + act * na, atoms, rew, done, gamma, vmin, vmax,
                                    atoms[1] - atoms[0], na, norm, false, aux_a ? aux_a + (int64_t)r * na : nullptr,
                                    aux_b ? aux_b + (int64_t)r * na : nullptr);
        if (t < na) S.dz[(int64_t)r * na + t] = dzs[t];
        if (t == 0) {
            S.rows[r] = ns;
            S.rows[Mp + r] = qo[act];
        }
    } else {
        if (aux_a && t < n) aux_a[(int64_t)r * n + t] = qt[t];
        if (t == 0) {
            const float y = dq_td_target(rew, done, gamma, qt[best]);
            if (aux_b) aux_b[r] = y;
            float sq;
            const float d = op_mse_row(qo[act], y, norm, &sq);
            S.rows[r] = sq;
            S.rows[Mp + r] = qo[act];
            dzs[0] = d;
            S.dz[r] = d;
        }
    }
    if (t == 0) S.act[r] = act;
    __syncthreads();
    const float* wa = w_online + (int64_t)act * na * kDaH;
    for (int k = t; k < kDaH; k += 256) dh[(int64_t)r * kDaH + k] = da_dh(dzs, na, wa, k);
}

// Workgroup j < J: dW[j, :] and db[j].  Workgroup J: scalars {mean loss term, mean q}.
__global__ __launch_bounds__(256) void da_wgrad_kernel(DaWs S, const float* __restrict__ h, float* __restrict__ dw, float* __restrict__ db,
                                                       float* __restrict__ scalars, int M, int Mp, int J, int na) {
    __shared__ double red[kOpFold];
    __shared__ int acts[kDaMaxRows];
    __shared__ float dzj[kDaMaxRows];
    const int t = threadIdx.x, j = blockIdx.x;
    if (j == J) {
        wg_fold_scalars(S.rows, Mp, M, red, scalars);
        return;
    }
    const int a = j / na, k0 = j - a * na;
    // the column of dz this output row reads, dense over the batch rows (stride 1: da_wgrad with na = 1, j = 0)
    for (int r = t; r < M; r += 256) {
        acts[r] = S.act[r];
        dzj[r] = S.dz[(int64_t)r * na + k0];
    }
    __syncthreads();
    for (int k = t; k < kDaH; k += 256) dw[(int64_t)j * kDaH + k] = da_wgrad(acts, dzj, 1, M, a, 0, h, k);
    if (t == 0) db[j] = da_wgrad(acts, dzj, 1, M, a, 0, nullptr, 0);
}

// actions[r] = argmax_a q[r, a]; z: N x J from qh_fwd_kernel.  One workgroup of 64 per row: thread a takes action a's atoms.
__global__ __launch_bounds__(64) void da_argmax_kernel(float* __restrict__ z, const float* __restrict__ atoms, int64_t* __restrict__ actions,
                                                       float* __restrict__ q_out, int n, int na) {
    __shared__ float qv[kDqMaxAct];
    const int r = blockIdx.x, t = threadIdx.x;
    float* zr = z + (int64_t)r * n * na;
    if (t < n) {
        const float q = (na > 1) ? dq_softmax_q(zr + t * na, na, atoms, zr + t * na) : zr[t];
        qv[t] = q;
        if (q_out) q_out[(int64_t)r * n + t] = q;
    }
    __syncthreads();
    if (t == 0) actions[r] = (int64_t)dq_argmax(qv, n);
}

static size_t da_update_workspace(int M, int hidden, int n, int na) {
    if (M < 1 || M > kDaMaxRows || !da_limits(hidden, n, na)) return 0;
    return (size_t)((int64_t)2 * M * n * na + 2 * op_mp(M) + (int64_t)M * na + M) * sizeof(float);
}

static int da_update_launch(bool c51, const char* fn, const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                            const float* b_target, const float* atoms, const int64_t* actions, const float* rewards, const float* dones,
                            double gamma, double v_min, double v_max, float* dh, float* dw, float* db, float* scalars_out, float* aux_a,
                            float* aux_b, int M, int hidden, int n, int na, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(h && h_next && w && b && w_target && b_target && actions && rewards && dones && dh && dw && db && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n, na)) return rc;
    if (c51) {
        MI355_REQUIRE(na >= 2 && atoms, MI355PPO_EINVAL, "%s: n_atoms=%d: the projection needs the atoms, at least two (delta_z = atoms[1] - atoms[0])",
                      fn, na);
    }
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, da_update_workspace(M, hidden, n, na))) return rc;
    hipStream_t s = as_stream(stream);
    const int J = n * na, Mp = (int)op_mp(M);
    const DaWs S = da_ws(workspace, M, J, na);
    const QhPasses H{{h, h_next}, {w, w_target}, {b, b_target}};              // 0: online on obs, 1: target on next_obs
    if (int rc = qh_fwd_launch<kDaH>(s, H, 2, S.z, M, J, na)) return rc;
    if (c51)
        hipLaunchKernelGGL(da_row_kernel<true>, dim3(M), dim3(256), 0, s, S, w, atoms, actions, rewards, dones, dh, aux_a, aux_b, M, Mp, n, na,
                           (float)gamma, (float)v_min, (float)v_max, (float)(1.0 / (double)M));
    else
        hipLaunchKernelGGL(da_row_kernel<false>, dim3(M), dim3(256), 0, s, S, w, (const float*)nullptr, actions, rewards, dones, dh, aux_a, aux_b, M,
                           Mp, n, 1, (float)gamma, 0.0f, 0.0f, (float)(2.0 / (double)M));
    if (int rc = check_launch("da_row_kernel")) return rc;
    hipLaunchKernelGGL(da_wgrad_kernel, dim3(J + 1), dim3(256), 0, s, S, h, dw, db, scalars_out, M, Mp, J, na);
    return check_launch("da_wgrad_kernel");
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_replay_add_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                                  const float* dones, uint8_t* ring_frames, int64_t* ring_actions, float* ring_rewards,
                                                  float* ring_dones, int64_t pos, int64_t slots, int n_envs, void* stream) {
    const char* fn = "mi355ppo_replay_add_u8";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_frames && ring_actions && ring_rewards && ring_dones, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(pos >= 0 && pos < slots && n_envs <= (1 << 16), MI355PPO_EINVAL, "%s: pos=%lld slots=%lld n_envs=%d: 0 <= pos < slots, n_envs <= 65536",
                  fn, (long long)pos, (long long)slots, n_envs);
    MI355_REQUIRE(aligned(ring_frames, 4), MI355PPO_EALIGN, "%s: the ring must be 4-byte aligned", fn);
    const int first = slots == 1 ? 1 : 0;                       // one slot: next_obs alone (it is what the reference leaves there)
    const unsigned gx = (unsigned)(((int64_t)n_envs * kDaPix + 255) / 256);
    hipLaunchKernelGGL(da_add_kernel, dim3(gx, 2 - first), dim3(256), 0, as_stream(stream), obs, next_obs, actions, rewards, dones,
                       reinterpret_cast<uint32_t*>(ring_frames), ring_actions, ring_rewards, ring_dones, pos, slots, n_envs, first);
    return check_launch("da_add_kernel");
}

extern "C" MI355PPO_API int mi355ppo_replay_gather_u8(const uint8_t* ring_frames, const int64_t* ring_actions, const float* ring_rewards,
                                                     const float* ring_dones, const int64_t* batch_inds, const int64_t* env_inds, int64_t slots,
                                                     int n_envs, uint8_t* frames_out, int64_t* actions_out, float* rewards_out, float* dones_out,
                                                     int M, void* stream) {
    const char* fn = "mi355ppo_replay_gather_u8";
    MI355_REQUIRE(ring_frames && ring_actions && ring_rewards && ring_dones && batch_inds && env_inds && frames_out && actions_out && rewards_out &&
                      dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(M >= 1 && M <= kDaMaxRows, MI355PPO_EINVAL, "%s: rows=%d: 1 <= rows <= %d", fn, M, kDaMaxRows);
    MI355_REQUIRE(aligned(ring_frames, 4) && aligned(frames_out, 4), MI355PPO_EALIGN, "%s: the ring and the batch must be 4-byte aligned", fn);
    return qh_gather_launch<true>(as_stream(stream), ring_frames, nullptr, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots,
                                  n_envs, frames_out, actions_out, rewards_out, dones_out, M);
}

extern "C" MI355PPO_API size_t mi355ppo_dqn_head_act_workspace_bytes(int N, int n_actions, int n_atoms) {
    if (N < 1 || N > kDaMaxRows || !da_limits(kDaH, n_actions, n_atoms)) return 0;
    return (size_t)N * n_actions * n_atoms * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_dqn_head_act_f32(const float* h, const float* w, const float* b, const float* atoms, int64_t* actions_out,
                                                     float* q_out, int N, int hidden, int n_actions, int n_atoms, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_dqn_head_act_f32";
    MI355_REQUIRE(h && w && b && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, N, hidden, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms == 1 || atoms, MI355PPO_EINVAL, "%s: n_atoms=%d needs the atoms", fn, n_atoms);
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_dqn_head_act_workspace_bytes(N, n_actions, n_atoms))) return rc;
    hipStream_t s = as_stream(stream);
    const int J = n_actions * n_atoms;
    float* z = static_cast<float*>(workspace);
    if (int rc = qh_fwd_launch<kDaH>(s, QhPasses{{h}, {w}, {b}}, 1, z, N, J, n_atoms)) return rc;
    hipLaunchKernelGGL(da_argmax_kernel, dim3(N), dim3(64), 0, s, z, atoms, actions_out, q_out, n_actions, n_atoms);
    return check_launch("da_argmax_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_dqn_head_workspace_bytes(int M, int n_actions, int n_atoms) {
    return da_update_workspace(M, kDaH, n_actions, n_atoms);
}

extern "C" MI355PPO_API int mi355ppo_dqn_head_td_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b,
                                                            const float* w_target, const float* b_target, const int64_t* actions,
                                                            const float* rewards, const float* dones, double gamma, float* dh, float* dw,
                                                            float* db, float* scalars_out, float* target_q_out, float* td_target_out, int M,
                                                            int hidden, int n_actions, void* workspace, size_t workspace_bytes, void* stream) {
    return da_update_launch(false, "mi355ppo_dqn_head_td_fwd_bwd_f32", h, h_next, w, b, w_target, b_target, nullptr, actions, rewards, dones, gamma,
                            0.0, 0.0, dh, dw, db, scalars_out, target_q_out, td_target_out, M, hidden, n_actions, 1, workspace, workspace_bytes,
                            stream);
}

extern "C" MI355PPO_API int mi355ppo_c51_head_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b, const float* w_target,
                                                         const float* b_target, const float* atoms, const int64_t* actions, const float* rewards,
                                                         const float* dones, double gamma, double v_min, double v_max, float* dh, float* dw,
                                                         float* db, float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M,
                                                         int hidden, int n_actions, int n_atoms, void* workspace, size_t workspace_bytes,
                                                         void* stream) {
    return da_update_launch(true, "mi355ppo_c51_head_fwd_bwd_f32", h, h_next, w, b, w_target, b_target, atoms, actions, rewards, dones, gamma, v_min,
                            v_max, dh, dw, db, scalars_out, next_pmfs_out, target_pmfs_out, M, hidden, n_actions, n_atoms, workspace,
                            workspace_bytes, stream);
}
