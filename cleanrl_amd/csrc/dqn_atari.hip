// Atari DQN / C51 (cleanrl/dqn_atari.py, cleanrl/c51_atari.py): the u8 frame ring of the reference's memory-optimised ReplayBuffer in
// device memory, and the wide Q head Linear(512, n_actions * n_atoms) with its loss, projection and backward (gfx950).  The NatureCNN
// trunk and Linear(3136, 512) in front of the head are the matrix-pipe kernels of conv*.hip / gemm*.hip; they run on the gathered batch.
//
//   add      one thread per pixel: the four planes of an (4, 84, 84) stack become one 4-byte store into the channels-last ring.  obs goes
//            to slot pos, next_obs to (pos + 1) % slots; with one slot only next_obs is written (it would win), so no two threads share a word.
//   gather   one thread per pixel word: frames (batch_inds, env_inds) and ((batch_inds + 1) % slots, env_inds) into (2M, 84, 84, 4).
//   forward  both heads in one launch, spread over 8-row tiles x 32-output tiles x {online, target}: h's rows sit in LDS, W streams from
//            L2 through a 32 x 64 LDS tile; thread (row, output) runs its dot product in ascending k.
//   row      one workgroup per batch row: the softmax of each action's atoms (one thread per action and network), the target's argmax,
//            td_target or the projection (one thread per atom), the loss terms, dz of the taken action's atoms and dh (two columns a thread).
//   wgrad    one workgroup per output row j: dW[j, :] and db[j] over the batch rows that took j's action, ascending; zeros elsewhere.  One
//            more workgroup folds the two row scalars in f64 slots (wg_fold_mean).
//
// Everything is plain f32 VALU: at batch 32 the step is latency-bound.  No entry point allocates or synchronises,
// none uses atomics; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "dqn_atari_rows.h"
#include "offpolicy_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kDaTJ = 32;            // outputs per forward tile
constexpr int kDaTK = 64;            // k-depth of the staged weight tile
constexpr int kDaTLd = kDaTK + 1;    // padded: lane j reads word j * 65 + k, 32 different banks

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

// grid (ceil(7056 / 256), 2M): frame y < M is the observation, y >= M the next observation of sample y - M
__global__ __launch_bounds__(256) void da_gather_kernel(const uint32_t* __restrict__ ring, const int64_t* __restrict__ ring_actions,
                                                        const float* __restrict__ ring_rewards, const float* __restrict__ ring_dones,
                                                        const int64_t* __restrict__ bi, const int64_t* __restrict__ ei, int64_t slots, int N,
                                                        uint32_t* __restrict__ frames, int64_t* __restrict__ actions, float* __restrict__ rewards,
                                                        float* __restrict__ dones, int M) {
    const int f = blockIdx.y, m = f < M ? f : f - M;
    const int64_t slot = op_clamp(bi[m], slots);
    const int e = (int)op_clamp(ei[m], N);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < kDaPix) frames[(int64_t)f * kDaPix + p] = ring[da_frame(f < M ? slot : da_next_slot(slot, slots), e, N) + p];
    if (f < M && p == 0) {
        actions[m] = ring_actions[slot * N + e];
        rewards[m] = ring_rewards[slot * N + e];
        dones[m] = ring_dones[slot * N + e];
    }
}

// ---------------------------------------------------------------------------------------------------------------- the heads
struct DaHeads {
    const float *h[2], *w[2], *b[2];           // 0: online on obs, 1: target on next_obs
};

// z[net][r, j] = b[j] + sum_k h[r, k] * W[j, k].  grid (ceil(J / 32), ceil(M / 8), nets); z: nets x M x J
__global__ __launch_bounds__(256) void da_fwd_kernel(DaHeads H, float* __restrict__ z, int M, int J) {
    __shared__ float hs[kOpRows * kDaH], wt[kDaTJ * kDaTLd];
    const int t = threadIdx.x, net = blockIdx.z, j0 = blockIdx.x * kDaTJ, r0 = blockIdx.y * kOpRows;
    const float* __restrict__ h = H.h[net];
    const float* __restrict__ W = H.w[net];
    for (int i = t; i < kOpRows * kDaH; i += 256) {
        const int r = i / kDaH;
        hs[i] = (r0 + r < M) ? h[(int64_t)r0 * kDaH + i] : 0.0f;
    }
    const int jj = t & (kDaTJ - 1), r = t / kDaTJ;
    const float* x = hs + r * kDaH;
    float acc = 0.0f;
    for (int k0 = 0; k0 < kDaH; k0 += kDaTK) {
        __syncthreads();                                    // hs is complete (first pass); the previous tile has been read
        for (int i = t; i < kDaTJ * kDaTK; i += 256) {
            const int wj = i / kDaTK, wk = i - wj * kDaTK;
            wt[wj * kDaTLd + wk] = (j0 + wj < J) ? W[(int64_t)(j0 + wj) * kDaH + k0 + wk] : 0.0f;
        }
        __syncthreads();
        for (int kk = 0; kk < kDaTK; ++kk) acc = op_mac(acc, x[k0 + kk], wt[jj * kDaTLd + kk]);
    }
    if (r0 + r < M && j0 + jj < J) z[((int64_t)net * M + r0 + r) * J + j0 + jj] = acc + H.b[net][j0 + jj];
}

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
        const float delta_z = atoms[1] - atoms[0];
        if (t < na) {
            const float p = zt[best * na + t];
            const C51Proj e = c51_proj_elem(rew, done, gamma, atoms[t], vmin, vmax, delta_z, na, p);
            pl[t] = e.l;
            pu[t] = e.u;
            pdl[t] = e.dml;
            pdu[t] = e.dmu;
            if (aux_a) aux_a[(int64_t)r * na + t] = p;
        }
        __syncthreads();
        if (t < na) {
            const float v = c51_proj_atom(t, pl, pu, pdl, pdu, na);
            tp[t] = v;
            if (aux_b) aux_b[(int64_t)r * na + t] = v;
        }
        __syncthreads();
        if (t < na) {
            const C51Loss e = c51_loss_elem(tp[t], zo[act * na + t], norm);
            pl[t] = e.term;
            pdl[t] = e.g;
            pdu[t] = e.gp;
        }
        __syncthreads();
        if (t == 0) {
            float s = 0.0f, dot = 0.0f;
            for (int k = 0; k < na; ++k) {
                s = s + pl[k];
                dot = dot + pdu[k];
            }
            dotv = dot;
            S.rows[r] = -s;
            S.rows[Mp + r] = qo[act];
        }
        __syncthreads();
        if (t < na) {
            const float d = c51_dlogit(zo[act * na + t], pdl[t], dotv);
            dzs[t] = d;
            S.dz[(int64_t)r * na + t] = d;
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
        for (int s = 0; s < 2; ++s) {
            const float m = wg_fold_mean(S.rows + (int64_t)s * Mp, M, red);
            if (t == 0) scalars[s] = m;
        }
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

// actions[r] = argmax_a q[r, a]; z: N x J from da_fwd_kernel.  One workgroup of 64 per row: thread a takes action a's atoms.
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
    DaHeads H;
    H.h[0] = h, H.w[0] = w, H.b[0] = b;
    H.h[1] = h_next, H.w[1] = w_target, H.b[1] = b_target;
    hipLaunchKernelGGL(da_fwd_kernel, dim3((J + kDaTJ - 1) / kDaTJ, op_tiles(M), 2), dim3(256), 0, s, H, S.z, M, J);
    if (int rc = check_launch("da_fwd_kernel")) return rc;
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
    hipLaunchKernelGGL(da_gather_kernel, dim3((kDaPix + 255) / 256, 2 * M), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint32_t*>(ring_frames), ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs,
                       reinterpret_cast<uint32_t*>(frames_out), actions_out, rewards_out, dones_out, M);
    return check_launch("da_gather_kernel");
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
    DaHeads H;
    H.h[0] = H.h[1] = h, H.w[0] = H.w[1] = w, H.b[0] = H.b[1] = b;
    hipLaunchKernelGGL(da_fwd_kernel, dim3((J + kDaTJ - 1) / kDaTJ, op_tiles(N), 1), dim3(256), 0, s, H, z, N, J);
    if (int rc = check_launch("da_fwd_kernel")) return rc;
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
