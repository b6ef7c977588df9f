// Rainbow (cleanrl/rainbow_atari.py): the prioritized n-step replay buffer in device memory and the noise composition of the four
// NoisyLinear layers (gfx950).  Row math: rainbow_rows.h.  The gather, the head's forward kernel and its categorical row are the
// ones dqn_atari.hip uses (qhead_wg.h).
//
//   add      one thread per pixel of obs and of next_obs: the four planes of a (4, 84, 84) stack become one 4-byte store into slot
//            pos of their ring.  Thread 0 of workgroup (0, 0) writes the action, the n-step reward and the done flag, sets the
//            leaf to max_priority ** alpha, walks its ancestors and bumps size.
//   sample   ONE workgroup: lane i draws its stratum's value from u[i], walks the tree and computes its weight; the weights' maximum is
//            folded through LDS and divided out.
//   gather   one thread per pixel word: the M obs frames, then the M next_obs frames, into (2M, 84, 84, 4) (qh_gather_kernel<false>).
//   update   ONE workgroup: the priorities and the running maximum; the leaves (of duplicate indices the highest batch position
//            writes); then the ancestors level by level from the deepest tree level, a barrier between levels.  Lanes that share a
//            parent compute the same sum from the same two words, so the level needs no atomics.
//   compose  one thread per element of the effective buffer: mu + sigma * eps.     grad   dmu = g, dsigma = g * eps.
//
// The tree kernels are single-workgroup and latency-bound (at most 1024 lanes, about 20 levels): plain f32 VALU and one f64 pow per lane.
// No entry point allocates or synchronises, none uses atomics; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "rainbow_rows.h"
#include "qhead_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// ---------------------------------------------------------------------------------------------------------------- the ring
// grid (ceil(7056 / 256), 2): y selects obs (0) / next_obs (1)
__global__ __launch_bounds__(256) void rb_add_kernel(const uint8_t* __restrict__ obs, const uint8_t* __restrict__ next_obs,
                                                     const int64_t* __restrict__ action, const float* __restrict__ reward,
                                                     const float* __restrict__ done, uint32_t* __restrict__ ring_obs,
                                                     uint32_t* __restrict__ ring_next, int64_t* __restrict__ ring_actions,
                                                     float* __restrict__ ring_rewards, float* __restrict__ ring_dones, float* tree,
                                                     const float* __restrict__ state, int64_t* __restrict__ size, int64_t pos, int64_t slots,
                                                     float alpha) {
    const int which = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < kDaPix) (which ? ring_next : ring_obs)[da_frame(pos, 0, 1) + p] = da_pack(which ? next_obs : obs, p);
    if (which == 0 && p == 0) {
        ring_actions[pos] = action[0];
        ring_rewards[pos] = reward[0];
        ring_dones[pos] = done[0];
        const int64_t leaf = rb_leaf(pos, slots);
        tree[leaf] = rb_pow(state[0], alpha);
        rb_propagate(tree, leaf);
        const int64_t s = size[0] + 1;
        size[0] = s < slots ? s : slots;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the tree
// numpy's max over B values held one per lane slot (lane i, i + 256, ...): folded through LDS, every thread returns it
__device__ float rb_wg_max(const float* vals, int B, float* red) {
    const int t = threadIdx.x;
    float m = vals[t < B ? t : 0];
    for (int i = t + 256; i < B; i += 256) m = rb_max(m, vals[i]);
    red[t] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] = rb_max(red[t], red[t + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// one workgroup of 256
__global__ __launch_bounds__(256) void rb_sample_kernel(const double* __restrict__ u, const float* __restrict__ tree,
                                                        const float* __restrict__ state, const int64_t* __restrict__ size, int64_t slots,
                                                        int64_t* __restrict__ indices, float* __restrict__ weights, int B) {
    __shared__ float w[kRbMaxBatch], red[256];
    const int t = threadIdx.x;
    const float total = tree[0], beta = state[1], n = (float)size[0];
    for (int i = t; i < B; i += 256) {
        const int64_t idx = rb_retrieve(tree, slots, rb_stratum(total, B, i, u[i]));
        indices[i] = idx;
        w[i] = rb_weight(n, tree[rb_leaf(idx, slots)], total, beta);
    }
    __syncthreads();
    const float wmax = rb_wg_max(w, B, red);
    for (int i = t; i < B; i += 256) weights[i] = w[i] / wmax;
}

// one workgroup of 256; lane i of the batch is thread i % 256
__global__ __launch_bounds__(256) void rb_update_kernel(const int64_t* __restrict__ indices, const float* __restrict__ loss, float* tree,
                                                        float* state, int64_t slots, float alpha, float eps, int B) {
    __shared__ int64_t node[kRbMaxBatch];
    __shared__ float pr[kRbMaxBatch], red[256];
    const int t = threadIdx.x;
    for (int i = t; i < B; i += 256) {
        node[i] = rb_leaf(op_clamp(indices[i], slots), slots);
        pr[i] = rb_priority(loss[i], eps);
    }
    __syncthreads();
    const float pm = rb_wg_max(pr, B, red);
    if (t == 0) state[0] = rb_running_max(state[0], pm);
    for (int i = t; i < B; i += 256) {
        bool last = true;                                       // the reference's serial loop: the highest batch position stays
        for (int j = i + 1; j < B; ++j) last = last && node[j] != node[i];
        if (last) tree[node[i]] = rb_pow(pr[i], alpha);
    }
    for (int d = rb_depth(2 * slots - 2); d >= 1; --d) {
        __syncthreads();                                        // level d is final: the leaves at d, the parents of level d + 1
        for (int i = t; i < B; i += 256) {
            const int64_t c = node[i];
            if (rb_depth(c) == d) {
                const int64_t p = (c - 1) / 2;
                tree[p] = tree[2 * p + 1] + tree[2 * p + 2];
                node[i] = p;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the noisy layers
// one thread per element, walked in the parameters' order
template <bool GRAD>
__global__ __launch_bounds__(256) void rb_noisy_kernel(RbSegs S, const float* __restrict__ src, const float* __restrict__ eps,
                                                       float* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= S.total) return;
    const int k = rb_seg_of(S, e);
    const int64_t o = e - S.eps[k];
    if constexpr (GRAD) {                                       // src: the effective buffer's gradient, dst: the flat gradient
        const float g = src[S.eff[k] + o];
        dst[S.mu[k] + o] = g;
        dst[S.sigma[k] + o] = g * eps[e];
    } else {                                                    // src: the parameters, dst: the effective buffer
        dst[S.eff[k] + o] = rb_compose(src[S.mu[k] + o], src[S.sigma[k] + o], eps[e]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the head
// forward: qh_fwd_kernel<kRbH2> (qhead_wg.h); passes 0: online on obs, 1: online on next_obs, 2: target on next_obs

// ws layout (floats): z (3 x M x J) | rows (2 x Mp: weighted loss | q) | dz (M x J)
struct RbWs {
    float *z, *rows, *dz;
};
static __host__ __device__ RbWs rb_ws(void* ws, int M, int J) {
    RbWs w;
    w.z = static_cast<float*>(ws);
    w.rows = w.z + (int64_t)3 * M * J;
    w.dz = w.rows + 2 * ((M + 63) / 64 * 64);
    return w;
}

// the dueling combine and the softmax of `passes` rows held in LDS (zs: passes x kDaMaxOut); qe[pass * kDqMaxAct + a] the expectations
__device__ void rb_dists(float* zs, float* qe, const float* __restrict__ support, int passes, int n, int na) {
    const int t = threadIdx.x;
    for (int i = t; i < passes * na; i += blockDim.x) rb_combine_col(zs + (i / na) * kDaMaxOut, n, na, i % na);
    __syncthreads();
    if (t < passes * n) {
        float* q = zs + (t / n) * kDaMaxOut + na + (t % n) * na;
        qe[(t / n) * kDqMaxAct + t % n] = dq_softmax_q(q, na, support, q);
    }
    __syncthreads();
}

// One workgroup per batch row.
__global__ __launch_bounds__(256) void rb_row_kernel(RbWs S, const float* __restrict__ w_online, const float* __restrict__ support,
                                                     const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                     const float* __restrict__ dones, const float* __restrict__ weights, float* __restrict__ dh,
                                                     float* __restrict__ loss_per_sample, int64_t* __restrict__ best_out,
                                                     float* __restrict__ next_pmfs, float* __restrict__ target_pmfs, int M, int Mp, int n, int na,
                                                     float gamma_n, float vmin, float vmax, float delta_z, float inv_m) {
    __shared__ float zs[3 * kDaMaxOut], qe[3 * kDqMaxAct], pl[kDqMaxAtoms], pu[kDqMaxAtoms], pdl[kDqMaxAtoms], pdu[kDqMaxAtoms], tp[kDqMaxAtoms],
        dq[kDqMaxAtoms], dqn[kDqMaxAtoms], dotv;
    const int t = threadIdx.x, r = blockIdx.x, J = (n + 1) * na;
    for (int i = t; i < 3 * J; i += 256) zs[(i / J) * kDaMaxOut + i % J] = S.z[((int64_t)(i / J) * M + r) * J + i % J];
    __syncthreads();
    rb_dists(zs, qe, support, 3, n, na);
    const int best = dq_argmax(qe + kDqMaxAct, n);                             // double Q: the online network picks on next_obs
    const int act = (int)op_clamp(actions[r], n);
    const float rew = rewards[r], done = dones[r], wr = weights[r];
    const float* pred = zs + na + act * na;                                    // online(obs) at the taken action
    const float ns = wg_c51_row({pl, pu, pdl, pdu, tp, dq, &dotv}, zs + 2 * kDaMaxOut + na + best * na, pred, support, rew, done, gamma_n, vmin,
                                vmax, delta_z, na, wr * inv_m, true, next_pmfs ? next_pmfs + (int64_t)r * na : nullptr,
                                target_pmfs ? target_pmfs + (int64_t)r * na : nullptr);      // the target's distribution at best
    if (t < na) dqn[t] = dq[t] / (float)n;
    if (t == 0) {
        loss_per_sample[r] = ns;
        S.rows[r] = ns * wr;
        S.rows[Mp + r] = qe[act];
        if (best_out) best_out[r] = best;
    }
    __syncthreads();
    for (int j = t; j < J; j += 256) S.dz[(int64_t)r * J + j] = j < na ? dq[j] : rb_dz_adv(dq, dqn, (j - na) / na, act, (j - na) % na);
    for (int c = t; c < kRbH2; c += 256) dh[(int64_t)r * kRbH2 + c] = rb_dh(dq, dqn, n, na, act, w_online, c);
}

// Workgroup j < J: dW_out[j, :] and db_out[j].  Workgroup J: scalars {loss, mean q}.
__global__ __launch_bounds__(256) void rb_wgrad_kernel(RbWs S, const float* __restrict__ h, float* __restrict__ dw, float* __restrict__ db,
                                                       float* __restrict__ scalars, int M, int Mp, int J, int na) {
    __shared__ double red[kOpFold];
    const int t = threadIdx.x, j = blockIdx.x;
    if (j == J) {
        wg_fold_scalars(S.rows, Mp, M, red, scalars);
        return;
    }
    for (int c = t; c < kRbHid; c += 256) dw[(int64_t)j * kRbHid + c] = rb_wgrad(S.dz, M, J, j, na, h, c);
    if (t == 0) db[j] = rb_wgrad(S.dz, M, J, j, na, nullptr, 0);
}

// actions[r] = argmax_a sum_k p[r, a, k] * support[k]; z: N x J from qh_fwd_kernel.  One workgroup of 128 per row.
__global__ __launch_bounds__(128) void rb_act_kernel(const float* __restrict__ z, const float* __restrict__ support, int64_t* __restrict__ actions,
                                                     float* __restrict__ q_out, int n, int na) {
    __shared__ float zs[kDaMaxOut], qe[kDqMaxAct];
    const int r = blockIdx.x, t = threadIdx.x, J = (n + 1) * na;
    for (int i = t; i < J; i += 128) zs[i] = z[(int64_t)r * J + i];
    __syncthreads();
    rb_dists(zs, qe, support, 1, n, na);
    if (q_out && t < n) q_out[(int64_t)r * n + t] = qe[t];
    if (t == 0) actions[r] = (int64_t)dq_argmax(qe, n);
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_rainbow_per_add_u8(const uint8_t* obs, const uint8_t* next_obs, const int64_t* action, const float* reward,
                                                       const float* done, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                                       float* ring_rewards, float* ring_dones, float* tree, float* state, int64_t* size,
                                                       int64_t pos, int64_t slots, double alpha, void* stream) {
    const char* fn = "mi355ppo_rainbow_per_add_u8";
    MI355_REQUIRE(obs && next_obs && action && reward && done && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && tree &&
                      state && size, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    MI355_REQUIRE(pos >= 0 && pos < slots, MI355PPO_EINVAL, "%s: pos=%lld slots=%lld: 0 <= pos < slots", fn, (long long)pos, (long long)slots);
    MI355_REQUIRE(aligned(ring_obs, 4) && aligned(ring_next_obs, 4), MI355PPO_EALIGN, "%s: the rings must be 4-byte aligned", fn);
    hipLaunchKernelGGL(rb_add_kernel, dim3((kDaPix + 255) / 256, 2), dim3(256), 0, as_stream(stream), obs, next_obs, action, reward, done,
                       reinterpret_cast<uint32_t*>(ring_obs), reinterpret_cast<uint32_t*>(ring_next_obs), ring_actions, ring_rewards, ring_dones,
                       tree, state, size, pos, slots, (float)alpha);
    return check_launch("rb_add_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_sample(const double* u, const float* tree, const float* state, const int64_t* size, int64_t slots,
                                                       int64_t* indices_out, float* weights_out, int B, void* stream) {
    const char* fn = "mi355ppo_rainbow_per_sample";
    MI355_REQUIRE(u && tree && state && size && indices_out && weights_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, B)) return rc;
    hipLaunchKernelGGL(rb_sample_kernel, dim3(1), dim3(256), 0, as_stream(stream), u, tree, state, size, slots, indices_out, weights_out, B);
    return check_launch("rb_sample_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_gather_u8(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                          const float* ring_rewards, const float* ring_dones, const int64_t* indices,
                                                          int64_t slots, uint8_t* frames_out, int64_t* actions_out, float* rewards_out,
                                                          float* dones_out, int M, void* stream) {
    const char* fn = "mi355ppo_rainbow_per_gather_u8";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && indices && frames_out && actions_out && rewards_out &&
                      dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, M)) return rc;
    MI355_REQUIRE(aligned(ring_obs, 4) && aligned(ring_next_obs, 4) && aligned(frames_out, 4), MI355PPO_EALIGN,
                  "%s: the rings and the batch must be 4-byte aligned", fn);
    return qh_gather_launch<false>(as_stream(stream), ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, indices, nullptr, slots, 1,
                                   frames_out, actions_out, rewards_out, dones_out, M);
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_update(const int64_t* indices, const float* loss_per_sample, float* tree, float* state,
                                                       int64_t slots, double alpha, double eps, int B, void* stream) {
    const char* fn = "mi355ppo_rainbow_per_update";
    MI355_REQUIRE(indices && loss_per_sample && tree && state, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, B)) return rc;
    hipLaunchKernelGGL(rb_update_kernel, dim3(1), dim3(256), 0, as_stream(stream), indices, loss_per_sample, tree, state, slots, (float)alpha,
                       (float)eps, B);
    return check_launch("rb_update_kernel");
}

static int rb_noisy_launch(bool grad, const char* fn, const float* src, const float* eps, float* dst, int n, int na, void* stream) {
    MI355_REQUIRE(src && eps && dst, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_noisy_shape(fn, n, na)) return rc;
    const RbSegs S = rb_segs(n, na);
    const unsigned gx = (unsigned)((S.total + 255) / 256);
    if (grad)
        hipLaunchKernelGGL(rb_noisy_kernel<true>, dim3(gx), dim3(256), 0, as_stream(stream), S, src, eps, dst);
    else
        hipLaunchKernelGGL(rb_noisy_kernel<false>, dim3(gx), dim3(256), 0, as_stream(stream), S, src, eps, dst);
    return check_launch("rb_noisy_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rainbow_noisy_compose_f32(const float* params, const float* eps, float* effective, int n_actions, int n_atoms,
                                                              void* stream) {
    return rb_noisy_launch(false, "mi355ppo_rainbow_noisy_compose_f32", params, eps, effective, n_actions, n_atoms, stream);
}

extern "C" MI355PPO_API int mi355ppo_rainbow_noisy_grad_f32(const float* effective_grad, const float* eps, float* grads, int n_actions,
                                                           int n_atoms, void* stream) {
    return rb_noisy_launch(true, "mi355ppo_rainbow_noisy_grad_f32", effective_grad, eps, grads, n_actions, n_atoms, stream);
}

extern "C" MI355PPO_API size_t mi355ppo_rainbow_head_act_workspace_bytes(int N, int n_actions, int n_atoms) {
    if (!rb_head_limits(N, n_actions, n_atoms)) return 0;
    return (size_t)N * (n_actions + 1) * n_atoms * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_rainbow_head_act_f32(const float* h, const float* w_out, const float* b_out, const float* support,
                                                         int64_t* actions_out, float* q_out, int N, int n_actions, int n_atoms, void* workspace,
                                                         size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_rainbow_head_act_f32";
    MI355_REQUIRE(h && w_out && b_out && support && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_head_shape(fn, N, n_actions, n_atoms)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_rainbow_head_act_workspace_bytes(N, n_actions, n_atoms))) return rc;
    hipStream_t s = as_stream(stream);
    const int J = (n_actions + 1) * n_atoms;
    float* z = static_cast<float*>(workspace);
    if (int rc = qh_fwd_launch<kRbH2>(s, QhPasses{{h}, {w_out}, {b_out}}, 1, z, N, J, n_atoms)) return rc;
    hipLaunchKernelGGL(rb_act_kernel, dim3(N), dim3(128), 0, s, z, support, actions_out, q_out, n_actions, n_atoms);
    return check_launch("rb_act_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_rainbow_head_workspace_bytes(int M, int n_actions, int n_atoms) {
    if (!rb_head_limits(M, n_actions, n_atoms)) return 0;
    return (size_t)((int64_t)4 * M * (n_actions + 1) * n_atoms + 2 * op_mp(M)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_rainbow_head_fwd_bwd_f32(const float* h, const float* h_next, const float* h_next_target, const float* w_out,
                                                             const float* b_out, const float* w_out_target, const float* b_out_target,
                                                             const float* support, const int64_t* actions, const float* rewards,
                                                             const float* dones, const float* weights, double gamma_n, double v_min, double v_max,
                                                             float* dh, float* dw_out, float* db_out, float* scalars_out, float* loss_per_sample,
                                                             int64_t* best_actions_out, float* next_pmfs_out, float* target_pmfs_out, int M,
                                                             int n_actions, int n_atoms, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_rainbow_head_fwd_bwd_f32";
    MI355_REQUIRE(h && h_next && h_next_target && w_out && b_out && w_out_target && b_out_target && support && actions && rewards && dones &&
                      weights && dh && dw_out && db_out && scalars_out && loss_per_sample, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_head_shape(fn, M, n_actions, n_atoms)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_rainbow_head_workspace_bytes(M, n_actions, n_atoms))) return rc;
    hipStream_t s = as_stream(stream);
    const int J = (n_actions + 1) * n_atoms, Mp = (int)op_mp(M);
    const RbWs S = rb_ws(workspace, M, J);
    const QhPasses H{{h, h_next, h_next_target}, {w_out, w_out, w_out_target}, {b_out, b_out, b_out_target}};
    if (int rc = qh_fwd_launch<kRbH2>(s, H, 3, S.z, M, J, n_atoms)) return rc;
    hipLaunchKernelGGL(rb_row_kernel, dim3(M), dim3(256), 0, s, S, w_out, support, actions, rewards, dones, weights, dh, loss_per_sample,
                       best_actions_out, next_pmfs_out, target_pmfs_out, M, Mp, n_actions, n_atoms, (float)gamma_n, (float)v_min, (float)v_max,
                       (float)((v_max - v_min) / (double)(n_atoms - 1)), (float)(1.0 / (double)M));
    if (int rc = check_launch("rb_row_kernel")) return rc;
    hipLaunchKernelGGL(rb_wgrad_kernel, dim3(J + 1), dim3(256), 0, s, S, h, dw_out, db_out, scalars_out, M, Mp, J, n_atoms);
    return check_launch("rb_wgrad_kernel");
}
