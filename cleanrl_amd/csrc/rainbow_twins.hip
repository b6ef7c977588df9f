// Host-pointer twins of rainbow.hip's entry points: the same row functions (rainbow_rows.h; the gather, the categorical row and the
// f64 slot fold are the headers' da_gather_host, c51_row_host and op_fold_mean_host) in plain serial C++.  They live in a
// file of their own, beside host_twins.hip, so that the stand-alone sanitizer driver (tools/rainbow_host_check.cpp) links them
// with api.hip alone.  The tree's ancestors are rebuilt the reference's way here, one _propagate per written leaf; the device
// rebuilds them level by level, and both leave every inner node equal to the f32 sum of its children's final values.
#include "common.h"
#include "rainbow_rows.h"
#include "offpolicy_rows.h"

#include <string.h>

#include <vector>

#pragma clang fp contract(off)

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_rainbow_per_add_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* action,
                                                           const float* reward, const float* done, uint8_t* ring_obs, uint8_t* ring_next_obs,
                                                           int64_t* ring_actions, float* ring_rewards, float* ring_dones, float* tree,
                                                           float* state, int64_t* size, int64_t pos, int64_t slots, double alpha) {
    const char* fn = "mi355ppo_rainbow_per_add_u8_cpu";
    MI355_REQUIRE(obs && next_obs && action && reward && done && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && tree &&
                      state && size, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    MI355_REQUIRE(pos >= 0 && pos < slots, MI355PPO_EINVAL, "%s: pos=%lld slots=%lld: 0 <= pos < slots", fn, (long long)pos, (long long)slots);
    for (int which = 0; which < 2; ++which) {
        const uint8_t* stack = which ? next_obs : obs;
        uint8_t* dst = (which ? ring_next_obs : ring_obs) + 4 * da_frame(pos, 0, 1);
        for (int p = 0; p < kDaPix; ++p) {
            const uint32_t v = da_pack(stack, p);
            memcpy(dst + 4 * (int64_t)p, &v, 4);
        }
    }
    ring_actions[pos] = action[0];
    ring_rewards[pos] = reward[0];
    ring_dones[pos] = done[0];
    const int64_t leaf = rb_leaf(pos, slots);
    tree[leaf] = rb_pow(state[0], (float)alpha);
    rb_propagate(tree, leaf);
    const int64_t s = size[0] + 1;
    size[0] = s < slots ? s : slots;
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_sample_cpu(const double* u, const float* tree, const float* state, const int64_t* size,
                                                           int64_t slots, int64_t* indices_out, float* weights_out, int B) {
    const char* fn = "mi355ppo_rainbow_per_sample_cpu";
    MI355_REQUIRE(u && tree && state && size && indices_out && weights_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, B)) return rc;
    const float total = tree[0], beta = state[1], n = (float)size[0];
    float wmax = 0.0f;
    for (int i = 0; i < B; ++i) {
        const int64_t idx = rb_retrieve(tree, slots, rb_stratum(total, B, i, u[i]));
        indices_out[i] = idx;
        weights_out[i] = rb_weight(n, tree[rb_leaf(idx, slots)], total, beta);
        wmax = i ? rb_max(wmax, weights_out[i]) : weights_out[i];
    }
    for (int i = 0; i < B; ++i) weights_out[i] = weights_out[i] / wmax;
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_gather_u8_cpu(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                              const float* ring_rewards, const float* ring_dones, const int64_t* indices,
                                                              int64_t slots, uint8_t* frames_out, int64_t* actions_out, float* rewards_out,
                                                              float* dones_out, int M) {
    const char* fn = "mi355ppo_rainbow_per_gather_u8_cpu";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && indices && frames_out && actions_out && rewards_out &&
                      dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, M)) return rc;
    da_gather_host(ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, indices, nullptr, slots, 1, false, frames_out, actions_out,
                   rewards_out, dones_out, M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rainbow_per_update_cpu(const int64_t* indices, const float* loss_per_sample, float* tree, float* state,
                                                           int64_t slots, double alpha, double eps, int B) {
    const char* fn = "mi355ppo_rainbow_per_update_cpu";
    MI355_REQUIRE(indices && loss_per_sample && tree && state, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_ring_shape(fn, slots)) return rc;
    if (int rc = rb_batch_shape(fn, B)) return rc;
    float pm = rb_priority(loss_per_sample[0], (float)eps);
    for (int i = 1; i < B; ++i) pm = rb_max(pm, rb_priority(loss_per_sample[i], (float)eps));
    state[0] = rb_running_max(state[0], pm);
    for (int i = 0; i < B; ++i) {
        const int64_t leaf = rb_leaf(op_clamp(indices[i], slots), slots);
        tree[leaf] = rb_pow(rb_priority(loss_per_sample[i], (float)eps), (float)alpha);
        rb_propagate(tree, leaf);
    }
    return MI355PPO_OK;
}

// the element counts are host arithmetic: one definition serves the device path too
extern "C" MI355PPO_API int64_t mi355ppo_rainbow_noisy_count(int n_actions, int n_atoms, int which) {
    if (!rb_noisy_limits(n_actions, n_atoms)) return 0;
    const RbSegs S = rb_segs(n_actions, n_atoms);
    return which ? S.params : S.total;
}

static int rb_noisy_host(bool grad, const char* fn, const float* src, const float* eps, float* dst, int n, int na) {
    MI355_REQUIRE(src && eps && dst, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_noisy_shape(fn, n, na)) return rc;
    const RbSegs S = rb_segs(n, na);
    for (int k = 0; k < kRbSegs; ++k)
        for (int64_t o = 0; o < S.cnt[k]; ++o) {
            if (grad) {
                const float g = src[S.eff[k] + o];
                dst[S.mu[k] + o] = g;
                dst[S.sigma[k] + o] = g * eps[S.eps[k] + o];
            } else {
                dst[S.eff[k] + o] = rb_compose(src[S.mu[k] + o], src[S.sigma[k] + o], eps[S.eps[k] + o]);
            }
        }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rainbow_noisy_compose_f32_cpu(const float* params, const float* eps, float* effective, int n_actions,
                                                                  int n_atoms) {
    return rb_noisy_host(false, "mi355ppo_rainbow_noisy_compose_f32_cpu", params, eps, effective, n_actions, n_atoms);
}

extern "C" MI355PPO_API int mi355ppo_rainbow_noisy_grad_f32_cpu(const float* effective_grad, const float* eps, float* grads, int n_actions,
                                                               int n_atoms) {
    return rb_noisy_host(true, "mi355ppo_rainbow_noisy_grad_f32_cpu", effective_grad, eps, grads, n_actions, n_atoms);
}

// ------------------------------------------------------------------------------------------------ the dueling distributional head
namespace {

// one row's outputs of one pass, combined and normalised: z (J) holds the value logits and then each action's distribution
void rb_row_dists(const float* hrow, const float* w, const float* b, const float* support, int n, int na, float* z, float* qe) {
    const int J = (n + 1) * na;
    for (int j = 0; j < J; ++j) z[j] = rb_head_dot(hrow, w, b, j, na);
    for (int k = 0; k < na; ++k) rb_combine_col(z, n, na, k);
    for (int a = 0; a < n; ++a) qe[a] = dq_softmax_q(z + na + a * na, na, support, z + na + a * na);
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_rainbow_head_act_f32_cpu(const float* h, const float* w_out, const float* b_out, const float* support,
                                                             int64_t* actions_out, float* q_out, int N, int n_actions, int n_atoms) {
    const char* fn = "mi355ppo_rainbow_head_act_f32_cpu";
    MI355_REQUIRE(h && w_out && b_out && support && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_head_shape(fn, N, n_actions, n_atoms)) return rc;
    std::vector<float> z((size_t)(n_actions + 1) * n_atoms), qe(n_actions);
    for (int r = 0; r < N; ++r) {
        rb_row_dists(h + (size_t)r * kRbH2, w_out, b_out, support, n_actions, n_atoms, z.data(), qe.data());
        if (q_out)
            for (int a = 0; a < n_actions; ++a) q_out[(size_t)r * n_actions + a] = qe[a];
        actions_out[r] = dq_argmax(qe.data(), n_actions);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rainbow_head_fwd_bwd_f32_cpu(const float* h, const float* h_next, const float* h_next_target,
                                                                 const float* w_out, const float* b_out, const float* w_out_target,
                                                                 const float* b_out_target, const float* support, const int64_t* actions,
                                                                 const float* rewards, const float* dones, const float* weights, double gamma_n,
                                                                 double v_min, double v_max, float* dh, float* dw_out, float* db_out,
                                                                 float* scalars_out, float* loss_per_sample, int64_t* best_actions_out,
                                                                 float* next_pmfs_out, float* target_pmfs_out, int M, int n_actions,
                                                                 int n_atoms) {
    const char* fn = "mi355ppo_rainbow_head_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h && h_next && h_next_target && w_out && b_out && w_out_target && b_out_target && support && actions && rewards && dones &&
                      weights && dh && dw_out && db_out && scalars_out && loss_per_sample, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = rb_head_shape(fn, M, n_actions, n_atoms)) return rc;
    const int n = n_actions, na = n_atoms, J = (n + 1) * na;
    const float gn = (float)gamma_n, vmin = (float)v_min, vmax = (float)v_max, delta_z = (float)((v_max - v_min) / (double)(na - 1)),
                inv_m = (float)(1.0 / (double)M);
    std::vector<float> zo(J), zn(J), zt(J), qo(n), qn(n), qt(n), tmp((size_t)5 * na), dq(na), dqn(na), dz((size_t)M * J), rows((size_t)2 * M);
    for (int r = 0; r < M; ++r) {
        rb_row_dists(h + (size_t)r * kRbH2, w_out, b_out, support, n, na, zo.data(), qo.data());
        rb_row_dists(h_next + (size_t)r * kRbH2, w_out, b_out, support, n, na, zn.data(), qn.data());
        rb_row_dists(h_next_target + (size_t)r * kRbH2, w_out_target, b_out_target, support, n, na, zt.data(), qt.data());
        const int best = dq_argmax(qn.data(), n), act = (int)op_clamp(actions[r], n);
        const float wr = weights[r];
        const float* pred = zo.data() + na + act * na;
        const float ns = c51_row_host(zt.data() + na + best * na, pred, support, rewards[r], dones[r], gn, vmin, vmax, delta_z, na, wr * inv_m, true,
                                      next_pmfs_out ? next_pmfs_out + (size_t)r * na : nullptr,
                                      target_pmfs_out ? target_pmfs_out + (size_t)r * na : nullptr, tmp.data(), dq.data());
        loss_per_sample[r] = ns;
        rows[r] = ns * wr;
        rows[(size_t)M + r] = qo[act];
        if (best_actions_out) best_actions_out[r] = best;
        for (int k = 0; k < na; ++k) dqn[k] = dq[k] / (float)n;
        for (int j = 0; j < J; ++j) dz[(size_t)r * J + j] = j < na ? dq[j] : rb_dz_adv(dq.data(), dqn.data(), (j - na) / na, act, (j - na) % na);
        for (int c = 0; c < kRbH2; ++c) dh[(size_t)r * kRbH2 + c] = rb_dh(dq.data(), dqn.data(), n, na, act, w_out, c);
    }
    for (int j = 0; j < J; ++j) {
        for (int c = 0; c < kRbHid; ++c) dw_out[(size_t)j * kRbHid + c] = rb_wgrad(dz.data(), M, J, j, na, h, c);
        db_out[j] = rb_wgrad(dz.data(), M, J, j, na, nullptr, 0);
    }
    for (int s = 0; s < 2; ++s) scalars_out[s] = op_fold_mean_host(rows.data() + (size_t)s * M, M);
    return MI355PPO_OK;
}
