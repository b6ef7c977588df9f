// Host-pointer twins of sac_atari.hip's entry points: the same row functions (sac_atari_rows.h; the gather and the dot products are
// dqn_atari_rows.h's da_gather_host, da_dot, da_dh and da_wgrad) in plain serial C++, in the device's orders: dot products ascending
// from 0.0f, the softmax and both expectations in ascending action order, dW / db over ascending batch rows, the scalars through the
// f64 slot fold.  Every output equals the device's bit for bit.  They live in a file of their own, beside host_twins.hip, so that
// the stand-alone sanitizer driver (tools/sac_atari_host_check.cpp) links them with api.hip alone.
#include "common.h"
#include "sac_atari_rows.h"

#include <string.h>

#include <vector>

#pragma clang fp contract(off)

using namespace mi355ppo;

namespace {

// z (M, n) = h W^T + b
void sd_forward_host(const float* h, const float* w, const float* b, int M, int n, float* z) {
    for (int r = 0; r < M; ++r)
        for (int j = 0; j < n; ++j) z[(size_t)r * n + j] = da_dot(h + (size_t)r * kDaH, w + (size_t)j * kDaH, b[j]);
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_replay_add2_u8_cpu(const uint8_t* obs, const uint8_t* next_obs, const int64_t* actions, const float* rewards,
                                                       const float* dones, uint8_t* ring_obs, uint8_t* ring_next_obs, int64_t* ring_actions,
                                                       float* ring_rewards, float* ring_dones, int64_t pos, int64_t slots, int n_envs) {
    const char* fn = "mi355ppo_replay_add2_u8_cpu";
    MI355_REQUIRE(obs && next_obs && actions && rewards && dones && ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = sd_ring_shape(fn, slots, n_envs, pos)) return rc;
    for (int which = 0; which < 2; ++which)
        for (int e = 0; e < n_envs; ++e) {
            const uint8_t* stack = (which ? next_obs : obs) + (int64_t)e * (kDaPlanes * kDaPix);
            uint8_t* dst = (which ? ring_next_obs : ring_obs) + 4 * da_frame(pos, e, n_envs);
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

extern "C" MI355PPO_API int mi355ppo_replay_gather2_u8_cpu(const uint8_t* ring_obs, const uint8_t* ring_next_obs, const int64_t* ring_actions,
                                                          const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                          const int64_t* env_inds, int64_t slots, int n_envs, uint8_t* frames_out,
                                                          int64_t* actions_out, float* rewards_out, float* dones_out, int M) {
    const char* fn = "mi355ppo_replay_gather2_u8_cpu";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && batch_inds && env_inds && frames_out && actions_out &&
                      rewards_out && dones_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_ring_shape(fn, slots, n_envs)) return rc;
    MI355_REQUIRE(M >= 1 && M <= kDaMaxRows, MI355PPO_EINVAL, "%s: rows=%d: 1 <= rows <= %d", fn, M, kDaMaxRows);
    da_gather_host(ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs, false, frames_out,
                   actions_out, rewards_out, dones_out, M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sacd_head_act_f32_cpu(const float* h, const float* w, const float* b, const float* noise_exp1,
                                                          int64_t* actions_out, float* probs_out, int N, int hidden, int n_actions) {
    const char* fn = "mi355ppo_sacd_head_act_f32_cpu";
    MI355_REQUIRE(h && w && b && noise_exp1 && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, N, hidden, n_actions, 1)) return rc;
    const int n = n_actions;
    std::vector<float> z((size_t)N * n);
    sd_forward_host(h, w, b, N, n, z.data());
    float p[kDqMaxAct], lp[kDqMaxAct];
    for (int r = 0; r < N; ++r) {
        sd_softmax(z.data() + (size_t)r * n, n, p, lp);
        if (probs_out)
            for (int a = 0; a < n; ++a) probs_out[(size_t)r * n + a] = p[a];
        actions_out[r] = (int64_t)sd_sample(p, noise_exp1 + (size_t)r * n, n);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sacd_critic_fwd_bwd_f32_cpu(const float* h_q1, const float* h_q2, const float* h_pi_next,
                                                                const float* h_q1t_next, const float* h_q2t_next, const float* w_q1,
                                                                const float* b_q1, const float* w_q2, const float* b_q2, const float* w_pi,
                                                                const float* b_pi, const float* w_q1t, const float* b_q1t, const float* w_q2t,
                                                                const float* b_q2t, const int64_t* actions, const float* rewards,
                                                                const float* dones, const float* alpha, double gamma, float* dh1, float* dh2,
                                                                float* dw1, float* db1, float* dw2, float* db2, float* scalars_out, float* v_out,
                                                                float* y_out, int M, int hidden, int n_actions) {
    const char* fn = "mi355ppo_sacd_critic_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h_q1 && h_q2 && h_pi_next && h_q1t_next && h_q2t_next && w_q1 && b_q1 && w_q2 && b_q2 && w_pi && b_pi && w_q1t && b_q1t && w_q2t &&
                      b_q2t && actions && rewards && dones && alpha && dh1 && dh2 && dw1 && db1 && dw2 && db2 && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, 1)) return rc;
    const int n = n_actions;
    const size_t mn = (size_t)M * n;
    std::vector<float> z(5 * mn), rows((size_t)4 * M), dz((size_t)2 * M);
    std::vector<int> act(M);
    sd_forward_host(h_q1, w_q1, b_q1, M, n, z.data());
    sd_forward_host(h_q2, w_q2, b_q2, M, n, z.data() + mn);
    sd_forward_host(h_pi_next, w_pi, b_pi, M, n, z.data() + 2 * mn);
    sd_forward_host(h_q1t_next, w_q1t, b_q1t, M, n, z.data() + 3 * mn);
    sd_forward_host(h_q2t_next, w_q2t, b_q2t, M, n, z.data() + 4 * mn);
    const float norm = (float)(2.0 / (double)M);
    for (int r = 0; r < M; ++r) {
        const float* zr = z.data() + (size_t)r * n;
        const SdCritic c = sd_critic_row(zr, zr + mn, zr + 2 * mn, zr + 3 * mn, zr + 4 * mn, n, actions[r], rewards[r], dones[r], alpha[0], (float)gamma,
                                         norm);
        rows[r] = c.sq1;
        rows[(size_t)M + r] = c.sq2;
        rows[(size_t)2 * M + r] = c.q1a;
        rows[(size_t)3 * M + r] = c.q2a;
        dz[r] = c.d1;
        dz[(size_t)M + r] = c.d2;
        act[r] = c.act;
        if (v_out) v_out[r] = c.V;
        if (y_out) y_out[r] = c.y;
        for (int k = 0; k < kDaH; ++k) {
            dh1[(size_t)r * kDaH + k] = da_dh(&c.d1, 1, w_q1 + (size_t)c.act * kDaH, k);
            dh2[(size_t)r * kDaH + k] = da_dh(&c.d2, 1, w_q2 + (size_t)c.act * kDaH, k);
        }
    }
    for (int c = 0; c < 2; ++c) {
        const float* h = c ? h_q2 : h_q1;
        const float* d = dz.data() + (size_t)c * M;
        float* dw = c ? dw2 : dw1;
        float* db = c ? db2 : db1;
        for (int a = 0; a < n; ++a) {
            for (int k = 0; k < kDaH; ++k) dw[(size_t)a * kDaH + k] = da_wgrad(act.data(), d, 1, M, a, 0, h, k);
            db[a] = da_wgrad(act.data(), d, 1, M, a, 0, nullptr, 0);
        }
    }
    for (int s = 0; s < 4; ++s) scalars_out[s] = sd_fold_host(rows.data() + (size_t)s * M, M, (double)M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_sacd_actor_fwd_bwd_f32_cpu(const float* h_pi, const float* h_q1, const float* h_q2, const float* w_pi,
                                                               const float* b_pi, const float* w_q1, const float* b_q1, const float* w_q2,
                                                               const float* b_q2, const float* alpha, double target_entropy, float* dh, float* dw,
                                                               float* db, float* entropy_rows_out, float* actor_loss_out, int M, int hidden,
                                                               int n_actions) {
    const char* fn = "mi355ppo_sacd_actor_fwd_bwd_f32_cpu";
    MI355_REQUIRE(h_pi && h_q1 && h_q2 && w_pi && b_pi && w_q1 && b_q1 && w_q2 && b_q2 && alpha && dh && dw && db && entropy_rows_out && actor_loss_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = da_shape(fn, M, hidden, n_actions, 1)) return rc;
    const int n = n_actions;
    const size_t mn = (size_t)M * n;
    std::vector<float> z(3 * mn), rows(M), dz(mn);
    sd_forward_host(h_pi, w_pi, b_pi, M, n, z.data());
    sd_forward_host(h_q1, w_q1, b_q1, M, n, z.data() + mn);
    sd_forward_host(h_q2, w_q2, b_q2, M, n, z.data() + 2 * mn);
    const float inv_mn = (float)(1.0 / ((double)M * (double)n));
    for (int r = 0; r < M; ++r) {
        const float* zr = z.data() + (size_t)r * n;
        float* d = dz.data() + (size_t)r * n;
        const SdActor a = sd_actor_row(zr, zr + mn, zr + 2 * mn, n, alpha[0], (float)target_entropy, inv_mn, d);
        rows[r] = a.s;
        entropy_rows_out[r] = a.e;
        for (int k = 0; k < kDaH; ++k) dh[(size_t)r * kDaH + k] = da_dh(d, n, w_pi, k);
    }
    for (int j = 0; j < n; ++j) {
        for (int k = 0; k < kDaH; ++k) dw[(size_t)j * kDaH + k] = sd_wgrad_dense(dz.data() + j, n, M, h_pi, k);
        db[j] = sd_wgrad_dense(dz.data() + j, n, M, nullptr, 0);
    }
    actor_loss_out[0] = sd_fold_host(rows.data(), M, (double)M * (double)n);
    return MI355PPO_OK;
}
