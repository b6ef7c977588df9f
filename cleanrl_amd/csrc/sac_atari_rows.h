// Row / element math of the discrete-SAC head kernels (sac_atari.hip: sac_atari.py) and their host twins (sac_atari_twins.hip): one
// definition compiled for both sides, so a twin returns the device's bits.  The frame words, the head's dot product, dh and the
// taken-action weight gradient are dqn_atari_rows.h's; op_exp / op_log / sac_soft_q / sac_actor_row are sac_rows.h's; op_mac, op_min,
// op_td_target and op_mse_row are offpolicy_rows.h's.
//
// * The buffer is the reference's plain ReplayBuffer (sac_atari.py does not pass optimize_memory_usage): TWO u8 rings (slots, n_envs,
//   84, 84, 4), channels-last; a step's obs goes to ring A at slot pos and its next_obs to ring B at the same slot.  Every offset into
//   a ring is 64-bit (da_frame): two default rings are 56.4 GB.
// * Five heads Linear(512, n) feed one update: the actor's fc_logits, fc_q of qf1 / qf2 and of their targets.
// * The softmax of a row's n logits: exp(z - max) through op_exp, the sum in ascending action order, logp = (z - max) - log(sum)
//   through op_log, p = exp(z - max) / sum.  Where a logit sits more than 87 below the maximum p is exactly 0 and logp stays finite.
// * V = sum_a p_a * (min(q1t_a, q2t_a) - alpha * logp_a) and s = sum_a p_a * (alpha * logp_a - min(q1_a, q2_a)) add in ascending a
//   from 0.0f;  y = rewards + ((1 - dones) * gamma) * V is the script's association (op_td_target), not dqn_atari.py's.
// * The actor's logit gradient is dz_j = (p_j * (t_j - s)) * 1 / (M n): the log_softmax path's own term, alpha * (p_j - p_j sum_a p_a),
//   is zero analytically and is left out.
#pragma once
#include "dqn_atari_rows.h"

namespace mi355ppo {

// Categorical(logits=z).probs and F.log_softmax(z) of one row, n <= kDqMaxAct
MI355_HD void sd_softmax(const float* z, int n, float* p, float* lp) {
    float mx = z[0];
    for (int a = 1; a < n; ++a) mx = (z[a] > mx) ? z[a] : mx;
    float s = 0.0f;
    for (int a = 0; a < n; ++a) {
        const float e = op_exp(z[a] - mx);
        p[a] = e;
        s = s + e;
    }
    const float ls = op_log(s);
    for (int a = 0; a < n; ++a) {
        lp[a] = (z[a] - mx) - ls;
        p[a] = p[a] / s;
    }
}

// One batch row of the critic update.  zq1 / zq2: the critics' q on obs; zpi / zq1t / zq2t: the actor's logits and the target
// critics' q on next_obs.  norm = 2 / M.
struct SdCritic {
    float V, y, d1, d2, sq1, sq2, q1a, q2a;
    int act;
};
MI355_HD SdCritic sd_critic_row(const float* zq1, const float* zq2, const float* zpi, const float* zq1t, const float* zq2t, int n, int64_t action,
                                float rew, float done, float alpha, float gamma, float norm) {
    float p[kDqMaxAct], lp[kDqMaxAct];
    sd_softmax(zpi, n, p, lp);
    SdCritic c;
    float v = 0.0f;
    for (int a = 0; a < n; ++a) v = v + p[a] * sac_soft_q(zq1t[a], zq2t[a], alpha, lp[a]);
    c.V = v;
    c.y = op_td_target(rew, done, gamma, v);
    c.act = (int)op_clamp(action, n);
    c.q1a = zq1[c.act];
    c.q2a = zq2[c.act];
    c.d1 = op_mse_row(c.q1a, c.y, norm, &c.sq1);
    c.d2 = op_mse_row(c.q2a, c.y, norm, &c.sq2);
    return c;
}

// One batch row of the actor update.  zpi: the actor's logits on obs; zq1 / zq2: the critics' q on obs (constants).  inv_mn =
// 1 / (M n); te: target_entropy.  dz (n) = d actor_loss / d logits of the row.
struct SdActor {
    float s;          // sum_a p_a * (alpha * logp_a - min(q1_a, q2_a)): the row's share of actor_loss * M n
    float e;          // sum_a p_a * (logp_a + target_entropy) / n: the row's share of the temperature loss
};
MI355_HD SdActor sd_actor_row(const float* zpi, const float* zq1, const float* zq2, int n, float alpha, float te, float inv_mn, float* dz) {
    float p[kDqMaxAct], lp[kDqMaxAct], t[kDqMaxAct];
    sd_softmax(zpi, n, p, lp);
    float s = 0.0f, e = 0.0f;
    for (int a = 0; a < n; ++a) {
        t[a] = sac_actor_row(alpha, lp[a], zq1[a], zq2[a]);
        s = s + p[a] * t[a];
        e = e + p[a] * (lp[a] + te);
    }
    for (int a = 0; a < n; ++a) dz[a] = (p[a] * (t[a] - s)) * inv_mn;
    SdActor r;
    r.s = s;
    r.e = e / (float)n;
    return r;
}

// Categorical.sample as the library draws it (catrow.h's rule): argmax_a p_a / q_a, q ~ Exp(1) supplied; the first maximum wins, a
// NaN never does
MI355_HD int sd_sample(const float* p, const float* q, int n) {
    int best = 0;
    float bestv = -__builtin_inff();
    for (int a = 0; a < n; ++a) {
        const float v = p[a] / q[a];
        if (v > bestv) {
            bestv = v;
            best = a;
        }
    }
    return best;
}

// dense dW[j, k] (h != nullptr) or db[j] (h == nullptr): dzj[r] = dz[r, j] over every batch row, ascending
MI355_HD float sd_wgrad_dense(const float* dzj, int64_t stride, int M, const float* h, int k) {
    float acc = 0.0f;
    for (int r = 0; r < M; ++r) acc = h ? op_mac(acc, dzj[r * stride], h[(int64_t)r * kDaH + k]) : acc + dzj[r * stride];
    return acc;
}

// sd_fold (sac_atari.hip) on the host, in its order: kOpFold f64 slots, then the slots in order; sum / denom
inline float sd_fold_host(const float* v, int M, double denom) {
    double tot = 0.0;
    for (int t = 0; t < kOpFold; ++t) {
        double s = 0.0;
        for (int k = t; k < M; k += kOpFold) s += (double)v[k];
        tot += s;
    }
    return (float)(tot / denom);
}

// host-side argument check of the ring entry points and of their twins
inline int sd_ring_shape(const char* fn, int64_t slots, int N, int64_t pos) {
    if (int rc = da_ring_shape(fn, slots, N)) return rc;
    MI355_REQUIRE(pos >= 0 && pos < slots && N <= (1 << 16), MI355PPO_EINVAL, "%s: pos=%lld slots=%lld n_envs=%d: 0 <= pos < slots, n_envs <= 65536",
                  fn, (long long)pos, (long long)slots, N);
    return MI355PPO_OK;
}

}  // namespace mi355ppo
