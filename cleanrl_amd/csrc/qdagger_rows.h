// Row math of the QDagger head kernels (qdagger.hip: qdagger_dqn_atari_impalacnn.py:192-195, 294-306, 403-415) and their host twins
// (host_twins.hip): one definition compiled for both sides, so a twin returns the device's bits.  op_mac / op_mse_row / op_clamp are
// offpolicy_rows.h's, op_exp / op_log sac_rows.h's, dq_argmax / dq_td_target dqn_rows.h's.
//
// * The head is Linear(256, n) on the post-ReLU h of Linear(3872, 256).  Every dot product starts at 0.0f and adds its products in
//   ascending index order through op_mac, then adds the bias.
// * One batch row:  td_target = r + gamma * max_j q_target[j] * (1 - d);  the TD term (td_target - q[a])^2;  with t = teacher_q / T
//   and s = q / T the distillation term  sum_j -softmax(t)[j] * (log_softmax(s)[j] - log_softmax(t)[j])  in ascending j.
//   softmax / log_softmax of a row v: mx = max v, e[j] = op_exp(v[j] - mx), sum ascending, p[j] = e[j] / sum,
//   logp[j] = (v[j] - mx) - op_log(sum).
// * loss = mean_r TD + distill_coeff * SUM_r distillation (the reference sums the KL over the batch; torch.mean of a scalar is a no-op).
// * dq[r, j] = [j == a_r] (2 / M) (q[r, a_r] - td_target_r) + (distill_coeff / T) (softmax(s_r)[j] - softmax(t_r)[j]): dense over the
//   actions.  dh[r, k] adds dq[r, j] * W[j, k] over ascending j; dW[j, k] adds dq[r, j] * h[r, k] over ALL rows in ascending r, db
//   likewise.  No atomics.
// * Scalars {loss, q_loss, distill_loss, mean q[r, a_r]}: the row terms through the f64 slot fold (kOpFold slots, then the slots in
//   order); q_loss and mean q are means, distill_loss the sum; loss = q_loss + distill_coeff * distill_loss in f32.
#pragma once
#include "dqn_rows.h"

namespace mi355ppo {

constexpr int kQdH = 256;            // hidden width: Linear(3872, 256)
constexpr int kQdMaxRows = 1024;     // batch rows of an update / of an act call

MI355_HD bool qd_limits(int M, int hidden, int n) { return M >= 1 && M <= kQdMaxRows && hidden == kQdH && n >= 2 && n <= kDqMaxAct; }
// host-side argument check of the entry points and of their twins
inline int qd_shape(const char* fn, int M, int hidden, int n) {
    MI355_REQUIRE(qd_limits(M, hidden, n), MI355PPO_EINVAL,
                  "%s: rows=%d hidden=%d n_actions=%d: the QDagger head takes 1 <= rows <= %d, hidden == %d, 2 <= n_actions <= %d", fn, M,
                  hidden, n, kQdMaxRows, kQdH, kDqMaxAct);
    return MI355PPO_OK;
}

// z[j] = b[j] + sum_k h[k] * W[j, k]
MI355_HD float qd_dot(const float* h, const float* w, float b) {
    float acc = 0.0f;
    for (int k = 0; k < kQdH; ++k) acc = op_mac(acc, h[k], w[k]);
    return acc + b;
}

// softmax and log_softmax of v[0..n) / T into p and logp
MI355_HD void qd_softmax(const float* v, int n, float T, float* p, float* logp) {
    float s[kDqMaxAct];
    float mx = v[0] / T;
    for (int j = 0; j < n; ++j) {
        s[j] = v[j] / T;
        mx = (s[j] > mx) ? s[j] : mx;
    }
    float sum = 0.0f;
    for (int j = 0; j < n; ++j) {
        p[j] = op_exp(s[j] - mx);
        sum = sum + p[j];
    }
    const float lse = op_log(sum);
    for (int j = 0; j < n; ++j) {
        p[j] = p[j] / sum;
        logp[j] = (s[j] - mx) - lse;
    }
}

struct QdRow {
    float sq, kl, qa, y;             // the TD term, the distillation term, q[a], td_target
};
// One row: qo / qt the online Q values on obs and the target's on next_obs, tq the teacher's raw Q values; norm = 2 / M,
// ck = distill_coeff / T.  Writes dq[0..n).
MI355_HD QdRow qd_row(const float* qo, const float* qt, const float* tq, int n, int act, float rew, float done, float gamma, float T, float norm,
                      float ck, float* dq) {
    QdRow R;
    R.y = dq_td_target(rew, done, gamma, qt[dq_argmax(qt, n)]);
    R.qa = qo[act];
    const float d = op_mse_row(R.qa, R.y, norm, &R.sq);
    float pt[kDqMaxAct], lpt[kDqMaxAct], ps[kDqMaxAct], lps[kDqMaxAct];
    qd_softmax(tq, n, T, pt, lpt);
    qd_softmax(qo, n, T, ps, lps);
    float kl = 0.0f;
    for (int j = 0; j < n; ++j) {
        kl = kl + (-pt[j]) * (lps[j] - lpt[j]);
        dq[j] = (j == act ? d : 0.0f) + ck * (ps[j] - pt[j]);
    }
    R.kl = kl;
    return R;
}

// dh[k] of one row: every action's row of W, ascending action
MI355_HD float qd_dh(const float* dq, int n, const float* w, int k) {
    float acc = 0.0f;
    for (int j = 0; j < n; ++j) acc = op_mac(acc, dq[j], w[(int64_t)j * kQdH + k]);
    return acc;
}
// dW[j, k] (h != nullptr) or db[j] (h == nullptr): all rows, ascending; dqj = column j of dq with stride ds
MI355_HD float qd_wgrad(const float* dqj, int ds, int M, const float* h, int k) {
    float acc = 0.0f;
    for (int r = 0; r < M; ++r) acc = h ? op_mac(acc, dqj[(int64_t)r * ds], h[(int64_t)r * kQdH + k]) : acc + dqj[(int64_t)r * ds];
    return acc;
}

// the f64 slot fold's SUM on the host (wg_fold_mean's order without the division)
inline float qd_fold_sum_host(const float* v, int M) {
    double tot = 0.0;
    for (int t = 0; t < kOpFold; ++t) {
        double s = 0.0;
        for (int k = t; k < M; k += kOpFold) s += (double)v[k];
        tot += s;
    }
    return (float)tot;
}
MI355_HD float qd_loss(float q_loss, float coeff, float distill) { return q_loss + coeff * distill; }

}  // namespace mi355ppo
