// Row math of the recurrent PQN tail (pqn_lstm.hip) and its host twins (host_twins.hip): one definition compiled for both sides.
// Reference: cleanrl/pqn_atari_envpool_lstm.py -- QNetwork.get_states (one nn.LSTM(512, 128) step with the done reset; the cell
// is lstm_cell_fwd of lstm_rows.h, shared with the sequence scans), q_func = Linear(128, A), and the TD loss of a minibatch.
//
// * pqn_lstm_q        q[a] = dot(wq[a, :], h) + bq[a]: lstm_dot128's four interleaved fmaf chains, then the bias.  The act kernel and
//                     the TD kernel both form q through it, so old[r] of a minibatch row equals the q the rollout would compute.
// * pqn_lstm_td_row   gather + mse_loss of one row and its gradient at old: (a, old, (ret - old)^2, g = -((2 / M) (ret - old))).
// * the weight gradient of q_func is summed over rows in ascending order, per workgroup of kPqnRows rows, then over workgroups:
//   dwq[a, k] = sum_{r: a_r = a} g_r h[r, k] (rows of another action are skipped, so an action that never occurs keeps exact
//   zeros), dbq[a] = sum_{r: a_r = a} g_r.
#pragma once
#include "lstm_rows.h"
#include "pqn_rows.h"

namespace mi355ppo {

template <class W, class V>
MI355_HD float pqn_lstm_q(const W& w, const V& h, float b) {
    return lstm_dot128(w, h) + b;
}

struct PqnLstmTd {
    int a;
    float old, sq, g;
};

// h: the row's 128 hidden units; wq (A, 128), bq (A).  `.long()` truncates the stored action; one outside [0, A) is clamped.
MI355_HD PqnLstmTd pqn_lstm_td_row(const float* h, const float* wq, const float* bq, int A, float action_f, float ret, float norm) {
    PqnLstmTd t;
    int a = (int)(int64_t)action_f;
    t.a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    t.old = pqn_lstm_q(wq + (size_t)t.a * kLstmH, h, bq[t.a]);
    const float d = ret - t.old;
    t.sq = d * d;
    t.g = -(norm * d);
    return t;
}

// Element e of one workgroup's partial of (dwq | dbq) (A * 128 + A floats) over rows [r0, r1): g / act are indexed by row - r0.
MI355_HD float pqn_lstm_grad_partial(int e, const float* h, const float* g, const int* act, int r0, int r1) {
    const int AH_a = e / kLstmH, k = e % kLstmH;
    float acc = 0.0f;
    for (int r = r0; r < r1; ++r)
        if (act[r - r0] == AH_a) acc = acc + g[r - r0] * h[(size_t)r * kLstmH + k];
    return acc;
}

MI355_HD float pqn_lstm_bias_partial(int a, const float* g, const int* act, int rows) {
    float acc = 0.0f;
    for (int r = 0; r < rows; ++r)
        if (act[r] == a) acc = acc + g[r];
    return acc;
}

MI355_HD int64_t pqn_lstm_mp(int M) { return ((int64_t)M + 63) / 64 * 64; }

}  // namespace mi355ppo
