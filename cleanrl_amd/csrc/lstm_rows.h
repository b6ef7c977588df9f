// Row / element math of the done-masked LSTM sequence kernels (lstm.hip) and of their host-pointer twins (host_twins.hip):
// one definition, compiled for both sides without FMA contraction, so the twins run the device kernels' own arithmetic.
//
// The recurrence is one layer of nn.LSTM(512, 128) with the reference's done reset (cleanrl/ppo_atari_lstm.py:140-158);
// gate order i, f, g, o (PyTorch's).  For t = 0 .. T-1, with (h_{-1}, c_{-1}) = (h0, c0):
//   keep_t = 1 - done[t]                        (a multiply, never a branch: a non-binary done scales the state)
//   hk_t = keep_t * h_{t-1},  ck_t = keep_t * c_{t-1}
//   a_t = gx[t] + W_hh hk_t                     (gx = x W_ih^T + b_ih + b_hh, formed outside the scan)
//   i, f, o = sigmoid(a_i, a_f, a_o),  g = tanh(a_g),  c_t = f ck_t + i g,  h_t = o tanh(c_t)
//
// Activation record (the forward writes it when asked, the backward reads it), 7 H floats per (t, b) in four planes:
//   [0,           T B 4H)  post-activation gates (T, B, 4, H): i, f, g, o
//   [T B 4H,      T B 5H)  c_t  (T, B, H)
//   [T B 5H,      T B 6H)  hk_t (T, B, H)   -- the masked previous hidden state the step multiplied by W_hh (dW_hh = dgx^T hk)
//   [T B 6H,      T B 7H)  ck_t (T, B, H)
#pragma once
#include "common.h"
#include <math.h>
#include <stddef.h>

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kLstmH = 128;               // hidden size: nn.LSTM(512, 128) of ppo_atari_lstm.py
constexpr int kLstmG = 4 * kLstmH;        // gate rows
constexpr int kLstmRec = 7 * kLstmH;      // record floats per (t, b)

inline size_t lstm_record_floats(int T, int B) { return (size_t)T * (size_t)B * kLstmRec; }

// Launch shape of the scans and of the kernels that walk the same chain (pqn_lstm.hip): workgroups of kLstmThreads threads own
// E envs each, E in {1, 2, 4, 8} the smallest that keeps ceil(B / E) workgroups within one per CU.  Thread tid owns the unit
// pairs (env e, unit u) p = tid + kLstmThreads r, e = p / kLstmH, u = p % kLstmH, r < kLstmPairs<E>.
constexpr int kLstmThreads = 512;
constexpr int kLstmCus = 256;

inline int lstm_envs_per_group(int B) {
    for (int e = 1; e < 8; e *= 2)
        if ((B + e - 1) / e <= kLstmCus) return e;
    return 8;
}

template <int E>
constexpr int kLstmPairs = (E * kLstmH + kLstmThreads - 1) / kLstmThreads;

// sum_k w[k] v[k] over the 128 columns: four interleaved fused multiply-add chains, folded (s0 + s1) + (s2 + s3).  The
// order is fixed, so a device thread (w in registers, v broadcast from LDS) and the host twin produce the same bits.
template <class W, class V>
MI355_HD float lstm_dot128(const W& w, const V& v) {
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
#pragma unroll
    for (int k = 0; k < kLstmH; k += 4) {
        s0 = fmaf(w[k + 0], v[k + 0], s0);
        s1 = fmaf(w[k + 1], v[k + 1], s1);
        s2 = fmaf(w[k + 2], v[k + 2], s2);
        s3 = fmaf(w[k + 3], v[k + 3], s3);
    }
    return (s0 + s1) + (s2 + s3);
}

// The backward's W_hh^T dgx is computed as four partial sums over the four gate blocks of 128 rows, folded in block order.
MI355_HD float lstm_fold4(float p0, float p1, float p2, float p3) { return ((p0 + p1) + p2) + p3; }

MI355_HD float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One cell: pre-activations (ai, af, ag, ao) and the masked previous cell state -> gates, c_t, h_t.
struct LstmCell {
    float i, f, g, o, c, h;
};

MI355_HD LstmCell lstm_cell_fwd(float ai, float af, float ag, float ao, float ck) {
    LstmCell s;
    s.i = lstm_sigmoid(ai);
    s.f = lstm_sigmoid(af);
    s.g = tanhf(ag);
    s.o = lstm_sigmoid(ao);
    s.c = s.f * ck + s.i * s.g;
    s.h = s.o * tanhf(s.c);
    return s;
}

// Its backward: dh / dc flowing into (h_t, c_t) -> the pre-activation gate gradients and d ck_t.
struct LstmCellGrad {
    float dai, daf, dag, dao, dck;
};

MI355_HD LstmCellGrad lstm_cell_bwd(float i, float f, float g, float o, float c, float ck, float dh, float dc_in) {
    LstmCellGrad d;
    const float tc = tanhf(c);
    const float dc = dc_in + (dh * o) * (1.0f - tc * tc);
    d.dai = (dc * g) * (i * (1.0f - i));
    d.daf = (dc * ck) * (f * (1.0f - f));
    d.dag = (dc * i) * (1.0f - g * g);
    d.dao = (dh * tc) * (o * (1.0f - o));
    d.dck = dc * f;
    return d;
}

}  // namespace mi355ppo
