// Row / element math of the SAC kernels (sac.hip: sac_continuous_action.py) and their host twins (host_twins.hip): one definition
// compiled for both sides, so a twin returns the device's bits.  The networks' dot products, the tile and group rules, op_tanh, op_min
// and op_td_target are offpolicy_rows.h's.
//
// * Actor is Linear(O, 256) - ReLU - Linear(256, 256) - ReLU and two heads Linear(256, A): fc_mean and fc_logstd.  .parameters() order
//   is fc1.w, fc1.b, fc2.w, fc2.b, fc_mean.w, fc_mean.b, fc_logstd.w, fc_logstd.b: fc_mean's bias sits between the two head matrices,
//   so the heads are two J = A heads, not one J = 2A head.
// * op_exp / op_log are built from +, *, / and exponent bits only, as op_tanh is (libm's expf / logf differ between host and device).
// * sac_elem is Actor.forward's tail and get_action on one (row, action) element in the reference's operation order; sac_elem_bwd is
//   the hand-derived backward of alpha * log_pi - min(q1, q2) through it.
#pragma once
#include "offpolicy_rows.h"

namespace mi355ppo {

// e^x = 2^n * P7(x - n ln 2), n = round(x / ln 2): |z| <= 0.347, the next Taylor term is below 6e-9 relative.  0 below -87, +inf
// above 88; NaN passes.
MI355_HD float op_exp(float x) {
    if (x != x) return x;
    if (x < -87.0f) return 0.0f;
    if (x > 88.0f) return __builtin_bit_cast(float, (uint32_t)0x7f800000u);
    const int n = (int)(x * 1.44269504f + (x < 0.0f ? -0.5f : 0.5f));
    const float fn = (float)n;
    float z = x - fn * 0.693145752f;            // ln 2 high part (exact product for |n| < 2^9)
    z = z - fn * 1.42860677e-06f;               // ln 2 low part
    float p = 1.0f / 5040.0f;
    p = p * z + 1.0f / 720.0f;
    p = p * z + 1.0f / 120.0f;
    p = p * z + 1.0f / 24.0f;
    p = p * z + 1.0f / 6.0f;
    p = p * z + 0.5f;
    p = p * z + 1.0f;
    p = p * z + 1.0f;
    return p * __builtin_bit_cast(float, (uint32_t)(n + 127) << 23);
}

// log v = e ln 2 + 2 atanh(s), v = m 2^e with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1): |s| <= 0.172, the series runs to
// s^9 / 9 (the next term is below 3e-9 relative).  Normal positive v; NaN passes, v < 0 gives NaN, v below the normal range -inf,
// +inf passes.
MI355_HD float op_log(float v) {
    if (v != v) return v;
    if (v < 0.0f) return __builtin_bit_cast(float, (uint32_t)0x7fc00000u);
    if (v < 1.17549435e-38f) return __builtin_bit_cast(float, (uint32_t)0xff800000u);
    const uint32_t bits = __builtin_bit_cast(uint32_t, v);
    if (bits >= 0x7f800000u) return v;
    int e = (int)(bits >> 23) - 127;
    float m = __builtin_bit_cast(float, (bits & 0x007fffffu) | 0x3f800000u);      // [1, 2)
    if (m > 1.41421354f) {
        m = m * 0.5f;
        e = e + 1;
    }
    const float f = m - 1.0f;                   // exact
    const float s = f / (2.0f + f);
    const float q = s * s;
    float p = 1.0f / 9.0f;
    p = p * q + 1.0f / 7.0f;
    p = p * q + 1.0f / 5.0f;
    p = p * q + 1.0f / 3.0f;
    p = p * q + 1.0f;
    const float fe = (float)e;
    const float lo = fe * 1.42860677e-06f + (s + s) * p;
    return fe * 0.693145752f + lo;              // exact product for |e| < 2^9
}

// ---- the actor's layout
MI355_HD int64_t sac_actor_count(int O, int A) { return op_net_count(O, A) + (int64_t)A * kOpH + A; }

struct SacNet {
    const float *w1, *b1, *w2, *b2, *wm, *bm, *ws, *bs;
    int K, A;
};
MI355_HD SacNet sac_net(const float* p, int O, int A) {
    SacNet n;
    n.K = O;
    n.A = A;
    n.w1 = p;
    n.b1 = n.w1 + (int64_t)kOpH * O;
    n.w2 = n.b1 + kOpH;
    n.b2 = n.w2 + kOpH * kOpH;
    n.wm = n.b2 + kOpH;
    n.bm = n.wm + (int64_t)A * kOpH;
    n.ws = n.bm + A;
    n.bs = n.ws + (int64_t)A * kOpH;
    return n;
}
// offsets of the eight tensors inside the actor's flat gradient
struct SacOff {
    int64_t w1, b1, w2, b2, wm, bm, ws, bs;
};
MI355_HD SacOff sac_off(int O, int A) {
    SacOff o;
    o.w1 = 0;
    o.b1 = (int64_t)kOpH * O;
    o.w2 = o.b1 + kOpH;
    o.b2 = o.w2 + kOpH * kOpH;
    o.wm = o.b2 + kOpH;
    o.bm = o.wm + (int64_t)A * kOpH;
    o.ws = o.bm + A;
    o.bs = o.ws + (int64_t)A * kOpH;
    return o;
}

// ---- get_action on one element
struct SacElem {
    float y;          // tanh(x_t)
    float action;     // y * action_scale + action_bias
    float std;        // exp(log_std)
    float th;         // tanh(u), u = fc_logstd's output
    float arg;        // action_scale * (1 - y^2) + 1e-6
    float lp;         // this element's term of log_prob
};
#define SAC_LOG_SQRT_2PI 0.91893853320467274178f     /* math.log(math.sqrt(2 * math.pi)) */

MI355_HD SacElem sac_elem(float mean, float u, float eps, float scale, float bias) {
    SacElem e;
    e.th = op_tanh(u);
    const float log_std = -5.0f + 3.5f * (e.th + 1.0f);        // LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (log_std + 1)
    e.std = op_exp(log_std);
    const float x = mean + e.std * eps;                        // normal.rsample()
    e.y = op_tanh(x);
    e.action = e.y * scale + bias;
    const float d = x - mean;
    const float var = e.std * e.std;
    float lp = (-(d * d)) / (2.0f * var) - log_std - SAC_LOG_SQRT_2PI;     // Normal.log_prob
    e.arg = scale * (1.0f - e.y * e.y) + 1e-6f;
    lp = lp - op_log(e.arg);                                   // the action bound
    e.lp = lp;
    return e;
}

// torch.min(a, b)'s backward: the weight a's gradient gets -- 1 to the smaller, 0.5 to each on a tie
MI355_HD float sac_min_w(float a, float b) { return (a < b) ? 1.0f : ((a == b) ? 0.5f : 0.0f); }

// (alpha * log_pi) - min_qf_pi of one row
MI355_HD float sac_actor_row(float alpha, float lp, float q1, float q2) { return alpha * lp - op_min(q1, q2); }
// torch.min(qf1_next_target, qf2_next_target) - alpha * next_state_log_pi
MI355_HD float sac_soft_q(float q1, float q2, float alpha, float lp) { return op_min(q1, q2) - alpha * lp; }

// d loss / d mean and d loss / d u of one element.  dact = d loss / d action (from the critics), glp = d loss / d log_pi of the row.
//   y      gets dact * scale and glp * 2 scale y / arg (the -log(scale (1 - y^2) + 1e-6) term);
//   x      gets that times 1 - y^2; Normal.log_prob's (x - mean)^2 term reaches mean and std only through x - mean = std * eps, where
//          its two contributions cancel (d/dx + d/dmean = 0; through std: -eps^2 / std + eps^2 / std = 0), so it is left out;
//   mean   gets dx;  log_std gets dx * std * eps (dx / dlog_std = std * eps) and -glp (the -log_std term);
//   u      gets that times 3.5 * (1 - tanh(u)^2).
MI355_HD void sac_elem_bwd(const SacElem& e, float eps, float scale, float dact, float glp, float* dmean, float* du) {
    const float dy = dact * scale + glp * (((2.0f * scale) * e.y) / e.arg);
    const float dx = dy * (1.0f - e.y * e.y);
    const float dls = dx * (e.std * eps) - glp;
    *dmean = dx;
    *du = dls * (3.5f * (1.0f - e.th * e.th));
}

// the entropy coefficient's loss and gradient given mean(log_pi + target_entropy) (f64 fold): both are -exp(log_alpha) * that mean
MI355_HD float sac_alpha_loss(float alpha_now, double mean_lp_te) { return (float)(-((double)alpha_now * mean_lp_te)); }

}  // namespace mi355ppo
