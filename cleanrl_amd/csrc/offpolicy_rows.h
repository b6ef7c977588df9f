// Row / element math of the off-policy kernels (offpolicy.hip: ddpg_continuous_action.py, td3_continuous_action.py) and their host
// twins (host_twins.hip): one definition compiled for both sides, so a twin returns the device's bits.
//
// * Actor and QNetwork of the two scripts are the same shape of network: Linear(K, 256) - ReLU - Linear(256, 256) - ReLU - Linear(256, J),
//   K = obs (actor) or obs + act (critic, on cat(obs, action)), J = act or 1; parameters in .parameters() order.
// * Every dot product starts at 0.0f and adds its products in ascending index order through op_mac, then adds the bias.
// * A batch is cut into tiles of kOpRows rows; tile i belongs to group i % G, G = op_groups(M).  A group's weight-gradient partial
//   is the sum of its tiles' sums (rows ascending inside a tile, tiles ascending); the flat gradient adds the groups in ascending order.
// * op_tanh is built from +, *, / and exponent bits only, so that host and device agree bit for bit (libm's tanhf would not).
#pragma once
#include "common.h"

namespace mi355ppo {

constexpr int kOpH = 256;            // hidden width of Actor / QNetwork
constexpr int kOpMaxObs = 512;       // K7's limits
constexpr int kOpMaxAct = 20;
constexpr int kOpRows = 8;           // rows per tile (one workgroup pass)
constexpr int kOpMaxGroups = 64;     // weight-gradient partials per launch
constexpr int kOpFold = 256;         // slots of the f64 row folds (loss / q means)

MI355_HD float op_mac(float acc, float x, float w) { return acc + x * w; }

MI355_HD int64_t op_net_count(int K, int J) { return (int64_t)kOpH * K + kOpH + (int64_t)kOpH * kOpH + kOpH + (int64_t)J * kOpH + J; }
MI355_HD int64_t op_actor_count(int O, int A) { return op_net_count(O, A); }
MI355_HD int64_t op_critic_count(int O, int A) { return op_net_count(O + A, 1); }

struct OpNet {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int K, J;
};
MI355_HD OpNet op_net(const float* p, int K, int J) {
    OpNet n;
    n.K = K;
    n.J = J;
    n.w1 = p;
    n.b1 = n.w1 + (int64_t)kOpH * K;
    n.w2 = n.b1 + kOpH;
    n.b2 = n.w2 + kOpH * kOpH;
    n.w3 = n.b2 + kOpH;
    n.b3 = n.w3 + (int64_t)J * kOpH;
    return n;
}
// offsets of the six tensors inside a network's flat gradient
struct OpOff {
    int64_t w1, b1, w2, b2, w3, b3;
};
MI355_HD OpOff op_off(int K, int J) {
    OpOff o;
    o.w1 = 0;
    o.b1 = (int64_t)kOpH * K;
    o.w2 = o.b1 + kOpH;
    o.b2 = o.w2 + kOpH * kOpH;
    o.w3 = o.b2 + kOpH;
    o.b3 = o.w3 + (int64_t)J * kOpH;
    return o;
}

MI355_HD int op_tiles(int M) { return (M + kOpRows - 1) / kOpRows; }
MI355_HD int op_groups(int M) {
    const int t = op_tiles(M);
    return t < kOpMaxGroups ? t : kOpMaxGroups;
}
MI355_HD int64_t op_clamp(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

MI355_HD float op_relu(float v) { return (v < 0.0f) ? 0.0f : v; }                      // NaN passes, as torch's relu
MI355_HD float op_relu_bwd(float out, float g) { return (out <= 0.0f) ? 0.0f : g; }    // threshold_backward
MI355_HD float op_clamp_f(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }   // NaN passes
MI355_HD float op_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }  // torch.min: NaN wins

// tanh from basic operations: |x| < 0.25 the odd series to x^11 (next term < 2e-10 relative); otherwise 1 - 2 / (e^{2|x|} + 1) with
// e^y = 2^n * P7(y - n ln 2).  Within 3e-7 of tanh; the backward uses 1 - t * t of the same t, as torch does.
MI355_HD float op_tanh(float x) {
    if (x != x) return x;
    const float t = x < 0.0f ? -x : x;
    float r;
    if (t < 0.25f) {
        const float s = t * t;
        float p = -1382.0f / 155925.0f;
        p = p * s + 62.0f / 2835.0f;
        p = p * s + -17.0f / 315.0f;
        p = p * s + 2.0f / 15.0f;
        p = p * s + -1.0f / 3.0f;
        p = p * s + 1.0f;
        r = t * p;
    } else if (t > 10.0f) {
        r = 1.0f;
    } else {
        const float y = t + t;
        const int n = (int)(y * 1.44269504f + 0.5f);
        const float fn = (float)n;
        float z = y - fn * 0.693145752f;            // ln 2 high part (exact product for n < 2^11)
        z = z - fn * 1.42860677e-06f;               // ln 2 low part
        float p = 1.0f / 5040.0f;
        p = p * z + 1.0f / 720.0f;
        p = p * z + 1.0f / 120.0f;
        p = p * z + 1.0f / 24.0f;
        p = p * z + 1.0f / 6.0f;
        p = p * z + 0.5f;
        p = p * z + 1.0f;
        p = p * z + 1.0f;
        const float e = p * __builtin_bit_cast(float, (uint32_t)(n + 127) << 23);
        r = 1.0f - 2.0f / (e + 1.0f);
    }
    return x < 0.0f ? -r : r;
}

// Actor.forward's last line on one element: tanh(mu) * action_scale + action_bias
MI355_HD float op_action(float t, float scale, float bias) { return t * scale + bias; }
// the rollout's `actions += normal(0, scale * exploration_noise)` and numpy's clip(low, high)
MI355_HD float op_explore(float a, float noise, float lo, float hi) { return op_clamp_f(a + noise, lo, hi); }
// TD3's target policy smoothing: (noise * policy_noise).clamp(-c, c) * action_scale, added, clamped to [low[0], high[0]]
MI355_HD float op_smooth(float a, float noise, float pn, float nc, float scale, float lo0, float hi0) {
    const float cn = op_clamp_f(noise * pn, -nc, nc) * scale;
    return op_clamp_f(a + cn, lo0, hi0);
}
// rewards + (1 - dones) * gamma * q, left to right
MI355_HD float op_td_target(float r, float d, float gamma, float q) { return r + ((1.0f - d) * gamma) * q; }
// F.mse_loss(q, y): the row's squared error and d loss / d q = (2 / M) * (q - y)
MI355_HD float op_mse_row(float q, float y, float norm, float* sq) {
    const float d = q - y;
    *sq = d * d;
    return norm * d;
}
// the actor's gradient at tanh's input: d(-mean q) / d action, through `* action_scale` and tanh
MI355_HD float op_dmu(float dact, float scale, float t) { return (dact * scale) * (1.0f - t * t); }
// args.tau * param + (1 - args.tau) * target_param
MI355_HD float op_polyak(float p, float t, float tau, float omt) { return tau * p + omt * t; }

// wg_fold_mean (offpolicy_wg.h) on the host, in its order: kOpFold f64 slots, then the slots in order
inline float op_fold_mean_host(const float* v, int M) {
    double tot = 0.0;
    for (int t = 0; t < kOpFold; ++t) {
        double s = 0.0;
        for (int k = t; k < M; k += kOpFold) s += (double)v[k];
        tot += s;
    }
    return (float)(tot / (double)M);
}

// host-side argument check of the device entry points and of their twins
inline int op_shape(const char* fn, int M, int O, int A) {
    MI355_REQUIRE(M > 0 && O > 0 && O <= kOpMaxObs && A > 0 && A <= kOpMaxAct, MI355PPO_EINVAL,
                  "%s: rows=%d obs_dim=%d act_dim=%d: the off-policy networks take 1 <= obs_dim <= %d, 1 <= act_dim <= %d", fn, M, O, A,
                  kOpMaxObs, kOpMaxAct);
    return MI355PPO_OK;
}

}  // namespace mi355ppo
