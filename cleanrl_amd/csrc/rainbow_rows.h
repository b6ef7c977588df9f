// Row / element math of the Rainbow kernels (rainbow.hip: rainbow_atari.py's PrioritizedReplayBuffer and NoisyLinear) and their host
// twins (rainbow_twins.hip): one definition compiled for both sides.  The frame words (da_pack, da_frame) and the host gather are
// dqn_atari_rows.h's, the projection (c51_proj_elem with l_eq_b) and the categorical row dqn_rows.h's.
//
// * Two u8 frame rings (slots, 84, 84, 4), channels-last: obs and next_obs of the n-step transition, no aliasing between them.
// * The sum tree is the reference's heap of 2 * slots - 1 f32 words: node p has the children 2p + 1 and 2p + 2, leaf i is node
//   slots - 1 + i.  When slots is not a power of two the leaves lie at two depths (rb_depth).  An inner node is ALWAYS the f32 sum
//   tree[2p + 1] + tree[2p + 2] of its children's current values, which is what the reference's serial _propagate leaves behind.
// * x ** y of NumPy's float32 scalars and arrays against a Python float is powf(x, (float)y).  Here it is pow((double)x,
//   (double)(float)y) rounded once to f32 (rb_pow): at most 1 ulp from either side's powf, and the same expression on host and device.
// * The walk of SumSegmentTree.retrieve runs in f32 from its first step: NumPy compares and subtracts a Python float against an
//   np.float32 in float32, so `value` is rounded to f32 before its first use (rb_retrieve).
// * state (2 f32 words in device memory): {max_priority, beta}; size is one int64 word.
#pragma once
#include <math.h>

#include "dqn_atari_rows.h"

namespace mi355ppo {

constexpr int kRbMaxBatch = 1024;    // rows of a sample / an update
constexpr int kRbFcIn = 3136;        // the trunk's features
constexpr int kRbHid = 512;          // hidden width of each stream
constexpr int kRbSegs = 8;           // {W, b} x {value, advantage} x {hidden layer, output layer}

MI355_HD float rb_pow(float x, float y) { return (float)pow((double)x, (double)y); }

MI355_HD int rb_depth(int64_t node) { return 63 - __builtin_clzll((unsigned long long)(node + 1)); }
MI355_HD int64_t rb_leaf(int64_t i, int64_t slots) { return slots - 1 + i; }

// tree[parent] from its children, from `node` up to the root (SumSegmentTree._propagate)
MI355_HD void rb_propagate(float* tree, int64_t node) {
    while (node > 0) {
        node = (node - 1) / 2;
        tree[node] = tree[2 * node + 1] + tree[2 * node + 2];
    }
}

// np.random.uniform(a, b) on the draw u of sample i out of B, a = segment * i, b = segment * (i + 1), segment = total / B in f32
MI355_HD double rb_stratum(float total, int B, int i, double u) {
    const float segment = total / (float)B;
    const float a = segment * (float)i, b = segment * (float)(i + 1);
    return (double)a + ((double)b - (double)a) * u;
}

// SumSegmentTree.retrieve -> the leaf's slot
MI355_HD int64_t rb_retrieve(const float* tree, int64_t slots, double value) {
    const int64_t words = 2 * slots - 1;
    float v = (float)value;
    int64_t idx = 0;
    while (2 * idx + 1 < words) {
        const int64_t left = 2 * idx + 1;
        const float tl = tree[left];
        if (v <= tl) {
            idx = left;
        } else {
            v = v - tl;
            idx = left + 1;
        }
    }
    return idx - (slots - 1);
}

// (size * p / p_total) ** -beta, before the division by the batch's maximum
MI355_HD float rb_weight(float size, float p, float total, float beta) { return rb_pow((size * p) / total, -beta); }
// numpy's max: a NaN wins
MI355_HD float rb_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }
// abs(loss) + eps
MI355_HD float rb_priority(float loss, float eps) { return (loss < 0.0f ? -loss : loss) + eps; }
// Python's max(max_priority, priorities.max()): the first argument stays unless the second is greater
MI355_HD float rb_running_max(float maxp, float pm) { return pm > maxp ? pm : maxp; }

MI355_HD bool rb_noisy_limits(int n, int na) { return n >= 2 && n <= kDqMaxAct && na >= 2 && na <= kDqMaxAtoms && (n + 1) * na <= kDaMaxOut; }

// The four NoisyLinear layers of a network, cut into 8 segments.  eff: the effective buffer W_fc (1024, 3136) | b_fc (1024) |
// W_out ((n + 1) * n_atoms, 512) | b_out, the value stream's rows first.  par: the head's parameters in torch's registration order,
// per layer weight_mu, weight_sigma, bias_mu, bias_sigma; layers value_head.0, value_head.2, advantage_head.0, advantage_head.2 (the
// gradient has the same layout).  eps: per layer weight_epsilon, bias_epsilon, in reset_noise()'s order.
struct RbSegs {
    int64_t eff[kRbSegs], mu[kRbSegs], sigma[kRbSegs], eps[kRbSegs], cnt[kRbSegs], total, params;
};
MI355_HD RbSegs rb_segs(int n, int na) {
    RbSegs s;
    const int64_t out[4] = {kRbHid, na, kRbHid, (int64_t)n * na};            // value.0, value.2, advantage.0, advantage.2
    const int64_t in[4] = {kRbFcIn, kRbHid, kRbFcIn, kRbHid};
    int64_t par = 0, eps = 0;
    for (int l = 0; l < 4; ++l) {
        const int64_t W = out[l] * in[l], b = out[l];
        const int ws = 2 * l, bs = 2 * l + 1;                                 // segment 2l: layer l's weight, 2l + 1: its bias
        s.mu[ws] = par, s.sigma[ws] = par + W, s.mu[bs] = par + 2 * W, s.sigma[bs] = par + 2 * W + b;
        s.eps[ws] = eps, s.eps[bs] = eps + W;
        s.cnt[ws] = W, s.cnt[bs] = b;
        par += 2 * W + 2 * b;
        eps += W + b;
    }
    const int order[kRbSegs] = {0, 4, 1, 5, 2, 6, 3, 7};                      // W_fc v | a, b_fc v | a, W_out v | a, b_out v | a
    int64_t e = 0;
    for (int k = 0; k < kRbSegs; ++k) {
        s.eff[order[k]] = e;
        e += s.cnt[order[k]];
    }
    s.total = e;
    s.params = par;
    return s;
}
// the segment that holds element e of the parameter-ordered walk 0 .. total (segment k starts at eps[k]: eps is dense in that order)
MI355_HD int rb_seg_of(const RbSegs& s, int64_t e) {
    int k = 0;
    while (k + 1 < kRbSegs && e >= s.eps[k + 1]) ++k;
    return k;
}
MI355_HD float rb_compose(float mu, float sigma, float eps) { return mu + sigma * eps; }

// ------------------------------------------------------------------------------------------------ the dueling distributional head
// h (rows, 1024): the post-ReLU output of the ONE Linear(3136, 1024) that holds both streams' hidden layers, the value stream's 512
// columns first.  W_out ((n + 1) * n_atoms, 512): the value stream's n_atoms rows read h[:, :512], the advantage rows h[:, 512:].
// z (J = (n + 1) * n_atoms): a row's outputs, value atoms first, then action-major advantage atoms.
constexpr int kRbH2 = 2 * kRbHid;
MI355_HD int rb_col0(int j, int na) { return j < na ? 0 : kRbHid; }                      // the first column of h that output j reads
MI355_HD float rb_head_dot(const float* hrow, const float* w, const float* b, int j, int na) {
    return da_dot(hrow + rb_col0(j, na), w + (int64_t)j * kRbHid, b[j]);
}
// the dueling combine of atom k, in place: adv[a, k] <- (v[k] + adv[a, k]) - mean_a adv[a, k]; the mean is the ascending sum / n
MI355_HD void rb_combine_col(float* z, int n, int na, int k) {
    float s = 0.0f;
    for (int a = 0; a < n; ++a) s = s + z[na + a * na + k];
    const float mean = s / (float)n;
    for (int a = 0; a < n; ++a) z[na + a * na + k] = (z[k] + z[na + a * na + k]) - mean;
}
// d loss / d (advantage logit of action a, atom k): the taken action carries dq, every action -dq / n (the mean's backward)
MI355_HD float rb_dz_adv(const float* dq, const float* dqn, int a, int act, int k) { return ((a == act) ? dq[k] : 0.0f) - dqn[k]; }
// dh[c] of one row: columns < 512 from the value rows, the others from the advantage rows, ascending output
MI355_HD float rb_dh(const float* dq, const float* dqn, int n, int na, int act, const float* w, int c) {
    float acc = 0.0f;
    if (c < kRbHid) {
        for (int k = 0; k < na; ++k) acc = op_mac(acc, dq[k], w[(int64_t)k * kRbHid + c]);
    } else {
        for (int a = 0; a < n; ++a)
            for (int k = 0; k < na; ++k) acc = op_mac(acc, rb_dz_adv(dq, dqn, a, act, k), w[(int64_t)(na + a * na + k) * kRbHid + c - kRbHid]);
    }
    return acc;
}
// dW_out[j, c] (h != nullptr) or db_out[j] (h == nullptr): over the batch rows, ascending; dz (M, J)
MI355_HD float rb_wgrad(const float* dz, int M, int J, int j, int na, const float* h, int c) {
    float acc = 0.0f;
    for (int r = 0; r < M; ++r) acc = h ? op_mac(acc, dz[(int64_t)r * J + j], h[(int64_t)r * kRbH2 + rb_col0(j, na) + c]) : acc + dz[(int64_t)r * J + j];
    return acc;
}
MI355_HD bool rb_head_limits(int M, int n, int na) { return M >= 1 && M <= kDaMaxRows && rb_noisy_limits(n, na); }
inline int rb_head_shape(const char* fn, int M, int n, int na) {
    MI355_REQUIRE(rb_head_limits(M, n, na), MI355PPO_EINVAL,
                  "%s: rows=%d n_actions=%d n_atoms=%d: the dueling head takes 1 <= rows <= %d, 2 <= n_actions <= %d, 2 <= n_atoms <= %d, "
                  "(n_actions + 1) * n_atoms <= %d", fn, M, n, na, kDaMaxRows, kDqMaxAct, kDqMaxAtoms, kDaMaxOut);
    return MI355PPO_OK;
}

// host-side argument checks of the entry points and of their twins
inline int rb_ring_shape(const char* fn, int64_t slots) {
    MI355_REQUIRE(slots > 0 && slots <= ((int64_t)1 << 40), MI355PPO_EINVAL, "%s: slots=%lld: 1 <= slots <= 2^40", fn, (long long)slots);
    return MI355PPO_OK;
}
inline int rb_batch_shape(const char* fn, int B) {
    MI355_REQUIRE(B >= 1 && B <= kRbMaxBatch, MI355PPO_EINVAL, "%s: rows=%d: 1 <= rows <= %d", fn, B, kRbMaxBatch);
    return MI355PPO_OK;
}
inline int rb_noisy_shape(const char* fn, int n, int na) {
    MI355_REQUIRE(rb_noisy_limits(n, na), MI355PPO_EINVAL,
                  "%s: n_actions=%d n_atoms=%d: the noisy dueling head takes 2 <= n_actions <= %d, 2 <= n_atoms <= %d, "
                  "(n_actions + 1) * n_atoms <= %d", fn, n, na, kDqMaxAct, kDqMaxAtoms, kDaMaxOut);
    return MI355PPO_OK;
}

}  // namespace mi355ppo
