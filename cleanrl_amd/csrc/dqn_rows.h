// Row / element math of the DQN / C51 kernels (dqn.hip: dqn.py, c51.py) and their host twins (host_twins.hip): one definition
// compiled for both sides, so a twin returns the device's bits.  Tiles, groups, op_mac, op_relu, op_clamp and op_mse_row are
// offpolicy_rows.h's; op_exp / op_log are sac_rows.h's.  The projection, the loss elements and c51_row_host also serve the Atari heads
// and Rainbow's (dqn_atari.hip, rainbow.hip and their twins).
//
// * QNetwork of both scripts is Linear(O, 120) - ReLU - Linear(120, 84) - ReLU - Linear(84, J), J = n (dqn.py) or n * n_atoms
//   (c51.py, viewed as (n, n_atoms)); parameters in .parameters() order.
// * Every dot product starts at 0.0f and adds its products in ascending index order through op_mac, then adds the bias.
// * The softmax of one action's atoms: exp(z - max) through op_exp, the sum and (pmfs * atoms).sum in ascending atom order.
// * The categorical projection adds in the order of the reference's two index_add_ calls per row: target atom k starts at 0 and
//   receives every d_m_l[j] with l[j] == k for ascending j, then every d_m_u[j] with u[j] == k for ascending j.
#pragma once
#include "sac_rows.h"

namespace mi355ppo {

constexpr int kDqH1 = 120;           // hidden widths of QNetwork
constexpr int kDqH2 = 84;
constexpr int kDqMaxObs = 512;       // limits of the fused path
constexpr int kDqMaxAct = 18;
constexpr int kDqMaxAtoms = 101;
constexpr int kDqMaxOut = 512;       // n * n_atoms

MI355_HD bool dq_limits(int O, int n, int na) {
    return O >= 1 && O <= kDqMaxObs && n >= 2 && n <= kDqMaxAct && na >= 1 && na <= kDqMaxAtoms && n * na <= kDqMaxOut;
}
// host-side argument check of the device entry points and of their twins
inline int dq_shape(const char* fn, int M, int O, int n, int na) {
    MI355_REQUIRE(M > 0 && dq_limits(O, n, na), MI355PPO_EINVAL,
                  "%s: rows=%d obs_dim=%d n_actions=%d n_atoms=%d: the fused Q networks take 1 <= obs_dim <= %d, 2 <= n_actions <= %d, "
                  "1 <= n_atoms <= %d, n_actions * n_atoms <= %d", fn, M, O, n, na, kDqMaxObs, kDqMaxAct, kDqMaxAtoms, kDqMaxOut);
    return MI355PPO_OK;
}
MI355_HD int64_t dq_count(int O, int J) { return (int64_t)kDqH1 * O + kDqH1 + kDqH2 * kDqH1 + kDqH2 + (int64_t)J * kDqH2 + J; }

struct DqNet {
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    int O, J;
};
MI355_HD DqNet dq_net(const float* p, int O, int J) {
    DqNet n;
    n.O = O;
    n.J = J;
    n.w1 = p;
    n.b1 = n.w1 + (int64_t)kDqH1 * O;
    n.w2 = n.b1 + kDqH1;
    n.b2 = n.w2 + kDqH2 * kDqH1;
    n.w3 = n.b2 + kDqH2;
    n.b3 = n.w3 + (int64_t)J * kDqH2;
    return n;
}
// offsets of the six tensors inside the flat gradient
struct DqOff {
    int64_t w1, b1, w2, b2, w3, b3;
};
MI355_HD DqOff dq_off(int O, int J) {
    DqOff o;
    o.w1 = 0;
    o.b1 = (int64_t)kDqH1 * O;
    o.w2 = o.b1 + kDqH1;
    o.b2 = o.w2 + kDqH2 * kDqH1;
    o.w3 = o.b2 + kDqH2;
    o.b3 = o.w3 + (int64_t)J * kDqH2;
    return o;
}

// torch.argmax(v): the lowest index of the maximum; a NaN is the maximum (the first one wins)
MI355_HD int dq_argmax(const float* v, int n) {
    int best = 0;
    for (int a = 1; a < n; ++a) {
        const float x = v[a], b = v[best];
        if ((b == b) && (x > b || x != x)) best = a;
    }
    return best;
}
// the ring's action (an index stored as f32: exact for n <= 18) back as an index inside [0, n)
MI355_HD int dq_action_index(float a, int n) {
    if (!(a >= 0.0f)) return 0;
    if (a >= (float)n) return n - 1;
    return (int)a;
}
// data.rewards.flatten() + args.gamma * target_max * (1 - data.dones.flatten()), left to right
MI355_HD float dq_td_target(float r, float d, float gamma, float mx) { return r + (gamma * mx) * (1.0f - d); }

// torch.softmax over one action's n_atoms logits into p (p may be z) -> (pmfs * atoms).sum()
MI355_HD float dq_softmax_q(const float* z, int na, const float* atoms, float* p) {
    float mx = z[0];
    for (int k = 1; k < na; ++k) mx = (z[k] > mx) ? z[k] : mx;
    float s = 0.0f;
    for (int k = 0; k < na; ++k) {
        const float e = op_exp(z[k] - mx);
        p[k] = e;
        s = s + e;
    }
    float q = 0.0f;
    for (int k = 0; k < na; ++k) {
        const float pk = p[k] / s;
        p[k] = pk;
        q = q + pk * atoms[k];
    }
    return q;
}

// c51.py's projection on one (row, atom j): next_atoms, tz, b, l, u, d_m_l, d_m_u.  l_eq_b: rainbow_atari.py's own (l == b) in place
// of c51.py's (l == u); the two differ where b rounds to just above n_atoms - 1 (l == u after the clamp, l != b), and gamma is its
// gamma ** n_step.
struct C51Proj {
    float l, u, dml, dmu;
};
MI355_HD C51Proj c51_proj_elem(float rew, float done, float gamma, float atom, float vmin, float vmax, float delta_z, int na, float p,
                               bool l_eq_b) {
    C51Proj e;
    const float next = rew + (gamma * atom) * (1.0f - done);
    const float tz = op_clamp_f(next, vmin, vmax);
    const float b = (tz - vmin) / delta_z;
    const float top = (float)(na - 1);
    e.l = op_clamp_f(__builtin_floorf(b), 0.0f, top);
    e.u = op_clamp_f(__builtin_ceilf(b), 0.0f, top);
    e.dml = ((e.u + ((l_eq_b ? e.l == b : e.l == e.u) ? 1.0f : 0.0f)) - b) * p;
    e.dmu = (b - e.l) * p;
    return e;
}
// target_pmfs[k] of one row: the serial order of index_add_(0, l, d_m_l) followed by index_add_(0, u, d_m_u)
MI355_HD float c51_proj_atom(int k, const float* l, const float* u, const float* dml, const float* dmu, int na) {
    const float fk = (float)k;
    float acc = 0.0f;
    for (int j = 0; j < na; ++j)
        if (l[j] == fk) acc = acc + dml[j];
    for (int j = 0; j < na; ++j)
        if (u[j] == fk) acc = acc + dmu[j];
    return acc;
}

// one atom of -(target_pmfs * old_pmfs.clamp(1e-5, 1 - 1e-5).log()).sum(-1).mean(): the product, d loss / d old_pmfs[k] (zero where
// the clamp is active, as clamp's backward is) and that times old_pmfs[k] (the softmax backward's dot product term)
struct C51Loss {
    float term, g, gp;
};
MI355_HD C51Loss c51_loss_elem(float tp, float p, float inv_m) {
    C51Loss e;
    const float lo = 1e-5f, hi = 0.99999f;        // float(1 - 1e-5)
    e.term = tp * op_log(op_clamp_f(p, lo, hi));
    e.g = (p >= lo && p <= hi) ? ((-tp) * inv_m) / p : 0.0f;
    e.gp = e.g * p;
    return e;
}
// softmax backward on the taken action's atoms
MI355_HD float c51_dlogit(float p, float g, float dot) { return p * (g - dot); }

// The categorical update of one row in serial form (wg_c51_row of qhead_wg.h on the host): the projection of pnext (the target's
// pmf at the chosen action) through next_row / target_row (optional outputs), the loss against pred (the online pmf at the taken
// action) and dq[k] = d loss / d logit k.  scale multiplies the row's gradient; tmp holds 5 * na floats.  Returns the row's loss.
inline float c51_row_host(const float* pnext, const float* pred, const float* atoms, float rew, float done, float gamma, float vmin, float vmax,
                          float delta_z, int na, float scale, bool l_eq_b, float* next_row, float* target_row, float* tmp, float* dq) {
    float *pl = tmp, *pu = pl + na, *pdl = pu + na, *pdu = pdl + na, *tp = pdu + na;
    for (int j = 0; j < na; ++j) {
        const C51Proj e = c51_proj_elem(rew, done, gamma, atoms[j], vmin, vmax, delta_z, na, pnext[j], l_eq_b);
        pl[j] = e.l, pu[j] = e.u, pdl[j] = e.dml, pdu[j] = e.dmu;
        if (next_row) next_row[j] = pnext[j];
    }
    for (int k = 0; k < na; ++k) {
        tp[k] = c51_proj_atom(k, pl, pu, pdl, pdu, na);
        if (target_row) target_row[k] = tp[k];
    }
    float s = 0.0f, dot = 0.0f;
    for (int k = 0; k < na; ++k) {
        const C51Loss e = c51_loss_elem(tp[k], pred[k], scale);
        pdl[k] = e.g;
        s = s + e.term;
        dot = dot + e.gp;
    }
    for (int k = 0; k < na; ++k) dq[k] = c51_dlogit(pred[k], pdl[k], dot);
    return -s;
}

}  // namespace mi355ppo
