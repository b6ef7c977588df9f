// Row / element math of the PQN kernels (pqn.hip) and their host twins (host_twins.hip): one definition compiled for both
// sides, so a twin returns the device's bits.  Reference: cleanrl/pqn.py and cleanrl/pqn_atari_envpool.py.
//
// * pqn_argmax            torch.argmax / torch.max(dim=-1) over one row: the first maximum wins; a NaN is the maximum and the
//                         first NaN wins.
// * pqn_qlambda_*         the "# Compute Q(lambda) targets" loop in its operation order, every Python scalar rounded to f32.
// * pqn_lin_ln_relu       Linear(K -> H) + LayerNorm(H) + ReLU of one row (QNetwork of pqn.py); pqn_ln_relu_bwd its gradient.
// * pqn_radam_elem        clip coefficient + torch's single-tensor RAdam step (torch/optim/radam.py) on one element.
//
// Scratch vectors of one row are addressed as p[j * s]: s = 1 for a row-major host buffer, s = the padded row count for the
// device's row-interleaved (lane = row, coalesced) buffers.  Every sum runs in ascending index order.
#pragma once
#include "common.h"

namespace mi355ppo {

constexpr int kPqnH1 = 120;          // pqn.py: Linear(obs, 120) -> LayerNorm(120)
constexpr int kPqnH2 = 84;           //         Linear(120, 84) -> LayerNorm(84)
constexpr int kPqnMaxObs = 64;
constexpr int kPqnMaxA = 18;
constexpr float kPqnLnEps = 1e-5f;   // nn.LayerNorm default
constexpr int kPqnRows = 256;        // rows per weight-gradient partial (one workgroup of the fwd_bwd kernel)
constexpr int kPqnSched = 8;         // floats per RAdam schedule slot: {bc1, lr, sqrt(bc2), rect, rectified, 0, 0, 0}

MI355_HD bool pqn_isnan(float x) { return x != x; }

MI355_HD int pqn_argmax(const float* q, int qs, int A) {
    int bi = 0;
    float best = q[0];
    for (int a = 1; a < A; ++a) {
        const float v = q[a * qs];
        if (!pqn_isnan(best) && (pqn_isnan(v) || v > best)) {
            best = v;
            bi = a;
        }
    }
    return bi;
}

// One env of the rollout's action logic: argmax, q at the greedy index, `rand < epsilon`, `where`.
MI355_HD int64_t pqn_egreedy(const float* q, int qs, int A, int64_t random_action, float u, float eps_f, float* value) {
    const int g = pqn_argmax(q, qs, A);
    *value = q[g * qs];
    return (u < eps_f) ? random_action : (int64_t)g;
}

// returns[T-1] = rewards + args.gamma * next_value * nextnonterminal
MI355_HD float pqn_qlambda_last(float r, float next_value, float next_done, float gamma) {
    const float nnt = 1.0f - next_done;
    return r + (gamma * next_value) * nnt;
}

// returns[t] = rewards + args.gamma * (args.q_lambda * returns[t+1] + (1 - args.q_lambda) * values[t+1]) * nextnonterminal
MI355_HD float pqn_qlambda_step(float r, float ret_next, float v_next, float d_next, float gamma, float lam, float oml) {
    const float nnt = 1.0f - d_next;
    return r + (gamma * ((lam * ret_next) + (oml * v_next))) * nnt;
}

// ------------------------------------------------------------------------------------------------ QNetwork of pqn.py
struct PqnNet {
    const float *w1, *b1, *g1, *be1, *w2, *b2, *g2, *be2, *w3, *b3;
    int O, A;
};

MI355_HD int64_t pqn_param_count(int O, int A) {
    return (int64_t)kPqnH1 * O + 3 * kPqnH1 + (int64_t)kPqnH2 * kPqnH1 + 3 * kPqnH2 + (int64_t)A * kPqnH2 + A;
}

// agent.parameters() order: network.0 (weight, bias), network.1 (LayerNorm weight, bias), network.3, network.4, network.6
MI355_HD PqnNet pqn_net(const float* p, int O, int A) {
    PqnNet n;
    n.O = O;
    n.A = A;
    n.w1 = p;
    n.b1 = n.w1 + kPqnH1 * O;
    n.g1 = n.b1 + kPqnH1;
    n.be1 = n.g1 + kPqnH1;
    n.w2 = n.be1 + kPqnH1;
    n.b2 = n.w2 + kPqnH2 * kPqnH1;
    n.g2 = n.b2 + kPqnH2;
    n.be2 = n.g2 + kPqnH2;
    n.w3 = n.be2 + kPqnH2;
    n.b3 = n.w3 + A * kPqnH2;
    return n;
}

// Linear(K -> H) + LayerNorm(H) (biased variance, eps 1e-5, affine) + ReLU of one row.  Writes xhat (the normalised row, kept
// for the backward) and a = relu(xhat * g + be); `a` may alias `xhat` when no backward follows.  H is a multiple of 4: four
// units' dot products run side by side (independent chains; each keeps its own k order).  Returns rstd.
MI355_HD float pqn_lin_ln_relu(const float* x, int xs, int K, const float* W, const float* b, const float* g, const float* be, int H,
                               float* xhat, float* a, int s) {
    for (int j = 0; j < H; j += 4) {
        const float* w0 = W + (int64_t)j * K;
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
        for (int k = 0; k < K; ++k) {
            const float xv = x[k * xs];
            c0 = c0 + xv * w0[k];
            c1 = c1 + xv * w0[K + k];
            c2 = c2 + xv * w0[2 * K + k];
            c3 = c3 + xv * w0[3 * K + k];
        }
        xhat[j * s] = c0 + b[j];
        xhat[(j + 1) * s] = c1 + b[j + 1];
        xhat[(j + 2) * s] = c2 + b[j + 2];
        xhat[(j + 3) * s] = c3 + b[j + 3];
    }
    float sum = 0.0f;
    for (int j = 0; j < H; ++j) sum = sum + xhat[j * s];
    const float mean = sum / (float)H;
    float var = 0.0f;
    for (int j = 0; j < H; ++j) {
        const float d = xhat[j * s] - mean;
        var = var + d * d;
    }
    var = var / (float)H;
    const float rstd = 1.0f / sqrtf(var + kPqnLnEps);
    for (int j = 0; j < H; ++j) {
        const float xh = (xhat[j * s] - mean) * rstd;
        const float y = xh * g[j] + be[j];
        xhat[j * s] = xh;
        a[j * s] = (y < 0.0f) ? 0.0f : y;          // relu; NaN passes as torch's does
    }
    return rstd;
}

// The output layer: q[c] = b3[c] + sum_k a2[k] * w3[c, k].
MI355_HD void pqn_head(const PqnNet& n, const float* a2, int s, float* q, int qs) {
    for (int c = 0; c < n.A; ++c) {
        const float* w = n.w3 + c * kPqnH2;
        float acc = 0.0f;
        for (int k = 0; k < kPqnH2; ++k) acc = acc + a2[k * s] * w[k];
        q[c * qs] = acc + n.b3[c];
    }
}

// QNetwork.forward of one row.  Scratch: xh1 / a1 (120), xh2 / a2 (84) at stride s (a may alias xh).
MI355_HD void pqn_row_forward(const PqnNet& n, const float* x, int xs, float* xh1, float* a1, float* xh2, float* a2, int s, float* q, int qs,
                              float* rstd) {
    rstd[0] = pqn_lin_ln_relu(x, xs, n.O, n.w1, n.b1, n.g1, n.be1, kPqnH1, xh1, a1, s);
    rstd[1] = pqn_lin_ln_relu(a1, s, kPqnH1, n.w2, n.b2, n.g2, n.be2, kPqnH2, xh2, a2, s);
    pqn_head(n, a2, s, q, qs);
}

// Gradient through ReLU and LayerNorm of one row, given da (gradient at the ReLU output) in dy: dy <- da * (a > 0) (the gradient
// at the LayerNorm output, whose row sums give d gamma / d beta), dz <- the gradient at the Linear output (closed form:
// rstd * (dxh - mean(dxh) - xhat * mean(dxh * xhat)), dxh = dy * gamma).
MI355_HD void pqn_ln_relu_bwd(const float* xh, const float* a, const float* g, float rstd, int H, float* dy, float* dz, int s) {
    float s1 = 0.0f, s2 = 0.0f;
    for (int j = 0; j < H; ++j) {
        const float d = (a[j * s] <= 0.0f) ? 0.0f : dy[j * s];   // threshold_backward: result <= 0 -> 0
        dy[j * s] = d;
        const float dxh = d * g[j];
        s1 = s1 + dxh;
        s2 = s2 + dxh * xh[j * s];
    }
    const float m1 = s1 / (float)H, m2 = s2 / (float)H;
    for (int j = 0; j < H; ++j) {
        const float dxh = dy[j * s] * g[j];
        dz[j * s] = rstd * ((dxh - m1) - xh[j * s] * m2);
    }
}

// d q -> (dy2, dz2, dy1, dz1) of one row.  dq has A entries at stride qs.
MI355_HD void pqn_row_backward(const PqnNet& n, const float* dq, int qs, const float* xh1, const float* a1, const float* xh2, const float* a2,
                               const float* rstd, float* dy1, float* dz1, float* dy2, float* dz2, int s) {
    for (int k = 0; k < kPqnH2; ++k) {
        float acc = 0.0f;
        for (int c = 0; c < n.A; ++c) acc = acc + dq[c * qs] * n.w3[c * kPqnH2 + k];
        dy2[k * s] = acc;
    }
    pqn_ln_relu_bwd(xh2, a2, n.g2, rstd[1], kPqnH2, dy2, dz2, s);
    for (int k = 0; k < kPqnH1; k += 4) {
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f;
        for (int j = 0; j < kPqnH2; ++j) {
            const float d = dz2[j * s];
            const float* w = n.w2 + j * kPqnH1 + k;
            c0 = c0 + d * w[0];
            c1 = c1 + d * w[1];
            c2 = c2 + d * w[2];
            c3 = c3 + d * w[3];
        }
        dy1[k * s] = c0;
        dy1[(k + 1) * s] = c1;
        dy1[(k + 2) * s] = c2;
        dy1[(k + 3) * s] = c3;
    }
    pqn_ln_relu_bwd(xh1, a1, n.g1, rstd[0], kPqnH1, dy1, dz1, s);
}

// The TD loss of one row: old = q[action] (the gather; `.long()` truncates, an index outside [0, A) is clamped), *sq = (ret - old)^2.
MI355_HD float pqn_td_old(const float* q, int qs, int A, float action_f, float ret, int* action, float* d, float* sq) {
    int a = (int)(int64_t)action_f;
    a = a < 0 ? 0 : (a >= A ? A - 1 : a);
    const float old = q[a * qs];
    *action = a;
    *d = ret - old;
    *sq = *d * *d;
    return old;
}

// ... and its gradient: d F.mse_loss(returns, old) / d old = -((2/M) * (ret - old)) in the action's column, 0 elsewhere.
// `norm` = (float)(2.0 / M), as mse_loss_backward forms it.  Returns old.
MI355_HD float pqn_td_row(const float* q, int qs, int A, float action_f, float ret, float norm, float* dq, int dqs, float* sq) {
    int a;
    float d;
    const float old = pqn_td_old(q, qs, A, action_f, ret, &a, &d, sq);
    for (int c = 0; c < A; ++c) dq[c * dqs] = 0.0f;
    dq[a * dqs] = -(norm * d);
    return old;
}

// Deterministic sums over rows (the TD scalars, the gradient's sum of squares): slot t of kPqnFold takes rows t, t + kPqnFold, ...
// in f64, then the slots are added in order.  The device runs slot t on thread t of one workgroup; the twins run the same loops.
constexpr int kPqnFold = 256;

// Workgroup 0's part of the TD scalars (a workgroup of kPqnFold threads): slot t = threadIdx.x adds rows t, t + 256, ... in f64;
// thread 0 adds the slots in order.
__device__ inline void pqn_fold_scalars(double so, double ss, int M, float* __restrict__ scalars) {
    __shared__ double s_old[kPqnFold], s_sq[kPqnFold];
    s_old[threadIdx.x] = so;
    s_sq[threadIdx.x] = ss;
    __syncthreads();
    if (threadIdx.x == 0) {
        double to = 0.0, ts = 0.0;
        for (int t = 0; t < kPqnFold; ++t) {
            to += s_old[t];
            ts += s_sq[t];
        }
        scalars[0] = (float)(ts / (double)M);                        // losses/td_loss
        scalars[1] = (float)(to / (double)M);                        // losses/q_values: old_val.mean()
    }
}

MI355_HD int64_t pqn_clamp_index(int64_t i, int64_t B) { return i < 0 ? 0 : (i >= B ? B - 1 : i); }

// Workgroups of the clip's sum-of-squares pass over n elements (each adds its kPqnFold slots in order into one partial).
MI355_HD int pqn_sumsq_blocks(int64_t n) {
    const int64_t b = (n + 2047) / 2048;
    return b < 1 ? 1 : (b > 256 ? 256 : (int)b);
}

// The parameter element e of the flat gradient as a sum over rows of buf[u1] * buf[u2] (u2 < 0: of buf[u1] alone).  The row
// buffer's units, in this order: x (O), xh1, a1, dy1, dz1 (120 each), xh2, a2, dy2, dz2 (84 each), dq (A), old, sq.
struct PqnUnits {
    int x, xh1, a1, dy1, dz1, xh2, a2, dy2, dz2, dq, old, sq, total;
};
MI355_HD PqnUnits pqn_units(int O, int A) {
    PqnUnits u;
    u.x = 0;
    u.xh1 = O;
    u.a1 = u.xh1 + kPqnH1;
    u.dy1 = u.a1 + kPqnH1;
    u.dz1 = u.dy1 + kPqnH1;
    u.xh2 = u.dz1 + kPqnH1;
    u.a2 = u.xh2 + kPqnH2;
    u.dy2 = u.a2 + kPqnH2;
    u.dz2 = u.dy2 + kPqnH2;
    u.dq = u.dz2 + kPqnH2;
    u.old = u.dq + A;
    u.sq = u.old + 1;
    u.total = u.sq + 1;
    return u;
}
MI355_HD void pqn_grad_units(int64_t e, int O, int A, int* u1, int* u2) {
    const PqnUnits u = pqn_units(O, A);
    int64_t o = e;
    if (o < (int64_t)kPqnH1 * O) { *u1 = u.dz1 + (int)(o / O); *u2 = u.x + (int)(o % O); return; }           // W1 = dz1 x^T
    o -= (int64_t)kPqnH1 * O;
    if (o < kPqnH1) { *u1 = u.dz1 + (int)o; *u2 = -1; return; }                                              // b1
    o -= kPqnH1;
    if (o < kPqnH1) { *u1 = u.dy1 + (int)o; *u2 = u.xh1 + (int)o; return; }                                  // LayerNorm(120).weight
    o -= kPqnH1;
    if (o < kPqnH1) { *u1 = u.dy1 + (int)o; *u2 = -1; return; }                                              // LayerNorm(120).bias
    o -= kPqnH1;
    if (o < kPqnH2 * kPqnH1) { *u1 = u.dz2 + (int)(o / kPqnH1); *u2 = u.a1 + (int)(o % kPqnH1); return; }  // W2 = dz2 a1^T
    o -= kPqnH2 * kPqnH1;
    if (o < kPqnH2) { *u1 = u.dz2 + (int)o; *u2 = -1; return; }
    o -= kPqnH2;
    if (o < kPqnH2) { *u1 = u.dy2 + (int)o; *u2 = u.xh2 + (int)o; return; }
    o -= kPqnH2;
    if (o < kPqnH2) { *u1 = u.dy2 + (int)o; *u2 = -1; return; }
    o -= kPqnH2;
    if (o < (int64_t)A * kPqnH2) { *u1 = u.dq + (int)(o / kPqnH2); *u2 = u.a2 + (int)(o % kPqnH2); return; }  // W3 = dq a2^T
    o -= (int64_t)A * kPqnH2;
    *u1 = u.dq + (int)o;                                                                                      // b3
    *u2 = -1;
}

// --------------------------------------------------------------------------------------------------------- RAdam
struct RAdamParams {
    float max_norm;
    float w1;        // (float)(1 - beta1)    lerp weight
    float beta2;
    float w2;        // (float)(1 - beta2)
    float eps;
    int nblocks;
};

// clip_grad_norm_'s multiply, then _single_tensor_radam in its operation order; c = one schedule slot (kPqnSched floats).
// Zeroes the gradient for the next backward.
MI355_HD void pqn_radam_elem(float& p, float& g, float& m, float& v, float coef, const RAdamParams& R, const float* c) {
    const float gg = g * coef;                               // grads.mul_(clip_coef_clamped)
    m = m + R.w1 * (gg - m);                                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * R.beta2;                                         // exp_avg_sq.mul_(beta2)
    v = v + (R.w2 * gg) * gg;                                //           .addcmul_(grad, grad, value=1 - beta2)
    float u = m / c[0];                                      // bias_corrected_exp_avg = exp_avg / bias_correction1
    u = u * c[1];                                            //   * lr
    if (c[4] != 0.0f) {                                      // rho_t > 5
        const float ad = (1.0f / (sqrtf(v) + R.eps)) * c[2]; //   * (bias_correction2 ** 0.5 / (exp_avg_sq.sqrt() + eps))
        u = u * ad;
        u = u * c[3];                                        //   * rect
    }
    p = p - u;                                               // param.add_(..., alpha=-1.0)
    g = 0.0f;
}

MI355_HD float pqn_clip_coef(double sumsq, float max_norm) {
    const float total = (float)sqrt(sumsq);
    float coef = max_norm / (total + 1e-6f);                 // clip_grad.py: max_norm / (total_norm + 1e-6), clamp(max=1.0)
    return coef > 1.0f ? 1.0f : coef;                        // (NaN stays NaN, as clamp keeps it)
}

}  // namespace mi355ppo
