// Row math of the episodic-memory attention core of ppo_trxl.py (trxl_attn.hip) and of its host-pointer twins
// (host_twins.hip): one definition, compiled for both sides without FMA contraction.
//
// The reference (cleanrl/ppo_trxl/ppo_trxl.py: Transformer.forward, TransformerLayer.forward, MultiHeadAttention.forward),
// for one sample, one layer, window rows j = 0 .. L-1 and head h (d = D / H columns):
//   x_j   = mem[ep, rows_j, layer, :] + pe[pos_j]            (pe absent when trxl_positional_encoding == "")
//   y_j   = LayerNorm_kv(x_j)                                 (biased variance, eps 1e-5, gamma / beta of norm_kv)
//   e_j   = q~_h . y_j,h                                      (q~_h = W_k^T q_h, formed by the caller: q . (W_k y) = (W_k^T q) . y)
//   s_j   = (mask_j ? e_j : -1e20) / sqrt(D)                  (the fill BEFORE the scale, and sqrt of the embed dim: a fully
//                                                              masked window is a uniform softmax over all L rows)
//   u_h   = sum_j softmax(s)_j y_j,h                          (the caller applies `values` and `fc_out` to u)
// Backward with du_h = d loss / d u_h, att_j = softmax(s)_j:
//   ds_j  = att_j (du_h . y_j,h - du_h . u_h)
//   g_j   = mask_j ? ds_j / sqrt(D) : 0                      (d loss / d e_j: a masked row's score is a constant)
//   dq~_h = sum_j g_j y_j,h
//   dy_j  = g_j q~_h + att_j du_h;   dgamma += dy_j * xhat_j;   dbeta += dy_j    (no gradient to the memory: the reference
//                                                                                stores detached layer inputs)
//
// Reductions.  A row of D floats is spread over the 64 lanes of a wave, C = D / 64 consecutive floats per lane; head h is
// the group of G = 64 / H consecutive lanes.  Sums over a row or a head are a serial sum of the lane's C terms followed by
// an xor butterfly over the lanes (offsets 32, 16, ... 1 for a row; G/2 ... 1 for a head), so every lane of the group ends
// with the same bits.  Wave w of the 4 in a workgroup streams rows j = w, w + 4, ...; its online softmax state per head is
// merged with the other waves' in wave order.  The host twins emulate the lanes and waves, so they run this arithmetic.
#pragma once
#include "common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kTrxlWaves = 4;            // waves per workgroup (one workgroup per sample)
constexpr int kTrxlMaxD = 512;
constexpr int kTrxlMaxL = 1024;
constexpr float kTrxlLnEps = 1e-5f;      // nn.LayerNorm default
constexpr float kTrxlFill = -1e20f;      // masked_fill value of MultiHeadAttention.forward

// Shape check shared by the kernels and the twins: D % 64 == 0, D <= 512, H divides 64 (and D), 1 <= L <= 1024.
MI355_HD bool trxl_shape_ok(int D, int H, int L) {
    return D > 0 && D % 64 == 0 && D <= kTrxlMaxD && H > 0 && H <= 64 && 64 % H == 0 && L >= 1 && L <= kTrxlMaxL;
}

// The divisor of the scores: sqrt(embed_dim) rounded to f32 (torch divides an f32 tensor by the Python float).
inline float trxl_sqrt_d(int D) { return (float)sqrt((double)D); }

MI355_HD float trxl_rstd(float var) { return 1.0f / sqrtf(var + kTrxlLnEps); }

MI355_HD float trxl_score(bool keep, float e, float sqrt_d) { return (keep ? e : kTrxlFill) / sqrt_d; }

// Online softmax state of one head over the rows a wave has seen: running max m, sum l = sum exp(s - m), and the lane's
// C columns of acc = sum exp(s - m) y.  The first row has m = -inf: exp(-inf) = 0 scales the empty state.
struct TrxlOnline {
    float m, l;
};

// Update with score s: returns the factor the old (l, acc) are scaled by and writes p = exp(s - m_new).
MI355_HD float trxl_online_step(TrxlOnline& st, float s, float& p) {
    const float mn = fmaxf(st.m, s);
    const float a = expf(st.m - mn);
    p = expf(s - mn);
    st.l = st.l * a + p;
    st.m = mn;
    return a;
}

// The wave merge factors: M = max_w m_w, f_w = exp(m_w - M) (0 for a wave that saw no row: m_w = -inf, l_w = 0).
MI355_HD float trxl_merge_max(const float* m) {
    float M = m[0];
    for (int w = 1; w < kTrxlWaves; ++w) M = fmaxf(M, m[w]);
    return M;
}

MI355_HD float trxl_merge_sum(const float* v, const float* f) {
    float s = v[0] * f[0];
    for (int w = 1; w < kTrxlWaves; ++w) s = s + v[w] * f[w];
    return s;
}

// att_j from the forward's statistics (max M, sum l of the head).
MI355_HD float trxl_att(float s, float M, float l) { return expf(s - M) / l; }

}  // namespace mi355ppo
