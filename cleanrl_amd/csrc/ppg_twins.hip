// Host-pointer twins of the PPG auxiliary-phase entry points (ppg.hip, and the split optimiser step of optim.hip): the row math of
// ppg_rows.h and adam_elem of ppo_rows.h compiled for the host, in the device kernels' orders -- rows dealt to tiles of kPpgRows, a
// tile's partial from 0.0f in ascending rows, the tiles in ascending order -- so a twin returns the device's bits.  No kernels in this
// file: tools/ppg_host_check.cpp builds it for the host alone under the sanitizers.
#include <math.h>

#include <vector>

#include "common.h"
#include "ppg_rows.h"
#include "ppo_rows.h"

#pragma clang fp contract(off)

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_ppg_aux_gather_u8_f32_cpu(const unsigned char* aux_obs, const int64_t* cols, float* out, int T, int n, int64_t R,
                                                              int64_t row_bytes) {
    const char* fn = "mi355ppo_ppg_aux_gather_u8_f32_cpu";
    if (int rc = ppg_gather_args(fn, aux_obs, cols, out, T, n, R, row_bytes)) return rc;
    for (int64_t r = 0; r < (int64_t)T * n; ++r) {
        const unsigned char* s = aux_obs + ppg_row_offset(r, n, R, cols) * row_bytes;
        float* d = out + r * row_bytes;
        for (int64_t k = 0; k < row_bytes; ++k) d[k] = ppg_u8_div255((float)s[k]);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_ppg_old_logits_f32_cpu(const float* h, const float* w, const float* b, const int64_t* cols, float* aux_pi, int T,
                                                           int n, int64_t R, int A, int hidden) {
    const char* fn = "mi355ppo_ppg_old_logits_f32_cpu";
    if (int rc = ppg_old_args(fn, h, w, b, cols, aux_pi, T, n, R, A, hidden)) return rc;
    for (int r = 0; r < T * n; ++r) {
        float z[kPpgJ];
        for (int j = 0; j < A; ++j) z[j] = ppg_dot(h + (int64_t)r * kPpgH, w + (int64_t)j * kPpgH) + b[j];
        ppg_lognorm_(z, A);
        float* o = aux_pi + ppg_row_offset(r, n, R, cols) * A;
        for (int j = 0; j < A; ++j) o[j] = z[j];
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_ppg_aux_fwd_bwd_f32_cpu(const float* h, const float* wa, const float* ba, const float* wc, const float* bc,
                                                            const float* wx, const float* bx, const float* aux_pi, const float* aux_returns,
                                                            const int64_t* cols, int T, int n, int64_t R, int A, int hidden, double beta_clone,
                                                            double inv_accum, float* scalars_out, float* dh, float* dwa, float* dba, float* dwc,
                                                            float* dbc, float* dwx, float* dbx, int accumulate) {
    const char* fn = "mi355ppo_ppg_aux_fwd_bwd_f32_cpu";
    const PpgAuxArgs a = ppg_aux_pack(h, wa, ba, wc, bc, wx, bx, aux_pi, aux_returns, cols, T, n, R, A, beta_clone, inv_accum, dh);
    const PpgGrads g{dwa, dba, dwc, dbc, dwx, dbx};
    if (int rc = ppg_aux_args(fn, a, g, scalars_out, T, hidden, accumulate)) return rc;
    const int M = a.M, J = A + 2, tiles = (M + kPpgRows - 1) / kPpgRows;
    std::vector<float> dz((size_t)M * kPpgJ, 0.0f);
    std::vector<double> sums((size_t)tiles * 3, 0.0);
    for (int b = 0; b < tiles; ++b) {
        const int r0 = b * kPpgRows, nr = (M - r0 < kPpgRows) ? M - r0 : kPpgRows;
        double s[3] = {0.0, 0.0, 0.0};
        for (int r = r0; r < r0 + nr; ++r) {
            const float* hr = h + (int64_t)r * kPpgH;
            float z[kPpgJ], old[kPpgJ];
            for (int j = 0; j < J; ++j) {
                const float* w = j < A ? wa + (int64_t)j * kPpgH : (j == A ? wc : wx);
                z[j] = ppg_dot(hr, w) + (j < A ? ba[j] : (j == A ? bc[0] : bx[0]));
            }
            const int64_t off = ppg_row_offset(r, n, R, cols);
            for (int j = 0; j < A; ++j) old[j] = aux_pi[off * A + j];
            double l3[3];
            float* d = dz.data() + (size_t)r * kPpgJ;
            ppg_aux_row(z, old, aux_returns[off], A, a.g_kl, a.g_v, d, l3);
            for (int q = 0; q < 3; ++q) s[q] += l3[q];
            for (int k = 0; k < kPpgH; ++k) dh[(int64_t)r * kPpgH + k] = ppg_dh(d, wa + k, kPpgH, wx[k], A);
        }
        for (int q = 0; q < 3; ++q) sums[(size_t)b * 3 + q] = s[q];
    }
    for (int e = 0; e < J * (kPpgH + 1); ++e) {
        int pi;
        float* out = ppg_grad_slot(g, e, A, &pi);
        const bool bias = e >= J * kPpgH;
        const int j = bias ? e - J * kPpgH : e >> 8, k = e & (kPpgH - 1);
        float acc = 0.0f;
        for (int b = 0; b < tiles; ++b) {
            const int r0 = b * kPpgRows, nr = (M - r0 < kPpgRows) ? M - r0 : kPpgRows;
            const float* dzj = dz.data() + (size_t)r0 * kPpgJ + j;
            acc = acc + (bias ? ppg_tile_partial_bias(dzj, kPpgJ, nr) : ppg_tile_partial(dzj, kPpgJ, h + (int64_t)r0 * kPpgH + k, nr));
        }
        *out = accumulate ? *out + acc : acc;
    }
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int b = 0; b < tiles; ++b) s += sums[(size_t)b * 3 + q];
        scalars_out[q] = ppg_scalar(s, M, q);
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_clip_adam_split_f32_cpu(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                                             int64_t n_split, double grad_scale, double max_grad_norm, double lr, double beta1,
                                                             double beta2, double eps, int64_t step_head, int64_t step_tail,
                                                             float* total_norm_out) {
    const char* fn = "mi355ppo_clip_adam_split_f32_cpu";
    MI355_REQUIRE(params && grads && exp_avg && exp_avg_sq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0 && n_split >= 0 && n_split <= n && step_head >= 1 && step_tail >= 1, MI355PPO_EINVAL,
                  "%s: n=%lld n_split=%lld step_head=%lld step_tail=%lld: n > 0, 0 <= n_split <= n, steps >= 1", fn, (long long)n, (long long)n_split,
                  (long long)step_head, (long long)step_tail);
    AdamParams A;                                   // as mi355ppo_clip_adam_split_f32 forms them (optim.hip)
    A.scale = (float)grad_scale;
    A.max_norm = (float)max_grad_norm;
    A.w1 = (float)(1.0 - beta1);
    A.beta2 = (float)beta2;
    A.w2 = (float)(1.0 - beta2);
    A.eps = (float)eps;
    A.nblocks = 1;
    A.zero_grads = 1;
    AdamParams B = A;
    A.neg_step = (float)(-(lr / (1.0 - pow(beta1, (double)step_head))));
    A.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step_head));
    B.neg_step = (float)(-(lr / (1.0 - pow(beta1, (double)step_tail))));
    B.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)step_tail));
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const float a = grads[i] * A.scale;
        s += (double)a * a;
    }
    const float total = (float)sqrt(s);
    float coef = A.max_norm / (total + 1e-6f);
    coef = fminf(coef, 1.0f);
    if (total_norm_out) *total_norm_out = total;
    for (int64_t i = 0; i < n; ++i) adam_elem(params[i], grads[i], exp_avg[i], exp_avg_sq[i], coef, i < n_split ? A : B);
    return MI355PPO_OK;
}
