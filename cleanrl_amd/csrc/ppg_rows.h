// Row / element math of the PPG auxiliary-phase kernels (ppg.hip: cleanrl/ppg_procgen.py:421-474) and their host-pointer twins,
// compiled for both sides, so a twin returns the device's bits.  op_mac is offpolicy_rows.h's, op_exp / op_log sac_rows.h's.
//
// * Flat row t * n + i of a minibatch is (t, cols[i]) of the (T, R, ...) auxiliary buffers -- flatten01 over (T, n); every offset
//   into them is 64-bit.  A cols entry outside [0, R) is clamped.
// * Every dot product starts at 0.0f and adds its products in ascending index order through op_mac, then adds the bias.
// * A normalised row: mx = max z, sum of op_exp(z - mx) in ascending action order, logp = (z - mx) - op_log(sum),
//   p = op_exp(z - mx) / sum.  The OLD row is normalised again (Categorical(logits=old)) and p_old = op_exp(logp_old).
// * kl_row = sum_j p_old (logp_old - logp_new) in ascending j; a term is inf where p_new == 0 and then 0 where p_old == 0 (torch's
//   _kl_categorical_categorical, in its order).  d kl_row / d z_j = p_new - p_old.
// * Rows are dealt to tiles of kPpgRows; a tile's partial of dz^T h starts at 0.0f and adds its rows in ascending order, the tiles'
//   partials are then added in ascending tile order from 0.0f.  The three loss sums do the same in f64.
#pragma once
#include "sac_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kPpgH = 256;              // hidden width of the IMPALA encoder's top
constexpr int kPpgMinA = 2, kPpgMaxA = 30;
constexpr int kPpgJ = 32;               // output tile: A logits, the critic at A, the auxiliary critic at A + 1
constexpr int kPpgRows = 8;             // rows of a tile (one workgroup; 8 KB of hidden rows in LDS)
constexpr int kPpgPart = kPpgJ * kPpgH + kPpgJ;      // floats of a tile's partial: dz^T h (32 x 256), then the 32 bias sums
constexpr int kPpgMaxRows = 1 << 16;    // rows of one loss / old-logits call

// x / 255.0f, correctly rounded, as the observation kernel forms it (obs.hip: one Newton residual step on the reciprocal product).
MI355_HD float ppg_u8_div255(float x) {
    const float r = 1.0f / 255.0f;
    const float q = x * r;
    const float e = fmaf(-q, 255.0f, x);
    return fmaf(e, r, q);
}

MI355_HD int64_t ppg_clamp_col(int64_t c, int64_t R) { return c < 0 ? 0 : (c >= R ? R - 1 : c); }

// Flat row -> t * R + cols[i]: the row's offset into a (T, R) buffer.
MI355_HD int64_t ppg_row_offset(int64_t row, int n, int64_t R, const int64_t* __restrict__ cols) {
    const int64_t t = row / n, i = row - t * n;
    return t * R + ppg_clamp_col(cols[i], R);
}

MI355_HD float ppg_dot(const float* __restrict__ h, const float* __restrict__ w) {
    float acc = 0.0f;
    for (int k = 0; k < kPpgH; ++k) acc = op_mac(acc, h[k], w[k]);
    return acc;
}

// max and log-sum-exp pieces of a row: returns mx, *lse = op_log(sum), *sum.
MI355_HD float ppg_row_lse(const float* z, int A, float* lse, float* sum_out) {
    float mx = z[0];
    for (int j = 1; j < A; ++j) mx = z[j] > mx ? z[j] : mx;
    float sum = 0.0f;
    for (int j = 0; j < A; ++j) sum = sum + op_exp(z[j] - mx);
    *lse = op_log(sum);
    *sum_out = sum;
    return mx;
}

// z -> (z - mx) - log sum exp(z - mx), in place.
MI355_HD void ppg_lognorm_(float* z, int A) {
    float lse, sum;
    const float mx = ppg_row_lse(z, A, &lse, &sum);
    for (int j = 0; j < A; ++j) z[j] = (z[j] - mx) - lse;
}

// One row of the auxiliary loss.  z: A logits, the value at A, the auxiliary value at A + 1; old: the stored row (OVERWRITTEN with
// its renormalised log-probabilities).  dz (A + 2): the gradient of (aux_value_loss + beta_clone kl + real_value_loss) inv_accum
// with g_kl = (float)(beta_clone inv_accum / M), g_v = (float)(inv_accum / M).  loss3 = {kl_row, (vx - ret)^2, (v - ret)^2}.
MI355_HD void ppg_aux_row(const float* z, float* old, float ret, int A, float g_kl, float g_v, float* dz, double* loss3) {
    ppg_lognorm_(old, A);
    float lse, sum;
    const float mx = ppg_row_lse(z, A, &lse, &sum);
    float kl = 0.0f;
    for (int j = 0; j < A; ++j) {
        const float pn = op_exp(z[j] - mx) / sum;
        const float lpn = (z[j] - mx) - lse;
        const float po = op_exp(old[j]);
        float term = po * (old[j] - lpn);
        if (pn == 0.0f) term = __builtin_bit_cast(float, (uint32_t)0x7f800000u);
        if (po == 0.0f) term = 0.0f;
        kl = kl + term;
        dz[j] = (pn - po) * g_kl;
    }
    const float dv = z[A] - ret, dx = z[A + 1] - ret;
    dz[A] = dv * g_v;
    dz[A + 1] = dx * g_v;
    loss3[0] = (double)kl;
    loss3[1] = (double)dx * (double)dx;
    loss3[2] = (double)dv * (double)dv;
}

// dh[k] of a row: the actor's A terms in ascending j, then the auxiliary critic's (the critic reads detached features).
MI355_HD float ppg_dh(const float* dz, const float* wa_col, int stride, float wx_k, int A) {
    float acc = 0.0f;
    for (int j = 0; j < A; ++j) acc = op_mac(acc, dz[j], wa_col[(int64_t)j * stride]);
    return op_mac(acc, dz[A + 1], wx_k);
}

// A tile's partial of one head-gradient element: rows ascending from 0.0f (a weight element; then a bias element).
MI355_HD float ppg_tile_partial(const float* dzj, int dz_stride, const float* hk, int nr) {
    float acc = 0.0f;
    for (int r = 0; r < nr; ++r) acc = op_mac(acc, dzj[r * dz_stride], hk[r * kPpgH]);
    return acc;
}

MI355_HD float ppg_tile_partial_bias(const float* dzj, int dz_stride, int nr) {
    float acc = 0.0f;
    for (int r = 0; r < nr; ++r) acc = acc + dzj[r * dz_stride];
    return acc;
}

// The logged means: kl (q == 0) is mean(kl_row), the two value losses 0.5 mean((v - ret)^2).
MI355_HD float ppg_scalar(double sum, int M, int q) { return q == 0 ? (float)(sum / (double)M) : (float)(0.5 * (sum / (double)M)); }

// ---- what the device entry points (ppg.hip) and their twins (ppg_twins.hip) share: argument packs and checks (before any launch)
struct PpgAuxArgs {
    const float *h, *wa, *ba, *wc, *bc, *wx, *bx, *aux_pi, *aux_returns;
    const int64_t* cols;
    float* dh;
    float* part;       // (tiles, kPpgPart)
    double* sums;      // (tiles, 3)
    int64_t R;
    int M, n, A;
    float g_kl, g_v;
};

struct PpgGrads {
    float *dwa, *dba, *dwc, *dbc, *dwx, *dbx;
};

// Element e of the head gradients: e < J * 256 is weight (j, k), the next J are the biases.  -> its place in the six tensors.
MI355_HD float* ppg_grad_slot(const PpgGrads& g, int e, int A, int* part_index) {
    const int J = A + 2;
    if (e < J * kPpgH) {
        const int j = e >> 8, k = e & (kPpgH - 1);
        *part_index = e;
        return j < A ? g.dwa + e : (j == A ? g.dwc + k : g.dwx + k);
    }
    const int j = e - J * kPpgH;
    *part_index = kPpgJ * kPpgH + j;
    return j < A ? g.dba + j : (j == A ? g.dbc : g.dbx);
}

// workspace: the tiles' loss sums (3 doubles each, rounded up to 16 bytes in all), then the tiles' partials (kPpgPart floats each)
inline size_t ppg_sums_bytes(int tiles) { return (((size_t)tiles * 3 * sizeof(double)) + 15) / 16 * 16; }

inline int ppg_dims(const char* fn, int T, int n, int64_t R, int64_t max_rows) {
    MI355_REQUIRE(T > 0 && n > 0 && R > 0 && (int64_t)n <= R, MI355PPO_EINVAL, "%s: T=%d n=%d R=%lld: all positive, n <= R", fn, T, n, (long long)R);
    MI355_REQUIRE((int64_t)T * n <= max_rows, MI355PPO_EINVAL, "%s: T * n = %lld rows exceed %lld", fn, (long long)T * n, (long long)max_rows);
    return MI355PPO_OK;
}

inline int ppg_head_dims(const char* fn, int A, int hidden) {
    MI355_REQUIRE(hidden == kPpgH, MI355PPO_EINVAL, "%s: hidden=%d: the kernel is written for %d", fn, hidden, kPpgH);
    MI355_REQUIRE(A >= kPpgMinA && A <= kPpgMaxA, MI355PPO_EINVAL, "%s: A=%d: %d <= A <= %d (A + 2 outputs fit one 32-output tile)", fn, A, kPpgMinA,
                  kPpgMaxA);
    return MI355PPO_OK;
}

inline int ppg_gather_args(const char* fn, const unsigned char* aux_obs, const int64_t* cols, float* out, int T, int n, int64_t R, int64_t row_bytes) {
    MI355_REQUIRE(aux_obs && cols && out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = ppg_dims(fn, T, n, R, 2147483647LL)) return rc;
    MI355_REQUIRE(row_bytes > 0 && row_bytes % 4 == 0 && row_bytes / 4 <= (int64_t)65535 * 1024, MI355PPO_EINVAL,
                  "%s: row_bytes=%lld must be a positive multiple of 4 (<= 256 MiB)", fn, (long long)row_bytes);
    MI355_REQUIRE(aligned(aux_obs, 4) && aligned(out, 16) && aligned(cols, 8), MI355PPO_EALIGN,
                  "%s: aux_obs must be 4-byte, out 16-byte, cols 8-byte aligned", fn);
    return MI355PPO_OK;
}

inline int ppg_old_args(const char* fn, const float* h, const float* w, const float* b, const int64_t* cols, float* aux_pi, int T, int n, int64_t R, int A,
                        int hidden) {
    MI355_REQUIRE(h && w && b && cols && aux_pi, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = ppg_head_dims(fn, A, hidden)) return rc;
    if (int rc = ppg_dims(fn, T, n, R, kPpgMaxRows)) return rc;
    MI355_REQUIRE(aligned(h, 4) && aligned(w, 4) && aligned(b, 4) && aligned(aux_pi, 4) && aligned(cols, 8), MI355PPO_EALIGN,
                  "%s: a pointer is not aligned to its element size", fn);
    return MI355PPO_OK;
}

inline int ppg_aux_args(const char* fn, const PpgAuxArgs& a, const PpgGrads& g, const float* scalars, int T, int hidden, int accumulate) {
    MI355_REQUIRE(a.h && a.wa && a.ba && a.wc && a.bc && a.wx && a.bx && a.aux_pi && a.aux_returns && a.cols && a.dh && scalars && g.dwa && g.dba &&
                      g.dwc && g.dbc && g.dwx && g.dbx,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = ppg_head_dims(fn, a.A, hidden)) return rc;
    if (int rc = ppg_dims(fn, T, a.n, a.R, kPpgMaxRows)) return rc;
    MI355_REQUIRE(accumulate == 0 || accumulate == 1, MI355PPO_EINVAL, "%s: accumulate=%d: 0 (overwrite) or 1 (add)", fn, accumulate);
    MI355_REQUIRE(aligned(a.h, 4) && aligned(a.wa, 4) && aligned(a.ba, 4) && aligned(a.wc, 4) && aligned(a.bc, 4) && aligned(a.wx, 4) && aligned(a.bx, 4) &&
                      aligned(a.aux_pi, 4) && aligned(a.aux_returns, 4) && aligned(a.cols, 8) && aligned(a.dh, 4) && aligned(scalars, 4) &&
                      aligned(g.dwa, 4) && aligned(g.dba, 4) && aligned(g.dwc, 4) && aligned(g.dbc, 4) && aligned(g.dwx, 4) && aligned(g.dbx, 4),
                  MI355PPO_EALIGN, "%s: a pointer is not aligned to its element size", fn);
    return MI355PPO_OK;
}

inline PpgAuxArgs ppg_aux_pack(const float* h, const float* wa, const float* ba, const float* wc, const float* bc, const float* wx, const float* bx,
                               const float* aux_pi, const float* aux_returns, const int64_t* cols, int T, int n, int64_t R, int A, double beta_clone,
                               double inv_accum, float* dh) {
    PpgAuxArgs a;
    a.h = h, a.wa = wa, a.ba = ba, a.wc = wc, a.bc = bc, a.wx = wx, a.bx = bx, a.aux_pi = aux_pi, a.aux_returns = aux_returns, a.cols = cols;
    a.dh = dh, a.part = nullptr, a.sums = nullptr;
    a.R = R, a.n = n, a.A = A;
    const int64_t M = (int64_t)T * n;
    a.M = M > 0 && M <= kPpgMaxRows ? (int)M : 0;
    a.g_kl = a.M ? (float)(beta_clone * inv_accum / (double)a.M) : 0.0f;
    a.g_v = a.M ? (float)(inv_accum / (double)a.M) : 0.0f;
    return a;
}

}  // namespace mi355ppo
