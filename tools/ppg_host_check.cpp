// Stand-alone driver of the PPG auxiliary-phase host twins (cleanrl_amd/csrc/ppg_twins.hip: the three operators of csrc/ppg.hip and
// the split optimiser step of csrc/optim.hip) for the address and undefined-behaviour sanitizers: its own main, every buffer a heap allocation of
// exactly the size the C ABI names.  (T, n, R, A) = (1, 1, 3, 2), (7, 1, 2, 15), (9, 4, 6, 30) and (64, 4, 5, 15) -- one row, one below a
// tile of 8 rows, past a tile, many tiles -- with cols unsorted, one of them out of range (clamped), an old row with a logit 120 below
// its maximum and one with -inf, accumulate 0 then 1.  It checks what it can without a reference: gathered bytes are byte / 255, the
// written aux_pi rows are normalised and the others untouched, the losses are finite and non-negative, every row of the logit
// gradient sums to zero (so the actor's bias gradient does), accumulate adds exactly, the split step equals, on each of its
// ranges, the step that puts the whole buffer on that side, and zeroes the gradient, and the refusals return MI355PPO_EINVAL.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/ppg_host_check.cpp \
//       cleanrl_amd/csrc/ppg_twins.hip cleanrl_amd/csrc/api.hip -o tools/ppg_host_check && tools/ppg_host_check
//
// (without the three -Xarch_host flags: a plain build).  Never loaded into python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mi355ppo.h"

namespace {

constexpr int kH = 256;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
float rndf() { return (float)((rnd() & 0xFFFFFF) / (double)(1 << 24) - 0.5); }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: a=%d b=%d: %s\n", __FILE__, __LINE__, ca, cb, #cond); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int run_case(int T, int n, int R, int A) {
    const int ca = T * n, cb = A, M = T * n;
    const int64_t row_bytes = 12;
    std::vector<int64_t> cols(n);
    for (int i = 0; i < n; ++i) cols[i] = R - 2 - i;                             // descending: unsorted, distinct, R - 1 left free
    if (n > 1) cols[n - 1] = R + 5;                                              // out of range: clamped onto R - 1
    const auto col = [&](int i) { return cols[i] >= R ? (int64_t)R - 1 : cols[i]; };
    // ---- gather
    std::vector<uint8_t> obs((size_t)T * R * row_bytes);
    for (auto& v : obs) v = (uint8_t)rnd();
    std::vector<float> x((size_t)M * row_bytes);
    CHECK(mi355ppo_ppg_aux_gather_u8_f32_cpu(obs.data(), cols.data(), x.data(), T, n, R, row_bytes) == 0);
    for (int r = 0; r < M; ++r)
        for (int k = 0; k < row_bytes; ++k)
            CHECK(x[(size_t)r * row_bytes + k] == (float)obs[((size_t)(r / n) * R + col(r % n)) * row_bytes + k] / 255.0f);
    CHECK(mi355ppo_ppg_aux_gather_u8_f32_cpu(obs.data(), cols.data(), x.data(), T, n, R, 10) == MI355PPO_EINVAL);
    // ---- old logits
    std::vector<float> h((size_t)M * kH), wa((size_t)A * kH), ba(A), wc(kH), bc(1), wx(kH), bx(1), pi((size_t)T * R * A, 7.0f), ret((size_t)T * R);
    for (auto& v : h) v = std::fabs(rndf());
    for (auto* w : {&wa, &ba, &wc, &bc, &wx, &bx, &ret})
        for (auto& v : *w) v = 0.3f * rndf();
    CHECK(mi355ppo_ppg_old_logits_f32_cpu(h.data(), wa.data(), ba.data(), cols.data(), pi.data(), T, n, R, A, kH) == 0);
    std::vector<char> written((size_t)T * R, 0);
    for (int r = 0; r < M; ++r) written[(size_t)(r / n) * R + col(r % n)] = 1;
    for (int64_t s = 0; s < (int64_t)T * R; ++s) {
        double p = 0.0;
        for (int j = 0; j < A; ++j) {
            if (!written[s]) CHECK(pi[s * A + j] == 7.0f);
            p += std::exp((double)pi[s * A + j]);
        }
        if (written[s]) CHECK(std::fabs(p - 1.0) < 1e-5);
        if (!written[s])
            for (int j = 0; j < A; ++j) pi[s * A + j] = rndf();                  // the loss reads only the cols' rows; fill the rest anyway
    }
    CHECK(mi355ppo_ppg_old_logits_f32_cpu(h.data(), wa.data(), ba.data(), cols.data(), pi.data(), T, n, R, 31, kH) == MI355PPO_EINVAL);
    CHECK(mi355ppo_ppg_old_logits_f32_cpu(h.data(), wa.data(), ba.data(), cols.data(), pi.data(), T, n, R, 1, kH) == MI355PPO_EINVAL);
    CHECK(mi355ppo_ppg_old_logits_f32_cpu(h.data(), wa.data(), ba.data(), cols.data(), pi.data(), T, n, R, A, 128) == MI355PPO_EINVAL);
    // ---- the loss: a logit 120 below the row's maximum, and -inf
    float* row0 = pi.data() + ((size_t)0 * R + col(0)) * A;
    float mx = row0[0];
    for (int j = 1; j < A; ++j) mx = row0[j] > mx ? row0[j] : mx;
    row0[A - 1] = mx - 120.0f;
    if (T > 1) pi[((size_t)(T - 1) * R + col(0)) * A] = -std::numeric_limits<float>::infinity();
    for (auto& v : wa) v = rndf();                                               // a new policy that differs from the stored one
    std::vector<float> sc(3), dh((size_t)M * kH), dwa((size_t)A * kH), dba(A), dwc(kH), dbc(1), dwx(kH), dbx(1);
    CHECK(mi355ppo_ppg_aux_fwd_bwd_f32_cpu(h.data(), wa.data(), ba.data(), wc.data(), bc.data(), wx.data(), bx.data(), pi.data(), ret.data(),
                                           cols.data(), T, n, R, A, kH, 0.5, 0.5, sc.data(), dh.data(), dwa.data(), dba.data(), dwc.data(),
                                           dbc.data(), dwx.data(), dbx.data(), 0) == 0);
    for (int q = 0; q < 3; ++q) CHECK(std::isfinite(sc[q]) && sc[q] >= (q == 0 ? -1e-6f : 0.0f));
    for (auto& v : dh) CHECK(std::isfinite(v));
    double sum_db = 0.0;
    for (int j = 0; j < A; ++j) sum_db += dba[j];
    CHECK(std::fabs(sum_db) < 1e-5);                                             // p_new and p_old both sum to one in every row
    const std::vector<float> dwa0 = dwa, dba0 = dba, dwc0 = dwc, dbc0 = dbc, dwx0 = dwx, dbx0 = dbx;
    CHECK(mi355ppo_ppg_aux_fwd_bwd_f32_cpu(h.data(), wa.data(), ba.data(), wc.data(), bc.data(), wx.data(), bx.data(), pi.data(), ret.data(),
                                           cols.data(), T, n, R, A, kH, 0.5, 0.5, sc.data(), dh.data(), dwa.data(), dba.data(), dwc.data(),
                                           dbc.data(), dwx.data(), dbx.data(), 1) == 0);
    for (size_t i = 0; i < dwa.size(); ++i) CHECK(dwa[i] == dwa0[i] + dwa0[i]);
    for (int j = 0; j < A; ++j) CHECK(dba[j] == dba0[j] + dba0[j]);
    for (int k = 0; k < kH; ++k) CHECK(dwc[k] == dwc0[k] + dwc0[k] && dwx[k] == dwx0[k] + dwx0[k]);
    CHECK(dbc[0] == dbc0[0] + dbc0[0] && dbx[0] == dbx0[0] + dbx0[0]);
    CHECK(mi355ppo_ppg_aux_fwd_bwd_f32_cpu(h.data(), wa.data(), ba.data(), wc.data(), bc.data(), wx.data(), bx.data(), pi.data(), ret.data(),
                                           cols.data(), T, n, R, A, kH, 0.5, 0.5, sc.data(), dh.data(), dwa.data(), dba.data(), dwc.data(),
                                           dbc.data(), dwx.data(), dbx.data(), 2) == MI355PPO_EINVAL);
    return 0;
}

int run_split(int64_t n, int64_t n_split) {
    const int ca = (int)n, cb = (int)n_split;
    std::vector<float> p(n), g(n), m(n), v(n);
    for (int64_t i = 0; i < n; ++i) p[i] = rndf(), g[i] = rndf(), m[i] = 0.01f * rndf(), v[i] = 1e-3f * std::fabs(rndf());
    std::vector<float> p1 = p, g1 = g, m1 = m, v1 = v, p2 = p, g2 = g, m2 = m, v2 = v;
    float norm = 0.0f, norm1 = 0.0f;
    CHECK(mi355ppo_clip_adam_split_f32_cpu(p.data(), g.data(), m.data(), v.data(), n, n_split, 0.5, 0.5, 5e-4, 0.9, 0.999, 1e-8, 7, 3, &norm) == 0);
    CHECK(mi355ppo_clip_adam_split_f32_cpu(p1.data(), g1.data(), m1.data(), v1.data(), n, n, 0.5, 0.5, 5e-4, 0.9, 0.999, 1e-8, 7, 1, &norm1) == 0);
    CHECK(mi355ppo_clip_adam_split_f32_cpu(p2.data(), g2.data(), m2.data(), v2.data(), n, 0, 0.5, 0.5, 5e-4, 0.9, 0.999, 1e-8, 1, 3, nullptr) == 0);
    CHECK(norm == norm1);
    for (int64_t i = 0; i < n; ++i) {
        const bool head = i < n_split;
        CHECK(p[i] == (head ? p1[i] : p2[i]) && m[i] == (head ? m1[i] : m2[i]) && v[i] == (head ? v1[i] : v2[i]) && g[i] == 0.0f);
    }
    CHECK(mi355ppo_clip_adam_split_f32_cpu(p.data(), g.data(), m.data(), v.data(), n, n + 1, 0.5, 0.5, 5e-4, 0.9, 0.999, 1e-8, 7, 3, nullptr) ==
          MI355PPO_EINVAL);
    CHECK(mi355ppo_clip_adam_split_f32_cpu(p.data(), g.data(), m.data(), v.data(), n, n_split, 0.5, 0.5, 5e-4, 0.9, 0.999, 1e-8, 0, 3, nullptr) ==
          MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    if (run_case(1, 1, 3, 2) || run_case(7, 1, 2, 15) || run_case(9, 4, 6, 30) || run_case(64, 4, 5, 15)) return 1;
    if (run_split(1, 0) || run_split(5, 5) || run_split(1001, 700) || run_split(4100, 4)) return 1;
    printf("ppg host check: ok\n");
    return 0;
}
