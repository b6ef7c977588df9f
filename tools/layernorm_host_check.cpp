// Stand-alone driver of the LayerNorm + ReLU host twins (cleanrl_amd/csrc/layernorm_twins.hip) and of kernel Q's pre-activation twin
// (cleanrl_amd/csrc/ma_atari_twins.hip) for the address and undefined-behaviour sanitizers: its own main, every buffer a heap allocation of
// exactly the size the C ABI names.  (rows, C, HW) = (1, 512, 1), (3, 64, 49), (5, 32, 400), (70, 64, 81) and (257, 512, 1) -- every row
// size of pqn_atari_envpool.py's network, one row, several forward workgroups, several backward slabs --, with and without mask bits, amax
// records and the act mask.  It checks what it can without a reference: a constant row gives relu(beta) exactly, the mask bits are a > 0,
// the amax records hold max a / max |dz|, every row of dz sums to (nearly) zero against gamma's spread, dbeta is the column sum of the
// masked dy, relu of the pre-activation is the ReLU forward twin's result bit for bit, and the refusals return MI355PPO_EINVAL.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/layernorm_host_check.cpp \
//       cleanrl_amd/csrc/layernorm_twins.hip cleanrl_amd/csrc/ma_atari_twins.hip cleanrl_amd/csrc/api.hip \
//       -o tools/layernorm_host_check && tools/layernorm_host_check
//
// (without the three -Xarch_host flags: a plain build).  Never loaded into python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mi355ppo.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
float rndf() { return (float)((rnd() & 0xFFFFFF) / (double)(1 << 24) - 0.5); }

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            fprintf(stderr, "%s:%d: rows=%d C=%d HW=%d: %s\n", __FILE__, __LINE__, rows, C, HW, #cond); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

float rec_value(const std::vector<uint32_t>& rec) {
    uint32_t m = 0;
    for (size_t i = 0; i < rec.size(); i += 16) m = rec[i] > m ? rec[i] : m;
    float f;
    memcpy(&f, &m, 4);
    return f;
}

int run_layernorm(int rows, int C, int HW, bool act_mask) {
    const int D = C * HW;
    const size_t n = (size_t)rows * D;
    std::vector<float> z(n), gamma(D), beta(D), dy(n), a(n), mean(rows), rstd(rows), dz(n), dg(D), db(D);
    for (auto& v : z) v = 4.0f * rndf() + 0.5f;
    for (auto& v : gamma) v = 1.0f + 0.4f * rndf();
    for (auto& v : beta) v = 0.6f * rndf();
    for (auto& v : dy) v = 2.0f * rndf();
    const int crow = rows / 2;
    for (int e = 0; e < D; ++e) z[(size_t)crow * D + e] = 1.7f;                  // a constant row: var = 0
    std::vector<uint32_t> bits(n / 32, 0xFFFFFFFFu), rec(MI355PPO_AMAX_WORDS, 0u), rec2(MI355PPO_AMAX_WORDS, 0u);
    CHECK(mi355ppo_layernorm_relu_fwd_f32_cpu(z.data(), gamma.data(), beta.data(), a.data(), mean.data(), rstd.data(), bits.data(), rec.data(),
                                              rows, C, HW, 1e-5) == 0);
    float amax = 0.0f;
    for (size_t f = 0; f < n; ++f) {
        CHECK(a[f] >= 0.0f && std::isfinite(a[f]));
        CHECK(((bits[f >> 5] >> (f & 31)) & 1u) == (a[f] > 0.0f ? 1u : 0u));
        amax = a[f] > amax ? a[f] : amax;
    }
    CHECK(rec_value(rec) == amax);
    for (int e = 0; e < D; ++e) {
        const int p = e / C, c = e - p * C;
        const float b = beta[(size_t)c * HW + p];
        CHECK(a[(size_t)crow * D + e] == (b > 0.0f ? b : 0.0f));
    }
    {                                                                             // without bits and record: the same activations
        std::vector<float> a2(n), m2(rows), r2(rows);
        CHECK(mi355ppo_layernorm_relu_fwd_f32_cpu(z.data(), gamma.data(), beta.data(), a2.data(), m2.data(), r2.data(), nullptr, nullptr, rows, C,
                                                  HW, 1e-5) == 0);
        CHECK(memcmp(a.data(), a2.data(), n * 4) == 0 && memcmp(mean.data(), m2.data(), (size_t)rows * 4) == 0);
    }
    if (!act_mask)
        for (size_t f = 0; f < n; ++f) dy[f] = a[f] > 0.0f ? dy[f] : 0.0f;
    CHECK(mi355ppo_layernorm_relu_bwd_f32_cpu(dy.data(), act_mask ? a.data() : nullptr, z.data(), mean.data(), rstd.data(), gamma.data(), dz.data(),
                                              dg.data(), db.data(), rec2.data(), rows, C, HW) == 0);
    float dmax = 0.0f;
    for (int r = 0; r < rows; ++r) {
        double s = 0.0, sa = 0.0;
        for (int e = 0; e < D; ++e) {
            const float v = dz[(size_t)r * D + e];
            CHECK(std::isfinite(v));
            s += v;
            sa += std::fabs(v);
            dmax = std::fabs(v) > dmax ? std::fabs(v) : dmax;
        }
        CHECK(std::fabs(s) <= 1e-5 * (sa + 1.0));                                 // dz is orthogonal to the constant vector
    }
    CHECK(rec_value(rec2) == dmax);
    for (int e = 0; e < D; ++e) {
        const int p = e / C, c = e - p * C;
        double s = 0.0;
        for (int r = 0; r < rows; ++r) s += (a[(size_t)r * D + e] > 0.0f) ? dy[(size_t)r * D + e] : 0.0f;
        CHECK(std::fabs((double)db[(size_t)c * HW + p] - s) <= 1e-5 * (std::fabs(s) + 1.0));
        CHECK(std::isfinite(dg[(size_t)c * HW + p]));
    }
    // refusals
    CHECK(mi355ppo_layernorm_relu_fwd_f32_cpu(nullptr, gamma.data(), beta.data(), a.data(), mean.data(), rstd.data(), nullptr, nullptr, rows, C, HW,
                                              1e-5) == MI355PPO_EINVAL);
    CHECK(mi355ppo_layernorm_relu_fwd_f32_cpu(z.data(), gamma.data(), beta.data(), a.data(), mean.data(), rstd.data(), nullptr, nullptr, 0, C, HW,
                                              1e-5) == MI355PPO_EINVAL);
    CHECK(mi355ppo_layernorm_relu_fwd_f32_cpu(z.data(), gamma.data(), beta.data(), a.data(), mean.data(), rstd.data(), nullptr, nullptr, rows, 6, HW,
                                              1e-5) == MI355PPO_EINVAL);
    CHECK(mi355ppo_layernorm_relu_bwd_f32_cpu(dy.data(), nullptr, z.data(), mean.data(), rstd.data(), gamma.data(), dz.data(), dg.data(), db.data(),
                                              nullptr, rows, 32768, 1) == MI355PPO_EINVAL);
    return 0;
}

int run_conv1q_pre(int images, bool with_inds) {
    const int rows = images, C = 4, HW = 84 * 84;                                // (for CHECK's message)
    const int src_rows = with_inds ? images + 2 : images;
    std::vector<uint8_t> frames((size_t)src_rows * 84 * 84 * 4);
    for (auto& v : frames) v = (uint8_t)rnd();
    std::vector<int64_t> inds(images);
    for (int i = 0; i < images; ++i) inds[i] = (int64_t)(rnd() % (uint32_t)src_rows);
    std::vector<float> W(32 * 4 * 8 * 8), bias(32), pre((size_t)images * 12800), act((size_t)images * 12800);
    for (auto& v : W) v = 0.1f * rndf();
    for (auto& v : bias) v = rndf();
    std::vector<unsigned char> pack(33408);                                      // mi355ppo_cnn_conv1q_pack_bytes() (csrc/conv1q_pack.h: kQPackBytes)
    CHECK(mi355ppo_cnn_conv1q_pack_cpu(W.data(), pack.data()) == 0);
    const int64_t* ip = with_inds ? inds.data() : nullptr;
    CHECK(mi355ppo_cnn_conv1q_pre_fwd_cpu(frames.data(), ip, pack.data(), bias.data(), pre.data(), images) == 0);
    CHECK(mi355ppo_cnn_conv1q_fwd_cpu(frames.data(), ip, pack.data(), bias.data(), act.data(), nullptr, images) == 0);
    bool negative = false;
    for (size_t f = 0; f < pre.size(); ++f) {
        negative = negative || pre[f] < 0.0f;
        CHECK((pre[f] > 0.0f ? pre[f] : 0.0f) == act[f]);
    }
    CHECK(negative);
    CHECK(mi355ppo_cnn_conv1q_pre_fwd_cpu(frames.data(), ip, pack.data(), bias.data(), pre.data(), 0) == MI355PPO_EINVAL);
    CHECK(mi355ppo_cnn_conv1q_pre_fwd_cpu(nullptr, ip, pack.data(), bias.data(), pre.data(), images) == MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    const int shapes[][3] = {{1, 512, 1}, {3, 64, 49}, {5, 32, 400}, {70, 64, 81}, {257, 512, 1}};
    for (const auto& s : shapes)
        for (int act = 0; act < 2; ++act)
            if (run_layernorm(s[0], s[1], s[2], act != 0)) return 1;
    if (run_conv1q_pre(1, false) || run_conv1q_pre(3, true)) return 1;
    printf("layernorm_host_check: ok\n");
    return 0;
}
