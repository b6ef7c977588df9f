// Stand-alone driver of the host twins of the fused ppo_pettingzoo_ma_atari path (cleanrl_amd/csrc/ma_atari_twins.hip: the store-time split,
// kernel Q's pack with the tap sums, its forward with the per-observation bias, the weight-gradient fold) for the address and
// undefined-behaviour sanitizers: its own main, every buffer a heap allocation of exactly the size the C ABI names.  M = 1, 3 and 33
// images out of M + 2 stored rows, gathered through a permuted `inds` and without one, indicator bytes (1, 0), (0, 1), (0, 0), (3, 250).
// It checks what it can without a reference: the split's rows and bytes, the flag (clean, one deviating byte at the last pixel of plane 5
// and at pixel (0, 1) of plane 4, and that a clean store leaves it set), the six-channel pack against the pack of the contiguous
// four-channel slice, the forward with all-zero indicator bytes against the plain forward bit for bit, every output against a direct
// double-precision sum, the fold's channels 0 - 3 as copies and its channels 4 / 5 as one value per (output channel, plane) that a
// second run reproduces, and the refusals.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/ma_atari_host_check.cpp \
//       cleanrl_amd/csrc/ma_atari_twins.hip cleanrl_amd/csrc/api.hip -o tools/ma_atari_host_check && tools/ma_atari_host_check
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

constexpr int kPix = 84 * 84, kPackBytes = 33408;
const uint8_t kMix[4][2] = {{1, 0}, {0, 1}, {0, 0}, {3, 250}};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
float rndf() { return (float)((rnd() & 0xFFFFFF) / (double)(1 << 24) - 0.5); }

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: M=%d inds=%d: %s\n", __FILE__, __LINE__, M, (int)gather, #cond); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int run_case(int M, bool gather) {
    const int R = M + 2;
    std::vector<uint8_t> frames((size_t)R * kPix * 6);
    for (auto& v : frames) v = (uint8_t)rnd();
    for (int f = 0; f < R; ++f)
        for (int p = 0; p < kPix; ++p) {
            frames[((size_t)f * kPix + p) * 6 + 4] = kMix[f % 4][0];
            frames[((size_t)f * kPix + p) * 6 + 5] = kMix[f % 4][1];
        }
    // ---- split
    std::vector<uint8_t> rows((size_t)R * kPix * 4), ind((size_t)R * 2);
    uint32_t flag = 0;
    CHECK(mi355ppo_ma_atari_split_u8_cpu(frames.data(), rows.data(), ind.data(), &flag, R) == 0 && flag == 0);
    for (int f = 0; f < R; ++f) {
        CHECK(ind[2 * f] == kMix[f % 4][0] && ind[2 * f + 1] == kMix[f % 4][1]);
        for (int p = 0; p < kPix; ++p) CHECK(memcmp(&rows[((size_t)f * kPix + p) * 4], &frames[((size_t)f * kPix + p) * 6], 4) == 0);
    }
    {
        std::vector<uint8_t> bad = frames, r2(rows.size()), i2(ind.size());
        bad[((size_t)(R - 1) * kPix + kPix - 1) * 6 + 5] ^= 1;
        uint32_t fl = 0;
        CHECK(mi355ppo_ma_atari_split_u8_cpu(bad.data(), r2.data(), i2.data(), &fl, R) == 0 && fl != 0 && r2 == rows && i2 == ind);
        CHECK(mi355ppo_ma_atari_split_u8_cpu(frames.data(), r2.data(), i2.data(), &fl, R) == 0 && fl != 0);      // sticky
        bad = frames;
        bad[(size_t)1 * 6 + 4] ^= 0x80;
        fl = 0;
        CHECK(mi355ppo_ma_atari_split_u8_cpu(bad.data(), r2.data(), i2.data(), &fl, R) == 0 && fl != 0);
        CHECK(mi355ppo_ma_atari_split_u8_cpu(frames.data(), r2.data(), i2.data(), nullptr, R) == MI355PPO_EINVAL);
        CHECK(mi355ppo_ma_atari_split_u8_cpu(frames.data(), r2.data(), i2.data(), &fl, 0) == MI355PPO_EINVAL);
    }
    // ---- pack
    std::vector<float> W6(32 * 6 * 64), W4(32 * 4 * 64), bias(32), tapsum(64);
    for (auto& v : W6) v = 0.1f * rndf();
    for (int n = 0; n < 32; ++n)
        for (int c = 0; c < 4; ++c) memcpy(&W4[(n * 4 + c) * 64], &W6[(n * 6 + c) * 64], 64 * sizeof(float));
    for (auto& v : bias) v = 0.2f * rndf();
    std::vector<uint8_t> pack(kPackBytes), pack4(kPackBytes);
    CHECK(mi355ppo_ma_atari_conv1_pack_f32_cpu(W6.data(), pack.data(), tapsum.data()) == 0);
    CHECK(mi355ppo_cnn_conv1q_pack_cpu(W4.data(), pack4.data()) == 0 && pack == pack4);
    for (int k = 0; k < 64; ++k) {
        double s = 0.0;
        for (int t = 0; t < 64; ++t) s += (double)W6[((k >> 1) * 6 + 4 + (k & 1)) * 64 + t];
        CHECK(tapsum[k] == (float)s);
    }
    CHECK(mi355ppo_ma_atari_conv1_pack_f32_cpu(W6.data(), pack.data(), nullptr) == MI355PPO_EINVAL);
    // ---- forward
    std::vector<int64_t> inds(M);
    for (int i = 0; i < M; ++i) inds[i] = R - 1 - i;                            // descending: the last M rows, permuted
    const int64_t* ip = gather ? inds.data() : nullptr;
    const auto row_of = [&](int i) { return gather ? (int)inds[i] : i; };
    std::vector<float> out((size_t)M * 400 * 32), out0(out.size()), outq(out.size());
    std::vector<uint32_t> bits((size_t)M * 400), bitsq(bits.size());
    std::vector<uint8_t> zero(ind.size(), 0);
    CHECK(mi355ppo_ma_atari_conv1_fwd_cpu(rows.data(), ip, ind.data(), pack.data(), tapsum.data(), bias.data(), out.data(), bits.data(), M) == 0);
    CHECK(mi355ppo_ma_atari_conv1_fwd_cpu(rows.data(), ip, zero.data(), pack.data(), tapsum.data(), bias.data(), out0.data(), nullptr, M) == 0);
    CHECK(mi355ppo_cnn_conv1q_fwd_cpu(rows.data(), ip, pack.data(), bias.data(), outq.data(), bitsq.data(), M) == 0);
    CHECK(memcmp(out0.data(), outq.data(), out.size() * sizeof(float)) == 0);
    for (int i = 0; i < M; ++i)
        for (int p = 0; p < 400; p += (i == 0 ? 1 : 57)) {                        // every pixel of the first image, a stride through the others
            const int gy = p / 20, gx = p % 20, r = row_of(i);
            uint32_t word = 0;
            for (int n = 0; n < 32; ++n) {
                double s = (double)bias[n] + (double)ind[2 * r] * tapsum[2 * n] + (double)ind[2 * r + 1] * tapsum[2 * n + 1];
                for (int c = 0; c < 4; ++c)
                    for (int kh = 0; kh < 8; ++kh)
                        for (int kw = 0; kw < 8; ++kw)
                            s += (double)rows[(((size_t)r * 84 + gy * 4 + kh) * 84 + gx * 4 + kw) * 4 + c] / 255.0 * W6[((n * 6 + c) * 8 + kh) * 8 + kw];
                const float got = out[((size_t)i * 400 + p) * 32 + n];
                CHECK(std::fabs((double)got - (s > 0.0 ? s : 0.0)) <= 1e-4);
                if (got > 0.0f) word |= 1u << n;
            }
            CHECK(bits[(size_t)i * 400 + p] == word);
        }
    CHECK(mi355ppo_ma_atari_conv1_fwd_cpu(rows.data(), ip, nullptr, pack.data(), tapsum.data(), bias.data(), out.data(), nullptr, M) == MI355PPO_EINVAL);
    CHECK(mi355ppo_ma_atari_conv1_fwd_cpu(rows.data(), ip, ind.data(), pack.data(), tapsum.data(), bias.data(), out.data(), nullptr, 0) == MI355PPO_EINVAL);
    // ---- fold
    std::vector<float> dz((size_t)M * 400 * 32), dW4(32 * 4 * 64), dW6(32 * 6 * 64, NAN), again(32 * 6 * 64, NAN);
    for (auto& v : dz) v = rndf();
    for (auto& v : dW4) v = rndf();
    CHECK(mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(dz.data(), ip, ind.data(), dW4.data(), dW6.data(), M) == 0);
    CHECK(mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(dz.data(), ip, ind.data(), dW4.data(), again.data(), M) == 0);
    CHECK(memcmp(dW6.data(), again.data(), dW6.size() * sizeof(float)) == 0);
    for (int n = 0; n < 32; ++n) {
        for (int c = 0; c < 4; ++c) CHECK(memcmp(&dW6[(n * 6 + c) * 64], &dW4[(n * 4 + c) * 64], 64 * sizeof(float)) == 0);
        for (int j = 0; j < 2; ++j) {
            double g = 0.0, mag = 0.0;
            for (int i = 0; i < M; ++i)
                for (int p = 0; p < 400; ++p) {
                    const double t = (double)ind[2 * row_of(i) + j] * dz[((size_t)i * 400 + p) * 32 + n];
                    g += t;
                    mag += std::fabs(t);
                }
            for (int t = 0; t < 64; ++t) CHECK(dW6[(n * 6 + 4 + j) * 64 + t] == dW6[(n * 6 + 4 + j) * 64]);
            CHECK(std::fabs((double)dW6[(n * 6 + 4 + j) * 64] - g) <= 1e-6 * (mag + 1.0));
        }
    }
    CHECK(mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(dz.data(), ip, ind.data(), dW4.data(), dW6.data(), 0) == MI355PPO_EINVAL);
    CHECK(mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(dz.data(), ip, ind.data(), nullptr, dW6.data(), M) == MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    for (int M : {1, 3, 33})
        for (bool gather : {false, true})
            if (run_case(M, gather)) return 1;
    printf("ma_atari host check: ok\n");
    return 0;
}
