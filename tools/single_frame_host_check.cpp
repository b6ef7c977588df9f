// Stand-alone driver of the host twins of the one-frame conv1 kernels (kernel Q1's pack, pre-activation forward and ReLU forward,
// cleanrl_amd/csrc/ma_atari_twins.hip) for the address and undefined-behaviour sanitizers: its own main, every buffer a heap allocation of
// exactly the size the C ABI names -- the frames exactly rows x 7,056 bytes, so a load past the last tap row of the last pixel is a report.
// 1 image, 3 images gathered with inds = {3, 0, 3} from 4 stored frames, and 5 images in place.  It checks what it can without a library
// reference: every pre-activation against a plain double convolution of the same bytes (1e-5), equal rows for equal source frames, a
// negative pre-activation somewhere, an all-zero weight giving the bias exactly, an all-255 frame under a one-hot weight giving w + bias to
// within the fixed-point step, and the refusals returning MI355PPO_EINVAL.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/single_frame_host_check.cpp \
//       cleanrl_amd/csrc/ma_atari_twins.hip cleanrl_amd/csrc/api.hip -o tools/single_frame_host_check && tools/single_frame_host_check
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

#define CHECK(cond)                                                                              \
    do {                                                                                         \
        if (!(cond)) {                                                                           \
            fprintf(stderr, "%s:%d: images=%d stored=%d: %s\n", __FILE__, __LINE__, images, stored, #cond); \
            return 1;                                                                            \
        }                                                                                        \
    } while (0)

constexpr int kImg = 84 * 84, kOut = 20 * 20 * 32;

int run(int images, int stored, const int64_t* inds) {
    const size_t pack_bytes = 8832;                                              // mi355ppo_cnn_conv1q1_pack_bytes() (csrc/conv1q1_pack.h: kQ1PackBytes)
    std::vector<uint8_t> frames((size_t)stored * kImg);
    for (auto& v : frames) v = (uint8_t)rnd();
    std::vector<float> W(32 * 64), bias(32), z((size_t)images * kOut);
    for (auto& v : W) v = 0.1f * rndf();
    for (auto& v : bias) v = rndf();
    std::vector<unsigned char> pack(pack_bytes);
    CHECK(mi355ppo_cnn_conv1q1_pack_cpu(W.data(), pack.data()) == 0);
    CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), z.data(), images) == 0);
    bool negative = false;
    for (int i = 0; i < images; ++i) {
        const uint8_t* f = frames.data() + (size_t)(inds ? inds[i] : i) * kImg;
        for (int p = 0; p < 400; ++p)
            for (int n = 0; n < 32; ++n) {
                double s = 0.0;
                for (int kh = 0; kh < 8; ++kh)
                    for (int kw = 0; kw < 8; ++kw) s += (double)W[(n * 8 + kh) * 8 + kw] * f[(4 * (p / 20) + kh) * 84 + 4 * (p % 20) + kw];
                const float got = z[((size_t)i * 400 + p) * 32 + n];
                CHECK(std::isfinite(got) && std::fabs((double)got - (s / 255.0 + bias[n])) <= 1e-5);
                negative = negative || got < 0.0f;
            }
    }
    CHECK(negative);
    {   // the ReLU twin: max(pre-activation, 0) to the bit, mask words of exactly images x 400 words, the maximum folded into slot 0 of a record
        std::vector<float> a((size_t)images * kOut);
        std::vector<uint32_t> bits((size_t)images * 400, 0xFFFFFFFFu), rec(256, 0u);
        CHECK(mi355ppo_cnn_conv1q1_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), a.data(), bits.data(), rec.data(), images) == 0);
        float amax = 0.0f;
        for (size_t e = 0; e < a.size(); ++e) {
            const float want = z[e] > 0.0f ? z[e] : 0.0f;
            CHECK(memcmp(&a[e], &want, 4) == 0);
            CHECK(((bits[e >> 5] >> (e & 31)) & 1u) == (want > 0.0f ? 1u : 0u));
            amax = want > amax ? want : amax;
        }
        CHECK(amax > 0.0f && memcmp(&rec[0], &amax, 4) == 0);
        for (int w = 1; w < 256; ++w) CHECK(rec[w] == 0u);
        std::vector<float> again((size_t)images * kOut);                          // neither mask words nor a record
        CHECK(mi355ppo_cnn_conv1q1_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), again.data(), nullptr, nullptr, images) == 0);
        CHECK(memcmp(again.data(), a.data(), a.size() * 4) == 0);
        CHECK(mi355ppo_cnn_conv1q1_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), a.data(), nullptr, nullptr, 0) == MI355PPO_EINVAL);
        CHECK(mi355ppo_cnn_conv1q1_fwd_cpu(frames.data(), inds, nullptr, bias.data(), a.data(), nullptr, nullptr, images) == MI355PPO_EINVAL);
    }
    if (inds)
        for (int i = 1; i < images; ++i)
            if (inds[i] == inds[0]) CHECK(memcmp(z.data(), z.data() + (size_t)i * kOut, (size_t)kOut * 4) == 0);
    {   // all-zero weight: the bias exactly; a one-hot weight on the last tap of an all-255 frame: w + bias
        std::vector<float> W0(32 * 64, 0.0f);
        CHECK(mi355ppo_cnn_conv1q1_pack_cpu(W0.data(), pack.data()) == 0);
        CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), z.data(), images) == 0);
        for (size_t e = 0; e < z.size(); ++e) CHECK(z[e] == bias[e & 31]);
        for (int n = 0; n < 32; ++n) W0[n * 64 + 63] = 0.25f + 0.01f * (float)n;
        std::vector<uint8_t> white((size_t)stored * kImg, 255);
        CHECK(mi355ppo_cnn_conv1q1_pack_cpu(W0.data(), pack.data()) == 0);
        CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(white.data(), inds, pack.data(), bias.data(), z.data(), images) == 0);
        for (size_t e = 0; e < z.size(); ++e) CHECK(std::fabs((double)z[e] - ((double)W0[(e & 31) * 64 + 63] + bias[e & 31])) <= 1e-6);
    }
    // refusals
    CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), z.data(), 0) == MI355PPO_EINVAL);
    CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(nullptr, inds, pack.data(), bias.data(), z.data(), images) == MI355PPO_EINVAL);
    CHECK(mi355ppo_cnn_conv1q1_pre_fwd_cpu(frames.data(), inds, pack.data(), bias.data(), nullptr, images) == MI355PPO_EINVAL);
    CHECK(mi355ppo_cnn_conv1q1_pack_cpu(nullptr, pack.data()) == MI355PPO_EINVAL);
    CHECK(mi355ppo_cnn_conv1q1_pack_cpu(W.data(), nullptr) == MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    const int64_t inds[3] = {3, 0, 3};
    if (run(1, 1, nullptr) || run(3, 4, inds) || run(5, 5, nullptr)) return 1;
    printf("single_frame_host_check: ok\n");
    return 0;
}
