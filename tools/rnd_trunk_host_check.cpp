// Stand-alone driver of the LeakyReLU host twins (cleanrl_amd/csrc/leaky_twins.hip) for the address and undefined-behaviour sanitizers: its
// own main, every buffer a heap allocation of exactly the size the C ABI names -- n floats, (n + 31) / 32 mask words, one amax record.
// n = 1, 13, 32, 33, 1000 and 12,800 (one element, less than a word, a word, one past it, no multiple of 32, conv1's row), out of place and in
// place, with and without mask bits and records.  It checks what it can without a reference: a = z > 0 ? z : z * 0.01f, the bits are z > 0
// with the bits past n zero, the records hold max |a| / max |dz|, dz = bit ? da : da * 0.01f, -0 stays -0, and the refusals return
// MI355PPO_EINVAL.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/rnd_trunk_host_check.cpp \
//       cleanrl_amd/csrc/leaky_twins.hip cleanrl_amd/csrc/api.hip -o tools/rnd_trunk_host_check && tools/rnd_trunk_host_check
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

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: n=%d in_place=%d: %s\n", __FILE__, __LINE__, n, (int)in_place, #cond); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

uint32_t bits_of(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

int run_leaky(int n, bool in_place, bool extras) {
    const float slope = 0.01f;
    const size_t words = ((size_t)n + 31) / 32;
    std::vector<float> z((size_t)n), da((size_t)n);
    for (auto& v : z) v = rndf() * 4.0f;
    for (auto& v : da) v = rndf();
    z[0] = -0.0f;
    if (n > 3) { z[1] = 0.0f; z[2] = -1.401298464e-45f; z[3] = 1.401298464e-45f; }
    const std::vector<float> z0 = z, da0 = da;
    std::vector<float> a_buf(in_place ? 0 : (size_t)n), dz_buf(in_place ? 0 : (size_t)n);
    float* const a = in_place ? z.data() : a_buf.data();
    float* const dz = in_place ? da.data() : dz_buf.data();
    std::vector<uint32_t> bits(words, 0xFFFFFFFFu), rec(MI355PPO_AMAX_WORDS, 0u), rec2(MI355PPO_AMAX_WORDS, 0u);
    CHECK(mi355ppo_leaky_relu_fwd_f32_cpu(z.data(), a, bits.data(), extras ? rec.data() : nullptr, n, 0.01) == 0);
    float amax = 0.0f;
    for (int e = 0; e < n; ++e) {
        const float want = z0[e] > 0.0f ? z0[e] : z0[e] * slope;
        CHECK(bits_of(a[e]) == bits_of(want));
        CHECK(((bits[(size_t)e >> 5] >> (e & 31)) & 1u) == (z0[e] > 0.0f ? 1u : 0u));
        amax = fmaxf(amax, fabsf(want));
    }
    for (size_t e = (size_t)n; e < 32 * words; ++e) CHECK(((bits[e >> 5] >> (e & 31)) & 1u) == 0u);
    CHECK(bits_of(a[0]) == 0x80000000u);                                         // -0 * 0.01f = -0
    if (extras) CHECK(rec[0] == bits_of(amax));
    CHECK(mi355ppo_leaky_relu_bwd_f32_cpu(da.data(), bits.data(), dz, extras ? rec2.data() : nullptr, n, 0.01) == 0);
    float dmax = 0.0f;
    for (int e = 0; e < n; ++e) {
        const float want = z0[e] > 0.0f ? da0[e] : da0[e] * slope;
        CHECK(bits_of(dz[e]) == bits_of(want));
        dmax = fmaxf(dmax, fabsf(want));
    }
    if (extras) CHECK(rec2[0] == bits_of(dmax));
    if (!extras) {                                                               // the forward without mask bits: the same values
        std::vector<float> b((size_t)n);
        CHECK(mi355ppo_leaky_relu_fwd_f32_cpu(z0.data(), b.data(), nullptr, nullptr, n, 0.01) == 0);
        for (int e = 0; e < n; ++e) CHECK(bits_of(b[e]) == bits_of(z0[e] > 0.0f ? z0[e] : z0[e] * slope));
    }
    CHECK(mi355ppo_leaky_relu_fwd_f32_cpu(z.data(), a, nullptr, nullptr, 0, 0.01) == MI355PPO_EINVAL);
    CHECK(mi355ppo_leaky_relu_fwd_f32_cpu(nullptr, a, nullptr, nullptr, n, 0.01) == MI355PPO_EINVAL);
    CHECK(mi355ppo_leaky_relu_bwd_f32_cpu(da.data(), nullptr, dz, nullptr, n, 0.01) == MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    const int sizes[] = {1, 13, 32, 33, 1000, 12800};
    for (int n : sizes)
        for (int in_place = 0; in_place < 2; ++in_place)
            for (int extras = 0; extras < 2; ++extras)
                if (run_leaky(n, in_place != 0, extras != 0)) return 1;
    printf("rnd_trunk_host_check: ok\n");
    return 0;
}
