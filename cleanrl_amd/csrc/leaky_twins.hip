// Host-pointer twins of the LeakyReLU kernels (leaky.hip): the element math is leaky_rows.h's own, compiled for the host -- a twin returns
// the device's bits.  A file of its own (as layernorm_twins.hip), so that tools/rnd_trunk_host_check.cpp builds it stand-alone for the
// sanitizers.  Serial.
#include "common.h"
#include "leaky_rows.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

#pragma clang fp contract(off)

using namespace mi355ppo;

namespace {

// the record's slot 0 |= bits of m (the device spreads its waves' maxima over the 16 slots; the record's value is their maximum)
void leaky_amax_fold_host(uint32_t* rec, float m) {
    uint32_t b;
    memcpy(&b, &m, 4);
    if (b > rec[0]) rec[0] = b;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_leaky_relu_fwd_f32_cpu(const float* z, float* a, uint32_t* mask_bits, uint32_t* a_amax, int64_t n,
                                                            double slope) {
    const char* fn = "mi355ppo_leaky_relu_fwd_f32_cpu";
    MI355_REQUIRE(z && a, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld (n > 0)", fn, (long long)n);
    const float s = (float)slope;
    float amax = 0.0f;
    for (int64_t w = 0; w * 32 < n; ++w) {
        uint32_t word = 0u;
        for (int b = 0; b < 32 && w * 32 + b < n; ++b) {
            const float v = z[w * 32 + b];           // (read before a is written: the twin may work in place too)
            const float o = leaky_fwd(v, s);
            a[w * 32 + b] = o;
            if (v > 0.0f) word |= 1u << b;
            amax = fmaxf(amax, fabsf(o));            // (a NaN is not recorded)
        }
        if (mask_bits) mask_bits[w] = word;
    }
    if (a_amax) leaky_amax_fold_host(a_amax, amax);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_leaky_relu_bwd_f32_cpu(const float* da, const uint32_t* mask_bits, float* dz, uint32_t* dz_amax, int64_t n,
                                                            double slope) {
    const char* fn = "mi355ppo_leaky_relu_bwd_f32_cpu";
    MI355_REQUIRE(da && mask_bits && dz, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld (n > 0)", fn, (long long)n);
    const float s = (float)slope;
    float amax = 0.0f;
    for (int64_t e = 0; e < n; ++e) {
        const float o = leaky_bwd(da[e], (mask_bits[e >> 5] >> (e & 31)) & 1u, s);
        dz[e] = o;
        amax = fmaxf(amax, fabsf(o));
    }
    if (dz_amax) leaky_amax_fold_host(dz_amax, amax);
    return MI355PPO_OK;
}
