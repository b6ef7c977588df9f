// Host-pointer twins of the LayerNorm + ReLU kernels (layernorm.hip): the element math is layernorm_rows.h's own, compiled for the host, and
// every sum runs in the device's order (a thread's quads ascending, ln_fold_host, the slabs ascending) -- a twin returns the device's bits.
// A file of its own (as ppg_twins.hip), so that tools/layernorm_host_check.cpp builds it stand-alone for the sanitizers.  Serial.
#include "common.h"
#include "layernorm_rows.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

#include <vector>

#pragma clang fp contract(off)

using namespace mi355ppo;

namespace {

int ln_check_host(const char* fn, int64_t rows, int C, int HW) {
    MI355_REQUIRE(rows > 0 && C > 0 && HW > 0 && C % 4 == 0 && (long long)C * HW <= kLnMaxD, MI355PPO_EINVAL,
                  "%s: rows=%lld C=%d HW=%d (rows > 0, C a positive multiple of 4, C * HW <= %d)", fn, (long long)rows, C, HW, kLnMaxD);
    return MI355PPO_OK;
}

// the record's slot 0 |= bits (the device spreads its waves' maxima over the 16 slots; the record's value is their maximum)
void amax_fold_host(uint32_t* rec, float m) {
    uint32_t b;
    memcpy(&b, &m, 4);
    if (b > rec[0]) rec[0] = b;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_layernorm_relu_fwd_f32_cpu(const float* z, const float* gamma, const float* beta, float* a, float* mean,
                                                                float* rstd, uint32_t* mask_bits, uint32_t* a_amax, int64_t rows, int C, int HW,
                                                                double eps) {
    const char* fn = "mi355ppo_layernorm_relu_fwd_f32_cpu";
    MI355_REQUIRE(z && gamma && beta && a && mean && rstd, MI355PPO_EINVAL, "%s: null pointer", fn);
    int rc = ln_check_host(fn, rows, C, HW);
    if (rc) return rc;
    const int D = C * HW;
    MI355_REQUIRE(!mask_bits || D % 32 == 0, MI355PPO_EINVAL, "%s: mask bits need C * HW %% 32 == 0 (%d)", fn, D);
    const LnShape sh = ln_shape(D);
    std::vector<double> v((size_t)sh.nt);
    float amax = 0.0f;
    for (int64_t r = 0; r < rows; ++r) {
        const float* zr = z + (size_t)r * D;
        for (int t = 0; t < sh.nt; ++t) {
            double s = 0.0;
            for (int k = 0; k < sh.kq; ++k) {
                const int e = 4 * (k * sh.nt + t);
                if (e < D)
                    for (int i = 0; i < 4; ++i) s = s + (double)zr[e + i];
            }
            v[(size_t)t] = s;
        }
        const double mean_d = ln_fold_host(v.data(), sh.nt) / (double)D;
        for (int t = 0; t < sh.nt; ++t) {
            double q = 0.0;
            for (int k = 0; k < sh.kq; ++k) {
                const int e = 4 * (k * sh.nt + t);
                if (e < D)
                    for (int i = 0; i < 4; ++i) {
                        const double d = (double)zr[e + i] - mean_d;
                        q = q + d * d;
                    }
            }
            v[(size_t)t] = q;
        }
        const double var_d = ln_fold_host(v.data(), sh.nt) / (double)D;
        const float m = (float)mean_d, rs = ln_rstd(var_d, (float)eps);
        mean[r] = m;
        rstd[r] = rs;
        for (int e = 0; e < D; ++e) {
            const int j = ln_param(e, C, HW);
            const float o = ln_out(zr[e], m, rs, gamma[j], beta[j]);
            a[(size_t)r * D + e] = o;
            amax = fmaxf(amax, o);
            if (mask_bits) {
                const size_t f = (size_t)r * D + e;
                if ((f & 31) == 0) mask_bits[f >> 5] = 0u;
                if (o > 0.0f) mask_bits[f >> 5] |= 1u << (f & 31);
            }
        }
    }
    if (a_amax) amax_fold_host(a_amax, amax);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_layernorm_relu_bwd_f32_cpu(const float* dy, const float* act, const float* z, const float* mean,
                                                                const float* rstd, const float* gamma, float* dz, float* dgamma, float* dbeta,
                                                                uint32_t* dz_amax, int64_t rows, int C, int HW) {
    const char* fn = "mi355ppo_layernorm_relu_bwd_f32_cpu";
    MI355_REQUIRE(dy && z && mean && rstd && gamma && dz && dgamma && dbeta, MI355PPO_EINVAL, "%s: null pointer", fn);
    int rc = ln_check_host(fn, rows, C, HW);
    if (rc) return rc;
    const int D = C * HW;
    const LnShape sh = ln_shape(D);
    const int slab_rows = ln_slab_rows(rows);
    const int64_t slabs = ln_slabs(rows);
    std::vector<double> v1((size_t)sh.nt), v2((size_t)sh.nt), tot((size_t)2 * D, 0.0);
    std::vector<float> sg((size_t)D), sb((size_t)D), xh((size_t)D), d((size_t)D), g((size_t)D);
    float amax = 0.0f;
    for (int64_t sl = 0; sl < slabs; ++sl) {
        for (int e = 0; e < D; ++e) sg[(size_t)e] = sb[(size_t)e] = 0.0f;
        for (int64_t r = sl * slab_rows; r < rows && r < (sl + 1) * slab_rows; ++r) {
            const size_t base = (size_t)r * D;
            const float m = mean[r], rs = rstd[r];
            for (int e = 0; e < D; ++e) {
                const float dd = (act && !(act[base + e] > 0.0f)) ? 0.0f : dy[base + e];
                d[(size_t)e] = dd;
                xh[(size_t)e] = ln_xhat(z[base + e], m, rs);
                g[(size_t)e] = dd * gamma[ln_param(e, C, HW)];
            }
            for (int t = 0; t < sh.nt; ++t) {
                double s1 = 0.0, s2 = 0.0;
                for (int k = 0; k < sh.kq; ++k) {
                    const int e = 4 * (k * sh.nt + t);
                    if (e < D) {
                        for (int i = 0; i < 4; ++i) s1 = s1 + (double)g[(size_t)e + i];
                        for (int i = 0; i < 4; ++i) s2 = s2 + (double)g[(size_t)e + i] * (double)xh[(size_t)e + i];
                    }
                }
                v1[(size_t)t] = s1;
                v2[(size_t)t] = s2;
            }
            const float m1 = (float)(ln_fold_host(v1.data(), sh.nt) / (double)D);
            const float m2 = (float)(ln_fold_host(v2.data(), sh.nt) / (double)D);
            for (int e = 0; e < D; ++e) {
                const float o = ln_dz(g[(size_t)e], xh[(size_t)e], rs, m1, m2);
                dz[base + e] = o;
                amax = fmaxf(amax, fabsf(o));
                sg[(size_t)e] = sg[(size_t)e] + d[(size_t)e] * xh[(size_t)e];
                sb[(size_t)e] = sb[(size_t)e] + d[(size_t)e];
            }
        }
        for (int e = 0; e < D; ++e) {          // the fold kernel: the slabs in ascending order, in double
            tot[(size_t)e] = tot[(size_t)e] + (double)sg[(size_t)e];
            tot[(size_t)D + e] = tot[(size_t)D + e] + (double)sb[(size_t)e];
        }
    }
    for (int e = 0; e < D; ++e) {
        const int j = ln_param(e, C, HW);
        dgamma[j] = (float)tot[(size_t)e];
        dbeta[j] = (float)tot[(size_t)D + e];
    }
    if (dz_amax) amax_fold_host(dz_amax, amax);
    return MI355PPO_OK;
}
