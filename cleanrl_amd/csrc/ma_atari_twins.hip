// Host-pointer twins of the fused ppo_pettingzoo_ma_atari path (ma_atari.hip, and kernel Q's pack / forward in conv1q.hip): the element
// math is ma_atari_rows.h's / conv1q_pack.h's own, compiled for the host, in the device's order -- a twin returns the device's bits.  A file
// of its own (as ppg_twins.hip), so that tools/ma_atari_host_check.cpp builds it stand-alone for the sanitizers.  Serial.
#include "common.h"
#include "conv1q_pack.h"
#include "conv1q1_pack.h"
#include "ma_atari_rows.h"

#include <math.h>
#include <stddef.h>
#include <string.h>

#include <vector>

#pragma clang fp contract(off)

using namespace mi355ppo;

namespace {

// conv1q_pack_body, serial: W (32, cs, 8, 8), channels 0 - 3 -> the pack (digits in operand layout, 128 * digit sums, scales)
void q_pack_host(const float* W, int cs, unsigned char* pack) {
    for (int n = 0; n < 32; ++n) {
        float m = 0.0f;
        for (int c = 0; c < kQC; ++c)
            for (int t = 0; t < 64; ++t) m = fmaxf(m, fabsf(W[(n * cs + c) * 64 + t]));
        int E = 0;
        if (m > 0.0f) (void)frexpf(m, &E);
        int sums[kQDigits] = {0, 0, 0, 0};
        for (int r = 0; r < 8; ++r)
            for (int e32 = 0; e32 < 32; ++e32) {
                const int kw = e32 >> 2, c = e32 & 3;
                long long q = llrint(ldexp((double)W[((n * cs + c) * 8 + r) * 8 + kw], 30 - E));
                int dig[kQDigits];
                for (int d = kQDigits - 1; d >= 0; --d) {
                    const int lo = (int)(((q + 128) & 255) - 128);
                    dig[d] = lo;
                    q = (q - lo) >> 8;
                }
                const int lh = e32 >> 4, e = e32 & 15;
                for (int d = 0; d < kQDigits; ++d) {
                    pack[((r * kQDigits + d) * 64 + lh * 32 + n) * 16 + e] = (unsigned char)(signed char)dig[d];
                    sums[d] += dig[d];
                }
            }
        for (int d = 0; d < kQDigits; ++d) {
            const int v = 128 * sums[d];
            memcpy(pack + kQAccOff + (d * 32 + n) * 4, &v, 4);
        }
        const float sc = (float)(ldexp(1.0, E - 6) / 255.0);
        memcpy(pack + kQScaleOff + n * 4, &sc, 4);
    }
}

// kernel Q, serial: exact integer dot products of the bytes with the pack's digits, then its epilogue; ind == nullptr: the plain bias
int q_fwd_host(const char* fn, const uint8_t* src, const int64_t* inds, const uint8_t* ind, const unsigned char* pack, const float* tapsum,
               const float* bias, float* dst, uint32_t* bits, int64_t images, bool pre = false) {
    MI355_REQUIRE(src && pack && bias && dst && (ind == nullptr) == (tapsum == nullptr), MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(images > 0, MI355PPO_EINVAL, "%s: images=%lld must be positive", fn, (long long)images);
    const signed char* dig = reinterpret_cast<const signed char*>(pack);
    for (int64_t img = 0; img < images; ++img) {
        const int64_t row = inds ? inds[img] : img;
        const uint8_t* frame = src + (size_t)row * (kQH * kQPitch);
        for (int p = 0; p < kQPerImg; ++p) {
            const int gy = p / kQG, gx = p - gy * kQG;
            uint32_t word = 0;
            for (int n = 0; n < 32; ++n) {
                int D[kQDigits] = {0, 0, 0, 0};
                for (int r = 0; r < kQRows; ++r) {
                    const uint8_t* taps = frame + (size_t)(gy * 4 + r) * kQPitch + gx * 4 * kQC;
                    for (int e32 = 0; e32 < 32; ++e32)
                        for (int d = 0; d < kQDigits; ++d)
                            D[d] += (int)taps[e32] * (int)dig[((r * kQDigits + d) * 64 + (e32 >> 4) * 32 + n) * 16 + (e32 & 15)];
                }
                float sc;
                memcpy(&sc, pack + kQScaleOff + n * 4, 4);
                const float b = ind ? ma_rowbias(bias[n], tapsum[2 * n], tapsum[2 * n + 1], ind[2 * row], ind[2 * row + 1]) : bias[n];
                const float v = pre ? ma_q_finish_pre(D, sc, b) : ma_q_finish(D, sc, b);
                dst[((size_t)img * kQPerImg + p) * 32 + n] = v;
                if (v > 0.0f) word |= 1u << n;
            }
            if (bits) bits[(size_t)img * kQPerImg + p] = word;
        }
    }
    return MI355PPO_OK;
}

// conv1q1_pack_body, serial: W (32, 1, 8, 8) -> kernel Q1's pack (conv1q1_pack.h's element functions)
void q1_pack_host(const float* W, unsigned char* pack) {
    for (int n = 0; n < 32; ++n) {
        float m = 0.0f;
        for (int t = 0; t < 64; ++t) m = fmaxf(m, fabsf(W[n * 64 + t]));
        const int E = q1_exp(m);
        int sums[kQDigits] = {0, 0, 0, 0};
        for (int r = 0; r < 8; ++r)
            for (int kw = 0; kw < 8; ++kw) {
                int dig[kQDigits];
                q1_digits(W[(n * 8 + r) * 8 + kw], E, dig);
                for (int d = 0; d < kQDigits; ++d) {
                    pack[q1_pack_index(n, r, kw, d)] = (unsigned char)(signed char)dig[d];
                    sums[d] += dig[d];
                }
            }
        for (int d = 0; d < kQDigits; ++d) {
            const int v = 128 * sums[d];
            memcpy(pack + kQ1AccOff + (d * 32 + n) * 4, &v, 4);
        }
        const float sc = q1_scale(E);
        memcpy(pack + kQ1ScaleOff + n * 4, &sc, 4);
    }
}

// kernel Q1, serial: exact integer dot products of the frame's bytes with the pack's digits, then kernel Q's epilogue -- pre: the
// pre-activation; otherwise the ReLU, with the mask words (bits) and the maximum folded into slot 0 of the amax record when given
int q1_fwd_host(const char* fn, const uint8_t* src, const int64_t* inds, const unsigned char* pack, const float* bias, float* dst,
                uint32_t* bits, uint32_t* amax, int64_t images, bool pre) {
    MI355_REQUIRE(src && pack && bias && dst, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(images > 0, MI355PPO_EINVAL, "%s: images=%lld must be positive", fn, (long long)images);
    const signed char* dig = reinterpret_cast<const signed char*>(pack);
    float vmax = 0.0f;
    for (int64_t img = 0; img < images; ++img) {
        const int64_t row = inds ? inds[img] : img;
        const uint8_t* frame = src + (size_t)row * kQ1Img;
        for (int p = 0; p < kQPerImg; ++p) {
            const int gy = p / kQG, gx = p - gy * kQG;
            uint32_t word = 0;
            for (int n = 0; n < 32; ++n) {
                int D[kQDigits] = {0, 0, 0, 0};
                for (int r = 0; r < 8; ++r) {
                    const uint8_t* taps = frame + (size_t)(gy * 4 + r) * kQ1Pitch + gx * 4;
                    for (int kw = 0; kw < 8; ++kw)
                        for (int d = 0; d < kQDigits; ++d) D[d] += (int)taps[kw] * (int)dig[q1_pack_index(n, r, kw, d)];
                }
                float sc;
                memcpy(&sc, pack + kQ1ScaleOff + n * 4, 4);
                const float v = pre ? ma_q_finish_pre(D, sc, bias[n]) : ma_q_finish(D, sc, bias[n]);
                dst[((size_t)img * kQPerImg + p) * 32 + n] = v;
                if (v > 0.0f) word |= 1u << n;
                if (!pre) vmax = fmaxf(vmax, v);
            }
            if (bits) bits[(size_t)img * kQPerImg + p] = word;
        }
    }
    if (amax) {                 // (as the LayerNorm twins: the device spreads its waves' maxima over the 16 slots, the record's value is their maximum)
        uint32_t b;
        memcpy(&b, &vmax, 4);
        if (b > amax[0]) amax[0] = b;
    }
    return MI355PPO_OK;
}

}  // namespace

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_pack_cpu(const float* W, void* pack) {
    MI355_REQUIRE(W && pack, MI355PPO_EINVAL, "mi355ppo_cnn_conv1q1_pack_cpu: null pointer");
    q1_pack_host(W, static_cast<unsigned char*>(pack));
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_pre_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias,
                                                             float* dst, int64_t images) {
    return q1_fwd_host("mi355ppo_cnn_conv1q1_pre_fwd_cpu", static_cast<const uint8_t*>(src_u8), inds, static_cast<const unsigned char*>(pack),
                       bias, dst, nullptr, nullptr, images, true);
}

// kernel Q1's ReLU forward (mi355ppo_cnn_conv1q1_fwd_bits / _fwd_amax): mask_bits and dst_amax may each be null
extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                         uint32_t* mask_bits, uint32_t* dst_amax, int64_t images) {
    return q1_fwd_host("mi355ppo_cnn_conv1q1_fwd_cpu", static_cast<const uint8_t*>(src_u8), inds, static_cast<const unsigned char*>(pack), bias,
                       dst, mask_bits, dst_amax, images, false);
}

extern "C" MI355PPO_API int mi355ppo_ma_atari_split_u8_cpu(const uint8_t* frames6, uint8_t* rows4, uint8_t* ind, uint32_t* flag, int64_t frames) {
    const char* fn = "mi355ppo_ma_atari_split_u8_cpu";
    MI355_REQUIRE(frames6 && rows4 && ind && flag, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(frames > 0, MI355PPO_EINVAL, "%s: frames=%lld must be positive", fn, (long long)frames);
    for (int64_t f = 0; f < frames; ++f) {
        const uint8_t* src = frames6 + (size_t)f * (kMaPix * kMaInC);
        const uint32_t v4 = src[4], v5 = src[5];
        ind[2 * f] = (uint8_t)v4;
        ind[2 * f + 1] = (uint8_t)v5;
        for (int g = 0; g < kMaGroups; ++g) {
            uint32_t w[6], o[4];
            memcpy(w, src + (size_t)g * 24, 24);
            if (ma_split4(w, o, v4, v5)) *flag |= 1u;        // sticky: only ever sets the bit
            memcpy(rows4 + ((size_t)f * kMaGroups + g) * 16, o, 16);
        }
    }
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q_pack_cpu(const float* W, void* pack) {
    MI355_REQUIRE(W && pack, MI355PPO_EINVAL, "mi355ppo_cnn_conv1q_pack_cpu: null pointer");
    q_pack_host(W, kQC, static_cast<unsigned char*>(pack));
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_ma_atari_conv1_pack_f32_cpu(const float* W6, void* pack, float* tapsum) {
    MI355_REQUIRE(W6 && pack && tapsum, MI355PPO_EINVAL, "mi355ppo_ma_atari_conv1_pack_f32_cpu: null pointer");
    q_pack_host(W6, kMaInC, static_cast<unsigned char*>(pack));
    for (int k = 0; k < 64; ++k) tapsum[k] = conv1q_tapsum(W6, k >> 1, k & 1);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                        uint32_t* mask_bits, int64_t images) {
    return q_fwd_host("mi355ppo_cnn_conv1q_fwd_cpu", static_cast<const uint8_t*>(src_u8), inds, nullptr, static_cast<const unsigned char*>(pack),
                      nullptr, bias, dst, mask_bits, images);
}

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q_pre_fwd_cpu(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                            int64_t images) {
    return q_fwd_host("mi355ppo_cnn_conv1q_pre_fwd_cpu", static_cast<const uint8_t*>(src_u8), inds, nullptr, static_cast<const unsigned char*>(pack),
                      nullptr, bias, dst, nullptr, images, true);
}

extern "C" MI355PPO_API int mi355ppo_ma_atari_conv1_fwd_cpu(const void* src_u8, const int64_t* inds, const uint8_t* ind, const void* pack,
                                                            const float* tapsum, const float* bias, float* dst, uint32_t* mask_bits,
                                                            int64_t images) {
    const char* fn = "mi355ppo_ma_atari_conv1_fwd_cpu";
    MI355_REQUIRE(ind && tapsum, MI355PPO_EINVAL, "%s: null pointer", fn);
    return q_fwd_host(fn, static_cast<const uint8_t*>(src_u8), inds, ind, static_cast<const unsigned char*>(pack), tapsum, bias, dst, mask_bits,
                      images);
}

extern "C" MI355PPO_API int mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu(const float* dz1, const int64_t* inds, const uint8_t* ind,
                                                                       const float* dW4, float* dW6, int64_t images) {
    const char* fn = "mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu";
    MI355_REQUIRE(dz1 && ind && dW4 && dW6, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(images > 0, MI355PPO_EINVAL, "%s: images=%lld must be positive", fn, (long long)images);
    const int64_t parts = ma_fold_parts(images);
    std::vector<double> part((size_t)parts * 64, 0.0);
    for (int64_t b = 0; b < parts; ++b)                        // the device's partition: ma_fold_part_kernel
        for (int n = 0; n < 32; ++n) {
            double acc4 = 0.0, acc5 = 0.0;
            for (int64_t img = b * kMaFoldImgs; img < images && img < (b + 1) * kMaFoldImgs; ++img) {
                double s = 0.0;
                for (int q = 0; q < kMaFoldStrips; ++q) s = s + ma_fold_strip(dz1 + (size_t)img * (kMaOutPix * 32), n, q);
                const int64_t row = inds ? inds[img] : img;
                acc4 = acc4 + (double)ind[2 * row] * s;
                acc5 = acc5 + (double)ind[2 * row + 1] * s;
            }
            part[(size_t)b * 64 + n] = acc4;
            part[(size_t)b * 64 + 32 + n] = acc5;
        }
    float g[64];
    for (int k = 0; k < 64; ++k) {                             // ma_fold_final_kernel
        double t = 0.0;
        for (int c = 0; c < kMaFoldChains; ++c) {
            double s = 0.0;
            for (int64_t b = c; b < parts; b += kMaFoldChains) s = s + part[(size_t)b * 64 + k];
            t = t + s;
        }
        g[k] = (float)t;
    }
    for (int e = 0; e < 32 * kMaInC * 64; ++e) {
        const int n = e / (kMaInC * 64), r = e - n * (kMaInC * 64), ch = r >> 6, t = r & 63;
        dW6[e] = ch < kMaOutC ? dW4[(n * kMaOutC + ch) * 64 + t] : g[(ch - kMaOutC) * 32 + n];
    }
    return MI355PPO_OK;
}
