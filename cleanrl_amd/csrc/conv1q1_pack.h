// Kernel Q1's integer-digit pack of Conv2d(1,32,8,s4).weight (conv1q1.hip: the first layer of pqn_atari_envpool_lstm.py on ONE uint8 frame),
// as a workgroup-wide device function plus the element functions its host twin (ma_atari_twins.hip) shares.  The arithmetic is kernel Q's
// (conv1q_pack.h): each weight rounded once to a 31-bit fixed-point number on its output channel's scale, four signed radix-256 digits; the
// layout is this kernel's own -- a pixel has K = 64 bytes (8 tap rows of 8), one v_mfma_i32_32x32x32_i8 consumes FOUR tap rows.
#pragma once
#include "common.h"
#include "conv1q_pack.h"

#include <math.h>

namespace mi355ppo {

constexpr int kQ1Groups = 2;                                      // matrix instructions per digit and tile: tap rows 0-3, 4-7
constexpr int kQ1DigBytes = kQ1Groups * kQDigits * 64 * 16;       // int8 digits in operand layout: [group][digit][lane][16] = 8,192
constexpr int kQ1AccOff = kQ1DigBytes;                            // int32 [digit][channel]: 128 * sum_k digit
constexpr int kQ1ScaleOff = kQ1AccOff + kQDigits * 32 * 4;        // f32 [channel]: 2^(E_n - 6) / 255
constexpr int kQ1PackBytes = kQ1ScaleOff + 32 * 4;                // 8,832
constexpr int kQ1Pitch = 84, kQ1Img = 84 * 84;                    // bytes per source row / frame

// byte of digit d of weight (n, tap row r, tap column kw): lane (lh, n) of group r / 4 holds tap rows 4 g + 2 lh and 4 g + 2 lh + 1, 8 bytes each
MI355_HD int q1_pack_index(int n, int r, int kw, int d) {
    const int g = r >> 2, lh = (r >> 1) & 1, e = (r & 1) * 8 + kw;
    return (((g * kQDigits + d) * 64 + lh * 32 + n) * 16) + e;
}

// E with 2^(E-1) <= m < 2^E (0 for m = 0)
MI355_HD int q1_exp(float m) {
    int E = 0;
    if (m > 0.0f) (void)frexpf(m, &E);
    return E;
}

// the four signed radix-256 digits of q = rint(w * 2^(30 - E)), most significant first
MI355_HD void q1_digits(float w, int E, int (&dig)[kQDigits]) {
    long long q = llrint(ldexp((double)w, 30 - E));
    for (int d = kQDigits - 1; d >= 0; --d) {
        const int lo = (int)(((q + 128) & 255) - 128);
        dig[d] = lo;
        q = (q - lo) >> 8;
    }
}

MI355_HD float q1_scale(int E) { return (float)(ldexp(1.0, E - 6) / 255.0); }

// One workgroup of 256 threads: W (32,1,8,8) f32 as torch stores it -> the pack.
__device__ __forceinline__ void conv1q1_pack_body(const float* __restrict__ W, unsigned char* __restrict__ pack) {
    __shared__ int s_E[32];
    __shared__ float s_max[32][8];
    __shared__ int s_sum[kQDigits][32][8];
    const int tid = threadIdx.x;
    const int n = tid >> 3, r = tid & 7;           // thread -> (channel n, tap row r): the 8 weights W[n][0][r][kw]
    {
        float m = 0.0f;
        for (int kw = 0; kw < 8; ++kw) m = fmaxf(m, fabsf(W[(n * 8 + r) * 8 + kw]));
        s_max[n][r] = m;
    }
    __syncthreads();
    if (tid < 32) {
        float m = 0.0f;
        for (int rr = 0; rr < 8; ++rr) m = fmaxf(m, s_max[tid][rr]);
        s_E[tid] = q1_exp(m);
    }
    __syncthreads();
    const int E = s_E[n];
    int sums[kQDigits] = {0, 0, 0, 0};
    for (int kw = 0; kw < 8; ++kw) {
        int dig[kQDigits];
        q1_digits(W[(n * 8 + r) * 8 + kw], E, dig);
        for (int d = 0; d < kQDigits; ++d) {
            pack[q1_pack_index(n, r, kw, d)] = (unsigned char)(signed char)dig[d];
            sums[d] += dig[d];
        }
    }
    for (int d = 0; d < kQDigits; ++d) s_sum[d][n][r] = sums[d];
    __syncthreads();
    if (tid < kQDigits * 32) {
        const int d = tid >> 5, nn = tid & 31;
        int s = 0;
        for (int rr = 0; rr < 8; ++rr) s += s_sum[d][nn][rr];
        reinterpret_cast<int*>(pack + kQ1AccOff)[d * 32 + nn] = 128 * s;
    }
    if (tid < 32) reinterpret_cast<float*>(pack + kQ1ScaleOff)[tid] = q1_scale(s_E[tid]);
}

}  // namespace mi355ppo
