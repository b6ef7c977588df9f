// Row / element math of the fused path of ppo_pettingzoo_ma_atari.py (ma_atari.hip, the row-bias instance of kernel Q in conv1q.hip)
// and of its host twins (ma_atari_twins.hip): one definition compiled for both sides, so a twin returns the device's bits.
//
// The script's observations are (84, 84, 6) u8: four stacked frames and two agent-indicator planes that are constant over a frame
// (ppo_pettingzoo_ma_atari.py:86-118).  A constant plane of value v adds  v * sum_{kh,kw} W1[n][c][kh][kw]  to every output pixel of
// channel n of conv1 -- a bias per observation -- and its weight gradient is one number for all 64 taps.  So:
//   * the rollout stores the four frame channels as (84, 84, 4) rows -- what kernels Q and P read -- and two indicator bytes per row
//     (ma_split4: also tells whether a plane is NOT constant);
//   * conv1's epilogue adds  ma_rowbias = fmaf(v5, S[n][1], fmaf(v4, S[n][0], b[n]))  with S the tap sums of channels 4 / 5 (the
//     indicator planes are not divided by 255, :104);
//   * the gradient of channels 4 / 5 is  g[n][j] = sum_img v_j(img) * sum_p dz1[img][p][n],  accumulated in double in ONE fixed order:
//     per image eight strips of 50 pixels (ma_fold_strip), the strips in ascending order, kMaFoldImgs images per partial in ascending
//     order, the partials in four interleaved chains, the chains in ascending order, one rounding to f32.
#pragma once
#include "common.h"

namespace mi355ppo {

constexpr int kMaPix = 84 * 84;          // pixels of an observation
constexpr int kMaInC = 6, kMaOutC = 4;   // channels delivered / stored
constexpr int kMaGroups = kMaPix / 4;    // a group = four pixels: 24 bytes in, 16 bytes out
constexpr int kMaOutPix = 400;           // conv1's 20 x 20 output pixels
constexpr int kMaFoldImgs = 4;           // images per partial of the gradient fold
constexpr int kMaFoldStrips = 8;         // strips of an image's pixels: strip q = pixels q, q + 8, ...
constexpr int kMaFoldChains = 4;         // chains of the final fold: chain c = partials c, c + 4, ...

// Four pixels of a six-channel frame (six little-endian words) -> their four frame channels (four words); -> does a byte of plane 4 / 5
// differ from v4 / v5 (the plane's value at pixel (0, 0))?
MI355_HD bool ma_split4(const uint32_t w[6], uint32_t out[4], uint32_t v4, uint32_t v5) {
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < kMaInC; ++c) {
            const int b = kMaInC * k + c;
            const uint32_t v = (w[b >> 2] >> (8 * (b & 3))) & 255u;
            if (c < kMaOutC) px |= v << (8 * c);
            else bad = bad || (v != (c == 4 ? v4 : v5));
        }
        out[k] = px;
    }
    return bad;
}

// conv1's bias of one observation and output channel
MI355_HD float ma_rowbias(float b, float s4, float s5, uint32_t v4, uint32_t v5) {
    return __builtin_fmaf((float)v5, s5, __builtin_fmaf((float)v4, s4, b));
}

// kernel Q's epilogue on the exact integer dot products D_j = sum_k v[k] * digit_j[k][n] (conv1q.hip): Horner, scale, bias, ReLU
MI355_HD float ma_q_finish(const int D[4], float scale, float bias) {
    float t = (float)D[3];
    t = __builtin_fmaf(t, 0.00390625f, (float)D[2]);
    t = __builtin_fmaf(t, 0.00390625f, (float)D[1]);
    t = __builtin_fmaf(t, 0.00390625f, (float)D[0]);
    float v = t * scale;
    v = v + bias;
    return v > 0.0f ? v : 0.0f;
}

// the same without the ReLU (kernel Q's PRE instance: the pre-activation a LayerNorm follows)
MI355_HD float ma_q_finish_pre(const int D[4], float scale, float bias) {
    float t = (float)D[3];
    t = __builtin_fmaf(t, 0.00390625f, (float)D[2]);
    t = __builtin_fmaf(t, 0.00390625f, (float)D[1]);
    t = __builtin_fmaf(t, 0.00390625f, (float)D[0]);
    float v = t * scale;
    return v + bias;
}

// strip q of channel n of one image's dz1 (400, 32), ascending pixels
MI355_HD double ma_fold_strip(const float* dz_img, int n, int q) {
    double s = 0.0;
    for (int p = q; p < kMaOutPix; p += kMaFoldStrips) s = s + (double)dz_img[p * 32 + n];
    return s;
}

inline int64_t ma_fold_parts(int64_t images) { return (images + kMaFoldImgs - 1) / kMaFoldImgs; }

}  // namespace mi355ppo
