// Row math of the LayerNorm + ReLU kernels (layernorm.hip) and of their host-pointer twins (layernorm_twins.hip): one definition compiled
// for both sides, so a twin returns the device's bits.
//
// pqn_atari_envpool.py's network is Conv -> LayerNorm -> ReLU three times, then Linear -> LayerNorm -> ReLU.  An activation row here is one
// sample in (H, W, C) order, D = C * HW floats; torch's LayerNorm([C, H, W]) keeps weight / bias in (C, H, W) order, so element
// e = p * C + c of a row reads parameter c * HW + p (ln_param).  Forward, per row:
//     mean = sum z / D,  var = sum (z - mean)^2 / D  (biased, two passes),  rstd = 1 / sqrt(var + eps),
//     a = max((z - mean) * rstd * gamma + beta, 0)
// Backward, with g = dy * gamma and xh = (z - mean) * rstd:
//     dz = rstd * ((g - mean_j g) - xh * mean_j (g * xh)),   dgamma[j] = sum_r dy * xh,   dbeta[j] = sum_r dy
//
// The order of every sum is a function of the shape alone.  A row is dealt to NT threads in float4 quads, thread t owning quads t, t + NT,
// ... (ln_shape: NT and the quads per thread from D); a thread adds its elements in ascending order in double, the NT partials are folded by
// ln_fold (the butterfly of wave_sum inside each wave of 64, then the waves in ascending order).  The column sums of the backward are added
// in f32 over the rows of a slab in ascending order (ln_slab_rows rows, from the row count alone), the slabs in ascending order in double.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kLnMaxD = 16384;           // floats of a row the kernels take (12,800 = conv1's 20 x 20 x 32 is the largest of the network)
constexpr int kLnMaxThreads = 1024;

struct LnShape {
    int nt;      // threads of a row's workgroup
    int kq;      // quads per thread (the last ones partly past the row)
};

// D % 4 == 0, 4 <= D <= kLnMaxD
MI355_HD LnShape ln_shape(int D) {
    if (D <= 1024) return {256, 1};
    if (D <= 4096) return {512, 2};
    if (D <= 8192) return {1024, 2};
    return {1024, 4};
}

// element e = p * C + c of a row -> index of its parameter in torch's (C, H, W) order
MI355_HD int ln_param(int e, int C, int HW) {
    const int p = e / C, c = e - p * C;
    return c * HW + p;
}

// rows a workgroup of the forward walks (gamma / beta stay in its registers) and rows of a slab of the backward
inline int ln_fwd_rows_per_wg(int64_t rows) {
    const int64_t r = (rows + 511) / 512;
    return (int)(r < 1 ? 1 : (r > 8 ? 8 : r));
}
inline int ln_slab_rows(int64_t rows) {
    const int64_t r = (rows + 255) / 256;
    return (int)(r < 4 ? 4 : (r > 64 ? 64 : r));
}
inline int64_t ln_slabs(int64_t rows) { return (rows + ln_slab_rows(rows) - 1) / ln_slab_rows(rows); }

// one element of the forward / backward, f32 with one rounding per operation
MI355_HD float ln_xhat(float z, float mean, float rstd) { return (z - mean) * rstd; }
MI355_HD float ln_out(float z, float mean, float rstd, float gamma, float beta) {
    const float y = ln_xhat(z, mean, rstd) * gamma + beta;
    return y > 0.0f ? y : 0.0f;
}
MI355_HD float ln_rstd(double var, float eps) { return 1.0f / sqrtf((float)var + eps); }
MI355_HD float ln_dz(float g, float xh, float rstd, float m1, float m2) { return rstd * ((g - m1) - xh * m2); }

// The host's replay of the workgroup fold: v[t] = thread t's partial, nt a multiple of 64.
inline double ln_fold_host(double* v, int nt) {
    double total = 0.0;
    for (int w = 0; w < nt / 64; ++w) {
        double* l = v + 64 * w;
        for (int off = 32; off > 0; off >>= 1) {
            double t[64];
            for (int i = 0; i < 64; ++i) t[i] = l[i] + l[i ^ off];
            for (int i = 0; i < 64; ++i) l[i] = t[i];
        }
        total = w == 0 ? l[0] : total + l[0];
    }
    return total;
}

}  // namespace mi355ppo
