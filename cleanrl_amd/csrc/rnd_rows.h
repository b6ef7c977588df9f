// Row / element math of the RND kernels (rnd.hip) and their host-pointer twins, compiled for both sides: the newest-frame
// normalisation, the exact per-pixel moments, the 512-feature squared distance, the env-axis reward filter with its running
// statistics, and the fold orders of the two loss scalars.  Everything here is a pure function of its inputs: integer sums,
// float64 with one rounding, f32 in one fixed order.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kRndPixels = 84 * 84;      // one frame
constexpr int kRndF = 512;               // features of the RND target / predictor networks
constexpr int kRndSlab = 256;            // rows whose x and x^2 one thread adds in 32 bits before the 64-bit fold
static_assert(255ull * 255ull * (unsigned long long)kRndSlab < (1ull << 32), "a slab's sum of squares must fit 32 bits");
constexpr int64_t kRndMaxBatch = (int64_t)1 << 24;      // B * S2 - S1^2 stays below 2^64 for B < 2^24
constexpr int kRndFold = 256;            // slots of the loss scalars' fold (slot t: rows t, t + 256, ... in f64; then the slots in order)
constexpr int kRndMaxT = 1024;           // scans (rollout steps) of the reward filter: one f64 partial each in LDS
constexpr int kRndNormRows = 8;          // rows of the normalise kernel per workgroup (mean / sd stay in registers)

MI355_HD int64_t rnd_clamp_index(int64_t i, int64_t B) { return i < 0 ? 0 : (i >= B ? B - 1 : i); }

// ((double)x - mean) / sd, clipped to [-5, 5] (a NaN passes, as through torch.clip), rounded once to f32.
MI355_HD float rnd_normalize(unsigned x, double mean, double sd) {
    double z = ((double)x - mean) / sd;
    z = z < -5.0 ? -5.0 : (z > 5.0 ? 5.0 : z);
    return (float)z;
}

// The pixel p of a frame addressed by a pixel stride and a byte offset: stride 4 reads the whole 4-byte pixel.
template <int STRIDE>
MI355_HD unsigned rnd_pixel(const unsigned char* row, int p, int off) {
    if (STRIDE == 4) return (reinterpret_cast<const uint32_t*>(row)[p] >> (8 * off)) & 0xFFu;
    return row[(int64_t)off + p];
}

// Lane `lane` (0..63) of a 512-feature row: the squares of a - b over features 4 lane .. 4 lane + 3 and 256 + 4 lane .. + 3, added
// in that order.  The 64 lanes are then folded by rnd_fold_lanes' butterfly (the device: wave_sum).
MI355_HD float rnd_lane_sq(const float* __restrict__ a, const float* __restrict__ b, int lane) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int f = k * 256 + 4 * lane;
#if defined(__HIP_DEVICE_COMPILE__)
        const float4 x = *reinterpret_cast<const float4*>(a + f), y = *reinterpret_cast<const float4*>(b + f);
        const float d0 = x.x - y.x, d1 = x.y - y.y, d2 = x.z - y.z, d3 = x.w - y.w;
#else
        const float d0 = a[f] - b[f], d1 = a[f + 1] - b[f + 1], d2 = a[f + 2] - b[f + 2], d3 = a[f + 3] - b[f + 3];
#endif
        acc = acc + d0 * d0;
        acc = acc + d1 * d1;
        acc = acc + d2 * d2;
        acc = acc + d3 * d3;
    }
    return acc;
}

// wave_sum's order on the host: v[l] += v[l ^ off] for off = 32, 16, .., 1 (every lane ends with the same value).
inline float rnd_fold_lanes(float* v) {
    for (int off = 32; off > 0; off >>= 1) {
        float w[64];
        for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}

inline float rnd_row_sq_host(const float* a, const float* b) {
    float v[64];
    for (int l = 0; l < 64; ++l) v[l] = rnd_lane_sq(a, b, l);
    return rnd_fold_lanes(v);
}

// RewardForwardFilter.update along the env axis: rewems = fl32(fl32(rewems * g) + r).
MI355_HD float rnd_filter_step(float rewems, float g, float r) {
    const float m = rewems * g;
    return m + r;
}

// Scan t of the filter (row = curiosity + t * N), pass 1: the f64 sum of the N filtered values in ascending n; the state after
// the last env goes to *rew_end, the filtered values to filtered_row when non-NULL.
MI355_HD double rnd_filter_scan_sum(const float* __restrict__ row, int N, float rew, float g, float* __restrict__ filtered_row,
                                    float* rew_end) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) {
        rew = rnd_filter_step(rew, g, row[n]);
        if (filtered_row) filtered_row[n] = rew;
        s += (double)rew;
    }
    *rew_end = rew;
    return s;
}

// Pass 2 (the same scan again): the f64 sum of (filtered - mean)^2 in ascending n.
MI355_HD double rnd_filter_scan_sq(const float* __restrict__ row, int N, float rew, float g, double mean) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) {
        rew = rnd_filter_step(rew, g, row[n]);
        const double d = (double)rew - mean;
        s += d * d;
    }
    return s;
}

// RunningMeanStd.update_from_moments on stats = (mean, var, count), in the host class's operation order.
MI355_HD void rnd_update_from_moments(double* stats, double batch_mean, double batch_var, double batch_count) {
    const double mean = stats[0], var = stats[1], count = stats[2];
    const double delta = batch_mean - mean;
    const double tot = count + batch_count;
    const double new_mean = mean + delta * batch_count / tot;
    const double m2 = var * count + batch_var * batch_count + delta * delta * count * batch_count / tot;
    stats[0] = new_mean;
    stats[1] = m2 / tot;
    stats[2] = tot;
}

// The loss's per-call constants, formed once on the host in double.
struct RndLossParams {
    float proportion;      // mask_m = u_m < proportion
    float v_scale;         // vf_coef / M
    int M, F;
    int64_t B;
};

MI355_HD float rnd_grad_scale(int count) { return (float)(1.0 / (512.0 * (double)(count < 1 ? 1 : count))); }

MI355_HD void rnd_loss_scalars(double sum_fwd, double sum_v, int count, int M, float* scalars) {
    scalars[0] = (float)(0.5 * (sum_v / (double)M));                            // 0.5 * mean (v_int - R_int)^2
    scalars[1] = (float)(sum_fwd / (double)(count < 1 ? 1 : count));            // masked mean of the rows' distillation error
}

}  // namespace mi355ppo
