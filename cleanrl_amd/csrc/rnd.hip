// Random Network Distillation (cleanrl/ppo_rnd_envpool.py): what the learner does around the two RND networks -- observation
// statistics, the networks' input, the intrinsic reward, its scaling, and the two loss terms K3 does not cover (gfx950).
//
// All five are bandwidth or latency kernels; the mappings keep one element's math on one lane (rnd_rows.h, which the host
// twins at the end of this file run unchanged):
//
//   normalize       one lane per pixel, kRndNormRows rows per workgroup (mean / sd of the pixel stay in registers); an NHWC frame
//                   is read as whole 4-byte pixels (coalesced), the newest frame's byte picked in a register; f64 arithmetic,
//                   one rounding to f32
//   obs_moments     (1) one lane per pixel adds x and x^2 over a slab of kRndSlab rows in 32 bits (the bound is a static_assert)
//                   (2) one lane per pixel adds the slabs' partials in 64 bits, ascending; the output is overwritten
//   intrinsic       one wave per row: rnd_lane_sq per lane (two float4 loads of each operand), wave_sum's butterfly, * 0.5
//   reward_filter   ONE workgroup: thread t runs scan t along the env axis twice (sum, then squared deviations, both f64 in
//                   ascending n); thread 0 adds the scans' partials in ascending t, applies update_from_moments to the device
//                   triple; all threads then divide the (T, N) rewards by (float)sqrt(var)
//   loss            (0) one workgroup counts the mask into the workspace (an integer: no order)
//                   (1) one wave per row: the row's mean squared error into the workspace, its masked gradient row, the value
//                       gradient
//                   (2) one workgroup folds the rows into the two scalars (kRndFold slots, f64, in order)
//
// No atomics, no allocation, no synchronisation: results are deterministic, every entry point can be captured into a graph.
#include <math.h>

#include <vector>

#include "common.h"
#include "rnd_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

template <int STRIDE>
__global__ __launch_bounds__(256) void rnd_normalize_kernel(const unsigned char* __restrict__ src, int64_t B, int64_t row_bytes, int off,
                                                            const int64_t* __restrict__ idx, const double* __restrict__ mean,
                                                            const double* __restrict__ sd, float* __restrict__ out, int M) {
    const int p = blockIdx.y * 256 + threadIdx.x;                   // rows on grid.x (no 65,535 limit), pixel blocks on grid.y
    if (p >= kRndPixels) return;
    const double mu = mean[p], s = sd[p];
    const int r0 = blockIdx.x * kRndNormRows;
    const int r1 = (r0 + kRndNormRows < M) ? r0 + kRndNormRows : M;
    for (int r = r0; r < r1; ++r) {
        const int64_t i = rnd_clamp_index(idx ? idx[r] : (int64_t)r, B);
        out[(int64_t)r * kRndPixels + p] = rnd_normalize(rnd_pixel<STRIDE>(src + i * row_bytes, p, off), mu, s);
    }
}

// (1) of the moments: part[slab][0][p] = sum x, part[slab][1][p] = sum x^2 over rows [slab * kRndSlab, +kRndSlab).
template <int STRIDE>
__global__ __launch_bounds__(256) void rnd_moments_slab_kernel(const unsigned char* __restrict__ src, int64_t B, int64_t row_bytes, int off,
                                                               uint32_t* __restrict__ part) {
    const int p = blockIdx.y * 256 + threadIdx.x;                   // slabs on grid.x (up to 65,536 of them), pixel blocks on grid.y
    if (p >= kRndPixels) return;
    const int64_t r0 = (int64_t)blockIdx.x * kRndSlab;
    const int64_t r1 = (r0 + kRndSlab < B) ? r0 + kRndSlab : B;
    uint32_t s1 = 0, s2 = 0;
#pragma unroll 8
    for (int64_t r = r0; r < r1; ++r) {
        const uint32_t x = rnd_pixel<STRIDE>(src + r * row_bytes, p, off);
        s1 += x;
        s2 += x * x;
    }
    uint32_t* o = part + (int64_t)blockIdx.x * 2 * kRndPixels;
    o[p] = s1;
    o[kRndPixels + p] = s2;
}

// (2) of the moments: sums[0][p], sums[1][p] = the slabs' partials added in 64 bits.
__global__ __launch_bounds__(256) void rnd_moments_fold_kernel(const uint32_t* __restrict__ part, int nslab, uint64_t* __restrict__ sums) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= kRndPixels) return;
    uint64_t s1 = 0, s2 = 0;
    for (int b = 0; b < nslab; ++b) {
        s1 += part[(int64_t)b * 2 * kRndPixels + p];
        s2 += part[(int64_t)b * 2 * kRndPixels + kRndPixels + p];
    }
    sums[p] = s1;
    sums[kRndPixels + p] = s2;
}

__global__ __launch_bounds__(256) void rnd_intrinsic_kernel(const float* __restrict__ target, const float* __restrict__ predict,
                                                            float* __restrict__ out, int N) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;                                              // whole waves leave together; no barrier below
    const int lane = threadIdx.x & 63;
    const float s = wave_sum(rnd_lane_sq(target + (int64_t)r * kRndF, predict + (int64_t)r * kRndF, lane));
    if (lane == 0) out[r] = s * 0.5f;
}

__global__ __launch_bounds__(256) void rnd_reward_filter_kernel(float* __restrict__ curiosity, float* __restrict__ rewems,
                                                                double* __restrict__ stats, float* __restrict__ filtered_out, int T, int N,
                                                                float g) {
    __shared__ double s_part[kRndMaxT];
    __shared__ float s_end[kRndMaxT];
    __shared__ double s_mean;
    __shared__ float s_div;
    const double count = (double)T * (double)N;
    for (int t = threadIdx.x; t < T; t += 256) {
        s_part[t] = rnd_filter_scan_sum(curiosity + (int64_t)t * N, N, rewems[t], g, filtered_out ? filtered_out + (int64_t)t * N : nullptr,
                                        &s_end[t]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += s_part[t];
        s_mean = s / count;
    }
    __syncthreads();                                                // thread 0 is done reading s_part; s_mean is written once
    const double mean = s_mean;
    for (int t = threadIdx.x; t < T; t += 256) s_part[t] = rnd_filter_scan_sq(curiosity + (int64_t)t * N, N, rewems[t], g, mean);
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < T; ++t) s += s_part[t];
        double st[3] = {stats[0], stats[1], stats[2]};
        rnd_update_from_moments(st, mean, s / count, (double)N);     // the count is len() of the (N, T) array, as the reference
        stats[0] = st[0];
        stats[1] = st[1];
        stats[2] = st[2];
        s_div = (float)sqrt(st[1]);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) rewems[t] = s_end[t];      // the second pass read the old state: written only now
    const float div = s_div;
    const int64_t total = (int64_t)T * N;
    for (int64_t i = threadIdx.x; i < total; i += 256) curiosity[i] = curiosity[i] / div;
}

// (0) of the loss: the mask count of the whole minibatch by one workgroup of 256 threads (integers: exact in any order).
__global__ __launch_bounds__(256) void rnd_loss_count_kernel(const float* __restrict__ u, int M, float proportion, int* __restrict__ count) {
    __shared__ int lds[4];
    int c = 0;
    for (int m = threadIdx.x; m < M; m += 256) c += (u[m] < proportion) ? 1 : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, MI355_WAVE);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) *count = lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(256) void rnd_loss_rows_kernel(const float* __restrict__ predict, const float* __restrict__ target,
                                                            const float* __restrict__ u, const float* __restrict__ v_int,
                                                            const float* __restrict__ int_returns, const int64_t* __restrict__ inds,
                                                            RndLossParams P, const int* __restrict__ count, float* __restrict__ row_mse,
                                                            float* __restrict__ d_predict, float* __restrict__ d_v_int) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= P.M) return;                                            // whole waves leave together; no barrier below
    const float scale = rnd_grad_scale(*count);
    const int lane = threadIdx.x & 63;
    const float* p = predict + (int64_t)r * kRndF;
    const float* t = target + (int64_t)r * kRndF;
    const float s = wave_sum(rnd_lane_sq(p, t, lane));
    const bool on = u[r] < P.proportion;
    float* g = d_predict + (int64_t)r * kRndF;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int f = k * 256 + 4 * lane;
        const float4 x = *reinterpret_cast<const float4*>(p + f), y = *reinterpret_cast<const float4*>(t + f);
        float4 o;
        o.x = on ? (2.0f * (x.x - y.x)) * scale : 0.0f;
        o.y = on ? (2.0f * (x.y - y.y)) * scale : 0.0f;
        o.z = on ? (2.0f * (x.z - y.z)) * scale : 0.0f;
        o.w = on ? (2.0f * (x.w - y.w)) * scale : 0.0f;
        *reinterpret_cast<float4*>(g + f) = o;
    }
    if (lane == 0) {
        row_mse[r] = s * (1.0f / 512.0f);
        d_v_int[r] = (v_int[r] - int_returns[rnd_clamp_index(inds[r], P.B)]) * P.v_scale;
    }
}

__global__ __launch_bounds__(kRndFold) void rnd_loss_fold_kernel(const float* __restrict__ row_mse, const float* __restrict__ u,
                                                                 const float* __restrict__ v_int, const float* __restrict__ int_returns,
                                                                 const int64_t* __restrict__ inds, RndLossParams P, const int* __restrict__ count,
                                                                 float* __restrict__ scalars) {
    __shared__ double s_f[kRndFold], s_v[kRndFold];
    double sf = 0.0, sv = 0.0;
    for (int m = threadIdx.x; m < P.M; m += kRndFold) {
        if (u[m] < P.proportion) sf += (double)row_mse[m];
        const double d = (double)(v_int[m] - int_returns[rnd_clamp_index(inds[m], P.B)]);
        sv += d * d;
    }
    s_f[threadIdx.x] = sf;
    s_v[threadIdx.x] = sv;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tf = 0.0, tv = 0.0;
        for (int k = 0; k < kRndFold; ++k) {
            tf += s_f[k];
            tv += s_v[k];
        }
        rnd_loss_scalars(tf, tv, *count, P.M, scalars);
    }
}

// Shared argument checks of the device entry points and their twins (before any HIP call).  The frame check is also rnd_conv1.hip's.
int rnd_frame_args(const char* fn, const void* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset) {
    MI355_REQUIRE(src, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%lld must be positive", fn, (long long)B);
    MI355_REQUIRE(pixel_stride == 1 || pixel_stride == 4, MI355PPO_EINVAL, "%s: pixel_stride=%d: 1 (a planar frame) or 4 (4-byte pixels)", fn,
                  pixel_stride);
    if (pixel_stride == 4) {
        MI355_REQUIRE(byte_offset >= 0 && byte_offset < 4 && row_bytes >= 4 * (int64_t)kRndPixels && row_bytes % 4 == 0, MI355PPO_EINVAL,
                      "%s: 4-byte pixels take 0 <= byte_offset < 4 and row_bytes a multiple of 4 that is >= %d (byte_offset=%lld row_bytes=%lld)", fn,
                      4 * kRndPixels, (long long)byte_offset, (long long)row_bytes);
        MI355_REQUIRE(aligned(src, 4), MI355PPO_EALIGN, "%s: rows of 4-byte pixels must be 4-byte aligned", fn);
    } else {
        MI355_REQUIRE(byte_offset >= 0 && byte_offset <= (int64_t)1 << 30 && row_bytes >= byte_offset + kRndPixels, MI355PPO_EINVAL,
                      "%s: a planar frame at byte_offset=%lld does not fit row_bytes=%lld", fn, (long long)byte_offset, (long long)row_bytes);
    }
    return MI355PPO_OK;
}

namespace {

int rnd_normalize_args(const char* fn, const void* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset, const int64_t* idx,
                       const double* mean, const double* sd, float* out, int M) {
    if (int rc = rnd_frame_args(fn, src, B, row_bytes, pixel_stride, byte_offset)) return rc;
    MI355_REQUIRE(mean && sd && out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && (idx || M <= B), MI355PPO_EINVAL, "%s: M=%d must be positive and, without an index, at most B=%lld", fn, M, (long long)B);
    MI355_REQUIRE(aligned(mean, 8) && aligned(sd, 8) && aligned(out, 4) && aligned(idx, 8), MI355PPO_EALIGN,
                  "%s: mean / sd / idx must be 8-byte aligned, out 4-byte aligned", fn);
    return MI355PPO_OK;
}

int rnd_moments_args(const char* fn, const void* src, int64_t B, int64_t row_bytes, int pixel_stride, int64_t byte_offset, uint64_t* sums) {
    if (int rc = rnd_frame_args(fn, src, B, row_bytes, pixel_stride, byte_offset)) return rc;
    MI355_REQUIRE(B < kRndMaxBatch, MI355PPO_EINVAL, "%s: B=%lld: B * S2 - S1^2 is exact in 64 bits only for B < 2^24", fn, (long long)B);
    MI355_REQUIRE(sums, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(sums, 8), MI355PPO_EALIGN, "%s: sums must be 8-byte aligned", fn);
    return MI355PPO_OK;
}

int rnd_intrinsic_args(const char* fn, const float* target, const float* predict, float* out, int N, int F) {
    MI355_REQUIRE(target && predict && out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(N > 0, MI355PPO_EINVAL, "%s: N=%d must be positive", fn, N);
    MI355_REQUIRE(F == kRndF, MI355PPO_EINVAL, "%s: F=%d: the kernel is written for %d features", fn, F, kRndF);
    MI355_REQUIRE(aligned(target, 16) && aligned(predict, 16) && aligned(out, 4), MI355PPO_EALIGN,
                  "%s: feature rows must be 16-byte aligned, out 4-byte aligned", fn);
    return MI355PPO_OK;
}

int rnd_filter_args(const char* fn, float* curiosity, float* rewems, double* stats3, float* filtered_out, int T, int N) {
    MI355_REQUIRE(curiosity && rewems && stats3, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(T > 0 && N > 0 && T <= kRndMaxT, MI355PPO_EINVAL, "%s: T=%d N=%d: 1 <= T <= %d, N >= 1", fn, T, N, kRndMaxT);
    MI355_REQUIRE(filtered_out != curiosity, MI355PPO_EINVAL, "%s: filtered_out must not alias curiosity", fn);
    MI355_REQUIRE(aligned(curiosity, 4) && aligned(rewems, 4) && aligned(stats3, 8) && aligned(filtered_out, 4), MI355PPO_EALIGN,
                  "%s: stats must be 8-byte aligned, the f32 tensors 4-byte aligned", fn);
    return MI355PPO_OK;
}

int rnd_loss_args(const char* fn, const float* predict, const float* target, const float* u, const float* v_int, const float* int_returns,
                  const int64_t* mb_inds, int64_t B, float* scalars_out, float* d_predict, float* d_v_int, int M, int F) {
    MI355_REQUIRE(predict && target && u && v_int && int_returns && mb_inds && scalars_out && d_predict && d_v_int, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && B > 0, MI355PPO_EINVAL, "%s: M=%d B=%lld must be positive", fn, M, (long long)B);
    MI355_REQUIRE(F == kRndF, MI355PPO_EINVAL, "%s: F=%d: the kernel is written for %d features", fn, F, kRndF);
    MI355_REQUIRE(aligned(predict, 16) && aligned(target, 16) && aligned(d_predict, 16), MI355PPO_EALIGN, "%s: feature rows must be 16-byte aligned", fn);
    MI355_REQUIRE(aligned(u, 4) && aligned(v_int, 4) && aligned(int_returns, 4) && aligned(mb_inds, 8) && aligned(scalars_out, 4) && aligned(d_v_int, 4),
                  MI355PPO_EALIGN, "%s: a pointer is not aligned to its element size", fn);
    return MI355PPO_OK;
}

RndLossParams rnd_loss_params(double update_proportion, double vf_coef, int M, int F, int64_t B) {
    RndLossParams P;
    P.proportion = (float)update_proportion;
    P.v_scale = (float)(vf_coef / (double)M);
    P.M = M;
    P.F = F;
    P.B = B;
    return P;
}

template <int STRIDE>
void rnd_moments_host(const unsigned char* src, int64_t B, int64_t row_bytes, int off, uint64_t* sums) {
    for (int p = 0; p < kRndPixels; ++p) {
        uint64_t s1 = 0, s2 = 0;
        for (int64_t r0 = 0; r0 < B; r0 += kRndSlab) {
            const int64_t r1 = (r0 + kRndSlab < B) ? r0 + kRndSlab : B;
            uint32_t a = 0, b = 0;
            for (int64_t r = r0; r < r1; ++r) {
                const uint32_t x = rnd_pixel<STRIDE>(src + r * row_bytes, p, off);
                a += x;
                b += x * x;
            }
            s1 += a;
            s2 += b;
        }
        sums[p] = s1;
        sums[kRndPixels + p] = s2;
    }
}

template <int STRIDE>
void rnd_normalize_host(const unsigned char* src, int64_t B, int64_t row_bytes, int off, const int64_t* idx, const double* mean, const double* sd,
                        float* out, int M) {
    for (int r = 0; r < M; ++r) {
        const int64_t i = rnd_clamp_index(idx ? idx[r] : (int64_t)r, B);
        for (int p = 0; p < kRndPixels; ++p)
            out[(int64_t)r * kRndPixels + p] = rnd_normalize(rnd_pixel<STRIDE>(src + i * row_bytes, p, off), mean[p], sd[p]);
    }
}

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_rnd_normalize_u8_f32(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride,
                                                         int64_t byte_offset, const int64_t* idx, const double* mean, const double* sd,
                                                         float* out, int M, void* stream) {
    const char* fn = "mi355ppo_rnd_normalize_u8_f32";
    if (int rc = rnd_normalize_args(fn, src, B, row_bytes, pixel_stride, byte_offset, idx, mean, sd, out, M)) return rc;
    const dim3 grid((M + kRndNormRows - 1) / kRndNormRows, (kRndPixels + 255) / 256);
    if (pixel_stride == 4)
        hipLaunchKernelGGL(rnd_normalize_kernel<4>, grid, dim3(256), 0, as_stream(stream), src, B, row_bytes, (int)byte_offset, idx, mean, sd, out, M);
    else
        hipLaunchKernelGGL(rnd_normalize_kernel<1>, grid, dim3(256), 0, as_stream(stream), src, B, row_bytes, (int)byte_offset, idx, mean, sd, out, M);
    return check_launch("rnd_normalize_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rnd_normalize_u8_f32_cpu(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride,
                                                             int64_t byte_offset, const int64_t* idx, const double* mean, const double* sd,
                                                             float* out, int M) {
    const char* fn = "mi355ppo_rnd_normalize_u8_f32_cpu";
    if (int rc = rnd_normalize_args(fn, src, B, row_bytes, pixel_stride, byte_offset, idx, mean, sd, out, M)) return rc;
    if (pixel_stride == 4)
        rnd_normalize_host<4>(src, B, row_bytes, (int)byte_offset, idx, mean, sd, out, M);
    else
        rnd_normalize_host<1>(src, B, row_bytes, (int)byte_offset, idx, mean, sd, out, M);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API size_t mi355ppo_rnd_obs_moments_workspace_bytes(int64_t B) {
    if (B <= 0 || B >= kRndMaxBatch) return 0;
    return (size_t)((B + kRndSlab - 1) / kRndSlab) * 2 * kRndPixels * sizeof(uint32_t);
}

extern "C" MI355PPO_API int mi355ppo_rnd_obs_moments_u8(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride,
                                                       int64_t byte_offset, uint64_t* sums, void* workspace, size_t workspace_bytes,
                                                       void* stream) {
    const char* fn = "mi355ppo_rnd_obs_moments_u8";
    if (int rc = rnd_moments_args(fn, src, B, row_bytes, pixel_stride, byte_offset, sums)) return rc;
    const size_t need = mi355ppo_rnd_obs_moments_workspace_bytes(B);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const int nslab = (int)((B + kRndSlab - 1) / kRndSlab);
    uint32_t* part = static_cast<uint32_t*>(workspace);
    const dim3 grid(nslab, (kRndPixels + 255) / 256);
    if (pixel_stride == 4)
        hipLaunchKernelGGL(rnd_moments_slab_kernel<4>, grid, dim3(256), 0, s, src, B, row_bytes, (int)byte_offset, part);
    else
        hipLaunchKernelGGL(rnd_moments_slab_kernel<1>, grid, dim3(256), 0, s, src, B, row_bytes, (int)byte_offset, part);
    if (int rc = check_launch("rnd_moments_slab_kernel")) return rc;
    hipLaunchKernelGGL(rnd_moments_fold_kernel, dim3((kRndPixels + 255) / 256), dim3(256), 0, s, part, nslab, sums);
    return check_launch("rnd_moments_fold_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rnd_obs_moments_u8_cpu(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride,
                                                           int64_t byte_offset, uint64_t* sums) {
    const char* fn = "mi355ppo_rnd_obs_moments_u8_cpu";
    if (int rc = rnd_moments_args(fn, src, B, row_bytes, pixel_stride, byte_offset, sums)) return rc;
    if (pixel_stride == 4)
        rnd_moments_host<4>(src, B, row_bytes, (int)byte_offset, sums);
    else
        rnd_moments_host<1>(src, B, row_bytes, (int)byte_offset, sums);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rnd_intrinsic_reward_f32(const float* target, const float* predict, float* out, int N, int F, void* stream) {
    const char* fn = "mi355ppo_rnd_intrinsic_reward_f32";
    if (int rc = rnd_intrinsic_args(fn, target, predict, out, N, F)) return rc;
    hipLaunchKernelGGL(rnd_intrinsic_kernel, dim3((N + 3) / 4), dim3(256), 0, as_stream(stream), target, predict, out, N);
    return check_launch("rnd_intrinsic_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rnd_intrinsic_reward_f32_cpu(const float* target, const float* predict, float* out, int N, int F) {
    const char* fn = "mi355ppo_rnd_intrinsic_reward_f32_cpu";
    if (int rc = rnd_intrinsic_args(fn, target, predict, out, N, F)) return rc;
    for (int r = 0; r < N; ++r) out[r] = rnd_row_sq_host(target + (int64_t)r * kRndF, predict + (int64_t)r * kRndF) * 0.5f;
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_rnd_reward_filter_f32(float* curiosity, float* rewems, double* stats3, float* filtered_out, int T, int N,
                                                          double gamma, void* stream) {
    const char* fn = "mi355ppo_rnd_reward_filter_f32";
    if (int rc = rnd_filter_args(fn, curiosity, rewems, stats3, filtered_out, T, N)) return rc;
    hipLaunchKernelGGL(rnd_reward_filter_kernel, dim3(1), dim3(256), 0, as_stream(stream), curiosity, rewems, stats3, filtered_out, T, N,
                       (float)gamma);
    return check_launch("rnd_reward_filter_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rnd_reward_filter_f32_cpu(float* curiosity, float* rewems, double* stats3, float* filtered_out, int T, int N,
                                                              double gamma) {
    const char* fn = "mi355ppo_rnd_reward_filter_f32_cpu";
    if (int rc = rnd_filter_args(fn, curiosity, rewems, stats3, filtered_out, T, N)) return rc;
    const float g = (float)gamma;
    const double count = (double)T * (double)N;
    std::vector<float> end(T);
    double s = 0.0;
    for (int t = 0; t < T; ++t)
        s += rnd_filter_scan_sum(curiosity + (int64_t)t * N, N, rewems[t], g, filtered_out ? filtered_out + (int64_t)t * N : nullptr, &end[t]);
    const double mean = s / count;
    s = 0.0;
    for (int t = 0; t < T; ++t) s += rnd_filter_scan_sq(curiosity + (int64_t)t * N, N, rewems[t], g, mean);
    rnd_update_from_moments(stats3, mean, s / count, (double)N);
    for (int t = 0; t < T; ++t) rewems[t] = end[t];
    const float div = (float)sqrt(stats3[1]);
    for (int64_t i = 0; i < (int64_t)T * N; ++i) curiosity[i] = curiosity[i] / div;
    return MI355PPO_OK;
}

// workspace: the mask count (an int in a 16-byte head), then the rows' mean squared errors
extern "C" MI355PPO_API size_t mi355ppo_rnd_loss_workspace_bytes(int M) { return M > 0 ? 16 + (size_t)M * sizeof(float) : 0; }

extern "C" MI355PPO_API int mi355ppo_rnd_loss_fwd_bwd_f32(const float* predict, const float* target, const float* u, double update_proportion,
                                                         const float* v_int, const float* int_returns, const int64_t* mb_inds, int64_t B,
                                                         double vf_coef, float* scalars_out, float* d_predict, float* d_v_int, int M, int F,
                                                         void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_rnd_loss_fwd_bwd_f32";
    if (int rc = rnd_loss_args(fn, predict, target, u, v_int, int_returns, mb_inds, B, scalars_out, d_predict, d_v_int, M, F)) return rc;
    const size_t need = mi355ppo_rnd_loss_workspace_bytes(M);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const RndLossParams P = rnd_loss_params(update_proportion, vf_coef, M, F, B);
    int* count = static_cast<int*>(workspace);
    float* row_mse = reinterpret_cast<float*>(static_cast<char*>(workspace) + 16);
    hipLaunchKernelGGL(rnd_loss_count_kernel, dim3(1), dim3(256), 0, s, u, M, P.proportion, count);
    if (int rc = check_launch("rnd_loss_count_kernel")) return rc;
    hipLaunchKernelGGL(rnd_loss_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, s, predict, target, u, v_int, int_returns, mb_inds, P, count,
                       row_mse, d_predict, d_v_int);
    if (int rc = check_launch("rnd_loss_rows_kernel")) return rc;
    hipLaunchKernelGGL(rnd_loss_fold_kernel, dim3(1), dim3(kRndFold), 0, s, row_mse, u, v_int, int_returns, mb_inds, P, count, scalars_out);
    return check_launch("rnd_loss_fold_kernel");
}

extern "C" MI355PPO_API int mi355ppo_rnd_loss_fwd_bwd_f32_cpu(const float* predict, const float* target, const float* u, double update_proportion,
                                                             const float* v_int, const float* int_returns, const int64_t* mb_inds, int64_t B,
                                                             double vf_coef, float* scalars_out, float* d_predict, float* d_v_int, int M, int F) {
    const char* fn = "mi355ppo_rnd_loss_fwd_bwd_f32_cpu";
    if (int rc = rnd_loss_args(fn, predict, target, u, v_int, int_returns, mb_inds, B, scalars_out, d_predict, d_v_int, M, F)) return rc;
    const RndLossParams P = rnd_loss_params(update_proportion, vf_coef, M, F, B);
    int count = 0;
    for (int m = 0; m < M; ++m) count += (u[m] < P.proportion) ? 1 : 0;
    const float scale = rnd_grad_scale(count);
    std::vector<float> row_mse(M);
    for (int r = 0; r < M; ++r) {
        const float* p = predict + (int64_t)r * kRndF;
        const float* t = target + (int64_t)r * kRndF;
        row_mse[r] = rnd_row_sq_host(p, t) * (1.0f / 512.0f);
        const bool on = u[r] < P.proportion;
        float* g = d_predict + (int64_t)r * kRndF;
        for (int f = 0; f < kRndF; ++f) g[f] = on ? (2.0f * (p[f] - t[f])) * scale : 0.0f;
        d_v_int[r] = (v_int[r] - int_returns[rnd_clamp_index(mb_inds[r], B)]) * P.v_scale;
    }
    double tf = 0.0, tv = 0.0;
    for (int k = 0; k < kRndFold; ++k) {
        double sf = 0.0, sv = 0.0;
        for (int m = k; m < M; m += kRndFold) {
            if (u[m] < P.proportion) sf += (double)row_mse[m];
            const double d = (double)(v_int[m] - int_returns[rnd_clamp_index(mb_inds[m], B)]);
            sv += d * d;
        }
        tf += sf;
        tv += sv;
    }
    rnd_loss_scalars(tf, tv, count, M, scalars_out);
    return MI355PPO_OK;
}
