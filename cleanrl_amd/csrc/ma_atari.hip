// The fused path of ppo_pettingzoo_ma_atari.py around the NatureCNN trunk kernels (MI355PPO_MA_ATARI=fused; ma_atari_rows.h says why the
// two agent-indicator planes of an (84, 84, 6) observation are a bias per observation):
//   * mi355ppo_ma_atari_split_u8: incoming six-channel frames -> the rollout's (84, 84, 4) rows + two indicator bytes per row, and a sticky
//     flag word when a plane is not constant (then the fused path does not apply and the learner says so);
//   * mi355ppo_ma_atari_conv1_wgrad_fold_f32: kernel P's (32, 4, 8, 8) weight gradient of the rows -> channels 0 - 3 of the (32, 6, 8, 8)
//     gradient, and channels 4 / 5 = sum_img v_j(img) * sum_p dz1[img][p][n] in one fixed order, no floating-point atomics.
// conv1's pack and forward with the per-observation bias are kernel Q's (conv1q.hip: mi355ppo_ma_atari_conv1_pack_f32 / _fwd_bits / _fwd_amax).
#include "common.h"
#include "ma_atari_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// One thread per group of four pixels: 24 bytes in (three 8-byte loads), 16 bytes out (one store).  Memory-bound: 42,336 B read and 28,224 B
// written per frame.
__global__ __launch_bounds__(256) void ma_split_kernel(const uint2* __restrict__ frames6, uint4* __restrict__ rows4, unsigned char* __restrict__ ind,
                                                       unsigned* __restrict__ flag, long long groups) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (g < groups) {
        const long long f = g / kMaGroups;
        const int k = (int)(g - f * kMaGroups);
        const uint2 head = frames6[f * (3 * kMaGroups)];                   // bytes 0..7 of the frame: pixel (0, 0) and the first two of (0, 1)
        const unsigned v4 = head.y & 255u, v5 = (head.y >> 8) & 255u;
        const uint2* src = frames6 + g * 3;
        const uint2 a = src[0], b = src[1], c = src[2];
        const uint32_t w[6] = {a.x, a.y, b.x, b.y, c.x, c.y};
        uint32_t o[4];
        bad = ma_split4(w, o, v4, v5);
        rows4[g] = make_uint4(o[0], o[1], o[2], o[3]);
        if (k == 0) {
            ind[2 * f] = (unsigned char)v4;
            ind[2 * f + 1] = (unsigned char)v5;
        }
    }
    if (bad) atomicOr(flag, 1u);                                           // sticky: only ever sets the bit
}

// Partial b = images [4 b, 4 b + 4): thread (q = tid / 32, n = tid % 32) adds strip q of channel n, thread n adds the eight strips and the
// image's two products onto the partial's two sums.  part: [b][j][n] doubles.
__global__ __launch_bounds__(256) void ma_fold_part_kernel(const float* __restrict__ dz1, const int64_t* __restrict__ inds, const unsigned char* __restrict__ ind,
                                                           double* __restrict__ part, long long images) {
    __shared__ double strips[kMaFoldStrips][32];
    const int tid = threadIdx.x, n = tid & 31, q = tid >> 5;
    const long long i0 = (long long)blockIdx.x * kMaFoldImgs;
    double acc4 = 0.0, acc5 = 0.0;
    for (int k = 0; k < kMaFoldImgs; ++k) {
        const long long img = i0 + k;
        if (img >= images) break;                                          // (block-uniform)
        strips[q][n] = ma_fold_strip(dz1 + img * (long long)(kMaOutPix * 32), n, q);
        __syncthreads();
        if (tid < 32) {
            double s = 0.0;
            for (int qq = 0; qq < kMaFoldStrips; ++qq) s = s + strips[qq][n];
            const long long row = inds ? inds[img] : img;
            acc4 = acc4 + (double)ind[2 * row] * s;
            acc5 = acc5 + (double)ind[2 * row + 1] * s;
        }
        __syncthreads();
    }
    if (tid < 32) {
        part[(long long)blockIdx.x * 64 + n] = acc4;
        part[(long long)blockIdx.x * 64 + 32 + n] = acc5;
    }
}

// One workgroup: the partials in four interleaved chains, the chains in order, one rounding; then every element of the (32, 6, 8, 8) gradient
// is written once -- channels 0 - 3 from kernel P's (32, 4, 8, 8) result, the 64 taps of channel 4 + j of output channel n = g[j][n].
__global__ __launch_bounds__(256) void ma_fold_final_kernel(const double* __restrict__ part, long long parts, const float* __restrict__ dW4,
                                                            float* __restrict__ dW6) {
    __shared__ double chain[kMaFoldChains][64];
    __shared__ float g[64];
    const int tid = threadIdx.x, k = tid & 63, c = tid >> 6;
    double s = 0.0;
    for (long long b = c; b < parts; b += kMaFoldChains) s = s + part[b * 64 + k];
    chain[c][k] = s;
    __syncthreads();
    if (tid < 64) {
        double t = 0.0;
        for (int cc = 0; cc < kMaFoldChains; ++cc) t = t + chain[cc][tid];
        g[tid] = (float)t;
    }
    __syncthreads();
    for (int e = tid; e < 32 * kMaInC * 64; e += 256) {
        const int n = e / (kMaInC * 64), r = e - n * (kMaInC * 64), ch = r >> 6, t = r & 63;
        dW6[e] = ch < kMaOutC ? dW4[(n * kMaOutC + ch) * 64 + t] : g[(ch - kMaOutC) * 32 + n];
    }
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_ma_atari_split_u8(const uint8_t* frames6, uint8_t* rows4, uint8_t* ind, uint32_t* flag, int64_t frames,
                                                       void* stream) {
    const char* fn = "mi355ppo_ma_atari_split_u8";
    MI355_REQUIRE(frames6 && rows4 && ind && flag, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(frames > 0 && frames <= (1 << 20), MI355PPO_EINVAL, "%s: frames=%lld out of range (1..1048576)", fn, (long long)frames);
    MI355_REQUIRE(aligned(frames6, 8) && aligned(rows4, 16) && aligned(flag, 4), MI355PPO_EALIGN,
                  "%s: frames must be 8-byte aligned, rows 16-byte aligned, the flag word 4-byte aligned", fn);
    const long long groups = (long long)frames * kMaGroups;
    hipLaunchKernelGGL(ma_split_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, as_stream(stream),
                       reinterpret_cast<const uint2*>(frames6), reinterpret_cast<uint4*>(rows4), ind, flag, groups);
    return check_launch(fn);
}

extern "C" MI355PPO_API size_t mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(int64_t images) {
    return images > 0 ? (size_t)ma_fold_parts(images) * 64 * sizeof(double) : 0;
}

extern "C" MI355PPO_API int mi355ppo_ma_atari_conv1_wgrad_fold_f32(const float* dz1, const int64_t* inds, const uint8_t* ind, const float* dW4,
                                                                   float* dW6, int64_t images, void* workspace, size_t workspace_bytes,
                                                                   void* stream) {
    const char* fn = "mi355ppo_ma_atari_conv1_wgrad_fold_f32";
    MI355_REQUIRE(dz1 && ind && dW4 && dW6, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(images > 0 && images <= (1 << 22), MI355PPO_EINVAL, "%s: images=%lld out of range (1..4194304)", fn, (long long)images);
    MI355_REQUIRE(aligned(dz1, 4) && aligned(inds, 8) && aligned(dW4, 4) && aligned(dW6, 4) && aligned(workspace, 8), MI355PPO_EALIGN,
                  "%s: misaligned pointer", fn);
    MI355_REQUIRE(workspace && workspace_bytes >= mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(images), MI355PPO_EWORKSPACE,
                  "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(images));
    const long long parts = ma_fold_parts(images);
    hipLaunchKernelGGL(ma_fold_part_kernel, dim3((unsigned)parts), dim3(256), 0, as_stream(stream), dz1, inds, ind, static_cast<double*>(workspace),
                       (long long)images);
    int rc = check_launch("ma_fold_part_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(ma_fold_final_kernel, dim3(1), dim3(256), 0, as_stream(stream), static_cast<const double*>(workspace), parts, dW4, dW6);
    return check_launch(fn);
}
