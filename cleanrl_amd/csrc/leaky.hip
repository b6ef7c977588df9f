// LeakyReLU over a flat f32 tensor, forward and backward (gfx950): what follows the pre-activation forwards (kernel Z's Z_BIAS epilogue) and
// the all-ones-mask data gradients in RNDModel's predictor / target stacks (cleanrl/ppo_rnd_envpool.py:188-233).  Element math: leaky_rows.h
// (shared with the host twins, leaky_twins.hip).
//
// A thread owns quads q, q + grid * 256, ... (elements 4 q .. 4 q + 3: one 16-byte load and store; the last quad of an n that is no multiple
// of 4 element by element, nothing past n is touched).  Eight neighbouring lanes hold the eight nibbles of one mask word and fold them with
// three shuffles, as the LayerNorm forward does.  Both kernels may work in place: a thread reads its quad before it writes it.  The amax record
// (f16split.h) takes one integer atomic max per wave -- no float atomics, the same bits on every call.  Bound by HBM: 4 bytes in, 4 out.
#include "common.h"
#include "f16split.h"
#include "leaky_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

__device__ __forceinline__ float4 leaky_load4(const float* __restrict__ p, long long e, long long n) {
    if (e + 3 < n) return *reinterpret_cast<const float4*>(p + e);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (e < n) v.x = p[e];
    if (e + 1 < n) v.y = p[e + 1];
    if (e + 2 < n) v.z = p[e + 2];
    return v;
}
__device__ __forceinline__ void leaky_store4(float* __restrict__ p, long long e, long long n, float4 v) {
    if (e + 3 < n) { *reinterpret_cast<float4*>(p + e) = v; return; }
    if (e < n) p[e] = v.x;
    if (e + 1 < n) p[e + 1] = v.y;
    if (e + 2 < n) p[e + 2] = v.z;
}
__device__ __forceinline__ float leaky_absmax4(float m, float4 v) {      // (a NaN is not recorded)
    return __builtin_fmaxf(m, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)),
                                              __builtin_fmaxf(__builtin_fabsf(v.z), __builtin_fabsf(v.w))));
}

template <bool BITS>
__global__ __launch_bounds__(256) void leaky_relu_fwd_kernel(const float* z, float* a, unsigned* __restrict__ bits, unsigned* __restrict__ amax,
                                                             long long n, float slope) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long nquads = (n + 3) / 4;
    float cmax = 0.0f;
    for (long long q0 = (long long)blockIdx.x * 256; q0 < nquads; q0 += (long long)gridDim.x * 256) {      // (uniform over the workgroup)
        const long long q = q0 + t, e = 4 * q;
        const float4 v = leaky_load4(z, e, n);       // elements past n: 0, whose bit is 0 and whose value is not stored
        const float4 o = make_float4(leaky_fwd(v.x, slope), leaky_fwd(v.y, slope), leaky_fwd(v.z, slope), leaky_fwd(v.w, slope));
        leaky_store4(a, e, n, o);
        cmax = leaky_absmax4(cmax, o);
        if constexpr (BITS) {
            unsigned w = ((v.x > 0.0f ? 1u : 0u) | (v.y > 0.0f ? 2u : 0u) | (v.z > 0.0f ? 4u : 0u) | (v.w > 0.0f ? 8u : 0u)) << (4 * (t & 7));
            w |= (unsigned)__shfl_xor((int)w, 1, 64);
            w |= (unsigned)__shfl_xor((int)w, 2, 64);
            w |= (unsigned)__shfl_xor((int)w, 4, 64);
            if ((t & 7) == 0 && q < nquads) bits[q >> 3] = w;
        }
    }
    if (amax) amax_commit(amax, __float_as_uint(cmax), blockIdx.x * 4 + wave, lane);      // (uniform; all lanes are here)
}

__global__ __launch_bounds__(256) void leaky_relu_bwd_kernel(const float* da, const unsigned* __restrict__ bits, float* dz,
                                                             unsigned* __restrict__ amax, long long n, float slope) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long nquads = (n + 3) / 4;
    float cmax = 0.0f;
    for (long long q0 = (long long)blockIdx.x * 256; q0 < nquads; q0 += (long long)gridDim.x * 256) {
        const long long q = q0 + t, e = 4 * q;
        if (q < nquads) {
            const float4 v = leaky_load4(da, e, n);
            const unsigned b = bits[q >> 3] >> (4 * (t & 7));
            const float4 o = make_float4(leaky_bwd(v.x, b & 1u, slope), leaky_bwd(v.y, b & 2u, slope), leaky_bwd(v.z, b & 4u, slope),
                                         leaky_bwd(v.w, b & 8u, slope));
            leaky_store4(dz, e, n, o);
            cmax = leaky_absmax4(cmax, o);           // (elements past n: da read as 0 -> 0)
        }
    }
    if (amax) amax_commit(amax, __float_as_uint(cmax), blockIdx.x * 4 + wave, lane);
}

static int leaky_grid(long long n) {
    const long long need = ((n + 3) / 4 + 255) / 256, cap = (long long)cu_count() * 8;
    return (int)(need < cap ? need : cap);
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_leaky_relu_fwd_f32(const float* z, float* a, uint32_t* mask_bits, uint32_t* a_amax, int64_t n, double slope,
                                                        void* stream) {
    const char* fn = "mi355ppo_leaky_relu_fwd_f32";
    MI355_REQUIRE(z && a, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld (n > 0)", fn, (long long)n);
    MI355_REQUIRE(aligned(z, 16) && aligned(a, 16) && aligned(mask_bits, 4) && aligned(a_amax, 64), MI355PPO_EALIGN,
                  "%s: z / a must be 16-byte aligned, the amax record 64-byte aligned", fn);
    const dim3 grid((unsigned)leaky_grid(n));
    if (mask_bits)
        hipLaunchKernelGGL(leaky_relu_fwd_kernel<true>, grid, dim3(256), 0, as_stream(stream), z, a, mask_bits, a_amax, (long long)n, (float)slope);
    else
        hipLaunchKernelGGL(leaky_relu_fwd_kernel<false>, grid, dim3(256), 0, as_stream(stream), z, a, mask_bits, a_amax, (long long)n, (float)slope);
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_leaky_relu_bwd_f32(const float* da, const uint32_t* mask_bits, float* dz, uint32_t* dz_amax, int64_t n,
                                                        double slope, void* stream) {
    const char* fn = "mi355ppo_leaky_relu_bwd_f32";
    MI355_REQUIRE(da && mask_bits && dz, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld (n > 0)", fn, (long long)n);
    MI355_REQUIRE(aligned(da, 16) && aligned(dz, 16) && aligned(mask_bits, 4) && aligned(dz_amax, 64), MI355PPO_EALIGN,
                  "%s: da / dz must be 16-byte aligned, the amax record 64-byte aligned", fn);
    hipLaunchKernelGGL(leaky_relu_bwd_kernel, dim3((unsigned)leaky_grid(n)), dim3(256), 0, as_stream(stream), da, mask_bits, dz, dz_amax,
                       (long long)n, (float)slope);
    return check_launch(fn);
}
