// LayerNorm + ReLU over channels-last activation rows, forward and backward (gfx950): what sits between the pre-activation forwards
// (kernel Q's PRE instance, kernel Z's Z_BIAS epilogue) and the next layer in pqn_atari_envpool.py's network.  Row math and the order of
// every sum: layernorm_rows.h (shared with the host twins, layernorm_twins.hip).
//
// Forward: a workgroup of ln_shape(D).nt threads walks ln_fwd_rows_per_wg(rows) rows; a row is read from HBM once into registers (at most
// four float4 per thread), reduced twice (sum, then squared deviations from the mean: double partials, wave butterfly, waves in order through
// LDS), normalised and stored with its mean / rstd, optionally its ReLU mask as bits (word w, bit b <-> flat element 32 w + b, the layout of
// the *_bits forwards) and its amax record (f16split.h).  gamma / beta are gathered from torch's (C, H, W) order once per workgroup.
// Backward: a workgroup walks a slab of ln_slab_rows(rows) rows, writes dz (and its amax record) and keeps the slab's column sums of dy * xh
// and dy in registers; they go to the caller's workspace, and one fold kernel adds the slabs in order in double -- no atomics, the same bits
// on every call.  Both kernels are bound by HBM: z (and dy) in, a (or dz) out.
#include "common.h"
#include "f16split.h"
#include "layernorm_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// sum of `v` over the workgroup in ln_fold_host's order, returned to every thread; `red` holds NT / 64 doubles
template <int NT>
__device__ __forceinline__ double ln_block_fold(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double total = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) total = total + red[w];
    __syncthreads();
    return total;
}

// the four parameters of quad e (e % 4 == 0, C % 4 == 0: four channels of one pixel) from torch's (C, H, W) order
__device__ __forceinline__ float4 ln_param4(const float* __restrict__ p, int e, int C, int HW) {
    const int i = ln_param(e, C, HW);
    return make_float4(p[i], p[i + HW], p[i + 2 * HW], p[i + 3 * HW]);
}

template <int NT, int KQ, bool BITS>
__global__ __launch_bounds__(NT) void ln_relu_fwd_kernel(const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         float* __restrict__ a, float* __restrict__ mean, float* __restrict__ rstd,
                                                         unsigned* __restrict__ bits, unsigned* __restrict__ amax, long long rows, int C, int HW,
                                                         int D, float eps, int rows_per_wg) {
    __shared__ double red[NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float4 gq[KQ], bq[KQ];
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const int e = 4 * (k * NT + t);
        gq[k] = bq[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (e < D) { gq[k] = ln_param4(gamma, e, C, HW); bq[k] = ln_param4(beta, e, C, HW); }
    }
    unsigned vmax = 0u;                        // bits of the largest value this lane stored (>= 0 after the ReLU)
    const long long r0 = (long long)blockIdx.x * rows_per_wg, r1 = r0 + rows_per_wg < rows ? r0 + rows_per_wg : rows;
    for (long long r = r0; r < r1; ++r) {
        const size_t base = (size_t)r * (size_t)D;
        float4 zq[KQ];
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int e = 4 * (k * NT + t);
            if (e < D) {
                zq[k] = *reinterpret_cast<const float4*>(z + base + e);
                s = s + (double)zq[k].x; s = s + (double)zq[k].y; s = s + (double)zq[k].z; s = s + (double)zq[k].w;
            }
        }
        const double mean_d = ln_block_fold<NT>(s, red) / (double)D;
        double q = 0.0;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int e = 4 * (k * NT + t);
            if (e < D) {
                const double d0 = (double)zq[k].x - mean_d, d1 = (double)zq[k].y - mean_d, d2 = (double)zq[k].z - mean_d, d3 = (double)zq[k].w - mean_d;
                q = q + d0 * d0; q = q + d1 * d1; q = q + d2 * d2; q = q + d3 * d3;
            }
        }
        const double var_d = ln_block_fold<NT>(q, red) / (double)D;
        const float m = (float)mean_d, rs = ln_rstd(var_d, eps);
        if (t == 0) { mean[r] = m; rstd[r] = rs; }
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int e = 4 * (k * NT + t);
            unsigned w = 0u;
            if (e < D) {
                const float4 o = make_float4(ln_out(zq[k].x, m, rs, gq[k].x, bq[k].x), ln_out(zq[k].y, m, rs, gq[k].y, bq[k].y),
                                             ln_out(zq[k].z, m, rs, gq[k].z, bq[k].z), ln_out(zq[k].w, m, rs, gq[k].w, bq[k].w));
                *reinterpret_cast<float4*>(a + base + e) = o;
                const float mx = __builtin_fmaxf(__builtin_fmaxf(o.x, o.y), __builtin_fmaxf(o.z, o.w));      // (a NaN is not recorded)
                vmax = __float_as_uint(mx) > vmax ? __float_as_uint(mx) : vmax;
                if constexpr (BITS)
                    w = ((o.x > 0.0f ? 1u : 0u) | (o.y > 0.0f ? 2u : 0u) | (o.z > 0.0f ? 4u : 0u) | (o.w > 0.0f ? 8u : 0u)) << (4 * (t & 7));
            }
            if constexpr (BITS) {              // eight lanes hold the eight nibbles of one word (D % 32 == 0: a word is whole or absent)
                w |= (unsigned)__shfl_xor((int)w, 1, 64);
                w |= (unsigned)__shfl_xor((int)w, 2, 64);
                w |= (unsigned)__shfl_xor((int)w, 4, 64);
                if ((t & 7) == 0 && e < D) bits[(base + (size_t)e) >> 5] = w;
            }
        }
    }
    if (amax) amax_commit(amax, vmax, blockIdx.x * (NT / 64) + wave, lane);      // (uniform; all lanes are here)
}

template <int NT, int KQ, bool ACT>
__global__ __launch_bounds__(NT) void ln_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ act, const float* __restrict__ z,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, float* __restrict__ dz, float* __restrict__ part,
                                                         unsigned* __restrict__ amax, long long rows, int C, int HW, int D, int slab_rows) {
    __shared__ double red[NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // gamma in the thread's quad order: in registers, or -- four quads per thread at 1,024 threads leave 128 registers: conv1's rows -- in LDS
    constexpr bool GL = KQ >= 4;
    __shared__ float4 gl[GL ? NT * KQ : 1];
    float4 gr[GL ? 1 : KQ], sg[KQ], sb[KQ];    // ... and the slab's column sums of dy * xh and dy
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const int e = 4 * (k * NT + t);
        sg[k] = sb[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        const float4 gv = e < D ? ln_param4(gamma, e, C, HW) : sg[k];
        if constexpr (GL) gl[k * NT + t] = gv;      // (read back by the same thread only: no barrier)
        else gr[k] = gv;
    }
    auto gq = [&](int k) -> float4 { if constexpr (GL) return gl[k * NT + t]; else return gr[k]; };
    float cmax = 0.0f;
    const long long r0 = (long long)blockIdx.x * slab_rows, r1 = r0 + slab_rows < rows ? r0 + slab_rows : rows;
    for (long long r = r0; r < r1; ++r) {
        const size_t base = (size_t)r * (size_t)D;
        const float m = mean[r], rs = rstd[r];
        float4 xq[KQ], dq[KQ];                 // xh and dy (under the mask)
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int e = 4 * (k * NT + t);
            if (e < D) {
                const float4 zz = *reinterpret_cast<const float4*>(z + base + e);
                float4 d = *reinterpret_cast<const float4*>(dy + base + e);
                if constexpr (ACT) {
                    const float4 aa = *reinterpret_cast<const float4*>(act + base + e);
                    d = make_float4(aa.x > 0.0f ? d.x : 0.0f, aa.y > 0.0f ? d.y : 0.0f, aa.z > 0.0f ? d.z : 0.0f, aa.w > 0.0f ? d.w : 0.0f);
                }
                xq[k] = make_float4(ln_xhat(zz.x, m, rs), ln_xhat(zz.y, m, rs), ln_xhat(zz.z, m, rs), ln_xhat(zz.w, m, rs));
                dq[k] = d;
                const float4 gm = gq(k);
                const float g0 = d.x * gm.x, g1 = d.y * gm.y, g2 = d.z * gm.z, g3 = d.w * gm.w;
                s1 = s1 + (double)g0; s1 = s1 + (double)g1; s1 = s1 + (double)g2; s1 = s1 + (double)g3;
                s2 = s2 + (double)g0 * (double)xq[k].x; s2 = s2 + (double)g1 * (double)xq[k].y;
                s2 = s2 + (double)g2 * (double)xq[k].z; s2 = s2 + (double)g3 * (double)xq[k].w;
            }
        }
        const float m1 = (float)(ln_block_fold<NT>(s1, red) / (double)D);
        const float m2 = (float)(ln_block_fold<NT>(s2, red) / (double)D);
#pragma unroll
        for (int k = 0; k < KQ; ++k) {
            const int e = 4 * (k * NT + t);
            if (e < D) {
                const float4 d = dq[k], x = xq[k], gm = gq(k);
                const float4 o = make_float4(ln_dz(d.x * gm.x, x.x, rs, m1, m2), ln_dz(d.y * gm.y, x.y, rs, m1, m2),
                                             ln_dz(d.z * gm.z, x.z, rs, m1, m2), ln_dz(d.w * gm.w, x.w, rs, m1, m2));
                *reinterpret_cast<float4*>(dz + base + e) = o;
                cmax = __builtin_fmaxf(cmax, __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(o.x), __builtin_fabsf(o.y)),
                                                             __builtin_fmaxf(__builtin_fabsf(o.z), __builtin_fabsf(o.w))));
                sg[k].x = sg[k].x + d.x * x.x; sg[k].y = sg[k].y + d.y * x.y; sg[k].z = sg[k].z + d.z * x.z; sg[k].w = sg[k].w + d.w * x.w;
                sb[k].x = sb[k].x + d.x; sb[k].y = sb[k].y + d.y; sb[k].z = sb[k].z + d.z; sb[k].w = sb[k].w + d.w;
            }
        }
    }
    float* const pg = part + (size_t)blockIdx.x * 2 * (size_t)D;
#pragma unroll
    for (int k = 0; k < KQ; ++k) {
        const int e = 4 * (k * NT + t);
        if (e < D) {
            *reinterpret_cast<float4*>(pg + e) = sg[k];
            *reinterpret_cast<float4*>(pg + D + e) = sb[k];
        }
    }
    if (amax) amax_commit(amax, __float_as_uint(cmax), blockIdx.x * (NT / 64) + wave, lane);
}

// dgamma / dbeta [ln_param(e)] = the slabs' partials of element e added in slab order in double, one rounding
__global__ __launch_bounds__(256) void ln_bwd_fold_kernel(const float* __restrict__ part, long long slabs, int C, int HW, int D,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * D) return;
    const int which = i >= D ? 1 : 0, e = i - which * D;
    const float* p = part + (size_t)which * (size_t)D + e;
    double s = 0.0;
    for (long long sl = 0; sl < slabs; ++sl) s = s + (double)p[(size_t)sl * 2 * (size_t)D];
    (which ? dbeta : dgamma)[ln_param(e, C, HW)] = (float)s;
}

static int ln_check(const char* fn, int64_t rows, int C, int HW) {
    MI355_REQUIRE(rows > 0 && C > 0 && HW > 0 && C % 4 == 0 && (long long)C * HW <= kLnMaxD, MI355PPO_EINVAL,
                  "%s: rows=%lld C=%d HW=%d (rows > 0, C a positive multiple of 4, C * HW <= %d)", fn, (long long)rows, C, HW, kLnMaxD);
    return MI355PPO_OK;
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_layernorm_relu_fwd_f32(const float* z, const float* gamma, const float* beta, float* a, float* mean,
                                                            float* rstd, uint32_t* mask_bits, uint32_t* a_amax, int64_t rows, int C, int HW,
                                                            double eps, void* stream) {
    const char* fn = "mi355ppo_layernorm_relu_fwd_f32";
    MI355_REQUIRE(z && gamma && beta && a && mean && rstd, MI355PPO_EINVAL, "%s: null pointer", fn);
    int rc = ln_check(fn, rows, C, HW);
    if (rc) return rc;
    const int D = C * HW;
    MI355_REQUIRE(!mask_bits || D % 32 == 0, MI355PPO_EINVAL, "%s: mask bits need C * HW %% 32 == 0 (%d)", fn, D);
    MI355_REQUIRE(aligned(z, 16) && aligned(a, 16) && aligned(gamma, 4) && aligned(beta, 4) && aligned(mean, 4) && aligned(rstd, 4) &&
                  aligned(mask_bits, 4) && aligned(a_amax, 64), MI355PPO_EALIGN, "%s: z / a must be 16-byte aligned, the amax record 64-byte aligned", fn);
    const int rpw = ln_fwd_rows_per_wg(rows);
    const dim3 grid((unsigned)((rows + rpw - 1) / rpw));
    const LnShape sh = ln_shape(D);
#define MI355_LN_FWD(NT_, KQ_)                                                                                                                    \
    do {                                                                                                                                          \
        if (mask_bits)                                                                                                                            \
            hipLaunchKernelGGL((ln_relu_fwd_kernel<NT_, KQ_, true>), grid, dim3(NT_), 0, as_stream(stream), z, gamma, beta, a, mean, rstd,        \
                               mask_bits, a_amax, (long long)rows, C, HW, D, (float)eps, rpw);                                                    \
        else                                                                                                                                      \
            hipLaunchKernelGGL((ln_relu_fwd_kernel<NT_, KQ_, false>), grid, dim3(NT_), 0, as_stream(stream), z, gamma, beta, a, mean, rstd,       \
                               mask_bits, a_amax, (long long)rows, C, HW, D, (float)eps, rpw);                                                    \
    } while (0)
    if (sh.nt == 256) MI355_LN_FWD(256, 1);
    else if (sh.nt == 512) MI355_LN_FWD(512, 2);
    else if (sh.kq == 2) MI355_LN_FWD(1024, 2);
    else MI355_LN_FWD(1024, 4);
#undef MI355_LN_FWD
    return check_launch(fn);
}

extern "C" MI355PPO_API size_t mi355ppo_layernorm_bwd_workspace_bytes(int64_t rows, int C, int HW) {
    if (rows <= 0 || C <= 0 || HW <= 0 || (long long)C * HW > kLnMaxD) return 0;
    return (size_t)ln_slabs(rows) * 2 * (size_t)C * (size_t)HW * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_layernorm_relu_bwd_f32(const float* dy, const float* act, const float* z, const float* mean, const float* rstd,
                                                            const float* gamma, float* dz, float* dgamma, float* dbeta, uint32_t* dz_amax,
                                                            int64_t rows, int C, int HW, void* ws, size_t ws_bytes, void* stream) {
    const char* fn = "mi355ppo_layernorm_relu_bwd_f32";
    MI355_REQUIRE(dy && z && mean && rstd && gamma && dz && dgamma && dbeta, MI355PPO_EINVAL, "%s: null pointer", fn);
    int rc = ln_check(fn, rows, C, HW);
    if (rc) return rc;
    const int D = C * HW;
    MI355_REQUIRE(aligned(dy, 16) && aligned(act, 16) && aligned(z, 16) && aligned(dz, 16) && aligned(mean, 4) && aligned(rstd, 4) &&
                  aligned(gamma, 4) && aligned(dgamma, 4) && aligned(dbeta, 4) && aligned(dz_amax, 64), MI355PPO_EALIGN,
                  "%s: dy / act / z / dz must be 16-byte aligned, the amax record 64-byte aligned", fn);
    const size_t need = mi355ppo_layernorm_bwd_workspace_bytes(rows, C, HW);
    MI355_REQUIRE(ws && aligned(ws, 16) && ws_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace of %zu bytes, %zu needed (mi355ppo_layernorm_bwd_workspace_bytes)",
                  fn, ws ? ws_bytes : (size_t)0, need);
    const int slab_rows = ln_slab_rows(rows);
    const long long slabs = ln_slabs(rows);
    float* const part = static_cast<float*>(ws);
    const LnShape sh = ln_shape(D);
#define MI355_LN_BWD(NT_, KQ_)                                                                                                                    \
    do {                                                                                                                                          \
        if (act)                                                                                                                                  \
            hipLaunchKernelGGL((ln_relu_bwd_kernel<NT_, KQ_, true>), dim3((unsigned)slabs), dim3(NT_), 0, as_stream(stream), dy, act, z, mean,    \
                               rstd, gamma, dz, part, dz_amax, (long long)rows, C, HW, D, slab_rows);                                             \
        else                                                                                                                                      \
            hipLaunchKernelGGL((ln_relu_bwd_kernel<NT_, KQ_, false>), dim3((unsigned)slabs), dim3(NT_), 0, as_stream(stream), dy, act, z, mean,   \
                               rstd, gamma, dz, part, dz_amax, (long long)rows, C, HW, D, slab_rows);                                             \
    } while (0)
    if (sh.nt == 256) MI355_LN_BWD(256, 1);
    else if (sh.nt == 512) MI355_LN_BWD(512, 2);
    else if (sh.kq == 2) MI355_LN_BWD(1024, 2);
    else MI355_LN_BWD(1024, 4);
#undef MI355_LN_BWD
    rc = check_launch(fn);
    if (rc) return rc;
    hipLaunchKernelGGL(ln_bwd_fold_kernel, dim3((unsigned)((2 * D + 255) / 256)), dim3(256), 0, as_stream(stream), part, slabs, C, HW, D, dgamma,
                       dbeta);
    return check_launch(fn);
}
