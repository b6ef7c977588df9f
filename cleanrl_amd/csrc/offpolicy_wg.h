// Workgroup-level device helpers of the off-policy kernels (offpolicy.hip: DDPG / TD3, sac.hip: SAC): one tile of kOpRows rows
// through a 256-wide layer (forward, head, masked data gradient, weight gradient), the f64 slot fold (wg_fold_scalars: the two row
// scalars of the Q heads in dqn_atari.hip / rainbow.hip), the ring gather and the host-side argument checks of the device entry points.  Included by the kernel files only; the row math and the shape check both
// sides share are in offpolicy_rows.h.
#pragma once
#include "common.h"
#include "offpolicy_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kOpT = 256;                           // threads per workgroup
constexpr int kOpKT = 8;                            // k-depth of the staged weight tile
constexpr int kOpTileLd = kOpH + 8;                 // padded row of the tile: 8 mod 32 banks (see wg_forward)
constexpr int kOpXS = kOpMaxObs + kOpMaxAct;        // stride of the input rows (obs | action)

// out[r, j] = act(b[j] + sum_k xin[r, k] * W[j, k]) for the tile's kOpRows rows and j < 256.  Ends with a barrier.
template <bool RELU>
__device__ void wg_forward(const float* xin, int xs, int K, const float* __restrict__ W, const float* __restrict__ b, float* out, int os,
                           float* tile) {
    const int t = threadIdx.x;
    float acc[kOpRows];
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) acc[r] = 0.0f;
    float nxt[kOpKT];
    // thread t stages elements idx = t + 256 * i: unit idx / 8, column idx % 8
#pragma unroll
    for (int i = 0; i < kOpKT; ++i) {
        const int idx = t + kOpT * i, j = idx / kOpKT, kk = idx % kOpKT;
        nxt[i] = (kk < K) ? W[(int64_t)j * K + kk] : 0.0f;
    }
    for (int k0 = 0; k0 < K; k0 += kOpKT) {
#pragma unroll
        for (int i = 0; i < kOpKT; ++i) {
            const int idx = t + kOpT * i;
            tile[(idx % kOpKT) * kOpTileLd + idx / kOpKT] = nxt[i];
        }
        __syncthreads();
        const int k1 = k0 + kOpKT;
        if (k1 < K) {
#pragma unroll
            for (int i = 0; i < kOpKT; ++i) {
                const int idx = t + kOpT * i, j = idx / kOpKT, kk = k1 + idx % kOpKT;
                nxt[i] = (kk < K) ? W[(int64_t)j * K + kk] : 0.0f;
            }
        }
        const int kn = (K - k0 < kOpKT) ? K - k0 : kOpKT;
        for (int kk = 0; kk < kn; ++kk) {
            const float w = tile[kk * kOpTileLd + t];
#pragma unroll
            for (int r = 0; r < kOpRows; ++r) acc[r] = op_mac(acc[r], xin[r * xs + k0 + kk], w);
        }
        __syncthreads();
    }
    const float bj = b[t];
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) {
        const float v = acc[r] + bj;
        out[r * os + t] = RELU ? op_relu(v) : v;
    }
    __syncthreads();
}

// out[r * J + j] = b[j] + sum_k h[r, k] * W[j, k] (k < 256) for r < kOpRows, j < J (J <= kOpMaxAct).  Ends with a barrier.
__device__ void wg_head(const float* h, int hs, const float* __restrict__ W, const float* __restrict__ b, int J, float* out) {
    const int t = threadIdx.x;
    if (t < kOpRows * J) {
        const int r = t / J, j = t % J;
        const float* w = W + j * kOpH;
        float acc = 0.0f;
        for (int k = 0; k < kOpH; ++k) acc = op_mac(acc, h[r * hs + k], w[k]);
        out[t] = acc + b[j];
    }
    __syncthreads();
}

// io[r, k] = relu'(io[r, k]) * sum_{j < J} dz[r * ds + j] * W[j * ldw + k] for k < 256 (in place over the layer's ReLU output).
__device__ void wg_dgrad_masked(const float* dz, int ds, int J, const float* __restrict__ W, int ldw, float* io, int ios) {
    const int t = threadIdx.x;
    float acc[kOpRows];
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) acc[r] = 0.0f;
    for (int j = 0; j < J; ++j) {
        const float w = W[(int64_t)j * ldw + t];
#pragma unroll
        for (int r = 0; r < kOpRows; ++r) acc[r] = op_mac(acc[r], dz[r * ds + j], w);
    }
#pragma unroll
    for (int r = 0; r < kOpRows; ++r) io[r * ios + t] = op_relu_bwd(io[r * ios + t], acc[r]);
    __syncthreads();
}

// part[e] (+)= sum_{r < nr} dz[r, j] * in[r, k], e = j * K + k; then the bias: part_b[j] (+)= sum_r dz[r, j].  Ends with a barrier.
__device__ void wg_wgrad(const float* dz, int ds, const float* in, int is, int J, int K, float* __restrict__ part_w, float* __restrict__ part_b,
                         bool first, int nr) {
    const int t = threadIdx.x;
    const int n = J * K;
    for (int e = t; e < n; e += kOpT) {
        const int j = e / K, k = e - j * K;
        float acc = 0.0f;
        for (int r = 0; r < nr; ++r) acc = op_mac(acc, dz[r * ds + j], in[r * is + k]);
        part_w[e] = first ? acc : part_w[e] + acc;
    }
    if (t < J) {
        float acc = 0.0f;
        for (int r = 0; r < nr; ++r) acc = acc + dz[r * ds + t];
        part_b[t] = first ? acc : part_b[t] + acc;
    }
    __syncthreads();
}

// mean over M rows: slot t adds rows t, t + 256, ... in f64, thread 0 adds the slots in order.  Valid in thread 0; ends with a barrier.
__device__ float wg_fold_mean(const float* __restrict__ v, int M, double* red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < M; k += kOpFold) s += (double)v[k];
    red[threadIdx.x] = s;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int t = 0; t < kOpFold; ++t) tot += red[t];
    __syncthreads();
    return (float)(tot / (double)M);
}

// scalars[s] = the mean of rows[s * Mp .. s * Mp + M) for the two row scalars of a head update (the extra workgroup of its wgrad kernel)
__device__ void wg_fold_scalars(const float* __restrict__ rows, int Mp, int M, double* red, float* __restrict__ scalars) {
    for (int s = 0; s < 2; ++s) {
        const float m = wg_fold_mean(rows + (int64_t)s * Mp, M, red);
        if (threadIdx.x == 0) scalars[s] = m;
    }
}

// The value of a uniform int behind an empty statement the optimiser cannot see through.  A network's six pointers derived from it
// are formed where a phase uses them and die with it; derived once in front of the tile loop they all stay in SGPRs across it
// (two networks, the partial's offsets and the ring: more than the 102 a wave has, so the allocator spilled them into VGPR lanes).
__device__ __forceinline__ int op_here(int v) {
    asm volatile("" : "+s"(v));
    return v;
}

struct OpRing {
    const float *obs, *next_obs, *actions, *rewards, *dones;
    const int64_t *bi, *ei;
    int64_t slots;
    int N;
};
__device__ __forceinline__ int64_t ring_row(const OpRing& R, int m) { return op_clamp(R.bi[m], R.slots) * R.N + op_clamp(R.ei[m], R.N); }

// ------------------------------------------------------------------------------------------------ host-side argument checks
static int64_t op_mp(int M) { return ((int64_t)M + 63) / 64 * 64; }

static int op_ring_args(const char* fn, OpRing& R, const float* obs, const float* next_obs, const float* actions, const float* rewards,
                        const float* dones, const int64_t* bi, const int64_t* ei, int64_t slots, int N) {
    MI355_REQUIRE(bi && ei, MI355PPO_EINVAL, "%s: null index pointer", fn);
    MI355_REQUIRE(slots > 0 && N > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, N);
    R.obs = obs;
    R.next_obs = next_obs;
    R.actions = actions;
    R.rewards = rewards;
    R.dones = dones;
    R.bi = bi;
    R.ei = ei;
    R.slots = slots;
    R.N = N;
    return MI355PPO_OK;
}

// the workspace of a *_fwd_bwd entry point: present, at least `need` bytes, 16-byte aligned
static int op_workspace_ok(const char* fn, const void* workspace, size_t workspace_bytes, size_t need) {
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    return MI355PPO_OK;
}

// grads[i] = sum of the G partials in ascending order and scalars[s] = sign * mean(rows s) for s < nsc (op_fold_kernel, offpolicy.hip)
int op_fold_launch(hipStream_t s, const float* part, int G, int64_t P, float* grads, const float* rows, int Mp, int M, int nsc, float sign,
                   float* scalars);

}  // namespace mi355ppo
