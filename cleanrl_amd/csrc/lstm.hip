// The done-masked LSTM sequence scans of ppo_atari_lstm.py (cleanrl/ppo_atari_lstm.py:140-158, get_states): forward and
// backward through all T steps in ONE launch each, instead of T length-1 nn.LSTM calls and their T autograd graphs.
// Math and record layout: lstm_rows.h.  Design:
//   * one workgroup of 512 threads owns E envs for all T steps: no grid-wide synchronisation, and one env's chain is walked in
//     a fixed order whatever B and E are (deterministic and batch-invariant);
//   * forward, row layout: thread j holds gate row W_hh[j, :] (128 f32) in VGPRs for the whole launch; the masked hidden
//     state hk is broadcast from LDS; after one barrier thread (e, u) runs the cell update with c in a register;
//   * backward, column layout: thread (q, k) holds W_hh[q*128 .. q*128+127, k]; each computes the partial of W_hh^T dgx over
//     its gate block, the four partials are folded through LDS by the thread that owns the unit;
//   * the next step's streamed inputs (gx / dh, done, the record) are loaded one step ahead, so that the global latency is
//     spent under the current step's product and barriers;
//   * E in {1, 2, 4, 8}: the smallest that keeps ceil(B / E) workgroups within one per CU.
#include "common.h"
#include "lstm_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {
namespace {

constexpr int kThreads = kLstmThreads;            // launch shape and the E rule: lstm_rows.h

// Unit pairs (env e, unit u) owned by thread tid: p = tid + 512 r, e = p / 128, u = p % 128.
template <int E>
constexpr int kPairs = kLstmPairs<E>;

template <int E>
__global__ __launch_bounds__(kThreads) void lstm_fwd_kernel(const float* __restrict__ gx, const float* __restrict__ w_hh,
                                                            const float* __restrict__ h0, const float* __restrict__ c0,
                                                            const float* __restrict__ done, float* __restrict__ hout,
                                                            float* __restrict__ hT, float* __restrict__ cT,
                                                            float* __restrict__ rec, int T, int B) {
    constexpr int P = kPairs<E>;
    __shared__ __attribute__((aligned(16))) float s_hk[E][kLstmH];
    __shared__ float s_a[E][kLstmG];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * E;
    const size_t TB = (size_t)T * B;

    float w[kLstmH];                                                   // gate row j = tid (once per launch; w_hh may be a
#pragma unroll                                                         // view at any 4-byte offset of the flat parameter buffer)
    for (int k = 0; k < kLstmH; ++k) w[k] = w_hh[(size_t)tid * kLstmH + k];
    float hk[P], ck[P], keep_next[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int p = tid + kThreads * r, e = p / kLstmH, u = p % kLstmH, b = b0 + e;
        hk[r] = 0.0f;
        ck[r] = 0.0f;
        keep_next[r] = 0.0f;
        if (e < E && b < B) {
            const float keep = 1.0f - done[b];
            hk[r] = keep * h0[(size_t)b * kLstmH + u];
            ck[r] = keep * c0[(size_t)b * kLstmH + u];
        }
        if (e < E) s_hk[e][u] = hk[r];
    }
    float gxv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) gxv[e] = (b0 + e < B) ? gx[(size_t)(b0 + e) * kLstmG + tid] : 0.0f;
    __syncthreads();

    for (int t = 0; t < T; ++t) {
        // ---- prefetch step t + 1's inputs
        float gxn[E];
#pragma unroll
        for (int e = 0; e < E; ++e) gxn[e] = (t + 1 < T && b0 + e < B) ? gx[((size_t)(t + 1) * B + b0 + e) * kLstmG + tid] : 0.0f;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int e = (tid + kThreads * r) / kLstmH, b = b0 + e;
            if (e < E && b < B && t + 1 < T) keep_next[r] = 1.0f - done[(size_t)(t + 1) * B + b];
        }
        // ---- a = gx + W_hh hk (row j = tid)
#pragma unroll
        for (int e = 0; e < E; ++e) s_a[e][tid] = gxv[e] + lstm_dot128(w, s_hk[e]);
        __syncthreads();
        // ---- the cell update of the owned units
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int p = tid + kThreads * r, e = p / kLstmH, u = p % kLstmH, b = b0 + e;
            if (e >= E) continue;
            const LstmCell s = lstm_cell_fwd(s_a[e][u], s_a[e][kLstmH + u], s_a[e][2 * kLstmH + u], s_a[e][3 * kLstmH + u], ck[r]);
            if (b < B) {
                const size_t row = (size_t)t * B + b;
                hout[row * kLstmH + u] = s.h;
                if (rec) {
                    float* g = rec + row * kLstmG + u;
                    g[0] = s.i;
                    g[kLstmH] = s.f;
                    g[2 * kLstmH] = s.g;
                    g[3 * kLstmH] = s.o;
                    rec[TB * 4 * kLstmH + row * kLstmH + u] = s.c;
                    rec[TB * 5 * kLstmH + row * kLstmH + u] = hk[r];
                    rec[TB * 6 * kLstmH + row * kLstmH + u] = ck[r];
                }
                if (t + 1 == T) {
                    hT[(size_t)b * kLstmH + u] = s.h;
                    cT[(size_t)b * kLstmH + u] = s.c;
                }
            }
            hk[r] = keep_next[r] * s.h;
            ck[r] = keep_next[r] * s.c;
            s_hk[e][u] = hk[r];
        }
#pragma unroll
        for (int e = 0; e < E; ++e) gxv[e] = gxn[e];
        __syncthreads();
    }
}

// Step t's streamed inputs of one owned unit in the backward.
struct BwdIn {
    float i, f, g, o, c, ck, dh, keep;
};

__device__ __forceinline__ BwdIn bwd_load(const float* __restrict__ rec, const float* __restrict__ dh, const float* __restrict__ done,
                                          size_t TB, int t, int B, int b, int u) {
    const size_t row = (size_t)t * B + b;
    const float* g = rec + row * kLstmG + u;
    BwdIn in;
    in.i = g[0];
    in.f = g[kLstmH];
    in.g = g[2 * kLstmH];
    in.o = g[3 * kLstmH];
    in.c = rec[TB * 4 * kLstmH + row * kLstmH + u];
    in.ck = rec[TB * 6 * kLstmH + row * kLstmH + u];
    in.dh = dh[row * kLstmH + u];
    in.keep = 1.0f - done[row];
    return in;
}

template <int E>
__global__ __launch_bounds__(kThreads) void lstm_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ dhT,
                                                            const float* __restrict__ dcT, const float* __restrict__ rec,
                                                            const float* __restrict__ w_hh, const float* __restrict__ done,
                                                            float* __restrict__ dgx, float* __restrict__ dh0, float* __restrict__ dc0,
                                                            int T, int B) {
    constexpr int P = kPairs<E>;
    __shared__ __attribute__((aligned(16))) float s_dg[E][kLstmG];
    __shared__ float s_part[E][4][kLstmH];
    const int tid = threadIdx.x;
    const int q = tid / kLstmH, k = tid % kLstmH;
    const int b0 = blockIdx.x * E;
    const size_t TB = (size_t)T * B;

    float w[kLstmH];                                                   // column k of gate block q
#pragma unroll
    for (int r = 0; r < kLstmH; ++r) w[r] = w_hh[(size_t)(q * kLstmH + r) * kLstmH + k];

    float dc[P], keep[P];
    BwdIn in[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int p = tid + kThreads * r, e = p / kLstmH, u = p % kLstmH, b = b0 + e;
        dc[r] = 0.0f;
        keep[r] = 0.0f;
        in[r] = BwdIn{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (e < E && b < B) {
            if (dcT) dc[r] = dcT[(size_t)b * kLstmH + u];
            in[r] = bwd_load(rec, dh, done, TB, T - 1, B, b, u);
        }
    }

    for (int t = T - 1; t >= 0; --t) {
        // ---- the owned units: dh into h_t (the heads' dh + W_hh^T dgx of step t+1, masked by keep_{t+1}) -> dgx[t]
        BwdIn nx[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int p = tid + kThreads * r, e = p / kLstmH, u = p % kLstmH, b = b0 + e;
            if (e >= E) continue;
            float carry = 0.0f;
            if (t == T - 1) {
                if (dhT && b < B) carry = dhT[(size_t)b * kLstmH + u];
            } else {
                carry = keep[r] * lstm_fold4(s_part[e][0][u], s_part[e][1][u], s_part[e][2][u], s_part[e][3][u]);
            }
            const LstmCellGrad d = lstm_cell_bwd(in[r].i, in[r].f, in[r].g, in[r].o, in[r].c, in[r].ck, in[r].dh + carry, dc[r]);
            s_dg[e][u] = d.dai;
            s_dg[e][kLstmH + u] = d.daf;
            s_dg[e][2 * kLstmH + u] = d.dag;
            s_dg[e][3 * kLstmH + u] = d.dao;
            keep[r] = in[r].keep;
            dc[r] = in[r].keep * d.dck;
            if (b < B) {
                float* o = dgx + ((size_t)t * B + b) * kLstmG + u;
                o[0] = d.dai;
                o[kLstmH] = d.daf;
                o[2 * kLstmH] = d.dag;
                o[3 * kLstmH] = d.dao;
                if (t == 0 && dc0) dc0[(size_t)b * kLstmH + u] = dc[r];
                nx[r] = t > 0 ? bwd_load(rec, dh, done, TB, t - 1, B, b, u) : in[r];      // step t-1, under the product below
            } else {
                nx[r] = in[r];
            }
        }
        __syncthreads();
        // ---- partial of W_hh^T dgx[t] over gate block q, column k
#pragma unroll
        for (int e = 0; e < E; ++e) s_part[e][q][k] = lstm_dot128(w, &s_dg[e][q * kLstmH]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < P; ++r) in[r] = nx[r];
    }
    if (dh0) {
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int p = tid + kThreads * r, e = p / kLstmH, u = p % kLstmH, b = b0 + e;
            if (e < E && b < B)
                dh0[(size_t)b * kLstmH + u] = keep[r] * lstm_fold4(s_part[e][0][u], s_part[e][1][u], s_part[e][2][u], s_part[e][3][u]);
        }
    }
}

template <int E>
int launch_fwd(const float* gx, const float* w_hh, const float* h0, const float* c0, const float* done, float* h, float* hT, float* cT,
               float* rec, int T, int B, hipStream_t s) {
    hipLaunchKernelGGL((lstm_fwd_kernel<E>), dim3((B + E - 1) / E), dim3(kThreads), 0, s, gx, w_hh, h0, c0, done, h, hT, cT, rec, T, B);
    return check_launch("mi355ppo_lstm_seq_fwd_f32");
}

template <int E>
int launch_bwd(const float* dh, const float* dhT, const float* dcT, const float* rec, const float* w_hh, const float* done, float* dgx,
               float* dh0, float* dc0, int T, int B, hipStream_t s) {
    hipLaunchKernelGGL((lstm_bwd_kernel<E>), dim3((B + E - 1) / E), dim3(kThreads), 0, s, dh, dhT, dcT, rec, w_hh, done, dgx, dh0, dc0, T, B);
    return check_launch("mi355ppo_lstm_seq_bwd_f32");
}

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_lstm_seq_fwd_f32(const float* gx, const float* w_hh, const float* h0, const float* c0, const float* done,
                                                      float* h, float* hT, float* cT, float* record, int T, int B, int H, void* stream) {
    const char* fn = "mi355ppo_lstm_seq_fwd_f32";
    MI355_REQUIRE(gx && w_hh && h0 && c0 && done && h && hT && cT, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(T > 0 && B > 0, MI355PPO_EINVAL, "%s: T=%d B=%d must be positive", fn, T, B);
    hipStream_t s = as_stream(stream);
    switch (lstm_envs_per_group(B)) {
        case 1: return launch_fwd<1>(gx, w_hh, h0, c0, done, h, hT, cT, record, T, B, s);
        case 2: return launch_fwd<2>(gx, w_hh, h0, c0, done, h, hT, cT, record, T, B, s);
        case 4: return launch_fwd<4>(gx, w_hh, h0, c0, done, h, hT, cT, record, T, B, s);
        default: return launch_fwd<8>(gx, w_hh, h0, c0, done, h, hT, cT, record, T, B, s);
    }
}

extern "C" MI355PPO_API int mi355ppo_lstm_seq_bwd_f32(const float* dh, const float* dhT, const float* dcT, const float* record,
                                                      const float* w_hh, const float* done, float* dgx, float* dh0, float* dc0, int T,
                                                      int B, int H, void* stream) {
    const char* fn = "mi355ppo_lstm_seq_bwd_f32";
    MI355_REQUIRE(dh && record && w_hh && done && dgx, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(T > 0 && B > 0, MI355PPO_EINVAL, "%s: T=%d B=%d must be positive", fn, T, B);
    hipStream_t s = as_stream(stream);
    switch (lstm_envs_per_group(B)) {
        case 1: return launch_bwd<1>(dh, dhT, dcT, record, w_hh, done, dgx, dh0, dc0, T, B, s);
        case 2: return launch_bwd<2>(dh, dhT, dcT, record, w_hh, done, dgx, dh0, dc0, T, B, s);
        case 4: return launch_bwd<4>(dh, dhT, dcT, record, w_hh, done, dgx, dh0, dc0, T, B, s);
        default: return launch_bwd<8>(dh, dhT, dcT, record, w_hh, done, dgx, dh0, dc0, T, B, s);
    }
}
