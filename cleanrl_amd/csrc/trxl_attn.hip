// The episodic-memory attention core of ppo_trxl.py (cleanrl/ppo_trxl/ppo_trxl.py: the window gather of
// batched_index_select, the positional encoding of Transformer.forward, norm_kv of TransformerLayer.forward and the keys /
// masked softmax / weighted sum of MultiHeadAttention.forward), forward and backward in one streaming pass each.
// Math: trxl_rows.h.  Design:
//   * one workgroup of 4 waves per sample: a sample's bits do not depend on B or on its place in the batch, and every sum
//     is folded in a fixed order (deterministic, no atomics);
//   * a window row is gathered straight from the episode pool (no whole-episode copy, no window tensor): lane l holds
//     columns [l C, l C + C) of the row, C = D / 64, and head h is the group of 64 / H consecutive lanes;
//   * LayerNorm by two wave butterflies, the score by one head-group butterfly, then one online-softmax update per head;
//     wave w streams rows w, w + 4, ...; the next row's loads are issued before the current row's arithmetic;
//   * the 4 waves' softmax states meet in LDS and are merged in wave order;
//   * the backward re-streams the window with the forward's statistics and writes per-sample d gamma / d beta rows, which a
//     second launch folds over the batch in a fixed order.
// Indices out of range (ep, rows, pos) are clamped -- never an out-of-bounds read -- and set the caller's error word.
#include "common.h"
#include "trxl_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {
namespace {

constexpr int kThreads = kTrxlWaves * MI355_WAVE;

struct TrxlArgs {
    const float* mem;
    const int64_t* ep;
    const int64_t* rows;
    const int64_t* pos;
    const unsigned char* mask;
    const float* pe;
    const float* gamma;
    const float* beta;
    const float* q;
    int E, T, layers, layer, P, B, L, D, H;
    int* err;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float group_sum(float v, int G) {
    for (int off = G >> 1; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int64_t clamp_idx(int64_t i, int64_t n, int* err) {
    if (i < 0 || i >= n) {
        if (err) *err = 1;                   // a plain (vector) global store; every offending lane writes the same value
        return i < 0 ? 0 : n - 1;
    }
    return i;
}

// The source rows of window row j: the memory row and, with a positional encoding, the table row.
template <int C>
__device__ __forceinline__ void load_row(const TrxlArgs& a, int64_t e, int j, int col0, float (&x)[C], float (&p)[C]) {
    const int64_t r = clamp_idx(a.rows[(size_t)blockIdx.x * a.L + j], a.T, a.err);
    const float* src = a.mem + (((size_t)e * a.T + (size_t)r) * a.layers + a.layer) * a.D + col0;
#pragma unroll
    for (int c = 0; c < C; ++c) x[c] = src[c];
    if (a.pe) {
        const int64_t ps = clamp_idx(a.pos[(size_t)blockIdx.x * a.L + j], a.P, a.err);
        const float* pr = a.pe + (size_t)ps * a.D + col0;
#pragma unroll
        for (int c = 0; c < C; ++c) p[c] = pr[c];
    }
}

// x (+ pe) -> xhat, y = xhat * gamma + beta.
template <int C>
__device__ __forceinline__ void norm_row(const TrxlArgs& a, float (&x)[C], const float (&p)[C], const float (&g)[C],
                                         const float (&bt)[C], float (&xh)[C], float (&y)[C]) {
    if (a.pe) {
#pragma unroll
        for (int c = 0; c < C; ++c) x[c] = x[c] + p[c];
    }
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) s = s + x[c];
    const float mean = wave_sum(s) / (float)a.D;
    float v = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xh[c] = x[c] - mean;
        v = v + xh[c] * xh[c];
    }
    const float rstd = trxl_rstd(wave_sum(v) / (float)a.D);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        xh[c] = xh[c] * rstd;
        y[c] = xh[c] * g[c] + bt[c];
    }
}

template <int C>
__device__ __forceinline__ float head_dot(const float (&a)[C], const float (&b)[C], int G) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) s = s + a[c] * b[c];
    return group_sum(s, G);
}

template <int C>
__global__ __launch_bounds__(kThreads) void trxl_attn_fwd_kernel(TrxlArgs a, float* __restrict__ u, float* __restrict__ stats,
                                                                 float sqrt_d) {
    __shared__ float s_m[kTrxlWaves][64];
    __shared__ float s_l[kTrxlWaves][64];
    __shared__ float s_acc[kTrxlWaves][kTrxlMaxD];
    const int w = threadIdx.x / MI355_WAVE, lane = threadIdx.x % MI355_WAVE;
    const int b = blockIdx.x, G = MI355_WAVE / a.H, h = lane / G, col0 = lane * C;
    const int64_t e = clamp_idx(a.ep[b], a.E, a.err);
    float g[C], bt[C], q[C], acc[C], x[C], p[C], xn[C], pn[C], xh[C], y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        g[c] = a.gamma[col0 + c];
        bt[c] = a.beta[col0 + c];
        q[c] = a.q[(size_t)b * a.D + col0 + c];
        acc[c] = 0.0f;
        p[c] = pn[c] = 0.0f;
    }
    TrxlOnline st{-INFINITY, 0.0f};
    if (w < a.L) load_row<C>(a, e, w, col0, x, p);
    for (int j = w; j < a.L; j += kTrxlWaves) {
        if (j + kTrxlWaves < a.L) load_row<C>(a, e, j + kTrxlWaves, col0, xn, pn);       // next row, under this row's math
        norm_row<C>(a, x, p, g, bt, xh, y);
        const float s = trxl_score(a.mask[(size_t)b * a.L + j] != 0, head_dot<C>(q, y, G), sqrt_d);
        float pj;
        const float f = trxl_online_step(st, s, pj);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            acc[c] = acc[c] * f + pj * y[c];
            x[c] = xn[c];
            p[c] = pn[c];
        }
    }
    if (lane % G == 0) {
        s_m[w][h] = st.m;
        s_l[w][h] = st.l;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) s_acc[w][col0 + c] = acc[c];
    __syncthreads();
    const int d = a.D / a.H;
    for (int col = threadIdx.x; col < a.D; col += kThreads) {
        const int hh = col / d;
        float m[kTrxlWaves], f[kTrxlWaves], l[kTrxlWaves], v[kTrxlWaves];
#pragma unroll
        for (int i = 0; i < kTrxlWaves; ++i) m[i] = s_m[i][hh];
        const float M = trxl_merge_max(m);
#pragma unroll
        for (int i = 0; i < kTrxlWaves; ++i) {
            f[i] = expf(m[i] - M);
            l[i] = s_l[i][hh];
            v[i] = s_acc[i][col];
        }
        const float lsum = trxl_merge_sum(l, f);
        u[(size_t)b * a.D + col] = trxl_merge_sum(v, f) / lsum;
        if (col % d == 0) {
            stats[((size_t)b * a.H + hh) * 2] = M;
            stats[((size_t)b * a.H + hh) * 2 + 1] = lsum;
        }
    }
}

template <int C>
__global__ __launch_bounds__(kThreads) void trxl_attn_bwd_kernel(TrxlArgs a, const float* __restrict__ u, const float* __restrict__ stats,
                                                                 const float* __restrict__ du, float* __restrict__ dq,
                                                                 float* __restrict__ dln_rows, float sqrt_d) {
    __shared__ float s_z[kTrxlWaves][kTrxlMaxD];
    __shared__ float s_dg[kTrxlWaves][kTrxlMaxD];
    __shared__ float s_db[kTrxlWaves][kTrxlMaxD];
    const int w = threadIdx.x / MI355_WAVE, lane = threadIdx.x % MI355_WAVE;
    const int b = blockIdx.x, G = MI355_WAVE / a.H, h = lane / G, col0 = lane * C;
    const int64_t e = clamp_idx(a.ep[b], a.E, a.err);
    float g[C], bt[C], q[C], dy_u[C], uu[C], x[C], p[C], xn[C], pn[C], xh[C], y[C], z[C], dg[C], db[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        g[c] = a.gamma[col0 + c];
        bt[c] = a.beta[col0 + c];
        q[c] = a.q[(size_t)b * a.D + col0 + c];
        dy_u[c] = du[(size_t)b * a.D + col0 + c];
        uu[c] = u[(size_t)b * a.D + col0 + c];
        z[c] = dg[c] = db[c] = 0.0f;
        p[c] = pn[c] = 0.0f;
    }
    const float M = stats[((size_t)b * a.H + h) * 2], lsum = stats[((size_t)b * a.H + h) * 2 + 1];
    const float duu = head_dot<C>(dy_u, uu, G);
    if (w < a.L) load_row<C>(a, e, w, col0, x, p);
    for (int j = w; j < a.L; j += kTrxlWaves) {
        if (j + kTrxlWaves < a.L) load_row<C>(a, e, j + kTrxlWaves, col0, xn, pn);
        norm_row<C>(a, x, p, g, bt, xh, y);
        const bool keep = a.mask[(size_t)b * a.L + j] != 0;
        const float s = trxl_score(keep, head_dot<C>(q, y, G), sqrt_d);
        const float att = trxl_att(s, M, lsum);
        const float ds = att * (head_dot<C>(dy_u, y, G) - duu);
        const float gs = keep ? ds / sqrt_d : 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            z[c] = z[c] + gs * y[c];
            const float dyc = gs * q[c] + att * dy_u[c];
            dg[c] = dg[c] + dyc * xh[c];
            db[c] = db[c] + dyc;
            x[c] = xn[c];
            p[c] = pn[c];
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        s_z[w][col0 + c] = z[c];
        s_dg[w][col0 + c] = dg[c];
        s_db[w][col0 + c] = db[c];
    }
    __syncthreads();
    const size_t BD = (size_t)a.B * a.D;
    for (int col = threadIdx.x; col < a.D; col += kThreads) {
        const size_t o = (size_t)b * a.D + col;
        dq[o] = ((s_z[0][col] + s_z[1][col]) + s_z[2][col]) + s_z[3][col];
        dln_rows[o] = ((s_dg[0][col] + s_dg[1][col]) + s_dg[2][col]) + s_dg[3][col];
        dln_rows[BD + o] = ((s_db[0][col] + s_db[1][col]) + s_db[2][col]) + s_db[3][col];
    }
}

// d gamma / d beta: the per-sample rows folded over b.  Column block of 64, wave w sums b = w, w + 4, ...; the waves' sums
// are added in wave order.  The order depends on B only.
__global__ __launch_bounds__(kThreads) void trxl_ln_fold_kernel(const float* __restrict__ dln_rows, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int B, int D) {
    __shared__ float s_p[2][kTrxlWaves][MI355_WAVE];
    const int w = threadIdx.x / MI355_WAVE, lane = threadIdx.x % MI355_WAVE;
    const int col = blockIdx.x * MI355_WAVE + lane;
    const size_t BD = (size_t)B * D;
    float sg = 0.0f, sb = 0.0f;
    for (int b = w; b < B; b += kTrxlWaves) {
        sg = sg + dln_rows[(size_t)b * D + col];
        sb = sb + dln_rows[BD + (size_t)b * D + col];
    }
    s_p[0][w][lane] = sg;
    s_p[1][w][lane] = sb;
    __syncthreads();
    if (w == 0) {
        dgamma[col] = ((s_p[0][0][lane] + s_p[0][1][lane]) + s_p[0][2][lane]) + s_p[0][3][lane];
        dbeta[col] = ((s_p[1][0][lane] + s_p[1][1][lane]) + s_p[1][2][lane]) + s_p[1][3][lane];
    }
}

int check_args(const char* fn, const TrxlArgs& a) {
    MI355_REQUIRE(a.mem && a.ep && a.rows && a.mask && a.gamma && a.beta && a.q, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(trxl_shape_ok(a.D, a.H, a.L), MI355PPO_EINVAL,
                  "%s: D=%d H=%d L=%d (need D %% 64 == 0, D <= 512, H dividing 64, 1 <= L <= 1024)", fn, a.D, a.H, a.L);
    MI355_REQUIRE(a.B > 0 && a.E > 0 && a.T > 0 && a.layers > 0 && a.layer >= 0 && a.layer < a.layers, MI355PPO_EINVAL,
                  "%s: B=%d E=%d T_ep=%d layers=%d layer=%d", fn, a.B, a.E, a.T, a.layers, a.layer);
    MI355_REQUIRE(!a.pe || (a.pos && a.P > 0), MI355PPO_EINVAL, "%s: pe needs pos and P > 0 (P=%d)", fn, a.P);
    return MI355PPO_OK;
}

TrxlArgs make_args(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep, const int64_t* rows, const int64_t* pos,
                   const uint8_t* mask, const float* pe, int P, const float* gamma, const float* beta, const float* q, int* err, int B, int L,
                   int D, int H) {
    return TrxlArgs{memory, ep, rows, pos, mask, pe, gamma, beta, q, E, T_ep, layers, layer, pe ? P : 0, B, L, D, H, err};
}

template <int C>
int launch_fwd(const TrxlArgs& a, float* u, float* stats, hipStream_t s) {
    hipLaunchKernelGGL((trxl_attn_fwd_kernel<C>), dim3(a.B), dim3(kThreads), 0, s, a, u, stats, trxl_sqrt_d(a.D));
    return check_launch("mi355ppo_trxl_attn_fwd_f32");
}

template <int C>
int launch_bwd(const TrxlArgs& a, const float* u, const float* stats, const float* du, float* dq, float* dln_rows, hipStream_t s) {
    hipLaunchKernelGGL((trxl_attn_bwd_kernel<C>), dim3(a.B), dim3(kThreads), 0, s, a, u, stats, du, dq, dln_rows, trxl_sqrt_d(a.D));
    return check_launch("mi355ppo_trxl_attn_bwd_f32");
}

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_trxl_attn_fwd_f32(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                       const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe,
                                                       int P, const float* gamma, const float* beta, const float* q, float* u,
                                                       float* stats, int* err, int B, int L, int D, int H, void* stream) {
    const char* fn = "mi355ppo_trxl_attn_fwd_f32";
    const TrxlArgs a = make_args(memory, E, T_ep, layers, layer, ep, rows, pos, mask, pe, P, gamma, beta, q, err, B, L, D, H);
    if (int r = check_args(fn, a)) return r;
    MI355_REQUIRE(u && stats, MI355PPO_EINVAL, "%s: null pointer", fn);
    hipStream_t s = as_stream(stream);
    switch (D / 64) {
        case 1: return launch_fwd<1>(a, u, stats, s);
        case 2: return launch_fwd<2>(a, u, stats, s);
        case 3: return launch_fwd<3>(a, u, stats, s);
        case 4: return launch_fwd<4>(a, u, stats, s);
        case 5: return launch_fwd<5>(a, u, stats, s);
        case 6: return launch_fwd<6>(a, u, stats, s);
        case 7: return launch_fwd<7>(a, u, stats, s);
        default: return launch_fwd<8>(a, u, stats, s);
    }
}

extern "C" MI355PPO_API int mi355ppo_trxl_attn_bwd_f32(const float* memory, int E, int T_ep, int layers, int layer, const int64_t* ep,
                                                       const int64_t* rows, const int64_t* pos, const uint8_t* mask, const float* pe,
                                                       int P, const float* gamma, const float* beta, const float* q, const float* u,
                                                       const float* stats, const float* du, float* dq, float* dln_rows, float* dgamma,
                                                       float* dbeta, int* err, int B, int L, int D, int H, void* stream) {
    const char* fn = "mi355ppo_trxl_attn_bwd_f32";
    const TrxlArgs a = make_args(memory, E, T_ep, layers, layer, ep, rows, pos, mask, pe, P, gamma, beta, q, err, B, L, D, H);
    if (int r = check_args(fn, a)) return r;
    MI355_REQUIRE(u && stats && du && dq && dln_rows && dgamma && dbeta, MI355PPO_EINVAL, "%s: null pointer", fn);
    hipStream_t s = as_stream(stream);
    int r;
    switch (D / 64) {
        case 1: r = launch_bwd<1>(a, u, stats, du, dq, dln_rows, s); break;
        case 2: r = launch_bwd<2>(a, u, stats, du, dq, dln_rows, s); break;
        case 3: r = launch_bwd<3>(a, u, stats, du, dq, dln_rows, s); break;
        case 4: r = launch_bwd<4>(a, u, stats, du, dq, dln_rows, s); break;
        case 5: r = launch_bwd<5>(a, u, stats, du, dq, dln_rows, s); break;
        case 6: r = launch_bwd<6>(a, u, stats, du, dq, dln_rows, s); break;
        case 7: r = launch_bwd<7>(a, u, stats, du, dq, dln_rows, s); break;
        default: r = launch_bwd<8>(a, u, stats, du, dq, dln_rows, s); break;
    }
    if (r) return r;
    hipLaunchKernelGGL(trxl_ln_fold_kernel, dim3(D / MI355_WAVE), dim3(kThreads), 0, s, dln_rows, dgamma, dbeta, B, D);
    return check_launch(fn);
}
