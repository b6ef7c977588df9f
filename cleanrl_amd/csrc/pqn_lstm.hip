// The recurrent tail of PQN (cleanrl/pqn_atari_envpool_lstm.py) as two entry points (gfx950).  Row math: pqn_lstm_rows.h (the LSTM
// cell and the dot product are lstm_rows.h's, e-greedy is pqn_rows.h's); design: DESIGN.md section 3.12.
//
//   act      one launch per rollout step: keep = 1 - done, ONE LSTM cell on (keep h, keep c) in the layout of lstm.hip's forward (a
//            workgroup of 512 threads owns E envs, thread j holds gate row W_hh[j, :] in VGPRs, the masked state is broadcast from
//            LDS), then q = Linear(128, A) as E x A dot products over the h rows that are already in LDS, then e-greedy (one thread
//            per env) and the step's storage rows.  h / c out may alias the inputs: the thread that reads a unit writes it.  With
//            the state and action outputs NULL it is the bootstrap's q(next_obs).
//   td       one minibatch's q_func + gather + mse_loss, forward and backward, in two launches like pqn.hip's mlp_td:
//            (1) workgroups of kPqnRows rows: thread = row forms old / g, then the workgroup writes its rows of dh (coalesced) and
//                its partial of (dwq | dbq), rows in ascending order;
//            (2) the partials are added in ascending workgroup order (OVERWRITING dwq / dbq); workgroup 0 folds the two scalars.
//
// Both are launch-latency-bound at every size the script runs (8 - 256 envs, minibatches of 256 - 8,192 rows).  No atomics, no
// allocation, no synchronisation: deterministic, batch-invariant (an env's chain does not depend on N or E), capturable.
#include "common.h"
#include "pqn_lstm_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {
namespace {

template <int E>
__global__ __launch_bounds__(kLstmThreads) void pqn_lstm_act_kernel(const float* __restrict__ gx, const float* __restrict__ w_hh,
                                                                    const float* h_in, const float* c_in,
                                                                    const float* __restrict__ done, const float* __restrict__ wq,
                                                                    const float* __restrict__ bq, const int64_t* __restrict__ rnd,
                                                                    const float* __restrict__ u, float eps, float* h_out, float* c_out,
                                                                    float* __restrict__ q_out, float* __restrict__ actions,
                                                                    float* __restrict__ values, int64_t* __restrict__ act_i64,
                                                                    float* __restrict__ done_row_out, int N, int A) {
    constexpr int P = kLstmPairs<E>;
    __shared__ __attribute__((aligned(16))) float s_h[E][kLstmH];      // keep * h_in, then h_out
    __shared__ float s_a[E][kLstmG];
    __shared__ float s_q[E][kPqnMaxA];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * E;

    float w[kLstmH];                                                   // gate row j = tid (w_hh may be a view at any 4-byte offset
#pragma unroll                                                         // of the flat parameter buffer)
    for (int k = 0; k < kLstmH; ++k) w[k] = w_hh[(size_t)tid * kLstmH + k];
    float ck[P];
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int p = tid + kLstmThreads * r, e = p / kLstmH, un = p % kLstmH, b = b0 + e;
        float hk = 0.0f;
        ck[r] = 0.0f;
        if (e < E && b < N) {
            const float keep = 1.0f - done[b];
            hk = keep * h_in[(size_t)b * kLstmH + un];
            ck[r] = keep * c_in[(size_t)b * kLstmH + un];
        }
        if (e < E) s_h[e][un] = hk;
    }
    __syncthreads();
    // ---- a = gx + W_hh hk (row j = tid)
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const float g = (b0 + e < N) ? gx[(size_t)(b0 + e) * kLstmG + tid] : 0.0f;
        s_a[e][tid] = g + lstm_dot128(w, s_h[e]);
    }
    __syncthreads();
    // ---- the cell update of the owned units; h replaces the masked state in LDS
#pragma unroll
    for (int r = 0; r < P; ++r) {
        const int p = tid + kLstmThreads * r, e = p / kLstmH, un = p % kLstmH, b = b0 + e;
        if (e >= E) continue;
        const LstmCell s = lstm_cell_fwd(s_a[e][un], s_a[e][kLstmH + un], s_a[e][2 * kLstmH + un], s_a[e][3 * kLstmH + un], ck[r]);
        if (b < N && h_out) {
            h_out[(size_t)b * kLstmH + un] = s.h;
            c_out[(size_t)b * kLstmH + un] = s.c;
        }
        s_h[e][un] = s.h;
    }
    __syncthreads();
    // ---- q_func: thread (e, a)
    if (tid < E * A) {
        const int e = tid / A, a = tid % A, b = b0 + e;
        const float qv = pqn_lstm_q(wq + (size_t)a * kLstmH, s_h[e], bq[a]);
        s_q[e][a] = qv;
        if (b < N && q_out) q_out[(size_t)b * A + a] = qv;
    }
    __syncthreads();
    // ---- e-greedy and the storage rows: thread e
    if (tid < E && b0 + tid < N) {
        const int b = b0 + tid;
        if (actions) {
            float v;
            const int64_t a = pqn_egreedy(s_q[tid], 1, A, rnd[b], u[b], eps, &v);
            actions[b] = (float)a;
            values[b] = v;
            if (act_i64) act_i64[b] = a;
        }
        if (done_row_out) done_row_out[b] = done[b];
    }
}

// (1) of a minibatch: rows [blockIdx.x * kPqnRows, +kPqnRows).  ws: old (Mp) | sq (Mp) | partials (nblk x (A * 128 + A)).
__global__ __launch_bounds__(kPqnRows) void pqn_lstm_td_kernel(const float* __restrict__ h, const int64_t* __restrict__ inds,
                                                               const float* __restrict__ b_actions, const float* __restrict__ b_returns,
                                                               const float* __restrict__ wq, const float* __restrict__ bq,
                                                               float* __restrict__ dh, float* __restrict__ ws, int M, int Mp, int A,
                                                               int64_t B, float norm) {
    __shared__ float s_g[kPqnRows];
    __shared__ int s_act[kPqnRows];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * kPqnRows;
    const int r1 = (r0 + kPqnRows < M) ? r0 + kPqnRows : M;
    const int r = r0 + tid;
    if (r < M) {
        const int64_t i = pqn_clamp_index(inds[r], B);
        const PqnLstmTd t = pqn_lstm_td_row(h + (size_t)r * kLstmH, wq, bq, A, b_actions[i], b_returns[i], norm);
        s_g[tid] = t.g;
        s_act[tid] = t.a;
        ws[r] = t.old;
        ws[Mp + r] = t.sq;
    }
    __syncthreads();
    for (int idx = tid; idx < (r1 - r0) * kLstmH; idx += kPqnRows) {
        const int rr = idx / kLstmH, k = idx % kLstmH;
        dh[(size_t)(r0 + rr) * kLstmH + k] = s_g[rr] * wq[(size_t)s_act[rr] * kLstmH + k];
    }
    const int AH = A * kLstmH;
    float* part = ws + 2 * (size_t)Mp + (size_t)blockIdx.x * (AH + A);
    for (int e = tid; e < AH; e += kPqnRows) part[e] = pqn_lstm_grad_partial(e, h, s_g, s_act, r0, r1);
    if (tid < A) part[AH + tid] = pqn_lstm_bias_partial(tid, s_g, s_act, r1 - r0);
}

// (2): dwq | dbq = the nblk partials in ascending order; workgroup 0 also folds the TD scalars.
__global__ __launch_bounds__(kPqnFold) void pqn_lstm_td_fold_kernel(const float* __restrict__ ws, int nblk, int M, int Mp, int A,
                                                                    float* __restrict__ dwq, float* __restrict__ dbq,
                                                                    float* __restrict__ scalars) {
    const int AH = A * kLstmH, P = AH + A;
    const int e = blockIdx.x * kPqnFold + threadIdx.x;
    if (e < P) {
        const float* part = ws + 2 * (size_t)Mp + e;
        float acc = 0.0f;
        for (int b = 0; b < nblk; ++b) acc = acc + part[(size_t)b * P];
        if (e < AH)
            dwq[e] = acc;
        else
            dbq[e - AH] = acc;
    }
    if (blockIdx.x != 0) return;
    double so = 0.0, ss = 0.0;
    for (int k = threadIdx.x; k < M; k += kPqnFold) {
        so += (double)ws[k];
        ss += (double)ws[Mp + k];
    }
    pqn_fold_scalars(so, ss, M, scalars);
}

template <int E, class... Args>
int launch_act(int N, hipStream_t s, Args... args) {
    hipLaunchKernelGGL((pqn_lstm_act_kernel<E>), dim3((N + E - 1) / E), dim3(kLstmThreads), 0, s, args...);
    return check_launch("mi355ppo_pqn_lstm_act_f32");
}

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_pqn_lstm_act_f32(const float* gx, const float* w_hh, const float* h_in, const float* c_in,
                                                     const float* done_in, const float* wq, const float* bq,
                                                     const int64_t* random_actions, const float* u, double epsilon, float* h_out,
                                                     float* c_out, float* q_out, float* actions_out, float* values_out,
                                                     int64_t* action_i64_out, float* done_row_out, int N, int H, int A, void* stream) {
    const char* fn = "mi355ppo_pqn_lstm_act_f32";
    MI355_REQUIRE(gx && w_hh && h_in && c_in && done_in && wq && bq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(!h_out == !c_out, MI355PPO_EINVAL, "%s: h_out and c_out are both given or both NULL", fn);
    MI355_REQUIRE(!actions_out == !values_out && (!actions_out || (random_actions && u)) && (actions_out || !action_i64_out),
                  MI355PPO_EINVAL, "%s: actions_out, values_out, random_actions and u go together (all NULL: the bootstrap form)", fn);
    MI355_REQUIRE(h_out || q_out || actions_out, MI355PPO_EINVAL, "%s: null pointer (no output)", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(N > 0 && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL, "%s: N=%d A=%d: N must be positive, 1 <= A <= %d", fn, N, A, kPqnMaxA);
    hipStream_t s = as_stream(stream);
    const float eps = (float)epsilon;
    switch (lstm_envs_per_group(N)) {
        case 1: return launch_act<1>(N, s, gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions, u, eps, h_out, c_out, q_out, actions_out,
                                     values_out, action_i64_out, done_row_out, N, A);
        case 2: return launch_act<2>(N, s, gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions, u, eps, h_out, c_out, q_out, actions_out,
                                     values_out, action_i64_out, done_row_out, N, A);
        case 4: return launch_act<4>(N, s, gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions, u, eps, h_out, c_out, q_out, actions_out,
                                     values_out, action_i64_out, done_row_out, N, A);
        default: return launch_act<8>(N, s, gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions, u, eps, h_out, c_out, q_out, actions_out,
                                      values_out, action_i64_out, done_row_out, N, A);
    }
}

extern "C" MI355PPO_API size_t mi355ppo_pqn_lstm_td_workspace_bytes(int M, int A) {
    if (M <= 0 || A <= 0) return 0;
    const int64_t nblk = ((int64_t)M + kPqnRows - 1) / kPqnRows;
    return (size_t)(2 * pqn_lstm_mp(M) + nblk * ((int64_t)A * kLstmH + A)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_pqn_lstm_td_fwd_bwd_f32(const float* h, const int64_t* mb_inds, const float* b_actions,
                                                            const float* b_returns, const float* wq, const float* bq, float* dh,
                                                            float* dwq, float* dbq, float* scalars_out, int M, int H, int A, int64_t B,
                                                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_pqn_lstm_td_fwd_bwd_f32";
    MI355_REQUIRE(h && mb_inds && b_actions && b_returns && wq && bq && dh && dwq && dbq && scalars_out, MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    MI355_REQUIRE(H == kLstmH, MI355PPO_EINVAL, "%s: H=%d (only %d)", fn, H, kLstmH);
    MI355_REQUIRE(M > 0 && B > 0 && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL, "%s: M=%d B=%lld A=%d: M, B must be positive, 1 <= A <= %d",
                  fn, M, (long long)B, A, kPqnMaxA);
    const size_t need = mi355ppo_pqn_lstm_td_workspace_bytes(M, A);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const int Mp = (int)pqn_lstm_mp(M);
    const int nblk = (M + kPqnRows - 1) / kPqnRows;
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(pqn_lstm_td_kernel, dim3(nblk), dim3(kPqnRows), 0, s, h, mb_inds, b_actions, b_returns, wq, bq, dh, ws, M, Mp, A, B,
                       (float)(2.0 / (double)M));
    if (int rc = check_launch("pqn_lstm_td_kernel")) return rc;
    const int P = A * kLstmH + A;
    hipLaunchKernelGGL(pqn_lstm_td_fold_kernel, dim3((P + kPqnFold - 1) / kPqnFold), dim3(kPqnFold), 0, s, ws, nblk, M, Mp, A, dwq, dbq,
                       scalars_out);
    return check_launch("pqn_lstm_td_fold_kernel");
}
