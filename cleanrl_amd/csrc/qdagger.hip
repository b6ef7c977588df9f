// The QDagger head (cleanrl/qdagger_dqn_atari_impalacnn.py:294-306, 403-415): Linear(256, n) of the IMPALA student, the TD loss against
// the target network and the distillation KL against the teacher's softmax, with the backward to h, W and b (gfx950).  Row math and
// orders: qdagger_rows.h.
//
//   forward  both heads in one launch (qh_fwd_kernel<256, 256>, qhead_wg.h): online on h, target on h_next.
//   row      one workgroup per batch row: thread 0 runs the row (td_target, both softmaxes, the two loss terms, dq over ALL actions),
//            then thread k writes dh[r, k].
//   wgrad    one workgroup per action j: dW[j, :] and db[j] over all batch rows, ascending (dq is dense, so no "rows that took this
//            action" walk).  One more workgroup folds the row terms in f64 slots into the four scalars.
//
// Three launches for an update, two for acting.  Plain f32 VALU: at batch 32 the step is latency-bound.  No entry point allocates or
// synchronises, none uses atomics; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "qdagger_rows.h"
#include "qhead_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// ws layout (floats): z (2 x M x n) | rows (3 x Mp: TD term | q[a] | distillation term) | dq (M x n)
struct QdWs {
    float *z, *rows, *dq;
};
static __host__ __device__ QdWs qd_ws(void* ws, int M, int n, int Mp) {
    QdWs w;
    w.z = static_cast<float*>(ws);
    w.rows = w.z + (int64_t)2 * M * n;
    w.dq = w.rows + 3 * Mp;
    return w;
}

__global__ __launch_bounds__(kQdH) void qd_row_kernel(QdWs S, const float* __restrict__ w_online, const float* __restrict__ teacher_q,
                                                      const int64_t* __restrict__ actions, const float* __restrict__ rewards,
                                                      const float* __restrict__ dones, float* __restrict__ dh, float* __restrict__ target_q,
                                                      float* __restrict__ td_target, int M, int Mp, int n, float gamma, float T, float norm,
                                                      float ck) {
    __shared__ float dqs[kDqMaxAct];
    const int t = threadIdx.x, r = blockIdx.x;
    if (t == 0) {
        float qo[kDqMaxAct], qt[kDqMaxAct], tq[kDqMaxAct], dq[kDqMaxAct];
        for (int j = 0; j < n; ++j) {
            qo[j] = S.z[(int64_t)r * n + j];
            qt[j] = S.z[((int64_t)M + r) * n + j];
            tq[j] = teacher_q[(int64_t)r * n + j];
        }
        const QdRow R = qd_row(qo, qt, tq, n, (int)op_clamp(actions[r], n), rewards[r], dones[r], gamma, T, norm, ck, dq);
        for (int j = 0; j < n; ++j) {
            dqs[j] = dq[j];
            S.dq[(int64_t)r * n + j] = dq[j];
            if (target_q) target_q[(int64_t)r * n + j] = qt[j];
        }
        if (td_target) td_target[r] = R.y;
        S.rows[r] = R.sq;
        S.rows[Mp + r] = R.qa;
        S.rows[2 * Mp + r] = R.kl;
    }
    __syncthreads();
    dh[(int64_t)r * kQdH + t] = qd_dh(dqs, n, w_online, t);
}

// the f64 slot fold's sum (wg_fold_mean's order without the division).  Valid in thread 0; ends with a barrier.
__device__ float qd_fold_sum(const float* __restrict__ v, int M, double* red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < M; k += kOpFold) s += (double)v[k];
    red[threadIdx.x] = s;
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int t = 0; t < kOpFold; ++t) tot += red[t];
    __syncthreads();
    return (float)tot;
}

// Workgroup j < n: dW[j, :] and db[j].  Workgroup n: scalars {loss, q_loss, distill_loss, mean q[a]}.
__global__ __launch_bounds__(kQdH) void qd_wgrad_kernel(QdWs S, const float* __restrict__ h, float* __restrict__ dw, float* __restrict__ db,
                                                        float* __restrict__ scalars, int M, int Mp, int n, float coeff) {
    static_assert(kQdH == kOpFold, "one thread per hidden column and per fold slot");
    __shared__ double red[kOpFold];
    __shared__ float dqj[kQdMaxRows];
    __shared__ float two[2];
    const int t = threadIdx.x, j = blockIdx.x;
    if (j == n) {
        wg_fold_scalars(S.rows, Mp, M, red, two);                    // {q_loss, mean q[a]}
        const float distill = qd_fold_sum(S.rows + 2 * Mp, M, red);
        if (t == 0) {
            scalars[0] = qd_loss(two[0], coeff, distill);
            scalars[1] = two[0];
            scalars[2] = distill;
            scalars[3] = two[1];
        }
        return;
    }
    for (int r = t; r < M; r += kQdH) dqj[r] = S.dq[(int64_t)r * n + j];
    __syncthreads();
    dw[(int64_t)j * kQdH + t] = qd_wgrad(dqj, 1, M, h, t);
    if (t == 0) db[j] = qd_wgrad(dqj, 1, M, nullptr, 0);
}

// actions[r] = argmax_a q[r, a] (ties to the lowest index, NaN is the maximum: dq_argmax); one thread per row
__global__ __launch_bounds__(256) void qd_argmax_kernel(const float* __restrict__ z, int64_t* __restrict__ actions, float* __restrict__ q_out,
                                                        int N, int n) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    float q[kDqMaxAct];
    for (int j = 0; j < n; ++j) {
        q[j] = z[(int64_t)r * n + j];
        if (q_out) q_out[(int64_t)r * n + j] = q[j];
    }
    actions[r] = (int64_t)dq_argmax(q, n);
}

static size_t qd_update_workspace(int M, int hidden, int n) {
    if (!qd_limits(M, hidden, n)) return 0;
    return (size_t)((int64_t)3 * M * n + 3 * op_mp(M)) * sizeof(float);
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API size_t mi355ppo_qdagger_head_act_workspace_bytes(int N, int n_actions) {
    return qd_limits(N, kQdH, n_actions) ? (size_t)N * n_actions * sizeof(float) : 0;
}

extern "C" MI355PPO_API int mi355ppo_qdagger_head_act_f32(const float* h, const float* w, const float* b, int64_t* actions_out, float* q_out,
                                                         int N, int hidden, int n_actions, void* workspace, size_t workspace_bytes,
                                                         void* stream) {
    const char* fn = "mi355ppo_qdagger_head_act_f32";
    MI355_REQUIRE(h && w && b && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = qd_shape(fn, N, hidden, n_actions)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, mi355ppo_qdagger_head_act_workspace_bytes(N, n_actions))) return rc;
    hipStream_t s = as_stream(stream);
    float* z = static_cast<float*>(workspace);
    if (int rc = (qh_fwd_launch<kQdH, kQdH>(s, QhPasses{{h}, {w}, {b}}, 1, z, N, n_actions, 1))) return rc;
    hipLaunchKernelGGL(qd_argmax_kernel, dim3((N + 255) / 256), dim3(256), 0, s, z, actions_out, q_out, N, n_actions);
    return check_launch("qd_argmax_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_qdagger_head_workspace_bytes(int M, int n_actions) { return qd_update_workspace(M, kQdH, n_actions); }

extern "C" MI355PPO_API int mi355ppo_qdagger_head_fwd_bwd_f32(const float* h, const float* h_next, const float* w, const float* b,
                                                             const float* w_target, const float* b_target, const float* teacher_q,
                                                             const int64_t* actions, const float* rewards, const float* dones, double gamma,
                                                             double temperature, double distill_coeff, float* dh, float* dw, float* db,
                                                             float* scalars_out, float* target_q_out, float* td_target_out, int M, int hidden,
                                                             int n_actions, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_qdagger_head_fwd_bwd_f32";
    MI355_REQUIRE(h && h_next && w && b && w_target && b_target && teacher_q && actions && rewards && dones && dh && dw && db && scalars_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = qd_shape(fn, M, hidden, n_actions)) return rc;
    MI355_REQUIRE(temperature > 0.0, MI355PPO_EINVAL, "%s: temperature=%g must be positive", fn, temperature);
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, qd_update_workspace(M, hidden, n_actions))) return rc;
    hipStream_t s = as_stream(stream);
    const int n = n_actions, Mp = (int)op_mp(M);
    const QdWs S = qd_ws(workspace, M, n, Mp);
    const QhPasses H{{h, h_next}, {w, w_target}, {b, b_target}};              // 0: online on obs, 1: target on next_obs
    if (int rc = (qh_fwd_launch<kQdH, kQdH>(s, H, 2, S.z, M, n, 1))) return rc;
    hipLaunchKernelGGL(qd_row_kernel, dim3(M), dim3(kQdH), 0, s, S, w, teacher_q, actions, rewards, dones, dh, target_q_out, td_target_out, M, Mp,
                       n, (float)gamma, (float)temperature, (float)(2.0 / (double)M), (float)(distill_coeff / temperature));
    if (int rc = check_launch("qd_row_kernel")) return rc;
    hipLaunchKernelGGL(qd_wgrad_kernel, dim3(n + 1), dim3(kQdH), 0, s, S, h, dw, db, scalars_out, M, Mp, n, (float)distill_coeff);
    return check_launch("qd_wgrad_kernel");
}
