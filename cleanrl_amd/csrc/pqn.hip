// PQN (cleanrl/pqn.py, cleanrl/pqn_atari_envpool.py): e-greedy action selection, the Q(lambda) return scan, the TD loss and
// its gradient, pqn.py's LayerNorm MLP (forward, act, minibatch forward + backward) and clip + RAdam on flat buffers (gfx950).
//
// Every launch here is latency-bound at the scripts' sizes (4 - 128 envs, minibatches of 128 - 256 rows), so the mappings are
// the simplest that keep one row's math on one lane -- the row functions of pqn_rows.h, which the host twins run unchanged:
//
//   egreedy         one lane per env: argmax (torch's first-maximum / first-NaN rule), q at the greedy index, u < f32(eps)
//   qlambda         one lane per env walks t = T-1 .. 0 (like K1); the bootstrap max over next_q joins the scan
//   td_loss         one lane per row writes the row of dq; workgroup 0 also folds the two scalars (kPqnFold slots, f64)
//   mlp_fwd / act   one lane per row, hidden vectors in LDS at stride 64 (conflict-free); act adds e-greedy and the stores
//   mlp_td          (1) workgroups of kPqnRows rows: each lane runs its row's forward, TD loss and backward into a
//                       row-interleaved workspace, then the workgroup's threads sum the rows into a per-workgroup partial of
//                       every parameter (ascending rows)
//                   (2) fold: every parameter's partials in ascending workgroup order into the flat gradient (overwritten);
//                       workgroup 0 also folds the TD scalars
//   clip_radam      (1) f64 sum of squares, kPqnFold slots per workgroup, folded in order into one partial per workgroup
//                   (2) every workgroup folds the partials in order, forms clip_grad_norm_'s coefficient and runs torch's
//                       single-tensor RAdam step per element; the gradient is zeroed for the next backward
//
// No atomics, no allocation, no synchronisation: results are deterministic, every entry point can be captured into a graph.
#include "common.h"
#include "pqn_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kPqnLds = kPqnH1 + kPqnH2 + kPqnMaxA;     // floats per row of the LDS scratch (x h1 | h2 | q)

__global__ __launch_bounds__(256) void pqn_egreedy_kernel(const float* __restrict__ q, const int64_t* __restrict__ rnd,
                                                          const float* __restrict__ u, float eps, float* __restrict__ actions,
                                                          float* __restrict__ values, int64_t* __restrict__ act_i64, int N, int A) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    float v;
    const int64_t a = pqn_egreedy(q + (int64_t)r * A, 1, A, rnd[r], u[r], eps, &v);
    actions[r] = (float)a;
    values[r] = v;
    if (act_i64) act_i64[r] = a;
}

__global__ __launch_bounds__(64) void pqn_qlambda_kernel(const float* __restrict__ rewards, const float* __restrict__ dones,
                                                         const float* __restrict__ values, const float* __restrict__ next_done,
                                                         const float* __restrict__ next_q, float* __restrict__ returns, int T, int N,
                                                         int A, float gamma, float lam, float oml) {
    const int n = blockIdx.x * 64 + threadIdx.x;
    if (n >= N) return;
    const float* nq = next_q + (int64_t)n * A;
    const float nv = nq[pqn_argmax(nq, 1, A)];                     // torch.max(q_network(next_obs), dim=-1)
    int64_t off = (int64_t)(T - 1) * N + n;
    float ret = pqn_qlambda_last(rewards[off], nv, next_done[n], gamma);
    returns[off] = ret;
    for (int t = T - 2; t >= 0; --t) {
        const int64_t o1 = off;
        off -= N;
        ret = pqn_qlambda_step(rewards[off], ret, values[o1], dones[o1], gamma, lam, oml);
        returns[off] = ret;
    }
}

__global__ __launch_bounds__(256) void pqn_td_loss_kernel(const float* __restrict__ q, const int64_t* __restrict__ inds,
                                                          const float* __restrict__ b_actions, const float* __restrict__ b_returns,
                                                          float* __restrict__ dq, float* __restrict__ scalars, int M, int A, int64_t B,
                                                          float norm) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r < M) {
        const int64_t i = pqn_clamp_index(inds[r], B);
        float sq;
        pqn_td_row(q + (int64_t)r * A, 1, A, b_actions[i], b_returns[i], norm, dq + (int64_t)r * A, 1, &sq);
    }
    if (blockIdx.x != 0) return;
    double so = 0.0, ss = 0.0;
    for (int k = threadIdx.x; k < M; k += kPqnFold) {
        const int64_t i = pqn_clamp_index(inds[k], B);
        int a;
        float d, sq;
        so += (double)pqn_td_old(q + (int64_t)k * A, 1, A, b_actions[i], b_returns[i], &a, &d, &sq);
        ss += (double)sq;
    }
    pqn_fold_scalars(so, ss, M, scalars);
}

// QNetwork.forward of 64 rows per workgroup (lane = row); ACT adds the rollout step's e-greedy and stores.
template <bool ACT>
__global__ __launch_bounds__(64) void pqn_mlp_fwd_kernel(const float* __restrict__ obs, const float* __restrict__ params, float* __restrict__ q_out,
                                                         int N, int O, int A, const int64_t* __restrict__ rnd, const float* __restrict__ u,
                                                         float eps, float* __restrict__ actions, float* __restrict__ values,
                                                         int64_t* __restrict__ act_i64, float* __restrict__ obs_row_out,
                                                         const float* __restrict__ done_in, float* __restrict__ done_row_out) {
    __shared__ float lds[kPqnLds * 64];
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= N) return;                                              // no barrier below: lanes are independent
    const PqnNet net = pqn_net(params, O, A);
    const float* x = obs + (int64_t)r * O;
    float* h1 = lds + threadIdx.x;
    float* h2 = h1 + kPqnH1 * 64;
    float rstd[2];
    if (!ACT) {
        pqn_row_forward(net, x, 1, h1, h1, h2, h2, 64, q_out + (int64_t)r * A, 1, rstd);
        return;
    }
    float* qr = h2 + kPqnH2 * 64;
    pqn_row_forward(net, x, 1, h1, h1, h2, h2, 64, qr, 64, rstd);
    float v;
    const int64_t a = pqn_egreedy(qr, 64, A, rnd[r], u[r], eps, &v);
    actions[r] = (float)a;
    values[r] = v;
    if (act_i64) act_i64[r] = a;
    if (obs_row_out)
        for (int k = 0; k < O; ++k) obs_row_out[(int64_t)r * O + k] = x[k];
    if (done_row_out) done_row_out[r] = done_in[r];
}

// (1) of a minibatch: rows [blockIdx.x * kPqnRows, +kPqnRows) through forward, TD loss and backward, then this workgroup's partial
// of every parameter's gradient.  ws: U units x Mp floats (row-interleaved), then the partials (nblk x P).
__global__ __launch_bounds__(kPqnRows) void pqn_mlp_td_kernel(const float* __restrict__ b_obs, int64_t B, const int64_t* __restrict__ inds,
                                                              const float* __restrict__ params, const float* __restrict__ b_actions,
                                                              const float* __restrict__ b_returns, float* __restrict__ ws, int M, int Mp,
                                                              int O, int A, float norm) {
    const PqnNet net = pqn_net(params, O, A);
    const PqnUnits U = pqn_units(O, A);
    const int r = blockIdx.x * kPqnRows + threadIdx.x;
    if (r < M) {
        const int64_t i = pqn_clamp_index(inds[r], B);
        float* w = ws + r;
        const float* src = b_obs + i * O;
        for (int k = 0; k < O; ++k) w[(int64_t)(U.x + k) * Mp] = src[k];
        float rstd[2];
        float* xh1 = w + (int64_t)U.xh1 * Mp;
        float* a1 = w + (int64_t)U.a1 * Mp;
        float* xh2 = w + (int64_t)U.xh2 * Mp;
        float* a2 = w + (int64_t)U.a2 * Mp;
        float* dq = w + (int64_t)U.dq * Mp;
        // q goes to the dq rows first, then the TD row turns it into dq in place (q[action] is read before any write)
        pqn_row_forward(net, w + (int64_t)U.x * Mp, Mp, xh1, a1, xh2, a2, Mp, dq, Mp, rstd);
        float sq;
        const float old = pqn_td_row(dq, Mp, A, b_actions[i], b_returns[i], norm, dq, Mp, &sq);
        w[(int64_t)U.old * Mp] = old;
        w[(int64_t)U.sq * Mp] = sq;
        pqn_row_backward(net, dq, Mp, xh1, a1, xh2, a2, rstd, w + (int64_t)U.dy1 * Mp, w + (int64_t)U.dz1 * Mp, w + (int64_t)U.dy2 * Mp,
                         w + (int64_t)U.dz2 * Mp, Mp);
    }
    __syncthreads();
    const int64_t P = pqn_param_count(O, A);
    const int r0 = blockIdx.x * kPqnRows;
    const int r1 = (r0 + kPqnRows < M) ? r0 + kPqnRows : M;
    float* part = ws + (int64_t)U.total * Mp + (int64_t)blockIdx.x * P;
    for (int64_t e = threadIdx.x; e < P; e += kPqnRows) {
        int u1, u2;
        pqn_grad_units(e, O, A, &u1, &u2);
        const float* p1 = ws + (int64_t)u1 * Mp;
        float acc = 0.0f;
        if (u2 < 0) {
            for (int k = r0; k < r1; ++k) acc = acc + p1[k];
        } else {
            const float* p2 = ws + (int64_t)u2 * Mp;
            for (int k = r0; k < r1; ++k) acc = acc + p1[k] * p2[k];
        }
        part[e] = acc;
    }
}

// (2) of a minibatch: grads[e] = sum of the nblk partials in ascending order; workgroup 0 also folds the TD scalars.
__global__ __launch_bounds__(256) void pqn_mlp_fold_kernel(const float* __restrict__ ws, int nblk, int64_t P, int M, int Mp,
                                                           int old_unit, int sq_unit, int64_t part_off, float* __restrict__ grads,
                                                           float* __restrict__ scalars) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < P) {
        const float* part = ws + part_off + e;
        float acc = 0.0f;
        for (int b = 0; b < nblk; ++b) acc = acc + part[(int64_t)b * P];
        grads[e] = acc;
    }
    if (blockIdx.x != 0) return;
    double so = 0.0, ss = 0.0;
    for (int k = threadIdx.x; k < M; k += kPqnFold) {
        so += (double)ws[(int64_t)old_unit * Mp + k];
        ss += (double)ws[(int64_t)sq_unit * Mp + k];
    }
    pqn_fold_scalars(so, ss, M, scalars);
}

// clip + RAdam, (1): partials[b] = sum over this workgroup's kPqnFold slots (in order) of sum (g_i)^2, slot (b, t) taking
// i = b * 256 + t, + G * 256, ...
__global__ __launch_bounds__(256) void pqn_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partials) {
    __shared__ double red[kPqnFold];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double a = (double)g[i];
        s += a * a;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < kPqnFold; ++k) t += red[k];
        partials[blockIdx.x] = t;
    }
}

struct PqnSlot {
    float c[kPqnSched];
};

__global__ __launch_bounds__(256) void pqn_radam_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        int64_t n, RAdamParams R, const double* __restrict__ partials,
                                                        PqnSlot slot, const float* __restrict__ sched, float* __restrict__ total_norm_out) {
    __shared__ float s_coef;
    __shared__ float s_c[kPqnSched];
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < R.nblocks; ++b) s += partials[b];
        s_coef = pqn_clip_coef(s, R.max_norm);
        if (blockIdx.x == 0 && total_norm_out) *total_norm_out = (float)sqrt(s);
    }
    if (threadIdx.x < kPqnSched) s_c[threadIdx.x] = sched ? sched[threadIdx.x] : slot.c[threadIdx.x];   // device table: captured replays
    __syncthreads();
    const float coef = s_coef;
    float c[kPqnSched];
#pragma unroll
    for (int k = 0; k < kPqnSched; ++k) c[k] = s_c[k];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        pqn_radam_elem(p[i], g[i], m[i], v[i], coef, R, c);
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_pqn_egreedy_f32(const float* q, const int64_t* random_actions, const float* u, double epsilon,
                                                    float* actions_out, float* values_out, int64_t* action_i64_out, int N, int A, void* stream) {
    const char* fn = "mi355ppo_pqn_egreedy_f32";
    MI355_REQUIRE(q && random_actions && u && actions_out && values_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(N > 0 && A > 0, MI355PPO_EINVAL, "%s: N=%d A=%d must be positive", fn, N, A);
    hipLaunchKernelGGL(pqn_egreedy_kernel, dim3((N + 255) / 256), dim3(256), 0, as_stream(stream), q, random_actions, u, (float)epsilon,
                       actions_out, values_out, action_i64_out, N, A);
    return check_launch("pqn_egreedy_kernel");
}

extern "C" MI355PPO_API int mi355ppo_pqn_qlambda_f32(const float* rewards, const float* dones, const float* values, const float* next_done,
                                                    const float* next_q, float* returns, int T, int N, int A, double gamma,
                                                    double q_lambda, void* stream) {
    const char* fn = "mi355ppo_pqn_qlambda_f32";
    MI355_REQUIRE(rewards && dones && values && next_done && next_q && returns, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(T > 0 && N > 0 && A > 0, MI355PPO_EINVAL, "%s: T=%d N=%d A=%d must be positive", fn, T, N, A);
    hipLaunchKernelGGL(pqn_qlambda_kernel, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), rewards, dones, values, next_done, next_q,
                       returns, T, N, A, (float)gamma, (float)q_lambda, (float)(1.0 - q_lambda));
    return check_launch("pqn_qlambda_kernel");
}

extern "C" MI355PPO_API int mi355ppo_pqn_td_loss_fwd_bwd_f32(const float* q, const int64_t* mb_inds, const float* b_actions, const float* b_returns,
                                                            float* dq, float* scalars_out, int M, int A, int64_t B, void* stream) {
    const char* fn = "mi355ppo_pqn_td_loss_fwd_bwd_f32";
    MI355_REQUIRE(q && mb_inds && b_actions && b_returns && dq && scalars_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && A > 0 && B > 0, MI355PPO_EINVAL, "%s: M=%d A=%d B=%lld must be positive", fn, M, A, (long long)B);
    hipLaunchKernelGGL(pqn_td_loss_kernel, dim3((M + 255) / 256), dim3(256), 0, as_stream(stream), q, mb_inds, b_actions, b_returns, dq,
                       scalars_out, M, A, B, (float)(2.0 / (double)M));
    return check_launch("pqn_td_loss_kernel");
}

static int pqn_mlp_shape(const char* fn, int N, int O, int A) {
    MI355_REQUIRE(N > 0 && O > 0 && O <= kPqnMaxObs && A > 0 && A <= kPqnMaxA, MI355PPO_EINVAL,
                  "%s: rows=%d obs_dim=%d n_actions=%d: the PQN MLP takes 1 <= obs_dim <= %d, 1 <= n_actions <= %d", fn, N, O, A, kPqnMaxObs,
                  kPqnMaxA);
    return MI355PPO_OK;
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_fwd_f32(const float* obs, const float* params, float* q_out, int N, int O, int A, void* stream) {
    const char* fn = "mi355ppo_pqn_mlp_fwd_f32";
    MI355_REQUIRE(obs && params && q_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = pqn_mlp_shape(fn, N, O, A)) return rc;
    hipLaunchKernelGGL(pqn_mlp_fwd_kernel<false>, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), obs, params, q_out, N, O, A, nullptr,
                       nullptr, 0.0f, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    return check_launch("pqn_mlp_fwd_kernel");
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_act_f32(const float* obs, const float* params, const int64_t* random_actions, const float* u,
                                                    double epsilon, float* actions_out, float* values_out, int64_t* action_i64_out,
                                                    float* obs_row_out, const float* done_in, float* done_row_out, int N, int O, int A,
                                                    void* stream) {
    const char* fn = "mi355ppo_pqn_mlp_act_f32";
    MI355_REQUIRE(obs && params && random_actions && u && actions_out && values_out && (!done_row_out || done_in), MI355PPO_EINVAL,
                  "%s: null pointer", fn);
    if (int rc = pqn_mlp_shape(fn, N, O, A)) return rc;
    hipLaunchKernelGGL(pqn_mlp_fwd_kernel<true>, dim3((N + 63) / 64), dim3(64), 0, as_stream(stream), obs, params, nullptr, N, O, A,
                       random_actions, u, (float)epsilon, actions_out, values_out, action_i64_out, obs_row_out, done_in, done_row_out);
    return check_launch("pqn_mlp_act_kernel");
}

static int64_t pqn_mp(int M) { return ((int64_t)M + 63) / 64 * 64; }

extern "C" MI355PPO_API size_t mi355ppo_pqn_mlp_td_workspace_bytes(int M, int O, int A) {
    if (M <= 0 || O <= 0 || A <= 0) return 0;
    const int64_t nblk = ((int64_t)M + kPqnRows - 1) / kPqnRows;
    return (size_t)(pqn_units(O, A).total * pqn_mp(M) + nblk * pqn_param_count(O, A)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_pqn_mlp_td_fwd_bwd_f32(const float* b_obs, int64_t B, const int64_t* mb_inds, const float* params,
                                                           const float* b_actions, const float* b_returns, float* grads, float* scalars_out,
                                                           int M, int O, int A, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_pqn_mlp_td_fwd_bwd_f32";
    MI355_REQUIRE(b_obs && mb_inds && params && b_actions && b_returns && grads && scalars_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%lld must be positive", fn, (long long)B);
    if (int rc = pqn_mlp_shape(fn, M, O, A)) return rc;
    const size_t need = mi355ppo_pqn_mlp_td_workspace_bytes(M, O, A);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const int Mp = (int)pqn_mp(M);
    const int nblk = (M + kPqnRows - 1) / kPqnRows;
    const PqnUnits U = pqn_units(O, A);
    const int64_t P = pqn_param_count(O, A);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(pqn_mlp_td_kernel, dim3(nblk), dim3(kPqnRows), 0, s, b_obs, B, mb_inds, params, b_actions, b_returns, ws, M, Mp, O, A,
                       (float)(2.0 / (double)M));
    if (int rc = check_launch("pqn_mlp_td_kernel")) return rc;
    hipLaunchKernelGGL(pqn_mlp_fold_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, ws, nblk, P, M, Mp, U.old, U.sq,
                       (int64_t)U.total * Mp, grads, scalars_out);
    return check_launch("pqn_mlp_fold_kernel");
}

// The constants of RAdam step `step` (1-based) as pqn_radam_elem consumes them, from torch's formulas in double:
// {bias_correction1, lr, bias_correction2 ** 0.5, rect, rho_t > 5, 0, 0, 0}.
extern "C" MI355PPO_API int mi355ppo_radam_schedule_f32(double lr, double beta1, double beta2, int64_t step, float* out8_host) {
    MI355_REQUIRE(out8_host && step >= 1, MI355PPO_EINVAL, "mi355ppo_radam_schedule_f32: null pointer or step=%lld < 1", (long long)step);
    const double st = (double)step;
    const double bc1 = 1.0 - pow(beta1, st);
    const double bc2 = 1.0 - pow(beta2, st);
    const double rho_inf = 2.0 / (1.0 - beta2) - 1.0;
    const double rho_t = rho_inf - 2.0 * st * pow(beta2, st) / bc2;
    const bool rectified = rho_t > 5.0;
    const double rect = rectified ? sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) : 0.0;
    out8_host[0] = (float)bc1;
    out8_host[1] = (float)lr;
    out8_host[2] = (float)pow(bc2, 0.5);
    out8_host[3] = (float)rect;
    out8_host[4] = rectified ? 1.0f : 0.0f;
    out8_host[5] = out8_host[6] = out8_host[7] = 0.0f;
    return MI355PPO_OK;
}

extern "C" MI355PPO_API size_t mi355ppo_clip_radam_workspace_bytes(int64_t n) {
    return (size_t)pqn_sumsq_blocks(n) * sizeof(double);
}

static int clip_radam_impl(const char* fn, float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double max_grad_norm,
                           double beta1, double beta2, double eps, const PqnSlot& slot, const float* sched, float* total_norm_out,
                           void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(params && grads && exp_avg && exp_avg_sq, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(n > 0, MI355PPO_EINVAL, "%s: n=%lld must be > 0", fn, (long long)n);
    const size_t need = mi355ppo_clip_radam_workspace_bytes(n);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 8), MI355PPO_EALIGN, "%s: workspace must be 8-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const int G = pqn_sumsq_blocks(n);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(pqn_sumsq_kernel, dim3(G), dim3(256), 0, s, grads, n, partials);
    if (int rc = check_launch("pqn_sumsq_kernel")) return rc;
    RAdamParams R;
    R.max_norm = (float)max_grad_norm;
    R.w1 = (float)(1.0 - beta1);
    R.beta2 = (float)beta2;
    R.w2 = (float)(1.0 - beta2);
    R.eps = (float)eps;
    R.nblocks = G;
    int64_t ublocks = (n + 255) / 256;
    if (ublocks > 2048) ublocks = 2048;
    hipLaunchKernelGGL(pqn_radam_kernel, dim3((unsigned)ublocks), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, n, R, partials, slot,
                       sched, total_norm_out);
    return check_launch("pqn_radam_kernel");
}

// clip_grad_norm_(max_grad_norm) + RAdam(lr, betas, eps) step `step` (1-based) on flat buffers; the step's constants travel as
// kernel arguments.
extern "C" MI355PPO_API int mi355ppo_clip_radam_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double max_grad_norm,
                                                   double lr, double beta1, double beta2, double eps, int64_t step, float* total_norm_out,
                                                   void* workspace, size_t workspace_bytes, void* stream) {
    PqnSlot slot;
    if (int rc = mi355ppo_radam_schedule_f32(lr, beta1, beta2, step, slot.c)) return rc;
    return clip_radam_impl("mi355ppo_clip_radam_f32", params, grads, exp_avg, exp_avg_sq, n, max_grad_norm, beta1, beta2, eps, slot, nullptr,
                           total_norm_out, workspace, workspace_bytes, stream);
}

// The same step with its schedule slot (the kPqnSched floats mi355ppo_radam_schedule_f32 writes) read from DEVICE memory: a captured
// launch replays with the next step's learning rate and corrections.  Bit-identical to mi355ppo_clip_radam_f32 for the same (lr, step).
extern "C" MI355PPO_API int mi355ppo_clip_radam_sched_f32(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                                                         double max_grad_norm, double beta1, double beta2, double eps, const float* sched8,
                                                         float* total_norm_out, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(sched8 && aligned(sched8, 4), MI355PPO_EINVAL, "mi355ppo_clip_radam_sched_f32: null or misaligned schedule slot");
    PqnSlot slot = {};
    return clip_radam_impl("mi355ppo_clip_radam_sched_f32", params, grads, exp_avg, exp_avg_sq, n, max_grad_norm, beta1, beta2, eps, slot, sched8,
                           total_norm_out, workspace, workspace_bytes, stream);
}
