// DQN / C51 (cleanrl/dqn.py, cleanrl/c51.py): the rollout's greedy action and the training step's forward + loss + backward over
// the device replay ring of offpolicy.hip (gfx950).
//
// At batch 128 and widths 120 / 84 every launch is latency-bound, so the mapping is plain f32 VALU.  A workgroup of 256 threads takes
// a tile of kOpRows rows through both networks; the rows' vectors live in LDS and the weights (20 KB before the last layer, up to
// 172 KB for it) are streamed from L2 by every workgroup, never held:
//
//   forward     thread (r, j) runs one dot product over the layer's inputs (LDS reads of row r, lane j walks row j of W).
//   q values    thread (r, a) runs the softmax of action a's atoms in place and (pmfs * atoms).sum in ascending atom order.
//   projection  thread (r, j) forms l, u, d_m_l, d_m_u of source atom j; thread (r, k) then walks j for target atom k: first the
//               d_m_l[j] with l[j] == k, then the d_m_u[j] with u[j] == k -- the reference's two serial index_add_ calls.
//   backward    thread (r, k) owns input unit k: sum_j dz[j] * W[j, k] reads W coalesced; the ReLU mask is applied in place.
//   gradient    thread e owns weight elements e, e + 256, ...: the tile's rows are added in ascending order and then into the
//               workgroup's partial (tiles ascending); a second launch (op_fold_kernel) adds the partials in workgroup order into
//               the flat gradient and folds the two row scalars in f64 slots.  No atomics anywhere.
//
// No entry point allocates or synchronises; every one validates before its first HIP call and takes the stream last.
#include "common.h"
#include "dqn_rows.h"
#include "offpolicy_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kDqXS = kDqMaxObs;                    // stride of the input rows
constexpr int kDqZS = kDqMaxOut;                    // stride of the output rows (logits / pmfs / their gradient)
constexpr int kDqPS = kDqMaxAtoms;                  // stride of the per-atom rows

// out[r, j] = act(b[j] + sum_k xin[r, k] * W[j, k]) for the tile's kOpRows rows and j < J.  Ends with a barrier.
template <bool RELU>
__device__ void dq_layer(const float* xin, int xs, int K, const float* __restrict__ W, const float* __restrict__ b, int J, float* out, int os) {
    J = op_here(J);                                 // the divisor's reciprocal is formed here, not kept in SGPRs across the tile loop
    for (int idx = threadIdx.x; idx < kOpRows * J; idx += kOpT) {
        const int r = idx / J, j = idx - r * J;
        const float* w = W + (int64_t)j * K;
        const float* x = xin + r * xs;
        float acc = 0.0f;
        for (int k = 0; k < K; ++k) acc = op_mac(acc, x[k], w[k]);
        const float v = acc + b[j];
        out[r * os + j] = RELU ? op_relu(v) : v;
    }
    __syncthreads();
}

__device__ void dq_forward(const DqNet& n, const float* x, float* h1, float* h2, float* z) {
    dq_layer<true>(x, kDqXS, n.O, n.w1, n.b1, kDqH1, h1, kDqH1);
    dq_layer<true>(h1, kDqH1, kDqH1, n.w2, n.b2, kDqH2, h2, kDqH2);
    dq_layer<false>(h2, kDqH2, kDqH2, n.w3, n.b3, n.J, z, kDqZS);
}

// qv[r, a]: with atoms, the pmfs of every action replace its logits in z and qv is (pmfs * atoms).sum; without, qv = z.  Barrier.
__device__ void dq_qvalues(float* z, int n, int na, const float* __restrict__ atoms, float* qv) {
    const int t = threadIdx.x;
    n = op_here(n);
    if (t < kOpRows * n) {
        const int r = t / n, a = t - r * n;
        float* za = z + r * kDqZS + a * na;
        qv[r * kDqMaxAct + a] = (na > 1) ? dq_softmax_q(za, na, atoms, za) : za[0];
    }
    __syncthreads();
}

// io[r, k] = relu'(io[r, k]) * sum_{j < J} dz[r * ds + j] * W[j * K + k] for k < K (in place over the layer's ReLU output).  Barrier.
__device__ void dq_dgrad_masked(const float* dz, int ds, int J, const float* __restrict__ W, int K, float* io, int ios) {
    K = op_here(K);
    for (int idx = threadIdx.x; idx < kOpRows * K; idx += kOpT) {
        const int r = idx / K, k = idx - r * K;
        float acc = 0.0f;
        for (int j = 0; j < J; ++j) acc = op_mac(acc, dz[r * ds + j], W[(int64_t)j * K + k]);
        io[r * ios + k] = op_relu_bwd(io[r * ios + k], acc);
    }
    __syncthreads();
}

// wg_wgrad with a bias loop (J reaches 512 here): part_w[j * K + k] (+)= sum_{r < nr} dz[r, j] * in[r, k], part_b[j] (+)= sum_r dz[r, j]
__device__ void dq_wgrad(const float* dz, int ds, const float* in, int is, int J, int K, float* __restrict__ part_w, float* __restrict__ part_b,
                         bool first, int nr) {
    K = op_here(K);
    const int n = J * K;
    for (int e = threadIdx.x; e < n; e += kOpT) {
        const int j = e / K, k = e - j * K;
        float acc = 0.0f;
        for (int r = 0; r < nr; ++r) acc = op_mac(acc, dz[r * ds + j], in[r * is + k]);
        part_w[e] = first ? acc : part_w[e] + acc;
    }
    for (int j = threadIdx.x; j < J; j += kOpT) {
        float acc = 0.0f;
        for (int r = 0; r < nr; ++r) acc = acc + dz[r * ds + j];
        part_b[j] = first ? acc : part_b[j] + acc;
    }
    __syncthreads();
}

__device__ void dq_gather(const float* __restrict__ src, const OpRing& R, int r0, int nr, int O, float* x) {
    O = op_here(O);
    for (int i = threadIdx.x; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        x[r * kDqXS + k] = (r < nr) ? src[ring_row(R, r0 + r) * O + k] : 0.0f;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(256) void dq_act_kernel(const float* __restrict__ obs, const float* __restrict__ params, const float* __restrict__ atoms,
                                                     int64_t* __restrict__ actions, float* __restrict__ q_out, int N, int O, int n, int na) {
    __shared__ float x[kOpRows * kDqXS], h1[kOpRows * kDqH1], h2[kOpRows * kDqH2], z[kOpRows * kDqZS], qv[kOpRows * kDqMaxAct];
    const int t = threadIdx.x, r0 = blockIdx.x * kOpRows;
    for (int i = t; i < kOpRows * O; i += kOpT) {
        const int r = i / O, k = i - r * O;
        x[r * kDqXS + k] = (r0 + r < N) ? obs[(int64_t)(r0 + r) * O + k] : 0.0f;
    }
    __syncthreads();
    dq_forward(dq_net(params, O, n * na), x, h1, h2, z);
    dq_qvalues(z, n, na, atoms, qv);
    if (q_out && t < kOpRows * n) {
        const int r = t / n, a = t - r * n;
        if (r0 + r < N) q_out[(int64_t)(r0 + r) * n + a] = qv[r * kDqMaxAct + a];
    }
    if (t < kOpRows && r0 + t < N) actions[r0 + t] = (int64_t)dq_argmax(qv + t * kDqMaxAct, n);
}

// ws: rows (2 x Mp: the row's loss term | its q value), then partials [G][P].  aux_a / aux_b (optional):
//   DQN  target_network(next_obs) (M, n) and td_target (M);  C51  next_pmfs (M, n_atoms) and target_pmfs (M, n_atoms).
template <bool C51>
__global__ __launch_bounds__(256) void dq_update_kernel(OpRing R, const float* __restrict__ online, const float* __restrict__ target,
                                                        const float* __restrict__ atoms, float* __restrict__ ws, float* __restrict__ aux_a,
                                                        float* __restrict__ aux_b, int M, int Mp, int O, int n, int na, int G, float gamma,
                                                        float vmin, float vmax, float norm) {
    constexpr int kP = C51 ? kOpRows * kDqPS : 1;
    __shared__ float x[kOpRows * kDqXS], h1[kOpRows * kDqH1], h2[kOpRows * kDqH2], z[kOpRows * kDqZS], qv[kOpRows * kDqMaxAct], yv[kOpRows],
        dq[kOpRows], pl[kP], pu[kP], pdl[kP], pdu[kP], tp[kP];
    __shared__ int act[kOpRows];
    const int t = threadIdx.x, g = blockIdx.x, J = n * na;
    const int64_t P = dq_count(O, J);
    float* part = ws + (int64_t)2 * Mp + (int64_t)g * P;
    float* rowa = ws;
    float* rowb = ws + Mp;
    const int ntiles = op_tiles(M);
    for (int tl = g; tl < ntiles; tl += G) {
        const int r0 = tl * kOpRows, nr = (M - r0 < kOpRows) ? M - r0 : kOpRows;
        const bool first = tl == g;
        // ---- the target network on next_obs
        dq_gather(R.next_obs, R, r0, nr, O, x);
        dq_forward(dq_net(target, op_here(O), J), x, h1, h2, z);
        dq_qvalues(z, n, na, atoms, qv);
        if constexpr (C51) {
            if (t < kOpRows) act[t] = dq_argmax(qv + t * kDqMaxAct, n);
            __syncthreads();
            const float delta_z = atoms[1] - atoms[0];
            for (int idx = t; idx < kOpRows * na; idx += kOpT) {
                const int r = idx / na, j = idx - r * na;
                C51Proj e;
                e.l = e.u = -1.0f;
                e.dml = e.dmu = 0.0f;
                if (r < nr) {
                    const int64_t row = ring_row(R, r0 + r);
                    const float p = z[r * kDqZS + act[r] * na + j];
                    e = c51_proj_elem(R.rewards[row], R.dones[row], gamma, atoms[j], vmin, vmax, delta_z, na, p, false);
                    if (aux_a) aux_a[(int64_t)(r0 + r) * na + j] = p;
                }
                pl[r * kDqPS + j] = e.l;
                pu[r * kDqPS + j] = e.u;
                pdl[r * kDqPS + j] = e.dml;
                pdu[r * kDqPS + j] = e.dmu;
            }
            __syncthreads();
            for (int idx = t; idx < kOpRows * na; idx += kOpT) {
                const int r = idx / na, k = idx - r * na;
                const float v = c51_proj_atom(k, pl + r * kDqPS, pu + r * kDqPS, pdl + r * kDqPS, pdu + r * kDqPS, na);
                tp[r * kDqPS + k] = v;
                if (aux_b && r < nr) aux_b[(int64_t)(r0 + r) * na + k] = v;
            }
            __syncthreads();
        } else {
            if (aux_a && t < kOpRows * n) {
                const int r = t / n, a = t - r * n;
                if (r < nr) aux_a[(int64_t)(r0 + r) * n + a] = qv[r * kDqMaxAct + a];
            }
            if (t < kOpRows) {
                float y = 0.0f;
                if (t < nr) {
                    const int64_t row = ring_row(R, r0 + t);
                    y = dq_td_target(R.rewards[row], R.dones[row], gamma, qv[t * kDqMaxAct + dq_argmax(qv + t * kDqMaxAct, n)]);
                    if (aux_b) aux_b[r0 + t] = y;
                }
                yv[t] = y;
            }
            __syncthreads();
        }
        // ---- the online network on obs, the loss and its gradient at the logits (into z)
        if (t < kOpRows) act[t] = (t < nr) ? dq_action_index(R.actions[ring_row(R, r0 + t)], n) : 0;
        dq_gather(R.obs, R, r0, nr, O, x);
        dq_forward(dq_net(online, op_here(O), J), x, h1, h2, z);
        dq_qvalues(z, n, na, atoms, qv);
        if constexpr (C51) {
            for (int idx = t; idx < kOpRows * na; idx += kOpT) {
                const int r = idx / na, k = idx - r * na;
                const C51Loss e = c51_loss_elem(tp[r * kDqPS + k], z[r * kDqZS + act[r] * na + k], norm);
                pl[r * kDqPS + k] = e.term;
                pdl[r * kDqPS + k] = e.g;
                pdu[r * kDqPS + k] = e.gp;
            }
            __syncthreads();
            if (t < kOpRows) {
                float s = 0.0f, dot = 0.0f;
                for (int k = 0; k < na; ++k) {
                    s = s + pl[t * kDqPS + k];
                    dot = dot + pdu[t * kDqPS + k];
                }
                yv[t] = dot;
                if (t < nr) {
                    rowa[r0 + t] = -s;
                    rowb[r0 + t] = qv[t * kDqMaxAct + act[t]];
                }
            }
            __syncthreads();
            for (int idx = t; idx < kOpRows * J; idx += kOpT) {
                const int r = idx / J, j = idx - r * J;
                const int a = j / na, k = j - a * na;
                z[r * kDqZS + j] = (r < nr && a == act[r]) ? c51_dlogit(z[r * kDqZS + j], pdl[r * kDqPS + k], yv[r]) : 0.0f;
            }
            __syncthreads();
        } else {
            if (t < kOpRows) {
                float d = 0.0f;
                if (t < nr) {
                    float sq;
                    const float q = qv[t * kDqMaxAct + act[t]];
                    d = op_mse_row(q, yv[t], norm, &sq);
                    rowa[r0 + t] = sq;
                    rowb[r0 + t] = q;
                }
                dq[t] = d;
            }
            __syncthreads();
            for (int idx = t; idx < kOpRows * J; idx += kOpT) {
                const int r = idx / J, j = idx - r * J;
                z[r * kDqZS + j] = (j == act[r]) ? dq[r] : 0.0f;
            }
            __syncthreads();
        }
        // ---- backward through the online network into the workgroup's partial
        {
            const int Oh = op_here(O);
            const DqNet qn = dq_net(online, Oh, J);
            const DqOff off = dq_off(Oh, J);
            dq_wgrad(z, kDqZS, h2, kDqH2, J, kDqH2, part + off.w3, part + off.b3, first, nr);
            dq_dgrad_masked(z, kDqZS, J, qn.w3, kDqH2, h2, kDqH2);
            dq_wgrad(h2, kDqH2, h1, kDqH1, kDqH2, kDqH1, part + off.w2, part + off.b2, first, nr);
            dq_dgrad_masked(h2, kDqH2, kDqH2, qn.w2, kDqH1, h1, kDqH1);
            dq_wgrad(h1, kDqH1, x, kDqXS, kDqH1, Oh, part + off.w1, part + off.b1, first, nr);
        }
    }
}

static size_t dq_workspace(int M, int O, int n, int na) {
    if (M <= 0 || !dq_limits(O, n, na)) return 0;
    return (size_t)(2 * op_mp(M) + (int64_t)op_groups(M) * dq_count(O, n * na)) * sizeof(float);
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_dqn_act_f32(const float* obs, const float* params, const float* atoms, int64_t* actions_out, float* q_out,
                                                int N, int O, int n_actions, int n_atoms, void* stream) {
    const char* fn = "mi355ppo_dqn_act_f32";
    MI355_REQUIRE(obs && params && actions_out, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = dq_shape(fn, N, O, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms == 1 || atoms, MI355PPO_EINVAL, "%s: n_atoms=%d needs the atoms", fn, n_atoms);
    hipLaunchKernelGGL(dq_act_kernel, dim3(op_tiles(N)), dim3(256), 0, as_stream(stream), obs, params, atoms, actions_out, q_out, N, O, n_actions,
                       n_atoms);
    return check_launch("dq_act_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_dqn_td_workspace_bytes(int M, int O, int n_actions) { return dq_workspace(M, O, n_actions, 1); }

extern "C" MI355PPO_API int mi355ppo_dqn_td_fwd_bwd_f32(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                                       const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                       const int64_t* env_inds, int64_t slots, int n_envs, const float* online,
                                                       const float* target, double gamma, float* grads, float* scalars_out, float* target_q_out,
                                                       float* td_target_out, int M, int O, int n_actions, void* workspace,
                                                       size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_dqn_td_fwd_bwd_f32";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && online && target && grads && scalars_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = dq_shape(fn, M, O, n_actions, 1)) return rc;
    OpRing R;
    if (int rc = op_ring_args(fn, R, ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, dq_workspace(M, O, n_actions, 1))) return rc;
    hipStream_t s = as_stream(stream);
    const int Mp = (int)op_mp(M), G = op_groups(M);
    const int64_t P = dq_count(O, n_actions);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(dq_update_kernel<false>, dim3(G), dim3(256), 0, s, R, online, target, (const float*)nullptr, ws, target_q_out, td_target_out,
                       M, Mp, O, n_actions, 1, G, (float)gamma, 0.0f, 0.0f, (float)(2.0 / (double)M));
    if (int rc = check_launch("dq_update_kernel<dqn>")) return rc;
    // rows: squared error | old_val -> scalars {td_loss, mean old_val}
    return op_fold_launch(s, ws + (int64_t)2 * Mp, G, P, grads, ws, Mp, M, 2, 1.0f, scalars_out);
}

extern "C" MI355PPO_API size_t mi355ppo_c51_workspace_bytes(int M, int O, int n_actions, int n_atoms) {
    return n_atoms >= 2 ? dq_workspace(M, O, n_actions, n_atoms) : 0;
}

extern "C" MI355PPO_API int mi355ppo_c51_fwd_bwd_f32(const float* ring_obs, const float* ring_next_obs, const float* ring_actions,
                                                    const float* ring_rewards, const float* ring_dones, const int64_t* batch_inds,
                                                    const int64_t* env_inds, int64_t slots, int n_envs, const float* online, const float* target,
                                                    const float* atoms, double gamma, double v_min, double v_max, float* grads,
                                                    float* scalars_out, float* next_pmfs_out, float* target_pmfs_out, int M, int O,
                                                    int n_actions, int n_atoms, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_c51_fwd_bwd_f32";
    MI355_REQUIRE(ring_obs && ring_next_obs && ring_actions && ring_rewards && ring_dones && online && target && atoms && grads && scalars_out,
                  MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int rc = dq_shape(fn, M, O, n_actions, n_atoms)) return rc;
    MI355_REQUIRE(n_atoms >= 2, MI355PPO_EINVAL, "%s: n_atoms=%d: the projection needs two atoms (delta_z = atoms[1] - atoms[0])", fn, n_atoms);
    OpRing R;
    if (int rc = op_ring_args(fn, R, ring_obs, ring_next_obs, ring_actions, ring_rewards, ring_dones, batch_inds, env_inds, slots, n_envs)) return rc;
    if (int rc = op_workspace_ok(fn, workspace, workspace_bytes, dq_workspace(M, O, n_actions, n_atoms))) return rc;
    hipStream_t s = as_stream(stream);
    const int Mp = (int)op_mp(M), G = op_groups(M);
    const int64_t P = dq_count(O, n_actions * n_atoms);
    float* ws = static_cast<float*>(workspace);
    hipLaunchKernelGGL(dq_update_kernel<true>, dim3(G), dim3(256), 0, s, R, online, target, atoms, ws, next_pmfs_out, target_pmfs_out, M, Mp, O,
                       n_actions, n_atoms, G, (float)gamma, (float)v_min, (float)v_max, (float)(1.0 / (double)M));
    if (int rc = check_launch("dq_update_kernel<c51>")) return rc;
    // rows: -(target_pmfs * log old_pmfs).sum | (old_pmfs * atoms).sum -> scalars {loss, mean old_val}
    return op_fold_launch(s, ws + (int64_t)2 * Mp, G, P, grads, ws, Mp, M, 2, 1.0f, scalars_out);
}
