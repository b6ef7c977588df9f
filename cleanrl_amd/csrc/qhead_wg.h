// Device pieces the Atari Q heads (dqn_atari.hip) and Rainbow's dueling head (rainbow.hip) share: the head forward kernel, the
// categorical row and the frame gather.  Included by the two kernel files only; the row math is dqn_rows.h / dqn_atari_rows.h /
// rainbow_rows.h, the serial forms of the last two pieces are c51_row_host and da_gather_host there.
#pragma once
#include "common.h"
#include "rainbow_rows.h"
#include "offpolicy_wg.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kQhTJ = 32;            // outputs per forward tile
constexpr int kQhTK = 64;            // k-depth of the staged weight tile
constexpr int kQhTLd = kQhTK + 1;    // padded: lane j reads word j * 65 + k, 32 different banks
static_assert(kRbHid == kDaH, "both heads' outputs read 512 hidden columns");

struct QhPasses {
    const float *h[3], *w[3], *b[3];           // one {h, W, b} per pass (grid z), up to three
};

// z[pass][r, j] = b[j] + sum_k h[r, col0(j) + k] * W[j, k], k < K (512; 256 for the QDagger head).  ROW: the row width of h -- K
// (col0 = 0) or kRbH2 (both streams' hidden columns, col0 = rb_col0(j, na)).  grid (ceil(J / 32), ceil(M / 8), passes); z: passes x M x J.  h's 8 rows sit in
// LDS (16 | 32 KB), W streams from L2 through a 32 x 64 LDS tile (8.3 KB); thread (row, output) runs its dot product in ascending k.
template <int ROW, int K = kDaH>
__global__ __launch_bounds__(256) void qh_fwd_kernel(QhPasses H, float* __restrict__ z, int M, int J, int na) {
    __shared__ float hs[kOpRows * ROW], wt[kQhTJ * kQhTLd];
    const int t = threadIdx.x, pass = blockIdx.z, j0 = blockIdx.x * kQhTJ, r0 = blockIdx.y * kOpRows;
    const float* __restrict__ h = H.h[pass];
    const float* __restrict__ W = H.w[pass];
    for (int i = t; i < kOpRows * ROW; i += 256) {
        const int r = i / ROW;
        hs[i] = (r0 + r < M) ? h[(int64_t)r0 * ROW + i] : 0.0f;
    }
    const int jj = t & (kQhTJ - 1), r = t / kQhTJ;
    const float* x = hs + r * ROW + (ROW == K ? 0 : rb_col0(j0 + jj, na));
    float acc = 0.0f;
    for (int k0 = 0; k0 < K; k0 += kQhTK) {
        __syncthreads();                                    // hs is complete (first pass); the previous tile has been read
        for (int i = t; i < kQhTJ * kQhTK; i += 256) {
            const int wj = i / kQhTK, wk = i - wj * kQhTK;
            wt[wj * kQhTLd + wk] = (j0 + wj < J) ? W[(int64_t)(j0 + wj) * K + k0 + wk] : 0.0f;
        }
        __syncthreads();
        for (int kk = 0; kk < kQhTK; ++kk) acc = op_mac(acc, x[k0 + kk], wt[jj * kQhTLd + kk]);
    }
    if (r0 + r < M && j0 + jj < J) z[((int64_t)pass * M + r0 + r) * J + j0 + jj] = acc + H.b[pass][j0 + jj];
}

template <int ROW, int K = kDaH>
static int qh_fwd_launch(hipStream_t s, const QhPasses& H, int passes, float* z, int M, int J, int na) {
    hipLaunchKernelGGL((qh_fwd_kernel<ROW, K>), dim3((J + kQhTJ - 1) / kQhTJ, op_tiles(M), passes), dim3(256), 0, s, H, z, M, J, na);
    return check_launch("qh_fwd_kernel");
}

// The categorical update of one batch row by its workgroup, over LDS arrays of n_atoms floats the caller owns: the projection of
// pnext (the target's pmf at the chosen action) into tp, the loss elements against pred (the online pmf at the taken action), thread
// 0's two serial sums and dq[k] = d loss / d logit k.  next_row / target_row: the row's optional next_pmfs / target_pmfs outputs.
// scale multiplies the row's gradient.  Four barriers; thread k < na leaves dq[k] without one.  Returns the row's loss in thread 0.
struct QhRowLds {
    float *pl, *pu, *pdl, *pdu, *tp, *dq, *dot;
};
__device__ __forceinline__ float wg_c51_row(const QhRowLds& L, const float* pnext, const float* pred, const float* __restrict__ atoms, float rew,
                                            float done, float gamma, float vmin, float vmax, float delta_z, int na, float scale, bool l_eq_b,
                                            float* __restrict__ next_row, float* __restrict__ target_row) {
    const int t = threadIdx.x;
    if (t < na) {
        const float p = pnext[t];
        const C51Proj e = c51_proj_elem(rew, done, gamma, atoms[t], vmin, vmax, delta_z, na, p, l_eq_b);
        L.pl[t] = e.l;
        L.pu[t] = e.u;
        L.pdl[t] = e.dml;
        L.pdu[t] = e.dmu;
        if (next_row) next_row[t] = p;
    }
    __syncthreads();
    if (t < na) {
        const float v = c51_proj_atom(t, L.pl, L.pu, L.pdl, L.pdu, na);
        L.tp[t] = v;
        if (target_row) target_row[t] = v;
    }
    __syncthreads();
    if (t < na) {
        const C51Loss e = c51_loss_elem(L.tp[t], pred[t], scale);
        L.pl[t] = e.term;
        L.pdl[t] = e.g;
        L.pdu[t] = e.gp;
    }
    __syncthreads();
    float s = 0.0f;
    if (t == 0) {
        float dot = 0.0f;
        for (int k = 0; k < na; ++k) {
            s = s + L.pl[k];
            dot = dot + L.pdu[k];
        }
        *L.dot = dot;
    }
    __syncthreads();
    if (t < na) L.dq[t] = c51_dlogit(pred[t], L.pdl[t], *L.dot);
    return -s;
}

// The batch's frames out of a u8 frame ring into (2M, 84, 84, 4): frame y < M is the observation of sample y, y >= M the next
// observation of sample y - M.  ALIASED: one ring, the next observation is ring_a's frame at da_next_slot; otherwise it is ring_b's
// frame at the same slot.  ei == nullptr: env 0.  grid (ceil(7056 / 256), 2M), one thread per pixel word.
template <bool ALIASED>
__global__ __launch_bounds__(256) void qh_gather_kernel(const uint32_t* __restrict__ ring_a, const uint32_t* __restrict__ ring_b,
                                                        const int64_t* __restrict__ ring_actions, const float* __restrict__ ring_rewards,
                                                        const float* __restrict__ ring_dones, const int64_t* __restrict__ bi,
                                                        const int64_t* __restrict__ ei, int64_t slots, int N, uint32_t* __restrict__ frames,
                                                        int64_t* __restrict__ actions, float* __restrict__ rewards, float* __restrict__ dones,
                                                        int M) {
    const int f = blockIdx.y, m = f < M ? f : f - M;
    const int64_t slot = op_clamp(bi[m], slots);
    const int e = ei ? (int)op_clamp(ei[m], N) : 0;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const uint32_t* __restrict__ src = (ALIASED || f < M) ? ring_a : ring_b;
    if (p < kDaPix) frames[(int64_t)f * kDaPix + p] = src[da_frame(ALIASED && f >= M ? da_next_slot(slot, slots) : slot, e, N) + p];
    if (f < M && p == 0) {
        actions[m] = ring_actions[slot * N + e];
        rewards[m] = ring_rewards[slot * N + e];
        dones[m] = ring_dones[slot * N + e];
    }
}

template <bool ALIASED>
static int qh_gather_launch(hipStream_t s, const uint8_t* ring_a, const uint8_t* ring_b, const int64_t* ring_actions, const float* ring_rewards,
                            const float* ring_dones, const int64_t* bi, const int64_t* ei, int64_t slots, int N, uint8_t* frames, int64_t* actions,
                            float* rewards, float* dones, int M) {
    hipLaunchKernelGGL(qh_gather_kernel<ALIASED>, dim3((kDaPix + 255) / 256, 2 * M), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(ring_a),
                       reinterpret_cast<const uint32_t*>(ring_b), ring_actions, ring_rewards, ring_dones, bi, ei, slots, N,
                       reinterpret_cast<uint32_t*>(frames), actions, rewards, dones, M);
    return check_launch("qh_gather_kernel");
}

}  // namespace mi355ppo
