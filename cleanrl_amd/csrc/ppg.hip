// Phasic Policy Gradient (cleanrl/ppg_procgen.py): what the auxiliary phase does around the IMPALA trunk -- the gather of whole stored
// rollouts, the old policy's normalised logits, and the three heads with the joint loss and its backward (gfx950).
//
// The arithmetic is tiny (1,024 x 256 x 17 multiply-adds per minibatch) and latency-bound: no matrix pipe.  Mappings (row math in
// ppg_rows.h, which the host twins of ppg_twins.hip run unchanged):
//
//   gather      grid = (rows, ceil(dwords_per_row / 1024)): obs.hip's streaming copy with the source row (t, cols[i]) formed per
//               workgroup in 64 bits; a lane loads 4 dwords and stores 4 float4
//   old_logits  one workgroup per kPpgRows rows: the actor's weight (stride 257: thread j's row on its own bank) and the tile's hidden
//               rows in LDS; thread (r, j) forms logit j of row r, thread r normalises row r, the tile writes its aux_pi rows
//   aux loss    (1) one workgroup per kPpgRows rows: all three heads' weights (33 KB) and the hidden rows (8 KB) in LDS; thread (r, j)
//                   forms output j of row r, thread r runs ppg_aux_row, thread k forms dh[., k] and column k of the tile's partial of
//                   dz^T h from the same LDS rows; the tile's three loss sums in f64
//               (2) one thread per head-gradient element adds the tiles' partials in ascending tile order and writes or adds once;
//                   three threads fold the loss sums
//
// No atomics, no allocation, no synchronisation: results are deterministic, every entry point can be captured into a graph.
#include "common.h"
#include "ppg_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kPpgWS = kPpgH + 1;       // LDS stride of a weight row: lanes j and j + 1 sit on neighbouring banks
constexpr int kPpgUnroll = 4;

__global__ __launch_bounds__(256) void ppg_gather_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ cols,
                                                         float* __restrict__ dst, int n, int64_t R, int64_t row_bytes, int dwords_per_row) {
    const int64_t r = blockIdx.x;
    const int64_t sr = ppg_row_offset(r, n, R, cols);
    const uint32_t* __restrict__ s = reinterpret_cast<const uint32_t*>(src + sr * row_bytes);
    float4* __restrict__ d = reinterpret_cast<float4*>(dst + r * row_bytes);
    const int base = blockIdx.y * (256 * kPpgUnroll) + threadIdx.x;
    uint32_t w[kPpgUnroll];
#pragma unroll
    for (int u = 0; u < kPpgUnroll; ++u) {
        const int k = base + u * 256;
        w[u] = (k < dwords_per_row) ? s[k] : 0u;
    }
#pragma unroll
    for (int u = 0; u < kPpgUnroll; ++u) {
        const int k = base + u * 256;
        if (k < dwords_per_row) {
            float4 o;
            o.x = ppg_u8_div255((float)(w[u] & 0xffu));
            o.y = ppg_u8_div255((float)((w[u] >> 8) & 0xffu));
            o.z = ppg_u8_div255((float)((w[u] >> 16) & 0xffu));
            o.w = ppg_u8_div255((float)(w[u] >> 24));
            d[k] = o;
        }
    }
}

// `rows` weight rows of one head -> LDS rows j0 .. j0 + rows - 1 (stride kPpgWS).
__device__ __forceinline__ void ppg_stage_w(const float* __restrict__ w, int rows, int j0, float* s_w) {
    for (int idx = threadIdx.x; idx < rows * kPpgH; idx += 256) s_w[(j0 + (idx >> 8)) * kPpgWS + (idx & (kPpgH - 1))] = w[idx];
}

// The tile's nr hidden rows -> LDS.
__device__ __forceinline__ void ppg_stage_h(const float* __restrict__ h, int r0, int nr, float* s_h) {
    for (int idx = threadIdx.x; idx < nr * kPpgH; idx += 256) s_h[idx] = h[(int64_t)r0 * kPpgH + idx];
}

__global__ __launch_bounds__(256) void ppg_old_logits_kernel(const float* __restrict__ h, const float* __restrict__ wa, const float* __restrict__ ba,
                                                             const int64_t* __restrict__ cols, float* __restrict__ aux_pi, int M, int n, int64_t R,
                                                             int A) {
    __shared__ float s_w[kPpgMaxA * kPpgWS];
    __shared__ float s_h[kPpgRows * kPpgH];
    __shared__ float s_z[kPpgRows * kPpgJ];
    const int r0 = blockIdx.x * kPpgRows;
    const int nr = (M - r0 < kPpgRows) ? M - r0 : kPpgRows;
    ppg_stage_w(wa, A, 0, s_w);
    ppg_stage_h(h, r0, nr, s_h);
    __syncthreads();
    const int r = threadIdx.x >> 5, j = threadIdx.x & 31;
    if (r < nr && j < A) s_z[r * kPpgJ + j] = ppg_dot(s_h + r * kPpgH, s_w + j * kPpgWS) + ba[j];
    __syncthreads();
    if (threadIdx.x < nr) ppg_lognorm_(s_z + threadIdx.x * kPpgJ, A);
    __syncthreads();
    if (r < nr && j < A) aux_pi[ppg_row_offset(r0 + r, n, R, cols) * A + j] = s_z[r * kPpgJ + j];
}

__global__ __launch_bounds__(256) void ppg_aux_rows_kernel(PpgAuxArgs a) {
    __shared__ float s_w[kPpgJ * kPpgWS];
    __shared__ float s_h[kPpgRows * kPpgH];
    __shared__ float s_z[kPpgRows * kPpgJ], s_old[kPpgRows * kPpgJ], s_dz[kPpgRows * kPpgJ];
    __shared__ double s_ls[kPpgRows * 3];
    const int A = a.A, J = a.A + 2, t = threadIdx.x;
    const int r0 = blockIdx.x * kPpgRows;
    const int nr = (a.M - r0 < kPpgRows) ? a.M - r0 : kPpgRows;
    ppg_stage_w(a.wa, A, 0, s_w);
    ppg_stage_w(a.wc, 1, A, s_w);
    ppg_stage_w(a.wx, 1, A + 1, s_w);
    ppg_stage_h(a.h, r0, nr, s_h);
    __syncthreads();
    const int r = t >> 5, j = t & 31;
    if (r < nr && j < J) {
        const float bias = j < A ? a.ba[j] : (j == A ? a.bc[0] : a.bx[0]);
        s_z[r * kPpgJ + j] = ppg_dot(s_h + r * kPpgH, s_w + j * kPpgWS) + bias;
        if (j < A) s_old[r * kPpgJ + j] = a.aux_pi[ppg_row_offset(r0 + r, a.n, a.R, a.cols) * A + j];
    }
    __syncthreads();
    if (t < nr) {
        const float ret = a.aux_returns[ppg_row_offset(r0 + t, a.n, a.R, a.cols)];
        double l3[3];
        ppg_aux_row(s_z + t * kPpgJ, s_old + t * kPpgJ, ret, A, a.g_kl, a.g_v, s_dz + t * kPpgJ, l3);
        s_ls[t * 3] = l3[0];
        s_ls[t * 3 + 1] = l3[1];
        s_ls[t * 3 + 2] = l3[2];
    }
    __syncthreads();
    for (int rr = 0; rr < nr; ++rr)
        a.dh[(int64_t)(r0 + rr) * kPpgH + t] = ppg_dh(s_dz + rr * kPpgJ, s_w + t, kPpgWS, s_w[(A + 1) * kPpgWS + t], A);
    float* part = a.part + (int64_t)blockIdx.x * kPpgPart;
    for (int jj = 0; jj < J; ++jj) part[jj * kPpgH + t] = ppg_tile_partial(s_dz + jj, kPpgJ, s_h + t, nr);
    if (t < J) part[kPpgJ * kPpgH + t] = ppg_tile_partial_bias(s_dz + t, kPpgJ, nr);
    if (t < 3) {
        double s = 0.0;
        for (int rr = 0; rr < nr; ++rr) s += s_ls[rr * 3 + t];
        a.sums[(int64_t)blockIdx.x * 3 + t] = s;
    }
}

__global__ __launch_bounds__(256) void ppg_aux_fold_kernel(const float* __restrict__ part, const double* __restrict__ sums, int tiles, int M, int A,
                                                           PpgGrads g, int accumulate, float* __restrict__ scalars) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < (A + 2) * (kPpgH + 1)) {
        int pi;
        float* out = ppg_grad_slot(g, e, A, &pi);
        float acc = 0.0f;
        for (int b = 0; b < tiles; ++b) acc = acc + part[(int64_t)b * kPpgPart + pi];
        *out = accumulate ? *out + acc : acc;
    }
    if (blockIdx.x == 0 && threadIdx.x < 3) {
        double s = 0.0;
        for (int b = 0; b < tiles; ++b) s += sums[(int64_t)b * 3 + threadIdx.x];
        scalars[threadIdx.x] = ppg_scalar(s, M, threadIdx.x);
    }
}

}  // namespace mi355ppo

using namespace mi355ppo;

// ------------------------------------------------------------------------------------------------------ entry points
extern "C" MI355PPO_API int mi355ppo_ppg_aux_gather_u8_f32(const unsigned char* aux_obs, const int64_t* cols, float* out, int T, int n, int64_t R,
                                                          int64_t row_bytes, void* stream) {
    const char* fn = "mi355ppo_ppg_aux_gather_u8_f32";
    if (int rc = ppg_gather_args(fn, aux_obs, cols, out, T, n, R, row_bytes)) return rc;
    const int dpr = (int)(row_bytes / 4);
    const dim3 grid((unsigned)((int64_t)T * n), (unsigned)((dpr + 256 * kPpgUnroll - 1) / (256 * kPpgUnroll)));
    hipLaunchKernelGGL(ppg_gather_kernel, grid, dim3(256), 0, as_stream(stream), aux_obs, cols, out, n, R, row_bytes, dpr);
    return check_launch("ppg_gather_kernel");
}

extern "C" MI355PPO_API int mi355ppo_ppg_old_logits_f32(const float* h, const float* w, const float* b, const int64_t* cols, float* aux_pi, int T,
                                                       int n, int64_t R, int A, int hidden, void* stream) {
    const char* fn = "mi355ppo_ppg_old_logits_f32";
    if (int rc = ppg_old_args(fn, h, w, b, cols, aux_pi, T, n, R, A, hidden)) return rc;
    const int M = T * n;
    hipLaunchKernelGGL(ppg_old_logits_kernel, dim3((M + kPpgRows - 1) / kPpgRows), dim3(256), 0, as_stream(stream), h, w, b, cols, aux_pi, M, n, R, A);
    return check_launch("ppg_old_logits_kernel");
}

extern "C" MI355PPO_API size_t mi355ppo_ppg_aux_workspace_bytes(int M, int A) {
    if (M <= 0 || M > kPpgMaxRows || A < kPpgMinA || A > kPpgMaxA) return 0;
    const int tiles = (M + kPpgRows - 1) / kPpgRows;
    return ppg_sums_bytes(tiles) + (size_t)tiles * kPpgPart * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_ppg_aux_fwd_bwd_f32(const float* h, const float* wa, const float* ba, const float* wc, const float* bc,
                                                        const float* wx, const float* bx, const float* aux_pi, const float* aux_returns,
                                                        const int64_t* cols, int T, int n, int64_t R, int A, int hidden, double beta_clone,
                                                        double inv_accum, float* scalars_out, float* dh, float* dwa, float* dba, float* dwc,
                                                        float* dbc, float* dwx, float* dbx, int accumulate, void* workspace,
                                                        size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_ppg_aux_fwd_bwd_f32";
    PpgAuxArgs a = ppg_aux_pack(h, wa, ba, wc, bc, wx, bx, aux_pi, aux_returns, cols, T, n, R, A, beta_clone, inv_accum, dh);
    const PpgGrads g{dwa, dba, dwc, dbc, dwx, dbx};
    if (int rc = ppg_aux_args(fn, a, g, scalars_out, T, hidden, accumulate)) return rc;
    const size_t need = mi355ppo_ppg_aux_workspace_bytes(a.M, A);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(workspace, 16), MI355PPO_EALIGN, "%s: workspace must be 16-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    const int tiles = (a.M + kPpgRows - 1) / kPpgRows;
    a.sums = static_cast<double*>(workspace);
    a.part = reinterpret_cast<float*>(static_cast<char*>(workspace) + ppg_sums_bytes(tiles));
    hipLaunchKernelGGL(ppg_aux_rows_kernel, dim3(tiles), dim3(256), 0, s, a);
    if (int rc = check_launch("ppg_aux_rows_kernel")) return rc;
    const int elems = (A + 2) * (kPpgH + 1);
    hipLaunchKernelGGL(ppg_aux_fold_kernel, dim3((elems + 255) / 256), dim3(256), 0, s, a.part, a.sums, tiles, a.M, A, g, accumulate, scalars_out);
    return check_launch("ppg_aux_fold_kernel");
}
