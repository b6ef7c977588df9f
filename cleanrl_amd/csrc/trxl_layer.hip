// The dense half of ppo_trxl.py's TransformerLayer (cleanrl/ppo_trxl/ppo_trxl.py: layer_norm_q, queries, keys.weight, values, fc_out, the skip,
// layer_norm_attn, fc_projection + ReLU, the skip) around the episodic-memory attention of trxl_attn.hip, on the matrix pipe, gfx950, wave 64.
//
// Mathematics.  queries / keys / values are per-head (d, d) matrices shared by the heads, d = D / H.  Expanded to block-diagonal (D, D)
// matrices the layer is three (D, D) GEMMs per direction:
//   pre    n1 = LN_q(x);  q~ = n1 A,  A = blockdiag(Wq^T Wk)                      (queries(...) @ keys.weight)
//   attn   u = mi355ppo_trxl_attn_fwd_f32(q~)
//   post   x1 = (u Wvo + b_o) + x,  Wvo[h d + k][n] = sum_i Wv[i][k] Wo[n][h d + i];  n2 = LN_attn(x1);  f = relu(n2 Wp^T + b_p);  y = f + x1
// and backwards:  df = dy [f > 0];  dn2 = df Wp;  dx1 = dy + LN_attn'(dn2);  du = dx1 Wvo^T;  (attention backward: du -> dq~);
// dn1 = dq~ A^T;  dx = LN_q'(dn1) + dx1.
//
// Arithmetic: the two-term f16 split of f16split.h (hi hi, hi lo, lo hi on v_mfma_f32_32x32x16_f16, f32 accumulation, exact power-of-two
// unscale).  One scale per packed matrix; one scale PER ROW for activation and gradient tiles, found by the wave that stages the row (finer
// than K8's per-tile scale -- DESIGN 3.25 -- and free here: a wave holds whole rows for the LayerNorms anyway).  LayerNorm statistics and
// their backward are exact f32 VALU with wave butterflies.  A and Wvo are formed at pack time with f64 accumulation and rounded to f32 once.
//
// Tiles.  A workgroup (4 waves) owns 32 rows at every D <= 512 and alternates two phases over one LDS tile:
//   row phase   wave w holds rows 8 w .. 8 w + 7, lane l columns l + 64 c (c < D / 64): LayerNorm forward / backward, the skips, the ReLU
//               mask, d gamma / d beta partial sums; ends by splitting each row into the hi / lo planes ([32][D] f16, pitch 2 D + 16 bytes).
//   GEMM phase  planes x packed matrix: wave w owns the 32-column tiles w, w + 4, ... (at most four accumulator tiles).  One k-step of all
//               D columns (D / 32 fragments of 2 KB: 64 lanes x 16 B of hi, then of lo) is one stage of a two-stage LDS ring: global ->
//               registers one step ahead -> LDS, one barrier per k-step (K8's ring).  The epilogue writes f32 results to global memory or
//               into the f32 tile ([32][D], pitch 4 D + 16 bytes) that ALIASES the planes: the next row phase reads all its rows into
//               registers, passes a barrier and only then overwrites them with planes.
// LDS at D = 512: 66,560 (planes) + 65,536 (ring) + 128 bytes.  Between GEMMs the ring is free: the d gamma / d beta partials of the four
// waves meet there and are added in wave order.
//
// Launches: pack (3: combined matrices + vectors, the three scale exponents, fragments in forward and transposed order); pre forward; post
// forward; post backward; pre backward; weight gradients (K8's scheme: 64 x 64 blocks of d W over slabs of 64-row slots, per-slot scales,
// LDS transpose reads), the fold in slab order (+ the LayerNorm partials in tile order), and the parameter-sized factor launch that maps
// the combined matrices' gradients to Wq, Wk, Wv, Wo (f64 accumulation).  No atomics: same inputs and slabs, same bits.
#include "common.h"
#include "f16split.h"
#include "trxl_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {
namespace {

typedef float t_f32x16 __attribute__((ext_vector_type(16)));
typedef short t_s16x4 __attribute__((ext_vector_type(4)));

constexpr int kTlRows = 32, kTlThreads = 256, kTlWaveRows = kTlRows / 4, kTlMaxC = kTrxlMaxD / 64;
constexpr int kTlFrag = 2048;                            // bytes of one (k-step, column tile) fragment pair: hi | lo
constexpr int kTlHeader = 256, kTlMaxSlabs = 8, kTlSlot = 64, kTlParams = 13;
// the parameters of one TransformerLayer in module order
enum { P_WV, P_WK, P_WQ, P_WO, P_BO, P_GQ, P_BQ, P_GKV, P_BKV, P_GA, P_BA, P_WP, P_BP };
// the pack's vectors, the matrices and their sections (forward order, transposed order)
enum { V_BO, V_BP, V_GQ, V_BQ, V_GA, V_BA, kTlVecs };
enum { M_A, M_VO, M_P };
enum { S_AF, S_AT, S_VF, S_VT, S_PF, S_PT, kTlSecs };
// the workspace's (B, D) planes and per-row statistics
enum { W_X1, W_F, W_N1, W_N2, W_DF, W_DX1, kTlPlanes };

struct TlPack {
    size_t vec, comb, sec[kTlSecs], total;               // byte offsets
};
MI355_HD TlPack tl_pack_geom(int D) {
    TlPack g;
    const size_t dd = (size_t)D * D;
    g.vec = kTlHeader;
    g.comb = g.vec + (size_t)kTlVecs * D * sizeof(float);
    size_t o = g.comb + 2 * dd * sizeof(float);
    for (int i = 0; i < kTlSecs; ++i) {
        g.sec[i] = o;
        o += dd * 4;                                     // (D / 16) k-steps x (D / 32) fragments x 2 KB
    }
    g.total = o;
    return g;
}

struct TlWs {
    size_t stats, lnpart, part, fold, part_floats, total;   // float offsets; planes start at 0, kTlPlanes x B x D
    int tiles;
};
MI355_HD TlWs tl_ws_geom(int B, int D) {
    TlWs g;
    g.tiles = (B + kTlRows - 1) / kTlRows;
    g.part_floats = 3 * ((size_t)D * D + D);             // per matrix: d W (D, D) | column sums of dz (D)
    g.stats = (size_t)kTlPlanes * B * D;                 // mean1 | rstd1 | mean2 | rstd2, B each (padded to 4 floats)
    g.lnpart = g.stats + 4 * (((size_t)B + 3) / 4 * 4);  // [tile][d gamma_attn | d beta_attn | d gamma_q | d beta_q][D]
    g.part = g.lnpart + (size_t)g.tiles * 4 * D;
    g.fold = g.part + (size_t)kTlMaxSlabs * g.part_floats;
    g.total = g.fold + g.part_floats;
    return g;
}
MI355_HD size_t tl_stat(const TlWs& g, int B, int q) { return g.stats + (size_t)q * (((size_t)B + 3) / 4 * 4); }

struct TlParams {
    const float* p[kTlParams];
};
struct TlGrads {
    float* g[kTlParams];
};

// ------------------------------------------------------------------------------------------------------------------------------- pack
// launch 1: A and Wvo as f32 (D, D) matrices (f64 accumulation, one rounding), and the six vectors
__global__ __launch_bounds__(256) void tl_combine_kernel(TlParams P, int D, int H, unsigned char* __restrict__ pack) {
    const TlPack g = tl_pack_geom(D);
    const int d = D / H;
    const size_t dd = (size_t)D * D, total = 2 * dd + (size_t)kTlVecs * D;
    float* const comb = reinterpret_cast<float*>(pack + g.comb);
    float* const vec = reinterpret_cast<float*>(pack + g.vec);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (i < 2 * dd) {
            const int m = i >= dd, K = (int)((i - m * dd) / D), N = (int)((i - m * dd) % D), h = K / d, k = K % d;
            double s = 0.0;
            if (m == 0) {
                if (N / d == h)
                    for (int q = 0; q < d; ++q) s += (double)P.p[P_WQ][q * d + k] * (double)P.p[P_WK][q * d + N % d];
            } else {
                for (int q = 0; q < d; ++q) s += (double)P.p[P_WV][q * d + k] * (double)P.p[P_WO][(size_t)N * D + h * d + q];
            }
            comb[i] = (float)s;
        } else {
            const int v = (int)((i - 2 * dd) / D), c = (int)((i - 2 * dd) % D);
            const int src = v == V_BO ? P_BO : v == V_BP ? P_BP : v == V_GQ ? P_GQ : v == V_BQ ? P_BQ : v == V_GA ? P_GA : P_BA;
            vec[i - 2 * dd] = P.p[src][c];
        }
    }
}

// launch 2: the scale exponent of A, Wvo, Wp (one block each)
__global__ __launch_bounds__(256) void tl_wmax_kernel(const float* __restrict__ wp, int D, unsigned char* __restrict__ pack) {
    __shared__ unsigned red[4];
    const TlPack g = tl_pack_geom(D);
    const size_t dd = (size_t)D * D;
    const float* const w = blockIdx.x == M_P ? wp : reinterpret_cast<const float*>(pack + g.comb) + blockIdx.x * dd;
    unsigned m = 0;
    for (size_t i = threadIdx.x; i < dd; i += 256) {
        const unsigned b = __float_as_uint(w[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    m = wave_umax(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        reinterpret_cast<int*>(pack)[blockIdx.x] = f16_scale_exp(a > b ? a : b);
    }
}

// launch 3: fragments.  blockIdx.y = section; a thread = one lane of one fragment.  Lane l of fragment (ks, nt) holds
// B[16 ks + 8 (l / 32) + j][32 nt + l % 32], j < 8.  B = A, Wvo, Wp^T in the forward sections, their transposes in the others.
__global__ __launch_bounds__(256) void tl_frag_kernel(const float* __restrict__ wp, int D, unsigned char* __restrict__ pack) {
    const TlPack g = tl_pack_geom(D);
    const int sec = blockIdx.y, m = sec >> 1, NT = D / 32;
    const bool swap = ((sec & 1) != 0) != (m == M_P);    // element (k, n) of B is S[n][k] instead of S[k][n]
    const float* const S = m == M_P ? wp : reinterpret_cast<const float*>(pack + g.comb) + (size_t)m * D * D;
    const float s = f16_pow2(reinterpret_cast<const int*>(pack)[m]);
    unsigned char* const dst = pack + g.sec[sec];
    const int units = (D / 16) * NT * 64;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        const int lane = u & 63, fr = u >> 6, nt = fr % NT, ks = fr / NT;
        const int n = 32 * nt + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
        unsigned short hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            f16_split1(swap ? S[(size_t)n * D + k] : S[(size_t)k * D + n], s, hi[j], lo[j]);
        }
        unsigned char* const p = dst + (size_t)fr * kTlFrag + lane * 16;
        *reinterpret_cast<uint4*>(p) = make_uint4(hi[0] | (unsigned)hi[1] << 16, hi[2] | (unsigned)hi[3] << 16, hi[4] | (unsigned)hi[5] << 16, hi[6] | (unsigned)hi[7] << 16);
        *reinterpret_cast<uint4*>(p + 1024) = make_uint4(lo[0] | (unsigned)lo[1] << 16, lo[2] | (unsigned)lo[3] << 16, lo[4] | (unsigned)lo[5] << 16, lo[6] | (unsigned)lo[7] << 16);
    }
}

// ------------------------------------------------------------------------------------------------------------------------ the row tile
struct TlLds {
    unsigned char planes[2 * kTlRows * (2 * kTrxlMaxD + 16)];      // hi plane | lo plane (pitch 2 D + 16), or the f32 tile (pitch 4 D + 16)
    unsigned char ring[2][(kTrxlMaxD / 32) * kTlFrag];
    int rexp[kTlRows];                                             // the rows' scale exponents
};

__device__ __forceinline__ const float* tl_vec(const unsigned char* pack, int v, int D) {
    return reinterpret_cast<const float*>(pack + kTlHeader) + (size_t)v * D;
}

// acc[j] = planes x B for the column tiles wave + 4 j, B from `sec` through the ring.  Ends behind a barrier: every wave has read its last
// fragments, so the caller may overwrite the planes and the ring.
__device__ __forceinline__ void tl_gemm(TlLds& L, const unsigned char* __restrict__ sec, int D, t_f32x16 (&acc)[4], int tid) {
    const int lane = tid & 63, wave = tid >> 6, NT = D / 32, ksteps = D / 16, per = NT / 2, pitch = 2 * D + 16;
    const size_t stage = (size_t)NT * kTlFrag;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
    s_u32x4 p[kTlMaxC] = {};                                       // a stage is NT * 128 16-byte units: NT / 2 per thread
#define TL_FETCH(s_)                                                                                              \
    _Pragma("unroll") for (int i = 0; i < kTlMaxC; ++i) if (i < per)                                              \
        p[i] = *reinterpret_cast<const s_u32x4*>(sec + (size_t)(s_) * stage + (size_t)(i * kTlThreads + tid) * 16);
#define TL_STASH(b_)                                                                                              \
    _Pragma("unroll") for (int i = 0; i < kTlMaxC; ++i) if (i < per)                                              \
        *reinterpret_cast<s_u32x4*>(L.ring[b_] + (i * kTlThreads + tid) * 16) = p[i];
    TL_FETCH(0)
    TL_STASH(0)
    __syncthreads();
    const unsigned char* const arow_hi = L.planes + (lane & 31) * pitch + 16 * (lane >> 5);
    const unsigned char* const arow_lo = arow_hi + kTlRows * pitch;
    for (int s = 0; s < ksteps; ++s) {
        if (s + 1 < ksteps) { TL_FETCH(s + 1) }
        const s_f16x8 a_hi = *reinterpret_cast<const s_f16x8*>(arow_hi + 32 * s), a_lo = *reinterpret_cast<const s_f16x8*>(arow_lo + 32 * s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = wave + 4 * j;
            if (t < NT) {
                const unsigned char* const fb = L.ring[s & 1] + t * kTlFrag + lane * 16;
                const s_f16x8 b_hi = *reinterpret_cast<const s_f16x8*>(fb), b_lo = *reinterpret_cast<const s_f16x8*>(fb + 1024);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc[j], 0, 0, 0);
            }
        }
        if (s + 1 < ksteps) { TL_STASH((s + 1) & 1) }
        __syncthreads();
    }
#undef TL_FETCH
#undef TL_STASH
}

// accumulator element e of column tile wave + 4 j: its row inside the tile and its column
#define TL_ROW(lane, e) (((e) & 3) + 8 * ((e) >> 2) + 4 * ((lane) >> 5))
#define TL_COL(t, lane) (32 * (t) + ((lane) & 31))
// for every live accumulator element: `body` sees j, e, r (tile row), c (column)
#define TL_FOR_ACC(D_, wave_, lane_, ...)                               \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                     \
        const int t_ = (wave_) + 4 * j;                                 \
        if (t_ < (D_) / 32) {                                           \
            const int c = TL_COL(t_, lane_);                            \
            _Pragma("unroll") for (int e = 0; e < 16; ++e) {            \
                const int r = TL_ROW(lane_, e);                         \
                __VA_ARGS__                                             \
            }                                                           \
        }                                                               \
    }
// for the lane's columns of a row: `body` sees q (register index) and c (column)
#define TL_FOR_COLS(C_, lane_, ...)                                     \
    _Pragma("unroll") for (int q = 0; q < kTlMaxC; ++q) if (q < (C_)) { \
        const int c = (lane_) + 64 * q;                                 \
        __VA_ARGS__                                                     \
    }

// the lane's values of tile row r -> the planes under the row's own scale (all 64 lanes)
__device__ __forceinline__ void tl_put_row(TlLds& L, int D, int r, const float (&v)[kTlMaxC], int lane) {
    const int C = D / 64, pitch = 2 * D + 16;
    unsigned m = 0;
    TL_FOR_COLS(C, lane, {
        (void)c;
        const unsigned b = __float_as_uint(v[q]) & 0x7fffffffu;
        m = b > m ? b : m;
    })
    const int ex = f16_scale_exp(wave_umax(m));
    const float s = f16_pow2(ex);
    TL_FOR_COLS(C, lane, {
        unsigned short h, l;
        f16_split1(v[q], s, h, l);
        *reinterpret_cast<unsigned short*>(L.planes + r * pitch + 2 * c) = h;
        *reinterpret_cast<unsigned short*>(L.planes + (kTlRows + r) * pitch + 2 * c) = l;
    })
    if (lane == 0) L.rexp[r] = ex;
}

// LayerNorm of the row in v (in place): biased variance, eps 1e-5
__device__ __forceinline__ void tl_ln_row(float (&v)[kTlMaxC], int D, const float* __restrict__ gamma, const float* __restrict__ beta, int lane,
                                          float& mean, float& rstd) {
    const int C = D / 64;
    float s = 0.0f;
    TL_FOR_COLS(C, lane, { (void)c; s = s + v[q]; })
    mean = wave_sum(s) / (float)D;
    float sq = 0.0f;
    TL_FOR_COLS(C, lane, {
        (void)c;
        v[q] = v[q] - mean;
        sq = sq + v[q] * v[q];
    })
    rstd = trxl_rstd(wave_sum(sq) / (float)D);
    TL_FOR_COLS(C, lane, { v[q] = (v[q] * rstd) * gamma[c] + beta[c]; })
}

// LayerNorm backward of one row: dn (grad of the output) in v -> grad of the input in v; dg / db collect d gamma / d beta of the lane's columns
__device__ __forceinline__ void tl_ln_row_bwd(float (&v)[kTlMaxC], int D, const float* __restrict__ xrow, float mean, float rstd,
                                              const float* __restrict__ gamma, int lane, float (&dg)[kTlMaxC], float (&db)[kTlMaxC]) {
    const int C = D / 64;
    float xh[kTlMaxC] = {};
    float s1 = 0.0f, s2 = 0.0f;
    TL_FOR_COLS(C, lane, {
        xh[q] = (xrow[c] - mean) * rstd;
        dg[q] = dg[q] + v[q] * xh[q];
        db[q] = db[q] + v[q];
        v[q] = v[q] * gamma[c];
        s1 = s1 + v[q];
        s2 = s2 + v[q] * xh[q];
    })
    s1 = wave_sum(s1) / (float)D;
    s2 = wave_sum(s2) / (float)D;
    TL_FOR_COLS(C, lane, { (void)c; v[q] = rstd * ((v[q] - s1) - xh[q] * s2); })
}

// the f32 tile -> the wave's eight rows in registers; behind the closing barrier the planes may be written
__device__ __forceinline__ void tl_take_rows(TlLds& L, int D, float (&rv)[kTlWaveRows][kTlMaxC], int tid) {
    const int lane = tid & 63, wave = tid >> 6, C = D / 64;
    const float* const tile = reinterpret_cast<const float*>(L.planes);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTlWaveRows; ++i) {
        TL_FOR_COLS(C, lane, { rv[i][q] = tile[(wave * kTlWaveRows + i) * (D + 4) + c]; })
    }
    __syncthreads();
}

// the four waves' d gamma / d beta sums of a tile, added in wave order -> lnpart[tile][which], [which + 1] (the ring is free between GEMMs)
__device__ __forceinline__ void tl_ln_partial(TlLds& L, int D, const float (&dg)[kTlMaxC], const float (&db)[kTlMaxC], float* __restrict__ out, int tid) {
    const int lane = tid & 63, wave = tid >> 6, C = D / 64;
    float* const red = reinterpret_cast<float*>(L.ring[0]);          // [4 waves][2][D]
    TL_FOR_COLS(C, lane, {
        red[(wave * 2) * D + c] = dg[q];
        red[(wave * 2 + 1) * D + c] = db[q];
    })
    __syncthreads();
    for (int i = tid; i < 2 * D; i += kTlThreads) out[i] = ((red[i] + red[2 * D + i]) + red[4 * D + i]) + red[6 * D + i];
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(kTlThreads) void tl_pre_fwd_kernel(const float* __restrict__ x, int B, int D, const unsigned char* __restrict__ pack,
                                                                float* __restrict__ qt, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) TlLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kTlRows, C = D / 64;
    const TlPack g = tl_pack_geom(D);
    const TlWs w = tl_ws_geom(B, D);
    const float *gq = tl_vec(pack, V_GQ, D), *bq = tl_vec(pack, V_BQ, D);
#pragma unroll 1
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        float v[kTlMaxC] = {};
        if (gr < B) {
            float mean, rstd;
            TL_FOR_COLS(C, lane, { v[q] = x[(size_t)gr * D + c]; })
            tl_ln_row(v, D, gq, bq, lane, mean, rstd);
            if (ws) {
                TL_FOR_COLS(C, lane, { ws[(size_t)W_N1 * B * D + (size_t)gr * D + c] = v[q]; })
                if (lane == 0) {
                    ws[tl_stat(w, B, 0) + gr] = mean;
                    ws[tl_stat(w, B, 1) + gr] = rstd;
                }
            }
        }
        tl_put_row(L, D, r, v, lane);
    }
    t_f32x16 acc[4];
    tl_gemm(L, pack + g.sec[S_AF], D, acc, tid);
    const int ea = reinterpret_cast<const int*>(pack)[M_A];
    TL_FOR_ACC(D, wave, lane, {
        if (row0 + r < B) qt[(size_t)(row0 + r) * D + c] = acc[j][e] * f16_unscale(L.rexp[r], ea);
    })
}

__global__ __launch_bounds__(kTlThreads) void tl_post_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u, int B, int D,
                                                                 const unsigned char* __restrict__ pack, float* __restrict__ y, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) TlLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kTlRows, C = D / 64;
    const TlPack g = tl_pack_geom(D);
    const TlWs w = tl_ws_geom(B, D);
    const int* const hdr = reinterpret_cast<const int*>(pack);
    const size_t BD = (size_t)B * D;
#pragma unroll 1
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        float v[kTlMaxC] = {};
        if (gr < B) {
            TL_FOR_COLS(C, lane, { v[q] = u[(size_t)gr * D + c]; })
        }
        tl_put_row(L, D, r, v, lane);
    }
    t_f32x16 acc[4], x1r[4];
    tl_gemm(L, pack + g.sec[S_VF], D, acc, tid);
    // x1 = (u Wvo + b_o) + x: kept in registers for the last skip, to the f32 tile for LN_attn, saved for the backward
    float* const tile = reinterpret_cast<float*>(L.planes);
    const float* const bo = tl_vec(pack, V_BO, D);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) x1r[j][e] = 0.0f;
    TL_FOR_ACC(D, wave, lane, {
        float val = 0.0f;
        if (row0 + r < B) {
            const size_t o = (size_t)(row0 + r) * D + c;
            val = (acc[j][e] * f16_unscale(L.rexp[r], hdr[M_VO]) + bo[c]) + x[o];
            if (ws) ws[W_X1 * BD + o] = val;
        }
        x1r[j][e] = val;
        tile[r * (D + 4) + c] = val;
    })
    float rv[kTlWaveRows][kTlMaxC] = {};
    tl_take_rows(L, D, rv, tid);
    const float *ga = tl_vec(pack, V_GA, D), *ba = tl_vec(pack, V_BA, D);
#pragma unroll
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        if (gr < B) {
            float mean, rstd;
            tl_ln_row(rv[i], D, ga, ba, lane, mean, rstd);
            if (ws) {
                TL_FOR_COLS(C, lane, { ws[W_N2 * BD + (size_t)gr * D + c] = rv[i][q]; })
                if (lane == 0) {
                    ws[tl_stat(w, B, 2) + gr] = mean;
                    ws[tl_stat(w, B, 3) + gr] = rstd;
                }
            }
        }
        tl_put_row(L, D, r, rv[i], lane);
    }
    tl_gemm(L, pack + g.sec[S_PF], D, acc, tid);
    const float* const bp = tl_vec(pack, V_BP, D);
    TL_FOR_ACC(D, wave, lane, {
        if (row0 + r < B) {
            const size_t o = (size_t)(row0 + r) * D + c;
            const float z = acc[j][e] * f16_unscale(L.rexp[r], hdr[M_P]) + bp[c];
            const float f = z > 0.0f ? z : 0.0f;
            y[o] = f + x1r[j][e];
            if (ws) ws[W_F * BD + o] = f;
        }
    })
}

// --------------------------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(kTlThreads) void tl_post_bwd_kernel(const float* __restrict__ dy, int B, int D, const unsigned char* __restrict__ pack,
                                                                 float* __restrict__ du, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) TlLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kTlRows, C = D / 64;
    const TlPack g = tl_pack_geom(D);
    const TlWs w = tl_ws_geom(B, D);
    const int* const hdr = reinterpret_cast<const int*>(pack);
    const size_t BD = (size_t)B * D;
    // df = dy [f > 0]: saved for the weight gradient, split for dn2 = df Wp
#pragma unroll 1
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        float v[kTlMaxC] = {};
        if (gr < B) {
            TL_FOR_COLS(C, lane, {
                const size_t o = (size_t)gr * D + c;
                v[q] = ws[W_F * BD + o] > 0.0f ? dy[o] : 0.0f;
                ws[W_DF * BD + o] = v[q];
            })
        }
        tl_put_row(L, D, r, v, lane);
    }
    t_f32x16 acc[4];
    tl_gemm(L, pack + g.sec[S_PT], D, acc, tid);
    float* const tile = reinterpret_cast<float*>(L.planes);
    TL_FOR_ACC(D, wave, lane, { tile[r * (D + 4) + c] = acc[j][e] * f16_unscale(L.rexp[r], hdr[M_P]); })
    float rv[kTlWaveRows][kTlMaxC] = {};
    tl_take_rows(L, D, rv, tid);
    // dx1 = dy + LN_attn'(dn2): saved (the skip into dx, and do of the weight gradient), split for du = dx1 Wvo^T
    float dg[kTlMaxC] = {}, db[kTlMaxC] = {};
    const float* const ga = tl_vec(pack, V_GA, D);
#pragma unroll
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        if (gr < B) {
            tl_ln_row_bwd(rv[i], D, ws + W_X1 * BD + (size_t)gr * D, ws[tl_stat(w, B, 2) + gr], ws[tl_stat(w, B, 3) + gr], ga, lane, dg, db);
            TL_FOR_COLS(C, lane, {
                const size_t o = (size_t)gr * D + c;
                rv[i][q] = dy[o] + rv[i][q];
                ws[W_DX1 * BD + o] = rv[i][q];
            })
        }
        tl_put_row(L, D, r, rv[i], lane);
    }
    tl_ln_partial(L, D, dg, db, ws + w.lnpart + (size_t)blockIdx.x * 4 * D, tid);
    tl_gemm(L, pack + g.sec[S_VT], D, acc, tid);
    TL_FOR_ACC(D, wave, lane, {
        if (row0 + r < B) du[(size_t)(row0 + r) * D + c] = acc[j][e] * f16_unscale(L.rexp[r], hdr[M_VO]);
    })
}

__global__ __launch_bounds__(kTlThreads) void tl_pre_bwd_kernel(const float* __restrict__ dqt, const float* __restrict__ x, int B, int D,
                                                                const unsigned char* __restrict__ pack, float* __restrict__ dx, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) TlLds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row0 = blockIdx.x * kTlRows, C = D / 64;
    const TlPack g = tl_pack_geom(D);
    const TlWs w = tl_ws_geom(B, D);
    const size_t BD = (size_t)B * D;
#pragma unroll 1
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int r = wave * kTlWaveRows + i, gr = row0 + r;
        float v[kTlMaxC] = {};
        if (gr < B) {
            TL_FOR_COLS(C, lane, { v[q] = dqt[(size_t)gr * D + c]; })
        }
        tl_put_row(L, D, r, v, lane);
    }
    t_f32x16 acc[4];
    tl_gemm(L, pack + g.sec[S_AT], D, acc, tid);
    float* const tile = reinterpret_cast<float*>(L.planes);
    const int ea = reinterpret_cast<const int*>(pack)[M_A];
    TL_FOR_ACC(D, wave, lane, { tile[r * (D + 4) + c] = acc[j][e] * f16_unscale(L.rexp[r], ea); })
    float rv[kTlWaveRows][kTlMaxC] = {};
    tl_take_rows(L, D, rv, tid);
    // dx = LN_q'(dn1) + dx1
    float dg[kTlMaxC] = {}, db[kTlMaxC] = {};
    const float* const gq = tl_vec(pack, V_GQ, D);
#pragma unroll
    for (int i = 0; i < kTlWaveRows; ++i) {
        const int gr = row0 + wave * kTlWaveRows + i;
        if (gr < B) {
            tl_ln_row_bwd(rv[i], D, x + (size_t)gr * D, ws[tl_stat(w, B, 0) + gr], ws[tl_stat(w, B, 1) + gr], gq, lane, dg, db);
            TL_FOR_COLS(C, lane, {
                const size_t o = (size_t)gr * D + c;
                dx[o] = rv[i][q] + ws[W_DX1 * BD + o];
            })
        }
    }
    tl_ln_partial(L, D, dg, db, ws + w.lnpart + ((size_t)blockIdx.x * 4 + 2) * D, tid);
}

// ------------------------------------------------------------------------------------------------------------------- weight gradients
// dW[n][k] = sum_r dz[r][n] a[r][k] for the three (dz, a) pairs (df, n2) -> d Wp; (dx1, u) -> d Wvo^T; (dq~, n1) -> d A^T.  K8's kernel
// (mlp256.hip): a workgroup = a 64 x 64 block of one d W over one slab of 64-row slots, a wave = one 32 x 32 tile; both operand blocks are
// split per slot into row records (128 B hi | 128 B lo | 64 B pad) and read as fragments by the LDS transpose read; a slot's products are
// accumulated apart and added to the running sum with their unscale.  The column sums of dz (exact f32) are the bias gradients.
struct TlWArgs {
    const float *dz[3], *a[3];
    int B, D, slots_per_slab, slots;
    float* part;
    size_t part_floats;
};
constexpr int kTlWP = 320, kTlWBuf = kTlSlot * kTlWP;

__global__ __launch_bounds__(kTlThreads) void tl_wgrad_kernel(TlWArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kTlWBuf];
    __shared__ unsigned wm[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tn = wave & 1, tk = wave >> 1;
    const int D = a.D, B = a.B, nb = D / 64, job = blockIdx.x / (nb * nb), blk = blockIdx.x % (nb * nb);
    const int n0 = 64 * (blk / nb), k0 = 64 * (blk % nb);
    const float *dz = a.dz[0], *av = a.a[0];
    if (job == 1) { dz = a.dz[1]; av = a.a[1]; }
    if (job == 2) { dz = a.dz[2]; av = a.a[2]; }
    const int slab = blockIdx.y, slot_lo = slab * a.slots_per_slab;
    const int nslots = min(a.slots_per_slab, a.slots - slot_lo);

    // a thread's units of a slot: rows tid / 16 + 16 i, columns 4 (tid % 16) .. + 3 of both blocks
    const int ur = tid >> 4, uc = 4 * (tid & 15);
    float pd[4][4], pa[4][4];
    auto load_slot = [&](int s) __attribute__((always_inline)) {
        const int rbase = (slot_lo + s) * kTlSlot;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rbase + ur + 16 * i;
            const bool live = r < B;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pd[i][c] = live ? dz[(size_t)r * D + n0 + uc + c] : 0.0f;
                pa[i][c] = live ? av[(size_t)r * D + k0 + uc + c] : 0.0f;
            }
        }
    };

    const int gq = lane >> 4, li = lane & 15, fr = li >> 2, c4 = li & 3, half = gq >> 1;
    const unsigned char* const fd = lds + (8 * half + fr) * kTlWP + (32 * tn + 16 * (gq & 1) + 4 * c4) * 2;
    const unsigned char* const fa = lds + kTlWBuf + (8 * half + fr) * kTlWP + (32 * tk + 16 * (gq & 1) + 4 * c4) * 2;
    typedef t_s16x4 __attribute__((address_space(3))) * lds_v4;
    auto tr2 = [&](const unsigned char* p0, const unsigned char* p1) __attribute__((always_inline)) -> s_f16x8 {
        const t_s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p0));
        const t_s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p1));
        const uint2 ux = __builtin_bit_cast(uint2, x), uy = __builtin_bit_cast(uint2, y);
        return __builtin_bit_cast(s_f16x8, (s_u32x4){ux.x, ux.y, uy.x, uy.y});
    };

    t_f32x16 total;
#pragma unroll
    for (int e = 0; e < 16; ++e) total[e] = 0.0f;
    float bsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    load_slot(0);
#pragma unroll 1
    for (int s = 0; s < nslots; ++s) {
        unsigned md = 0, ma = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned bd = __float_as_uint(pd[i][c]) & 0x7fffffffu, ba = __float_as_uint(pa[i][c]) & 0x7fffffffu;
                md = bd > md ? bd : md;
                ma = ba > ma ? ba : ma;
            }
        md = wave_umax(md);
        ma = wave_umax(ma);
        if (lane == 0) { wm[wave][0] = md; wm[wave][1] = ma; }
        __syncthreads();                                   // the maxima are out; the previous slot's fragments have been read
        unsigned xd = 0, xa = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            xd = wm[q][0] > xd ? wm[q][0] : xd;
            xa = wm[q][1] > xa ? wm[q][1] : xa;
        }
        const int ed = f16_scale_exp(xd), ea = f16_scale_exp(xa);
        const float sd = f16_pow2(ed), sa = f16_pow2(ea);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned short dh[4], dl[4], ah[4], al[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f16_split1(pd[i][c], sd, dh[c], dl[c]);
                f16_split1(pa[i][c], sa, ah[c], al[c]);
                bsum[c] += pd[i][c];
            }
            unsigned char* const rd = lds + (ur + 16 * i) * kTlWP + 2 * uc;
            unsigned char* const ra = rd + kTlWBuf;
            *reinterpret_cast<uint2*>(rd) = make_uint2(dh[0] | (unsigned)dh[1] << 16, dh[2] | (unsigned)dh[3] << 16);
            *reinterpret_cast<uint2*>(rd + 128) = make_uint2(dl[0] | (unsigned)dl[1] << 16, dl[2] | (unsigned)dl[3] << 16);
            *reinterpret_cast<uint2*>(ra) = make_uint2(ah[0] | (unsigned)ah[1] << 16, ah[2] | (unsigned)ah[3] << 16);
            *reinterpret_cast<uint2*>(ra + 128) = make_uint2(al[0] | (unsigned)al[1] << 16, al[2] | (unsigned)al[3] << 16);
        }
        __syncthreads();
        if (s + 1 < nslots) load_slot(s + 1);
        t_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const unsigned char* const p = fd + 16 * h * kTlWP;
            const unsigned char* const q = fa + 16 * h * kTlWP;
            const s_f16x8 d_hi = tr2(p, p + 4 * kTlWP), d_lo = tr2(p + 128, p + 4 * kTlWP + 128);
            const s_f16x8 a_hi = tr2(q, q + 4 * kTlWP), a_lo = tr2(q + 128, q + 4 * kTlWP + 128);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_hi, a_hi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_hi, a_lo, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_lo, a_hi, acc, 0, 0, 0);
        }
        const float un = f16_unscale(ed, ea);
#pragma unroll
        for (int e = 0; e < 16; ++e) total[e] += acc[e] * un;
    }

    // this slab's partial of the block: accumulator e = dW[n0 + 32 tn + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][k0 + 32 tk + lane % 32]
    float* const pw = a.part + (size_t)slab * a.part_floats + (size_t)job * ((size_t)D * D + D);
    const int k = k0 + 32 * tk + (lane & 31);
#pragma unroll
    for (int e = 0; e < 16; ++e) pw[(size_t)(n0 + 32 * tn + TL_ROW(lane, e)) * D + k] = total[e];
    if (k0 == 0) {                                         // the 16 row groups' column sums of dz, added in a fixed order
        __syncthreads();
        float* const red = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int c = 0; c < 4; ++c) red[ur * 64 + uc + c] = bsum[c];
        __syncthreads();
        if (tid < 64) {
            float sum = 0.0f;
            for (int q = 0; q < 16; ++q) sum += red[q * 64 + tid];
            pw[(size_t)D * D + n0 + tid] = sum;
        }
    }
}

// the slabs' partials in slab order -> `fold` (the combined matrices' gradients, for the factor launch); d Wp, d b_p, d b_o and the LayerNorm
// partials in tile order are ADDED into the parameters' gradients
__global__ __launch_bounds__(256) void tl_fold_kernel(const float* __restrict__ ws, TlWs w, int slabs, int D, float* __restrict__ fold, TlGrads G) {
    const size_t seg = (size_t)D * D + D, total = w.part_floats + 4 * (size_t)D;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (i < w.part_floats) {
            float sum = ws[w.part + i];
            for (int s = 1; s < slabs; ++s) sum += ws[w.part + (size_t)s * w.part_floats + i];
            fold[i] = sum;
            const int m = (int)(i / seg);
            const size_t o = i % seg;
            if (m == 0) {
                if (o < (size_t)D * D) G.g[P_WP][o] += sum;
                else G.g[P_BP][o - (size_t)D * D] += sum;
            } else if (m == 1 && o >= (size_t)D * D) {
                G.g[P_BO][o - (size_t)D * D] += sum;
            }
        } else {
            const int q = (int)((i - w.part_floats) / D), c = (int)((i - w.part_floats) % D);
            float sum = 0.0f;
            for (int t = 0; t < w.tiles; ++t) sum += ws[w.lnpart + ((size_t)t * 4 + q) * D + c];
            G.g[q == 0 ? P_GA : q == 1 ? P_BA : q == 2 ? P_GQ : P_BQ][c] += sum;
        }
    }
}

// the factor launch: fold = [GP | . | GVO (n, k) = d Wvo^T | . | GA (n, k) = d A^T | .] -> d Wq, d Wk, d Wv (d, d) and d Wo (D, D), ADDED
//   dA_blk[k][j] = sum_h GA[h d + j][h d + k];  dWq[i][k] = sum_j dA_blk[k][j] Wk[i][j];  dWk[i][j] = sum_k Wq[i][k] dA_blk[k][j]
//   dWo[n][h d + i] = sum_k GVO[n][h d + k] Wv[i][k];  dWv[i][k] = sum_h sum_n GVO[n][h d + k] Wo[n][h d + i]
__global__ __launch_bounds__(256) void tl_factor_kernel(const float* __restrict__ fold, TlParams P, TlGrads G, int D, int H) {
    const int d = D / H, lane = threadIdx.x & 63;
    const size_t seg = (size_t)D * D + D, dd = (size_t)d * d, total = 3 * dd + (size_t)D * D;
    const float *GVO = fold + seg, *GA = fold + 2 * seg;
    // a wave = one element: the lanes stride over the sum's terms (f64), one butterfly adds them in a fixed order
    for (size_t i = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < total; i += (size_t)gridDim.x * 4) {
        double s = 0.0;
        float* dst;
        if (i < 2 * dd) {
            const bool wq = i < dd;
            const int row = (int)((i % dd) / d), col = (int)((i % dd) % d);       // (i, k) of dWq or (i, j) of dWk
            const float* const W = wq ? P.p[P_WK] : P.p[P_WQ];
            for (int t = lane; t < d * H; t += 64) {
                const int m = t / H, h = t % H, k = wq ? col : m, j = wq ? m : col;
                s += (double)GA[(size_t)(h * d + j) * D + h * d + k] * (double)W[row * d + m];
            }
            dst = G.g[wq ? P_WQ : P_WK] + i % dd;
        } else if (i < 3 * dd) {
            const int row = (int)((i - 2 * dd) / d), k = (int)((i - 2 * dd) % d);
            for (int t = lane; t < H * D; t += 64) {
                const int h = t / D, n = t % D;
                s += (double)GVO[(size_t)n * D + h * d + k] * (double)P.p[P_WO][(size_t)n * D + h * d + row];
            }
            dst = G.g[P_WV] + (i - 2 * dd);
        } else {
            const size_t o = i - 3 * dd;
            const int n = (int)(o / D), h = (int)(o % D) / d, row = (int)(o % D) % d;
            for (int k = lane; k < d; k += 64) s += (double)GVO[(size_t)n * D + h * d + k] * (double)P.p[P_WV][row * d + k];
            dst = G.g[P_WO] + o;
        }
        s = wave_sum(s);
        if (lane == 0) *dst += (float)s;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------ entry
int tl_check_dims(const char* fn, int B, int D, int H) {
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%d must be positive", fn, B);
    MI355_REQUIRE(trxl_shape_ok(D, H, 1), MI355PPO_EINVAL, "%s: D=%d H=%d (need D %% 64 == 0, D <= 512, H dividing 64)", fn, D, H);
    return MI355PPO_OK;
}

int tl_check_ws(const char* fn, const void* ws, size_t bytes, int B, int D, bool required) {
    if (!ws && !required) return MI355PPO_OK;
    const size_t need = tl_ws_geom(B, D).total * sizeof(float);
    MI355_REQUIRE(ws && bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn, ws ? bytes : (size_t)0, need);
    MI355_REQUIRE(aligned(ws, 16), MI355PPO_EALIGN, "%s: the workspace must be 16-byte aligned", fn);
    return MI355PPO_OK;
}

int tl_fill_params(const char* fn, const void* const* params, TlParams& P) {
    MI355_REQUIRE(params, MI355PPO_EINVAL, "%s: null parameter pointer block", fn);
    for (int i = 0; i < kTlParams; ++i) {
        MI355_REQUIRE(params[i] || i == P_GKV || i == P_BKV, MI355PPO_EINVAL, "%s: null parameter pointer %d", fn, i);
        MI355_REQUIRE(aligned(params[i], 4), MI355PPO_EALIGN, "%s: misaligned parameter pointer %d", fn, i);
        P.p[i] = static_cast<const float*>(params[i]);
    }
    return MI355PPO_OK;
}

unsigned tl_tiles(int B) { return (unsigned)((B + kTlRows - 1) / kTlRows); }

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API size_t mi355ppo_trxl_layer_pack_bytes(int D, int H) { return trxl_shape_ok(D, H, 1) ? tl_pack_geom(D).total : 0; }

extern "C" MI355PPO_API size_t mi355ppo_trxl_layer_workspace_bytes(int B, int D, int H) {
    return (B > 0 && trxl_shape_ok(D, H, 1)) ? tl_ws_geom(B, D).total * sizeof(float) : 0;
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_pack_f32(const void* const* params, int D, int H, void* pack, size_t pack_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_pack_f32";
    int rc = tl_check_dims(fn, 1, D, H);
    if (rc) return rc;
    TlParams P = {};
    if ((rc = tl_fill_params(fn, params, P))) return rc;
    MI355_REQUIRE(pack, MI355PPO_EINVAL, "%s: null pack", fn);
    MI355_REQUIRE(aligned(pack, 16), MI355PPO_EALIGN, "%s: the pack must be 16-byte aligned", fn);
    const TlPack g = tl_pack_geom(D);
    MI355_REQUIRE(pack_bytes >= g.total, MI355PPO_EWORKSPACE, "%s: pack %zu bytes < required %zu", fn, pack_bytes, g.total);
    hipStream_t s = as_stream(stream);
    unsigned char* const pk = static_cast<unsigned char*>(pack);
    hipLaunchKernelGGL(tl_combine_kernel, dim3((unsigned)((2 * (size_t)D * D + kTlVecs * D + 255) / 256)), dim3(256), 0, s, P, D, H, pk);
    if ((rc = check_launch("tl_combine_kernel"))) return rc;
    hipLaunchKernelGGL(tl_wmax_kernel, dim3(3), dim3(256), 0, s, P.p[P_WP], D, pk);
    if ((rc = check_launch("tl_wmax_kernel"))) return rc;
    hipLaunchKernelGGL(tl_frag_kernel, dim3((unsigned)((D / 16) * (D / 32) * 64 / 256), kTlSecs), dim3(256), 0, s, P.p[P_WP], D, pk);
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_pre_fwd_f32(const float* x, int B, int D, int H, const void* pack, float* qt, void* workspace,
                                                            size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_pre_fwd_f32";
    int rc = tl_check_dims(fn, B, D, H);
    if (rc) return rc;
    MI355_REQUIRE(x && pack && qt, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(x, 4) && aligned(qt, 4) && aligned(pack, 16), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    if ((rc = tl_check_ws(fn, workspace, workspace_bytes, B, D, false))) return rc;
    hipLaunchKernelGGL(tl_pre_fwd_kernel, dim3(tl_tiles(B)), dim3(kTlThreads), 0, as_stream(stream), x, B, D, static_cast<const unsigned char*>(pack), qt,
                       static_cast<float*>(workspace));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_post_fwd_f32(const float* x, const float* u, int B, int D, int H, const void* pack, float* y,
                                                             void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_post_fwd_f32";
    int rc = tl_check_dims(fn, B, D, H);
    if (rc) return rc;
    MI355_REQUIRE(x && u && pack && y, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(x, 4) && aligned(u, 4) && aligned(y, 4) && aligned(pack, 16), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    if ((rc = tl_check_ws(fn, workspace, workspace_bytes, B, D, false))) return rc;
    hipLaunchKernelGGL(tl_post_fwd_kernel, dim3(tl_tiles(B)), dim3(kTlThreads), 0, as_stream(stream), x, u, B, D, static_cast<const unsigned char*>(pack), y,
                       static_cast<float*>(workspace));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_post_bwd_f32(const float* dy, int B, int D, int H, const void* pack, float* du, void* workspace,
                                                             size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_post_bwd_f32";
    int rc = tl_check_dims(fn, B, D, H);
    if (rc) return rc;
    MI355_REQUIRE(dy && pack && du, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(dy, 4) && aligned(du, 4) && aligned(pack, 16), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    if ((rc = tl_check_ws(fn, workspace, workspace_bytes, B, D, true))) return rc;
    hipLaunchKernelGGL(tl_post_bwd_kernel, dim3(tl_tiles(B)), dim3(kTlThreads), 0, as_stream(stream), dy, B, D, static_cast<const unsigned char*>(pack), du,
                       static_cast<float*>(workspace));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_pre_bwd_f32(const float* dqt, const float* x, int B, int D, int H, const void* pack, float* dx,
                                                            void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_pre_bwd_f32";
    int rc = tl_check_dims(fn, B, D, H);
    if (rc) return rc;
    MI355_REQUIRE(dqt && x && pack && dx, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(dqt, 4) && aligned(x, 4) && aligned(dx, 4) && aligned(pack, 16), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    if ((rc = tl_check_ws(fn, workspace, workspace_bytes, B, D, true))) return rc;
    hipLaunchKernelGGL(tl_pre_bwd_kernel, dim3(tl_tiles(B)), dim3(kTlThreads), 0, as_stream(stream), dqt, x, B, D, static_cast<const unsigned char*>(pack), dx,
                       static_cast<float*>(workspace));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_trxl_layer_wgrad_f32(const float* u, const float* dqt, const void* const* params, void* const* grads, int B, int D,
                                                          int H, int slabs, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_trxl_layer_wgrad_f32";
    int rc = tl_check_dims(fn, B, D, H);
    if (rc) return rc;
    MI355_REQUIRE(u && dqt && grads, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(u, 4) && aligned(dqt, 4), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    MI355_REQUIRE(slabs >= 0 && slabs <= kTlMaxSlabs, MI355PPO_EINVAL, "%s: slabs=%d outside 0..%d (0: the default)", fn, slabs, kTlMaxSlabs);
    TlParams P = {};
    if ((rc = tl_fill_params(fn, params, P))) return rc;
    TlGrads G = {};
    for (int i = 0; i < kTlParams; ++i) {
        MI355_REQUIRE(grads[i] || i == P_GKV || i == P_BKV, MI355PPO_EINVAL, "%s: null gradient pointer %d", fn, i);
        MI355_REQUIRE(aligned(grads[i], 4), MI355PPO_EALIGN, "%s: misaligned gradient pointer %d", fn, i);
        G.g[i] = static_cast<float*>(grads[i]);
    }
    if ((rc = tl_check_ws(fn, workspace, workspace_bytes, B, D, true))) return rc;
    float* const ws = static_cast<float*>(workspace);
    const TlWs w = tl_ws_geom(B, D);
    const size_t BD = (size_t)B * D;
    TlWArgs a = {};
    a.dz[0] = ws + W_DF * BD;  a.a[0] = ws + W_N2 * BD;
    a.dz[1] = ws + W_DX1 * BD; a.a[1] = u;
    a.dz[2] = dqt;             a.a[2] = ws + W_N1 * BD;
    a.B = B; a.D = D; a.part = ws + w.part; a.part_floats = w.part_floats;
    a.slots = (B + kTlSlot - 1) / kTlSlot;
    const int want = slabs ? slabs : kTlMaxSlabs;
    a.slots_per_slab = (a.slots + want - 1) / want;
    const int used = (a.slots + a.slots_per_slab - 1) / a.slots_per_slab;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(tl_wgrad_kernel, dim3((unsigned)(3 * (D / 64) * (D / 64)), (unsigned)used), dim3(kTlThreads), 0, s, a);
    if ((rc = check_launch("tl_wgrad_kernel"))) return rc;
    hipLaunchKernelGGL(tl_fold_kernel, dim3((unsigned)((w.part_floats + 4 * (size_t)D + 1023) / 1024)), dim3(256), 0, s, ws, w, used, D, ws + w.fold, G);
    if ((rc = check_launch("tl_fold_kernel"))) return rc;
    const int d = D / H;
    hipLaunchKernelGGL(tl_factor_kernel, dim3((unsigned)((3 * (size_t)d * d + (size_t)D * D + 3) / 4)), dim3(256), 0, s, ws + w.fold, P, G, D, H);
    return check_launch(fn);
}
