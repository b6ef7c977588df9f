// K8 -- two independent O -> 256 -> 256 -> n_out tanh MLPs (actor mean and critic of ppo_continuous_action_isaacgym.py) on the matrix pipe,
// gfx950, wave 64.  The 64-64 family K7 (mlp.hip) is a one-wave VALU latency chain; at 256 x 256 and minibatches of 32,768 rows the work is
// GEMMs whose intermediates (h1, h2, dz2, dz1: 32 MB each per network) would each make an HBM round trip if the layers ran one by one.  Here a
// workgroup owns a ROW TILE of 64 rows and walks the whole layer chain with the tile's activations resident in LDS as split f16 terms.
//
// Arithmetic: the two-term f16 split of f16split.h (hi hi, hi lo, lo hi on v_mfma_f32_32x32x16_f16, f32 accumulation, exact power-of-two
// unscale in the epilogue).  Operand scales:
//   * weights: one power of two per matrix from its maximum (pack launch 1), stored in the pack's header;
//   * tanh activations: fixed 2^14 -- they lie in (-1, 1), so no record is needed and nothing can overflow;
//   * observation tile, gradient tiles: one scale PER ROW TILE, from the tile's own maximum, found by the workgroup while it stages the tile.
//     Deterministic, no amax record, no fill launch, and rows far below the tensor's maximum keep their bits (a departure from the per-tensor
//     records of the conv kernels: DESIGN 3.25).
//
// Launches:
//   pack (2)   m256_wmax_kernel: the six matrices' scale exponents; m256_pack_kernel: hi / lo terms in MFMA B-fragment order -- W1, W2, W3 as the
//              forward reads them, W3 and W2 again as the data gradient reads them -- and the biases.  Fragment (k-step ks, column tile nt) is
//              2 KB: 64 lanes x 16 B of hi, then of lo; the tiles of one k-step are contiguous (one ring stage).
//   forward    grid (row tiles, 2 networks), 4 waves.  Rows gathered through `inds`, split once into LDS ([64][256] hi and lo planes, pitch
//              528 B: the 16-byte fragment reads of 16 consecutive rows cover the 64 banks once).  Wave (mt, nh) owns rows 32 mt .. + 31 and columns
//              128 nh .. + 127: four accumulator tiles.  The weights of one k-step (16 KB) stream from the pack through a two-stage LDS ring:
//              global -> registers one step ahead -> LDS, one barrier per k-step.  tanh(acc + b) goes back into the activation planes in place.
//              Layer 3 is one 32-column tile (waves nh = 0).  With `save` the f32 h1 / h2 are also written for the backward pass.
//   dgrad      same tile, same ring: dz3 tile (K padded to 32) -> dh2 = dz3 W3 -> dz2 = dh2 (1 - h2^2) (scaled by its own tile maximum, stays in
//              LDS) -> dh1 = dz2 W2 -> dz1.  dz2 / dz1 leave as f32 for the weight gradients; no gradient w.r.t. the observations.
//   wgrad      dW_l = dz_l^T a_{l-1}: reduction over rows.  Workgroup = a 64 x 64 block of one dW over one SLAB of rows, wave = one 32 x 32 tile.
//              Slots of 64 rows: both operand blocks are split once into row records (128 B hi | 128 B lo | 64 B pad) and read as fragments
//              by the LDS transpose read (ds_read_b64_tr_b16, kernel H's addressing).  Each slot has its own scales, so a slot's products are
//              accumulated apart and added to the running sum with their unscale.  Bias gradients: column sums of the same dz blocks (exact f32).
//   fold       partials added in slab order, no atomics; the sums are ADDED into the gradient tensors (K7's contract).
#include "common.h"
#include "f16split.h"

#pragma clang fp contract(off)

namespace mi355ppo {

typedef float m_f32x16 __attribute__((ext_vector_type(16)));
typedef short m_s16x4 __attribute__((ext_vector_type(4)));

constexpr int kM256H = 256, kM256MaxObs = 256, kM256MaxOut = 32, kM256Rows = 64, kM256Threads = 256;
constexpr int kM256Frag = 2048;                          // bytes of one (k-step, column tile) fragment pair: hi | lo
constexpr int kM256Stage = 8 * kM256Frag;                // one k-step of 256 columns
constexpr int kM256Pitch = 2 * kM256H + 16;              // bytes of one activation row in a plane
constexpr int kM256Plane = kM256Rows * kM256Pitch;
constexpr int kM256Header = 256;
constexpr int kM256BiasFloats = 2 * kM256H + 32;         // b1 | b2 | b3 (padded) of one network
constexpr int kM256MaxSlabs = 8;
constexpr int kM256ActExp = 14;                          // tanh activations: |h| < 1 -> scaled below 2^14

// ---- pack geometry (host and device)
struct M256Pack {
    int ks1;                                             // k-steps of layer 1: ceil(O / 16)
    size_t f1, f2, f3, t3, t2, net_bytes, bias, total;   // section offsets inside a network's block; block size; bias offset; total bytes
};
MI355_HD M256Pack m256_pack_geom(int O) {
    M256Pack g;
    g.ks1 = (O + 15) / 16;
    g.f1 = 0;
    g.f2 = g.f1 + (size_t)g.ks1 * kM256Stage;
    g.f3 = g.f2 + (size_t)16 * kM256Stage;
    g.t3 = g.f3 + (size_t)16 * kM256Frag;
    g.t2 = g.t3 + (size_t)2 * kM256Stage;
    g.net_bytes = g.t2 + (size_t)16 * kM256Stage;
    g.bias = kM256Header + 2 * g.net_bytes;
    g.total = g.bias + (size_t)2 * kM256BiasFloats * sizeof(float);
    return g;
}
// gradient floats of one network (w1 | b1 | w2 | b2 | w3 | b3) and the workspace layout, in floats
MI355_HD size_t m256_grad_floats(int O, int nout) { return (size_t)kM256H * O + kM256H + (size_t)kM256H * kM256H + kM256H + (size_t)nout * kM256H + nout; }
MI355_HD size_t m256_plane_floats(int M) { return (size_t)2 * M * kM256H; }               // one saved tensor of both networks
MI355_HD size_t m256_part_floats(int O, int nout) { return m256_grad_floats(O, nout) + m256_grad_floats(O, 1); }

struct M256Nets {
    const float* w[2][3];
    const float* b[2][3];
};

// ---- pack launch 1: scale exponent of every matrix (block = (network, layer))
__global__ __launch_bounds__(256) void m256_wmax_kernel(M256Nets nets, int O, int nout, int* __restrict__ header) {
    __shared__ unsigned red[4];
    const int net = blockIdx.x / 3, l = blockIdx.x % 3;
    const int no = net == 0 ? nout : 1;
    const size_t n = l == 0 ? (size_t)kM256H * O : (l == 1 ? (size_t)kM256H * kM256H : (size_t)no * kM256H);
    const float* const w = nets.w[net][l];
    unsigned m = 0;
    for (size_t i = threadIdx.x; i < n; i += 256) {
        const unsigned b = __float_as_uint(w[i]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    m = wave_umax(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
        header[net * 3 + l] = f16_scale_exp(a > b ? a : b);
    }
}

// ---- pack launch 2: fragments and biases.  blockIdx.y = network * 5 + section (F1, F2, F3, T3, T2); a thread = one lane of one fragment.
// Forward section of W (N, K) (torch's (out, in)): B[k][n] = W[n][k]; transposed section: B[k][n] = W[k][n].  Lane l of fragment (ks, nt)
// holds B[16 ks + 8 (l / 32) + j][32 nt + l % 32], j < 8; elements outside the matrix are zero.
__global__ __launch_bounds__(256) void m256_pack_kernel(M256Nets nets, int O, int nout, unsigned char* __restrict__ pack) {
    const M256Pack g = m256_pack_geom(O);
    const int net = blockIdx.y / 5, sec = blockIdx.y % 5;
    const int no = net == 0 ? nout : 1;
    const int* const header = reinterpret_cast<const int*>(pack);
    const int layer = sec == 0 ? 0 : (sec == 1 || sec == 4 ? 1 : 2);
    const bool transposed = sec >= 3;
    const int rows = layer == 2 ? no : kM256H, cols = layer == 0 ? O : kM256H;          // W is (rows, cols)
    const int nt_n = sec == 2 ? 1 : 8, ks_n = sec == 0 ? g.ks1 : (sec == 3 ? 2 : 16);
    const size_t off = sec == 0 ? g.f1 : (sec == 1 ? g.f2 : (sec == 2 ? g.f3 : (sec == 3 ? g.t3 : g.t2)));
    const float* const w = nets.w[net][layer];
    const float s = f16_pow2(header[net * 3 + layer]);
    unsigned char* const dst = pack + kM256Header + (size_t)net * g.net_bytes + off;
    const int units = ks_n * nt_n * 64;
    for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        const int lane = u & 63, fr = u >> 6, nt = fr % nt_n, ks = fr / nt_n;
        const int n = 32 * nt + (lane & 31), k0 = 16 * ks + 8 * (lane >> 5);
        unsigned short hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            float v = 0.0f;
            if (!transposed) {
                if (n < rows && k < cols) v = w[(size_t)n * cols + k];
            } else {
                if (k < rows && n < cols) v = w[(size_t)k * cols + n];
            }
            f16_split1(v, s, hi[j], lo[j]);
        }
        unsigned char* const p = dst + (size_t)fr * kM256Frag + lane * 16;
        *reinterpret_cast<uint4*>(p) = make_uint4(hi[0] | (unsigned)hi[1] << 16, hi[2] | (unsigned)hi[3] << 16, hi[4] | (unsigned)hi[5] << 16, hi[6] | (unsigned)hi[7] << 16);
        *reinterpret_cast<uint4*>(p + 1024) = make_uint4(lo[0] | (unsigned)lo[1] << 16, lo[2] | (unsigned)lo[3] << 16, lo[4] | (unsigned)lo[5] << 16, lo[6] | (unsigned)lo[7] << 16);
    }
    if (sec == 0 && blockIdx.x == 0) {
        float* const bd = reinterpret_cast<float*>(pack + g.bias) + net * kM256BiasFloats;
        for (int i = threadIdx.x; i < kM256BiasFloats; i += 256) {
            float v = 0.0f;
            if (i < kM256H) v = nets.b[net][0][i];
            else if (i < 2 * kM256H) v = nets.b[net][1][i - kM256H];
            else if (i - 2 * kM256H < no) v = nets.b[net][2][i - 2 * kM256H];
            bd[i] = v;
        }
    }
}

// ---- the tile's LDS: two activation planes, the weight ring, four words for the tile maximum
struct M256Lds {
    unsigned char hi[kM256Plane], lo[kM256Plane];
    unsigned char ring[2][kM256Stage];
    unsigned wmax[4];
};

// one layer of the chain: acc[j] (+)= act[64][16 ksteps] x B, B from `sec` (ksteps stages of NT fragments) through the ring.  NT = 8: wave
// (mt, nh) takes column tiles 4 nh + j; NT = 1: the waves nh = 0 take the one tile, the others only move the ring.  Ends behind a barrier:
// every wave has read its last fragments, so the caller may overwrite the planes and the ring.
template <int NT>
__device__ __forceinline__ void m256_gemm(M256Lds& L, const unsigned char* __restrict__ sec, int ksteps, m_f32x16 (&acc)[4], int tid) {
    constexpr int UNITS = NT * 128, PER = (UNITS + kM256Threads - 1) / kM256Threads;          // 16-byte units of a stage; per thread
    const int lane = tid & 63, wave = tid >> 6, mt = wave & 1, nh = wave >> 1;
    const bool mine = NT == 8 || nh == 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
    // the stage's 16-byte units of this thread, one step ahead of the ring, in named registers (an indexed array ends up in LDS)
    uint4 p0 = {}, p1 = {}, p2 = {}, p3 = {};
    static_assert(PER == 4 || PER == 1, "a stage is four units per thread (256 columns) or one for half the threads (32 columns)");
#define M256_SRC(s_, i_) (*reinterpret_cast<const uint4*>(sec + (size_t)(s_) * (NT * kM256Frag) + (size_t)((i_) * kM256Threads + tid) * 16))
#define M256_DST(buf_, i_) (*reinterpret_cast<uint4*>(L.ring[buf_] + ((i_) * kM256Threads + tid) * 16))
#define M256_FETCH(s_)                                                                              \
    if constexpr (PER == 4) {                                                                       \
        p0 = M256_SRC(s_, 0); p1 = M256_SRC(s_, 1); p2 = M256_SRC(s_, 2); p3 = M256_SRC(s_, 3);     \
    } else if (tid < UNITS) {                                                                       \
        p0 = M256_SRC(s_, 0);                                                                       \
    }
#define M256_STASH(buf_)                                                                            \
    if constexpr (PER == 4) {                                                                       \
        M256_DST(buf_, 0) = p0; M256_DST(buf_, 1) = p1; M256_DST(buf_, 2) = p2; M256_DST(buf_, 3) = p3; \
    } else if (tid < UNITS) {                                                                       \
        M256_DST(buf_, 0) = p0;                                                                     \
    }
    M256_FETCH(0)
    M256_STASH(0)
    __syncthreads();
    const unsigned char* const arow_hi = L.hi + (32 * mt + (lane & 31)) * kM256Pitch + 16 * (lane >> 5);
    const unsigned char* const arow_lo = L.lo + (32 * mt + (lane & 31)) * kM256Pitch + 16 * (lane >> 5);
    for (int s = 0; s < ksteps; ++s) {
        if (s + 1 < ksteps) { M256_FETCH(s + 1) }
        if (mine) {
            const s_f16x8 a_hi = *reinterpret_cast<const s_f16x8*>(arow_hi + 32 * s), a_lo = *reinterpret_cast<const s_f16x8*>(arow_lo + 32 * s);
#pragma unroll
            for (int j = 0; j < (NT == 8 ? 4 : 1); ++j) {
                const unsigned char* const fb = L.ring[s & 1] + (NT == 8 ? 4 * nh + j : 0) * kM256Frag + lane * 16;
                const s_f16x8 b_hi = *reinterpret_cast<const s_f16x8*>(fb), b_lo = *reinterpret_cast<const s_f16x8*>(fb + 1024);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc[j], 0, 0, 0);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc[j], 0, 0, 0);
            }
        }
        if (s + 1 < ksteps) { M256_STASH((s + 1) & 1) }
        __syncthreads();
    }
#undef M256_FETCH
#undef M256_STASH
#undef M256_SRC
#undef M256_DST
}

// the tile maximum of per-lane maxima (bit patterns of non-negative floats); every thread of the workgroup calls it
__device__ __forceinline__ unsigned m256_tile_max(M256Lds& L, unsigned m, int tid) {
    m = wave_umax(m);
    __syncthreads();                                       // the previous round's readers are done with wmax
    if ((tid & 63) == 0) L.wmax[tid >> 6] = m;
    __syncthreads();
    const unsigned a = L.wmax[0] > L.wmax[1] ? L.wmax[0] : L.wmax[1], b = L.wmax[2] > L.wmax[3] ? L.wmax[2] : L.wmax[3];
    return a > b ? a : b;
}

// stage a [64][kp] tile (kp a multiple of 16, <= 256) into the planes under its own scale: element (r, c) = src(r, c), zero outside the tensor.
// Two passes over the source (the second hits L2): maximum, then split.  Returns the scale exponent.
template <typename F>
__device__ __forceinline__ int m256_stage_tile(M256Lds& L, int kp, int tid, F src) {
    unsigned m = 0;
    for (int idx = tid; idx < kM256Rows * kp; idx += kM256Threads) {
        const unsigned b = __float_as_uint(src(idx / kp, idx % kp)) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    const int e = f16_scale_exp(m256_tile_max(L, m, tid));
    const float s = f16_pow2(e);
    for (int idx = tid; idx < kM256Rows * kp; idx += kM256Threads) {
        const int r = idx / kp, c = idx % kp;
        unsigned short h, l;
        f16_split1(src(r, c), s, h, l);
        *reinterpret_cast<unsigned short*>(L.hi + r * kM256Pitch + 2 * c) = h;
        *reinterpret_cast<unsigned short*>(L.lo + r * kM256Pitch + 2 * c) = l;
    }
    return e;
}

// accumulator element e of column tile j of wave (mt, nh): tile row and column inside the 64 x 256 tile
#define M256_ROW(mt, lane, e) (32 * (mt) + ((e) & 3) + 8 * ((e) >> 2) + 4 * ((lane) >> 5))
#define M256_COL(nh, lane, j) (128 * (nh) + 32 * (j) + ((lane) & 31))

struct M256FwdArgs {
    const float* obs;
    const int64_t* inds;
    int M, O, nout;
    const unsigned char* pack;
    float *mean, *value, *save;                            // save: h1 [2][M][256] then h2 [2][M][256], or null
};

__global__ __launch_bounds__(kM256Threads) void m256_fwd_kernel(M256FwdArgs a) {
    __shared__ __attribute__((aligned(16))) M256Lds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt = wave & 1, nh = wave >> 1;
    const int net = blockIdx.y, row0 = blockIdx.x * kM256Rows, M = a.M, O = a.O;
    const int no = net == 0 ? a.nout : 1;
    const M256Pack g = m256_pack_geom(O);
    const int* const header = reinterpret_cast<const int*>(a.pack);
    const unsigned char* const nb = a.pack + kM256Header + (size_t)net * g.net_bytes;
    const float* const bias = reinterpret_cast<const float*>(a.pack + g.bias) + net * kM256BiasFloats;

    // ---- the observation tile: gathered, split once under the tile's scale
    const int e_x = m256_stage_tile(L, 16 * g.ks1, tid, [&](int r, int c) -> float {
        if (row0 + r >= M || c >= O) return 0.0f;
        const size_t src = a.inds ? (size_t)a.inds[row0 + r] : (size_t)(row0 + r);
        return a.obs[src * O + c];
    });

    m_f32x16 acc[4];
    // ---- layers 1 and 2: tanh(acc + b) back into the planes (scale 2^14), f32 copy to `save`
#pragma unroll 1
    for (int layer = 0; layer < 2; ++layer) {
        m256_gemm<8>(L, nb + (layer == 0 ? g.f1 : g.f2), layer == 0 ? g.ks1 : 16, acc, tid);
        const float un = f16_unscale(layer == 0 ? e_x : kM256ActExp, header[net * 3 + layer]);
        const float sh = f16_pow2(kM256ActExp);
        float* const sv = a.save ? a.save + (size_t)layer * m256_plane_floats(M) + (size_t)net * M * kM256H : nullptr;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = M256_COL(nh, lane, j);
            const float b = bias[layer * kM256H + c];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = M256_ROW(mt, lane, e);
                const float h = tanhf(acc[j][e] * un + b);
                if (sv && row0 + r < M) sv[(size_t)(row0 + r) * kM256H + c] = h;
                unsigned short hh, hl;
                f16_split1(h, sh, hh, hl);
                *reinterpret_cast<unsigned short*>(L.hi + r * kM256Pitch + 2 * c) = hh;
                *reinterpret_cast<unsigned short*>(L.lo + r * kM256Pitch + 2 * c) = hl;
            }
        }
    }
    // ---- layer 3: one 32-column tile
    m256_gemm<1>(L, nb + g.f3, 16, acc, tid);
    if (nh == 0) {
        const float un = f16_unscale(kM256ActExp, header[net * 3 + 2]);
        const int c = lane & 31;
        if (c < no) {
            const float b = bias[2 * kM256H + c];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = row0 + M256_ROW(mt, lane, e);
                if (r < M) {
                    const float v = acc[0][e] * un + b;
                    if (net == 0) a.mean[(size_t)r * no + c] = v;
                    else a.value[r] = v;
                }
            }
        }
    }
}

struct M256DgradArgs {
    const float *dmean, *dvalue;
    int M, O, nout;
    const unsigned char* pack;
    const float *h1, *h2;                                  // [2][M][256]
    float *dz2, *dz1;                                      // [2][M][256]
};

__global__ __launch_bounds__(kM256Threads) void m256_dgrad_kernel(M256DgradArgs a) {
    __shared__ __attribute__((aligned(16))) M256Lds L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt = wave & 1, nh = wave >> 1;
    const int net = blockIdx.y, row0 = blockIdx.x * kM256Rows, M = a.M;
    const int no = net == 0 ? a.nout : 1;
    const M256Pack g = m256_pack_geom(a.O);
    const int* const header = reinterpret_cast<const int*>(a.pack);
    const unsigned char* const nb = a.pack + kM256Header + (size_t)net * g.net_bytes;
    const float* const dz3 = net == 0 ? a.dmean : a.dvalue;

    const int e3 = m256_stage_tile(L, 32, tid, [&](int r, int c) -> float {
        return (row0 + r < M && c < no) ? dz3[(size_t)(row0 + r) * no + c] : 0.0f;
    });

    m_f32x16 acc[4];
    // ---- dh2 = dz3 W3;  dz2 = dh2 (1 - h2^2): to HBM as f32 and back into the planes under its own tile scale
    m256_gemm<8>(L, nb + g.t3, 2, acc, tid);
    {
        const float un = f16_unscale(e3, header[net * 3 + 2]);
        const float* const h = a.h2 + (size_t)net * M * kM256H;
        float* const out = a.dz2 + (size_t)net * M * kM256H;
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = M256_COL(nh, lane, j);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = row0 + M256_ROW(mt, lane, e);
                float d = 0.0f;
                if (r < M) {
                    const float y = h[(size_t)r * kM256H + c];
                    d = (acc[j][e] * un) * (1.0f - y * y);
                    out[(size_t)r * kM256H + c] = d;
                }
                acc[j][e] = d;
                const unsigned b = __float_as_uint(d) & 0x7fffffffu;
                m = b > m ? b : m;
            }
        }
        const int e2 = f16_scale_exp(m256_tile_max(L, m, tid));
        const float s = f16_pow2(e2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = M256_COL(nh, lane, j);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = M256_ROW(mt, lane, e);
                unsigned short hh, hl;
                f16_split1(acc[j][e], s, hh, hl);
                *reinterpret_cast<unsigned short*>(L.hi + r * kM256Pitch + 2 * c) = hh;
                *reinterpret_cast<unsigned short*>(L.lo + r * kM256Pitch + 2 * c) = hl;
            }
        }
        // ---- dh1 = dz2 W2;  dz1 = dh1 (1 - h1^2)
        m256_gemm<8>(L, nb + g.t2, 16, acc, tid);
        const float un1 = f16_unscale(e2, header[net * 3 + 1]);
        const float* const y1 = a.h1 + (size_t)net * M * kM256H;
        float* const out1 = a.dz1 + (size_t)net * M * kM256H;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = M256_COL(nh, lane, j);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = row0 + M256_ROW(mt, lane, e);
                if (r < M) {
                    const float y = y1[(size_t)r * kM256H + c];
                    out1[(size_t)r * kM256H + c] = (acc[j][e] * un1) * (1.0f - y * y);
                }
            }
        }
    }
}

// ---- weight gradients
struct M256WJob {
    const float *dz, *a;                                   // (M, N) with pitch ldd; (rows, K) with pitch lda
    int N, K, ldd, lda, gather, a_fixed, nbk, first;       // gather: a's rows through inds; a_fixed: tanh operand (scale 2^14); blocks along K; first block index
    size_t off_w, off_b;                                   // in a slab's partial
};
struct M256WArgs {
    M256WJob job[6];
    const int64_t* inds;
    int M, tiles_per_slab, tiles;
    float* part;
    size_t part_floats;
};
constexpr int kM256WP = 320;                               // row record: 128 B hi | 128 B lo | 64 B pad -- 64 (mod 256), as kernel H's
constexpr int kM256WBuf = kM256Rows * kM256WP;

__global__ __launch_bounds__(kM256Threads) void m256_wgrad_kernel(M256WArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * kM256WBuf];
    __shared__ unsigned wm[4][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tn = wave & 1, tk = wave >> 1;
    int ji = 0;
#pragma unroll
    for (int q = 1; q < 6; ++q)
        if ((int)blockIdx.x >= a.job[q].first) ji = q;
    const M256WJob J = a.job[ji];
    const int blk = blockIdx.x - J.first, bn = blk / J.nbk, bk = blk % J.nbk;
    const int n0 = 64 * bn, k0 = 64 * bk, M = a.M;
    const int slab = blockIdx.y, tile_lo = slab * a.tiles_per_slab;
    const int nslots = min(a.tiles_per_slab, a.tiles - tile_lo);

    // a thread's units of a slot: rows tid / 16 + 16 i, columns 4 (tid % 16) .. + 3 of both blocks
    const int ur = tid >> 4, uc = 4 * (tid & 15);
    float pd[4][4], pa[4][4];
    auto load_slot = [&](int s) __attribute__((always_inline)) {
        const int rbase = (tile_lo + s) * kM256Rows;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rbase + ur + 16 * i;
            const bool live = r < M;
            const size_t ar = live ? (J.gather && a.inds ? (size_t)a.inds[r] : (size_t)r) : 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int n = n0 + uc + c, k = k0 + uc + c;
                pd[i][c] = (live && n < J.N) ? J.dz[(size_t)r * J.ldd + n] : 0.0f;
                pa[i][c] = (live && k < J.K) ? J.a[ar * J.lda + k] : 0.0f;
            }
        }
    };

    // fragment addresses (kernel H): lane (g, r, c4) passes row 8 half + r of the k-step, columns 16 (g & 1) + 4 c4 .. + 3 of its tile
    const int g = lane >> 4, li = lane & 15, fr = li >> 2, c4 = li & 3, half = g >> 1;
    const unsigned char* const fd = lds + (8 * half + fr) * kM256WP + (32 * tn + 16 * (g & 1) + 4 * c4) * 2;
    const unsigned char* const fa = lds + kM256WBuf + (8 * half + fr) * kM256WP + (32 * tk + 16 * (g & 1) + 4 * c4) * 2;
    typedef m_s16x4 __attribute__((address_space(3))) * lds_v4;
    auto tr2 = [&](const unsigned char* p0, const unsigned char* p1) __attribute__((always_inline)) -> s_f16x8 {
        const m_s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p0));
        const m_s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4)(p1));
        const uint2 ux = __builtin_bit_cast(uint2, x), uy = __builtin_bit_cast(uint2, y);
        return __builtin_bit_cast(s_f16x8, (s_u32x4){ux.x, ux.y, uy.x, uy.y});
    };

    m_f32x16 total;
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
        for (int w = 0; w < 4; ++w) {
            xd = wm[w][0] > xd ? wm[w][0] : xd;
            xa = wm[w][1] > xa ? wm[w][1] : xa;
        }
        const int ed = f16_scale_exp(xd), ea = J.a_fixed ? kM256ActExp : f16_scale_exp(xa);
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
            unsigned char* const rd = lds + (ur + 16 * i) * kM256WP + 2 * uc;
            unsigned char* const ra = rd + kM256WBuf;
            *reinterpret_cast<uint2*>(rd) = make_uint2(dh[0] | (unsigned)dh[1] << 16, dh[2] | (unsigned)dh[3] << 16);
            *reinterpret_cast<uint2*>(rd + 128) = make_uint2(dl[0] | (unsigned)dl[1] << 16, dl[2] | (unsigned)dl[3] << 16);
            *reinterpret_cast<uint2*>(ra) = make_uint2(ah[0] | (unsigned)ah[1] << 16, ah[2] | (unsigned)ah[3] << 16);
            *reinterpret_cast<uint2*>(ra + 128) = make_uint2(al[0] | (unsigned)al[1] << 16, al[2] | (unsigned)al[3] << 16);
        }
        __syncthreads();
        if (s + 1 < nslots) load_slot(s + 1);
        m_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const unsigned char* const p = fd + 16 * h * kM256WP;
            const unsigned char* const q = fa + 16 * h * kM256WP;
            const s_f16x8 d_hi = tr2(p, p + 4 * kM256WP), d_lo = tr2(p + 128, p + 4 * kM256WP + 128);
            const s_f16x8 a_hi = tr2(q, q + 4 * kM256WP), a_lo = tr2(q + 128, q + 4 * kM256WP + 128);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_hi, a_hi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_hi, a_lo, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(d_lo, a_hi, acc, 0, 0, 0);
        }
        const float un = f16_unscale(ed, ea);
#pragma unroll
        for (int e = 0; e < 16; ++e) total[e] += acc[e] * un;
    }

    // ---- this slab's partial of the block: accumulator e = dW[n0 + 32 tn + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][k0 + 32 tk + lane % 32]
    float* const pw = a.part + (size_t)slab * a.part_floats;
    const int k = k0 + 32 * tk + (lane & 31);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int n = n0 + 32 * tn + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        if (n < J.N && k < J.K) pw[J.off_w + (size_t)n * J.K + k] = total[e];
    }
    // ---- bias gradient: the 16 row groups' column sums, added in a fixed order (the k-block 0 workgroups)
    if (bk == 0) {
        __syncthreads();                                   // the last slot's fragments have been read: the buffer is free
        float* const red = reinterpret_cast<float*>(lds);
#pragma unroll
        for (int c = 0; c < 4; ++c) red[ur * 64 + uc + c] = bsum[c];
        __syncthreads();
        if (tid < 64 && n0 + tid < J.N) {
            float sum = 0.0f;
            for (int q = 0; q < 16; ++q) sum += red[q * 64 + tid];
            pw[J.off_b + n0 + tid] = sum;
        }
    }
}

// ---- fold: the slabs' partials in slab order, added into the twelve gradient tensors
struct M256FoldArgs {
    float* dst[12];
    size_t end[12];                                        // running ends of the segments inside a partial
    const float* part;
    size_t part_floats;
    int slabs;
};
__global__ __launch_bounds__(256) void m256_fold_kernel(M256FoldArgs f) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < f.part_floats; i += (size_t)gridDim.x * 256) {
        float sum = f.part[i];
        for (int s = 1; s < f.slabs; ++s) sum += f.part[(size_t)s * f.part_floats + i];
        int seg = 0;
#pragma unroll
        for (int q = 0; q < 11; ++q)
            if (i >= f.end[q]) seg = q + 1;
        float* const d = f.dst[seg] + (i - (seg ? f.end[seg - 1] : 0));
        *d += sum;
    }
}

static int m256_check_dims(const char* fn, int M, int O, int nout) {
    MI355_REQUIRE(M > 0, MI355PPO_EINVAL, "%s: M=%d must be positive", fn, M);
    MI355_REQUIRE(O >= 1 && O <= kM256MaxObs, MI355PPO_EINVAL, "%s: observation width %d outside 1..%d", fn, O, kM256MaxObs);
    MI355_REQUIRE(nout >= 1 && nout <= kM256MaxOut, MI355PPO_EINVAL, "%s: %d actor outputs outside 1..%d", fn, nout, kM256MaxOut);
    return MI355PPO_OK;
}

static int m256_fill_nets(const char* fn, const void* const* actor, const void* const* critic, M256Nets& n) {
    MI355_REQUIRE(actor && critic, MI355PPO_EINVAL, "%s: null network pointer block", fn);
    const void* const* p[2] = {actor, critic};
    for (int t = 0; t < 2; ++t)
        for (int l = 0; l < 3; ++l) {
            MI355_REQUIRE(p[t][2 * l] && p[t][2 * l + 1], MI355PPO_EINVAL, "%s: null parameter pointer", fn);
            MI355_REQUIRE(aligned(p[t][2 * l], 4) && aligned(p[t][2 * l + 1], 4), MI355PPO_EALIGN, "%s: misaligned parameter pointer", fn);
            n.w[t][l] = static_cast<const float*>(p[t][2 * l]);
            n.b[t][l] = static_cast<const float*>(p[t][2 * l + 1]);
        }
    return MI355PPO_OK;
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API size_t mi355ppo_mlp256_pack_bytes(int O, int n_out) {
    if (O < 1 || O > kM256MaxObs || n_out < 1 || n_out > kM256MaxOut) return 0;
    return m256_pack_geom(O).total;
}

extern "C" MI355PPO_API size_t mi355ppo_mlp256_workspace_bytes(int M, int O, int n_out) {
    if (M <= 0 || O < 1 || O > kM256MaxObs || n_out < 1 || n_out > kM256MaxOut) return 0;
    return (4 * m256_plane_floats(M) + (size_t)kM256MaxSlabs * m256_part_floats(O, n_out)) * sizeof(float);
}

extern "C" MI355PPO_API int mi355ppo_mlp256_pack_f32(const void* const* actor, const void* const* critic, int O, int n_out, void* pack,
                                                    size_t pack_bytes, void* stream) {
    const char* fn = "mi355ppo_mlp256_pack_f32";
    int rc = m256_check_dims(fn, 1, O, n_out);
    if (rc) return rc;
    M256Nets n = {};
    if ((rc = m256_fill_nets(fn, actor, critic, n))) return rc;
    MI355_REQUIRE(pack, MI355PPO_EINVAL, "%s: null pack", fn);
    MI355_REQUIRE(aligned(pack, 16), MI355PPO_EALIGN, "%s: the pack must be 16-byte aligned", fn);
    MI355_REQUIRE(pack_bytes >= m256_pack_geom(O).total, MI355PPO_EWORKSPACE, "%s: pack %zu bytes < required %zu", fn, pack_bytes, m256_pack_geom(O).total);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(m256_wmax_kernel, dim3(6), dim3(256), 0, s, n, O, n_out, static_cast<int*>(pack));
    if ((rc = check_launch("m256_wmax_kernel"))) return rc;
    hipLaunchKernelGGL(m256_pack_kernel, dim3(16, 10), dim3(256), 0, s, n, O, n_out, static_cast<unsigned char*>(pack));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_mlp256_fwd_f32(const float* obs, const int64_t* inds, int M, int O, int n_out, const void* pack, float* mean,
                                                   float* value, void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_mlp256_fwd_f32";
    int rc = m256_check_dims(fn, M, O, n_out);
    if (rc) return rc;
    MI355_REQUIRE(obs && pack && mean && value, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(obs, 4) && aligned(inds, 8) && aligned(pack, 16) && aligned(mean, 4) && aligned(value, 4) && aligned(workspace, 16),
                  MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    if (workspace) {
        const size_t need = mi355ppo_mlp256_workspace_bytes(M, O, n_out);
        MI355_REQUIRE(workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn, workspace_bytes, need);
    }
    M256FwdArgs a = {obs, inds, M, O, n_out, static_cast<const unsigned char*>(pack), mean, value, static_cast<float*>(workspace)};
    hipLaunchKernelGGL(m256_fwd_kernel, dim3((unsigned)((M + kM256Rows - 1) / kM256Rows), 2), dim3(kM256Threads), 0, as_stream(stream), a);
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_mlp256_dgrad_f32(const float* dmean, const float* dvalue, int M, int O, int n_out, const void* pack,
                                                     void* workspace, size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_mlp256_dgrad_f32";
    int rc = m256_check_dims(fn, M, O, n_out);
    if (rc) return rc;
    MI355_REQUIRE(dmean && dvalue && pack, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(dmean, 4) && aligned(dvalue, 4) && aligned(pack, 16) && aligned(workspace, 16), MI355PPO_EALIGN, "%s: misaligned pointer", fn);
    const size_t need = mi355ppo_mlp256_workspace_bytes(M, O, n_out);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    float* const ws = static_cast<float*>(workspace);
    const size_t pl = m256_plane_floats(M);
    M256DgradArgs a = {dmean, dvalue, M, O, n_out, static_cast<const unsigned char*>(pack), ws, ws + pl, ws + 2 * pl, ws + 3 * pl};
    hipLaunchKernelGGL(m256_dgrad_kernel, dim3((unsigned)((M + kM256Rows - 1) / kM256Rows), 2), dim3(kM256Threads), 0, as_stream(stream), a);
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_mlp256_wgrad_f32(const float* obs, const int64_t* inds, const float* dmean, const float* dvalue, int M, int O,
                                                     int n_out, void* const* actor_grads, void* const* critic_grads, int slabs, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    const char* fn = "mi355ppo_mlp256_wgrad_f32";
    int rc = m256_check_dims(fn, M, O, n_out);
    if (rc) return rc;
    MI355_REQUIRE(obs && dmean && dvalue && actor_grads && critic_grads, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(slabs >= 0 && slabs <= kM256MaxSlabs, MI355PPO_EINVAL, "%s: slabs=%d outside 0..%d (0: the default)", fn, slabs, kM256MaxSlabs);
    MI355_REQUIRE(aligned(obs, 4) && aligned(inds, 8) && aligned(dmean, 4) && aligned(dvalue, 4) && aligned(workspace, 16), MI355PPO_EALIGN,
                  "%s: misaligned pointer", fn);
    const size_t need = mi355ppo_mlp256_workspace_bytes(M, O, n_out);
    MI355_REQUIRE(workspace && workspace_bytes >= need, MI355PPO_EWORKSPACE, "%s: workspace %zu bytes < required %zu", fn,
                  workspace ? workspace_bytes : (size_t)0, need);
    M256FoldArgs f = {};
    void* const* gp[2] = {actor_grads, critic_grads};
    for (int t = 0; t < 2; ++t)
        for (int q = 0; q < 6; ++q) {
            MI355_REQUIRE(gp[t][q], MI355PPO_EINVAL, "%s: null gradient pointer", fn);
            MI355_REQUIRE(aligned(gp[t][q], 4), MI355PPO_EALIGN, "%s: misaligned gradient pointer", fn);
            f.dst[6 * t + q] = static_cast<float*>(gp[t][q]);
        }
    float* const ws = static_cast<float*>(workspace);
    const size_t pl = m256_plane_floats(M), mh = (size_t)M * kM256H;
    const float *h1 = ws, *h2 = ws + pl, *dz2 = ws + 2 * pl, *dz1 = ws + 3 * pl;
    M256WArgs a = {};
    a.inds = inds; a.M = M; a.part = ws + 4 * pl; a.part_floats = m256_part_floats(O, n_out);
    a.tiles = (M + kM256Rows - 1) / kM256Rows;
    const int want = slabs ? slabs : kM256MaxSlabs;
    a.tiles_per_slab = (a.tiles + want - 1) / want;
    const int used = (a.tiles + a.tiles_per_slab - 1) / a.tiles_per_slab;
    size_t off = 0;
    int first = 0;
    for (int t = 0; t < 2; ++t) {
        const int no = t == 0 ? n_out : 1;
        const int Ns[3] = {kM256H, kM256H, no}, Ks[3] = {O, kM256H, kM256H};
        const float* dzs[3] = {dz1 + t * mh, dz2 + t * mh, t == 0 ? dmean : dvalue};
        const float* as[3] = {obs, h1 + t * mh, h2 + t * mh};
        for (int l = 0; l < 3; ++l) {
            M256WJob& J = a.job[3 * t + l];
            J.dz = dzs[l]; J.a = as[l]; J.N = Ns[l]; J.K = Ks[l]; J.ldd = l == 2 ? no : kM256H; J.lda = Ks[l];
            J.gather = l == 0; J.a_fixed = l != 0; J.nbk = (Ks[l] + 63) / 64; J.first = first;
            first += ((Ns[l] + 63) / 64) * J.nbk;
            J.off_w = off; off += (size_t)Ns[l] * Ks[l]; f.end[6 * t + 2 * l] = off;
            J.off_b = off; off += Ns[l]; f.end[6 * t + 2 * l + 1] = off;
        }
    }
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(m256_wgrad_kernel, dim3((unsigned)first, (unsigned)used), dim3(kM256Threads), 0, s, a);
    if ((rc = check_launch("m256_wgrad_kernel"))) return rc;
    f.part = a.part; f.part_floats = a.part_floats; f.slabs = used;
    hipLaunchKernelGGL(m256_fold_kernel, dim3((unsigned)((a.part_floats + 1023) / 1024)), dim3(256), 0, s, f);
    return check_launch(fn);
}
