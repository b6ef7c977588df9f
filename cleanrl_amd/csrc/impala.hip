// The IMPALA-CNN trunk of ppo_procgen.py / ppg_procgen.py (cleanrl/ppo_procgen.py:86-124, cleanrl/ppg_procgen.py:123-165) on
// channels-last f32 activations: forward, and backward to every conv weight and bias.  Math, tie rule, orders and layouts:
// impala_rows.h.  Design:
//   * kernel IC (imp_conv_kernel): one 3x3 convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32).  A workgroup
//     stages its band of input rows (with a zero halo, ReLU applied when the layer's input is ReLU'd) and the layer's packed
//     weights in LDS; each of its 4 waves owns 4 accumulator tiles of 16 pixels x 16 channels.  The same kernel runs the data
//     gradient (flipped, transposed weights) with the ReLU-mask / residual-gradient epilogue;
//   * kernel IW (imp_wgrad_kernel): weight + bias gradient; a workgroup walks a fixed run of bands and writes one partial,
//     kernel IF (imp_fold_kernel) adds the partials in order.  No atomics: deterministic;
//   * max pool forward (value + argmax byte) and backward are separate element-wise launches.
// One launch per layer and pass: 19 forward, 47 backward.
//   * the `pooled` entry points (64 family) take the pools into the conv launches: kernel ICP (imp_convpool_kernel) is a
//     sequence's conv + bias + pool with the pre-pool plane in LDS; in the backward imp_unpool fills kernel IW's s_dy and the
//     data-gradient instance of kernel IC's s_in from the pooled gradient and the argmax bytes.  No pre-pool plane in HBM, the
//     same bits; 16 launches forward, 44 backward.
// The geometry is a function of (C_in, C_out, H) alone, so the same kernels serve two frame families (impala_rows.h): 64x64x3
// f32 frames (ppo_procgen / ppg_procgen) and 84x84x4 u8 Atari stacks (qdagger_dqn_atari_impalacnn.py:164-184), whose planes
// 84 / 42 / 21 / 11 tile into ragged bands with dead slots.  The 84 family's layer 0 stages the ring's bytes directly (one
// 4-byte pixel = four channels byte / 255.0f); no f32 copy of the frames exists.
#include "common.h"
#include "impala_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct ImpParams {
    const float* p[kImpParams];
};

// ---------------------------------------------------------------------------------------------------------- weight packing
template <int F>
__global__ __launch_bounds__(256) void imp_pack_kernel(ImpParams prm, float* __restrict__ wp) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= kImpPackFloats) return;
    int piece = 0;
    while (piece < 2 * kImpLayers - 2) {
        const int l = piece < kImpLayers ? piece : piece - kImpLayers + 1;
        const bool dg = piece >= kImpLayers;
        if (e < imp_pack_offset(l, dg) + imp_pack_floats(l, dg)) break;
        ++piece;
    }
    const bool dg = piece >= kImpLayers;
    const int l = dg ? piece - kImpLayers + 1 : piece;
    const int cin = imp_layer_cin(F, l), cout = imp_layer_cout(l);
    const int nt_count = (dg ? cin : cout) / 16;
    const int i = e - imp_pack_offset(l, dg);
    const int ks = i / (nt_count * 64), nt = (i / 64) % nt_count, lane = i % 64;
    const int k = 4 * ks + lane / 16, n = 16 * nt + lane % 16;
    wp[e] = dg ? imp_wt_dgrad(prm.p[2 * l], cin, cout, k, n) : imp_wt_fwd(prm.p[2 * l], cin, k, n);
}

// Stage the input rows around output rows y0 .. y0 + RI - 3 into LDS: NI images x RI rows (y0 - 1 .. y0 + RI - 2) x (H + 2) columns
// x CP channels, zero outside the image.  RI = R + 2 for a band of kernel IC / IW; kernel ICP stages the rows of its conv band.
// TIN = uint8_t (the 84 family's frames, CI = 4): the pixel's four bytes in one load, each imp_u8'd.
template <int CI, int CO, int H, bool RELU_IN, int RI = imp_geom(CI, CO, H).R + 2, int NI = imp_geom(CI, CO, H).NI, typename TIN>
__device__ __forceinline__ void imp_stage(float* s_in, const TIN* __restrict__ in, int64_t img0, int y0, int B) {
    constexpr bool U8 = sizeof(TIN) == 1;
    static_assert(!U8 || (CI == 4 && !RELU_IN), "u8 frames: four channels, layer 0");
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    constexpr int Q = G.CP / 4;
    for (int e = threadIdx.x; e < NI * RI * G.COLS * Q; e += kImpThreads) {
        const int q = e % Q, cell = e / Q, r = cell / G.COLS, c = cell % G.COLS;
        const int li = r / RI, y = y0 + r % RI - 1, x = c - 1;
        const int64_t img = img0 + li;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (img < B && y >= 0 && y < H && x >= 0 && x < H) {
            const TIN* src = in + ((img * H + y) * H + x) * CI + 4 * q;
            if constexpr (U8) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(src);
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = imp_u8((uint8_t)(w >> (8 * j)));
            } else if constexpr (CI % 4 == 0) {
                v = *reinterpret_cast<const f32x4*>(src);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = 4 * q + j < CI ? src[j] : 0.0f;
            }
            if constexpr (RELU_IN) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = imp_relu(v[j]);
            }
        }
        *reinterpret_cast<f32x4*>(s_in + cell * G.S + 4 * q) = v;
    }
}

// Un-pool into LDS (the `pooled` backward: the pre-pool gradient plane never exists in HBM).  Rows ya .. ya + NR - 1 x columns
// -HALO .. H + HALO - 1 x C channels of image img's pre-pool gradient go to dst, `stride` floats per cell, zero outside the image.
// First the pooled-gradient rows g and argmax rows arg (both (B, H/2, H/2, C)) that those rows' windows reach -- the outputs
// floor(y / 2) and ceil(y / 2), at most NR / 2 + 1 rows -- are staged in s_g / s_a by 16-byte loads; after a barrier every cell is
// imp_pool_grad's sum over them.  The caller's barrier follows.
constexpr int imp_unpool_rows(int nr) { return nr / 2 + 1; }
template <int C, int H, int NR, int HALO>
__device__ __forceinline__ void imp_unpool(float* dst, int stride, float* s_g, uint8_t* s_a, const float* __restrict__ g,
                                           const uint8_t* __restrict__ arg, int64_t img, int ya) {
    constexpr int HP = imp_half(H), ROW = HP * C, COLS = H + 2 * HALO, Q = C / 4;
    static_assert(H % 2 == 0 && NR % 2 == 0 && ROW % 16 == 0, "whole 16-byte loads of the argmax rows");
    const int yl = ya < 0 ? 0 : ya, yh = ya + NR < H ? ya + NR : H;              // the live rows [yl, yh)
    const int oya = yl / 2, oyb = yh / 2 < HP - 1 ? yh / 2 : HP - 1;
    const int n = (oyb - oya + 1) * ROW;                                         // <= imp_unpool_rows(NR) * ROW
    const int64_t o = (img * HP + oya) * ROW;
    for (int e = threadIdx.x; e < n / 4; e += kImpThreads) reinterpret_cast<f32x4*>(s_g)[e] = reinterpret_cast<const f32x4*>(g + o)[e];
    for (int e = threadIdx.x; e < n / 16; e += kImpThreads) reinterpret_cast<uint4*>(s_a)[e] = reinterpret_cast<const uint4*>(arg + o)[e];
    __syncthreads();
    for (int e = threadIdx.x; e < NR * COLS * Q; e += kImpThreads) {
        const int q = e % Q, cell = e / Q, y = ya + cell / COLS, x = cell % COLS - HALO;
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (y >= 0 && y < H && x >= 0 && x < H) {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = imp_pool_grad(s_g + 4 * q + j, s_a + 4 * q + j, HP, C, y, x, oya);
        }
        *reinterpret_cast<f32x4*>(dst + cell * stride + 4 * q) = v;
    }
}

// ------------------------------------------------------------------------------------------------- kernel IC: convolution
// DGRAD = false: out = conv(relu?(in)) + bias (+ res).  DGRAD = true: out = (mask > 0 ? conv(in) : 0) (+ res), in = dY.
// UNPOOL (a data gradient of the 64 family): dY is the max pool's backward of the pooled gradient `in` through `arg`, produced in
// the staging (imp_unpool); its staged rows borrow the weights' LDS, which is filled afterwards.
template <int CI, int CO, int H, bool RELU_IN, bool DGRAD, typename TIN, bool UNPOOL = false>
__global__ __launch_bounds__(kImpThreads) void imp_conv_kernel(const TIN* __restrict__ in, const float* __restrict__ wp,
                                                               const float* __restrict__ bias, const float* __restrict__ mask,
                                                               const float* __restrict__ res, float* __restrict__ out, int B,
                                                               const uint8_t* __restrict__ arg) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    static_assert(G.LIVE <= G.PIX && (G.NI == 1 || (G.R == H && G.LIVE == G.PIX)) && G.MT * G.NT == 4 && G.KP % 4 == 0, "tiling");
    constexpr bool RAGGED = G.LIVE < G.PIX || H % G.R != 0;          // false for the 64 family: no dead slots, no dead rows
    __shared__ __attribute__((aligned(16))) float s_in[G.LDS_IN];
    __shared__ __attribute__((aligned(16))) float s_w[G.LDS_W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, kq = lane >> 4;
    int64_t img0;
    int y0;
    imp_band(G, H, blockIdx.x, &img0, &y0);

    if constexpr (UNPOOL) {
        constexpr int PG = imp_unpool_rows(G.R + 2) * imp_half(H) * CI;
        static_assert(DGRAD && !RELU_IN && !RAGGED && G.NI == 1 && G.CP == CI && sizeof(TIN) == 4 && PG + PG / 4 <= G.LDS_W, "un-pool staging");
        imp_unpool<CI, H, G.R + 2, 1>(s_in, G.S, s_w, reinterpret_cast<uint8_t*>(s_w + PG), in, arg, img0, y0 - 1);
        __syncthreads();                                              // the staged pooled rows are read: the weights may land
    }
    for (int e = tid; e < G.LDS_W / 4; e += kImpThreads)
        reinterpret_cast<f32x4*>(s_w)[e] = reinterpret_cast<const f32x4*>(wp)[e];
    if constexpr (!UNPOOL) imp_stage<CI, CO, H, RELU_IN>(s_in, in, img0, y0, B);
    __syncthreads();

    int abase[G.MT];
#pragma unroll
    for (int mt = 0; mt < G.MT; ++mt) {
        int p = wave * 16 * G.MT + mt * 16 + lrow;
        if constexpr (RAGGED) p = p < G.LIVE ? p : 0;                 // a dead slot reads slot 0's cells
        const int li = p / (G.R * H), q = p % (G.R * H);
        abase[mt] = ((li * (G.R + 2) + q / H) * G.COLS + q % H) * G.S + kq;
    }
    f32x4 acc[G.MT][G.NT];
#pragma unroll
    for (int mt = 0; mt < G.MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < G.NT; ++nt) acc[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < G.KS; ++ks) {
        const int tap = 4 * ks / G.CP, ci0 = 4 * ks % G.CP;
        const int off = ((tap / 3) * G.COLS + tap % 3) * G.S + ci0;
        float a[G.MT], b[G.NT];
#pragma unroll
        for (int mt = 0; mt < G.MT; ++mt) a[mt] = s_in[abase[mt] + off];
#pragma unroll
        for (int nt = 0; nt < G.NT; ++nt) b[nt] = s_w[(ks * G.NT + nt) * 64 + lane];
#pragma unroll
        for (int mt = 0; mt < G.MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < G.NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
    }

    const int64_t pix0 = (img0 * H + y0) * H;
#pragma unroll
    for (int mt = 0; mt < G.MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = wave * 16 * G.MT + mt * 16 + kq * 4 + r;
            if (img0 + p / (G.R * H) >= B) continue;
            if constexpr (RAGGED)
                if (p >= G.LIVE || y0 + p / H >= H) continue;         // dead slot / dead row of the image's last band
#pragma unroll
            for (int nt = 0; nt < G.NT; ++nt) {
                const int n = nt * 16 + lrow;
                const int64_t o = (pix0 + p) * CO + n;
                float v;
                if constexpr (DGRAD)
                    v = imp_epi_dgrad(acc[mt][nt][r], mask ? mask + o : nullptr, res ? res + o : nullptr);
                else
                    v = imp_epi_fwd(acc[mt][nt][r], bias[n], res ? res + o : nullptr);
                out[o] = v;
            }
        }
}

// ------------------------------------------------------------------- kernel ICP: convolution + bias + max pool (`pooled` forward)
// A sequence's first conv with its pool: the pre-pool plane lives in LDS only.  A workgroup owns RP pooled rows oy0 .. oy0 + RP - 1
// of one image, so the conv rows 2 oy0 - 1 .. 2 (oy0 + RP - 1) + 1: CR = 2 RP + 1 rows, of which the first is the band above's
// last, recomputed (row -1 of an image's first band is computed from the zero halo and never read by a window); at H = 16 the
// band is the image, CR = H.  Its CR H / 16 pixel tiles x CO / 16 channel tiles split evenly over the 4 waves, TPW pixel tiles of
// one channel tile each: (CI, CO, H) = (3, 16, 64): RP 2, 20 tiles, 5 a wave; (16, 32, 32): RP 4, 36 tiles, 9 a wave; (32, 32,
// 16): 32 tiles, 8 a wave.  The k-loop is kernel IC's (same packed weights, same k order: every conv value is the fused path's
// fmaf chain whatever the banding).  Behind a barrier the epilogue writes acc + bias into the LDS conv plane, which lies over
// the staged input and weights (pitch CO + 4 floats a pixel: the four pixel quarters of a tile store to distinct banks); behind
// another, each thread scans its pooled outputs' windows from it by imp_pool_window and stores P and the argmax byte, channels
// fastest: a band's outputs are one contiguous run of both planes.
constexpr int imp_pool_band_rows(int h) { return h >= 64 ? 2 : (h >= 32 ? 4 : h / 2); }
template <int CI, int CO, int H>
__global__ __launch_bounds__(kImpThreads) void imp_convpool_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                                   const float* __restrict__ bias, float* __restrict__ P,
                                                                   uint8_t* __restrict__ arg, int B) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    constexpr int HP = H / 2, RP = imp_pool_band_rows(H), BPI = HP / RP;
    constexpr bool WHOLE = RP == HP;
    constexpr int CR = WHOLE ? H : 2 * RP + 1, PT = CR * H / 16, WM = 4 / G.NT, TPW = PT / WM, PS = CO + 4;
    constexpr int LDS_IN = (CR + 2) * G.COLS * G.S, LDS_C = CR * H * PS;
    constexpr int LDS = LDS_IN + G.LDS_W > LDS_C ? LDS_IN + G.LDS_W : LDS_C;
    static_assert(H % 16 == 0 && HP % RP == 0 && 4 % G.NT == 0 && PT % WM == 0 && LDS_IN % 4 == 0 && G.KP % 4 == 0, "tiling");
    __shared__ __attribute__((aligned(16))) float lds[LDS];
    float *s_in = lds, *s_w = lds + LDS_IN, *s_c = lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, kq = lane >> 4;
    const int wn = wave % G.NT, wm = wave / G.NT;
    const int64_t img = blockIdx.x / BPI;
    const int oy0 = (int)(blockIdx.x % BPI) * RP, cy0 = WHOLE ? 0 : 2 * oy0 - 1;

    for (int e = tid; e < G.LDS_W / 4; e += kImpThreads)
        reinterpret_cast<f32x4*>(s_w)[e] = reinterpret_cast<const f32x4*>(wp)[e];
    imp_stage<CI, CO, H, false, CR + 2, 1>(s_in, in, img, cy0, B);
    __syncthreads();

    int abase[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int p = (wm * TPW + t) * 16 + lrow;
        abase[t] = ((p / H) * G.COLS + p % H) * G.S + kq;
    }
    f32x4 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int ks = 0; ks < G.KS; ++ks) {
        const int tap = 4 * ks / G.CP, ci0 = 4 * ks % G.CP;
        const int off = ((tap / 3) * G.COLS + tap % 3) * G.S + ci0;
        float a[TPW];
#pragma unroll
        for (int t = 0; t < TPW; ++t) a[t] = s_in[abase[t] + off];
        const float b = s_w[(ks * G.NT + wn) * 64 + lane];
#pragma unroll
        for (int t = 0; t < TPW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], b, acc[t], 0, 0, 0);
    }
    __syncthreads();                                                  // every wave's operand reads are done: the conv plane may land

    const int n = wn * 16 + lrow;
    const float bn = bias[n];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_c[((wm * TPW + t) * 16 + kq * 4 + r) * PS + n] = imp_epi_fwd(acc[t][r], bn, nullptr);
    __syncthreads();

    const int64_t o0 = (img * HP + oy0) * HP * CO;
    for (int e = tid; e < RP * HP * CO; e += kImpThreads) {
        const int ch = e % CO, ox = (e / CO) % HP, oy = oy0 + e / (CO * HP);
        uint8_t a;
        P[o0 + e] = imp_pool_window(s_c + ch, H, cy0, H, PS, oy, ox, &a);
        arg[o0 + e] = a;
    }
}

// ---------------------------------------------------------------------------------------- kernel IW: weight + bias gradient
// part[q][co][j] = sum over the pixels of part q's bands of dy[p][co] * a[p][j] (a: the conv's input columns, 1 at j = KP).
// UNPOOL (a sequence's first conv in the 64 family): dy is the pooled gradient and s_dy is filled by imp_unpool through `arg`.
template <int CI, int CO, int H, bool RELU_IN, typename TIN, bool UNPOOL = false>
__global__ __launch_bounds__(kImpThreads) void imp_wgrad_kernel(const TIN* __restrict__ in, const float* __restrict__ dy,
                                                                float* __restrict__ part, int B, int64_t bands, int parts,
                                                                const uint8_t* __restrict__ arg) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    constexpr int CT = CO / 16, JT = G.JP / 16, TILES = CT * JT, TPW = (TILES + 3) / 4;
    constexpr int PG = UNPOOL ? imp_unpool_rows(G.R) * imp_half(H) * CO : 16;    // the staged pooled gradient rows (argmax: a byte each)
    static_assert(!UNPOOL || (G.NI == 1 && G.LIVE == G.PIX && H % G.R == 0), "un-pool staging: whole bands of one image");
    __shared__ __attribute__((aligned(16))) float s_in[G.LDS_IN];
    __shared__ __attribute__((aligned(16))) float s_dy[G.PIX * CO];
    __shared__ __attribute__((aligned(16))) float s_pg[PG];
    __shared__ __attribute__((aligned(16))) uint8_t s_pa[PG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lrow = lane & 15, kq = lane >> 4;

    int boff[TPW];
    float bconst[TPW];
    bool bload[TPW], bhi[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = wave + 4 * i, j = (t % JT) * 16 + lrow;
        const bool tap = t < TILES && j < G.KP;
        const int k = tap ? j : 0;
        boff[i] = ((k / G.CP / 3) * G.COLS + (k / G.CP) % 3) * G.S + k % G.CP;
        bload[i] = tap;
        bconst[i] = (t < TILES && j == G.KP) ? 1.0f : 0.0f;
        bhi[i] = t / JT == 1;
    }
    f32x4 acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    int64_t b0, b1;
    imp_part_range(bands, parts, blockIdx.x, &b0, &b1);
    for (int64_t b = b0; b < b1; ++b) {
        int64_t img0;
        int y0;
        imp_band(G, H, b, &img0, &y0);
        const int npix = imp_band_pixels(G, H, img0, y0, B);
        const int64_t pix0 = (img0 * H + y0) * H;
        __syncthreads();                                              // the previous band's reads are done
        if constexpr (UNPOOL) {
            imp_unpool<CO, H, G.R, 0>(s_dy, CO, s_pg, s_pa, dy, arg, img0, y0);
        } else {
            for (int e = tid; e < npix * CO / 4; e += kImpThreads)
                reinterpret_cast<f32x4*>(s_dy)[e] = reinterpret_cast<const f32x4*>(dy + pix0 * CO)[e];
        }
        imp_stage<CI, CO, H, RELU_IN>(s_in, in, img0, y0, B);
        __syncthreads();
        constexpr bool TAIL = (G.R * H) % 4 != 0 || H % 4 != 0;       // a band's pixel count may be no multiple of 4
        for (int pg = 0; pg < (npix + 3) / 4; ++pg) {
            int p = 4 * pg + kq;
            bool dead = false;
            if constexpr (TAIL) {
                dead = p >= npix;                                     // enters the chain as 0 * 0 (impala_rows.h)
                p = dead ? 0 : p;
            }
            const int li = p / (G.R * H), q = p % (G.R * H);
            const int pb = ((li * (G.R + 2) + q / H) * G.COLS + q % H) * G.S;
            float a0 = s_dy[p * CO + lrow];
            float a1 = CT > 1 ? s_dy[p * CO + 16 + lrow] : 0.0f;
            if constexpr (TAIL) {
                a0 = dead ? 0.0f : a0;
                a1 = dead ? 0.0f : a1;
            }
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                if (wave + 4 * i >= TILES) continue;                  // wave-uniform
                float bv = s_in[pb + boff[i]];
                bv = bload[i] ? bv : bconst[i];
                if constexpr (TAIL) bv = dead ? 0.0f : bv;
                acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(bhi[i] ? a1 : a0, bv, acc[i], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int t = wave + 4 * i;
        if (t >= TILES) continue;
        const int ct = t / JT, j = (t % JT) * 16 + lrow;
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((int64_t)blockIdx.x * CO + ct * 16 + kq * 4 + r) * G.JP + j] = acc[i][r];
    }
}

// --------------------------------------------------------------------------------------------------- kernel IF: the fold
// 16 outputs x kImpFoldGroups runs per workgroup: each thread adds one run of parts (loads unrolled, adds in order), then the
// first group adds the run sums in order.
__global__ __launch_bounds__(256) void imp_fold_kernel(const float* __restrict__ part, int parts, int ci, int co, int cp, int jp,
                                                       float* __restrict__ gw, float* __restrict__ gb) {
    static_assert(16 * kImpFoldGroups == 256, "fold block");
    __shared__ float s_run[kImpFoldGroups][16];
    const int g = threadIdx.x / 16, tl = threadIdx.x % 16, t = blockIdx.x * 16 + tl;
    const bool live = t < co * jp;
    int q0, q1;
    imp_fold_range(parts, g, &q0, &q1);
    float s = 0.0f;
    if (live) {
        int q = q0;
        for (; q + 8 <= q1; q += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = part[(int64_t)(q + i) * co * jp + t];
#pragma unroll
            for (int i = 0; i < 8; ++i) s = s + v[i];
        }
        for (; q < q1; ++q) s = s + part[(int64_t)q * co * jp + t];
    }
    s_run[g][tl] = s;
    __syncthreads();
    if (g != 0 || !live) return;
    const int n = t / jp, j = t % jp, kp = 9 * cp;
    if (j > kp || (j < kp && j % cp >= ci)) return;
    float r = 0.0f;
#pragma unroll
    for (int i = 0; i < kImpFoldGroups; ++i) r = r + s_run[i][tl];
    if (j == kp)
        gb[n] = r;
    else
        gw[((size_t)n * ci + j % cp) * 9 + j / cp] = r;
}

// ---------------------------------------------------------------------------------------------------------------- max pool
__global__ __launch_bounds__(256) void imp_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           uint8_t* __restrict__ arg, int64_t total, int h, int c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ho = imp_half(h);
    const int ch = (int)(i % c);
    const int64_t o = i / c;
    const int ox = (int)(o % ho), oy = (int)((o / ho) % ho);
    const int64_t img = o / ((int64_t)ho * ho);
    uint8_t a;
    y[i] = imp_pool_window(x + img * h * h * c + ch, h, 0, h, c, oy, ox, &a);
    arg[i] = a;
}

__global__ __launch_bounds__(256) void imp_pool_bwd_kernel(const float* __restrict__ g, const uint8_t* __restrict__ arg,
                                                           float* __restrict__ dx, int64_t total, int h, int c) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int ho = imp_half(h);
    const int ch = (int)(i % c);
    const int64_t o = i / c;
    const int ix = (int)(o % h), iy = (int)((o / h) % h);
    const int64_t img = o / ((int64_t)h * h);
    const int64_t base = img * ho * ho * c + ch;
    dx[i] = imp_pool_grad(g + base, arg + base, ho, c, iy, ix);
}

// ---------------------------------------------------------------------------------------------------------------- launches
unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <int CI, int CO, int H, bool RELU_IN, bool DGRAD, typename TIN>
void conv(const TIN* in, const float* wp, const float* bias, const float* mask, const float* res, float* out, int B, hipStream_t s) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    hipLaunchKernelGGL((imp_conv_kernel<CI, CO, H, RELU_IN, DGRAD, TIN>), dim3((unsigned)imp_bands(G, H, B)), dim3(kImpThreads), 0, s, in, wp,
                       bias, mask, res, out, B, nullptr);
}

// `pooled`: the sequence's conv + pool in one launch; the data gradient of that conv from the pooled gradient g through arg.
template <int CI, int CO, int H>
void convpool(const float* in, const float* wp, const float* bias, float* P, uint8_t* arg, int B, hipStream_t s) {
    constexpr int BPI = H / 2 / imp_pool_band_rows(H);
    hipLaunchKernelGGL((imp_convpool_kernel<CI, CO, H>), dim3((unsigned)B * BPI), dim3(kImpThreads), 0, s, in, wp, bias, P, arg, B);
}

template <int CI, int CO, int H>
void conv_unpool(const float* g, const uint8_t* arg, const float* wp, float* out, int B, hipStream_t s) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    hipLaunchKernelGGL((imp_conv_kernel<CI, CO, H, false, true, float, true>), dim3((unsigned)imp_bands(G, H, B)), dim3(kImpThreads), 0, s, g,
                       wp, nullptr, nullptr, nullptr, out, B, arg);
}

// UNPOOL: dy is the pooled gradient, un-pooled through arg in the staging.
template <int CI, int CO, int H, bool RELU_IN, bool UNPOOL = false, typename TIN>
void wgrad(const TIN* in, const float* dy, float* part, float* gw, float* gb, int B, hipStream_t s, const uint8_t* arg = nullptr) {
    constexpr ImpGeom G = imp_geom(CI, CO, H);
    const int64_t bands = imp_bands(G, H, B);
    const int parts = imp_parts(bands);
    hipLaunchKernelGGL((imp_wgrad_kernel<CI, CO, H, RELU_IN, TIN, UNPOOL>), dim3(parts), dim3(kImpThreads), 0, s, in, dy, part, B, bands, parts,
                       arg);
    hipLaunchKernelGGL(imp_fold_kernel, dim3((CO * G.JP + 15) / 16), dim3(256), 0, s, part, parts, CI, CO, G.CP, G.JP, gw, gb);
}

void pool_fwd(const float* x, float* y, uint8_t* arg, int B, int h, int c, hipStream_t s) {
    const int64_t total = (int64_t)B * imp_half(h) * imp_half(h) * c;
    hipLaunchKernelGGL(imp_pool_fwd_kernel, dim3(blocks256(total)), dim3(256), 0, s, x, y, arg, total, h, c);
}

void pool_bwd(const float* g, const uint8_t* arg, float* dx, int B, int h, int c, hipStream_t s) {
    const int64_t total = (int64_t)B * h * h * c;
    hipLaunchKernelGGL(imp_pool_bwd_kernel, dim3(blocks256(total)), dim3(256), 0, s, g, arg, dx, total, h, c);
}

// Workspace regions (bytes, 256-aligned): packed weights | conv / pool scratch of the largest plane | (backward) two
// gradient planes and a temporary of the residual size | weight-gradient partials.
size_t al256(size_t n) { return (n + 255) / 256 * 256; }
constexpr int64_t imp_conv0_plane(int f) { return (int64_t)imp_fam_h(f) * imp_fam_h(f) * 16; }   // sequence 0's conv output, per image
constexpr int64_t imp_res_plane(int f) { return imp_plane(f, 0); }      // the largest residual-block tensor, per image
static_assert(imp_res_plane(kImpFam64) == 32 * 32 * 16 && imp_plane(kImpFam84, 0) >= imp_plane(kImpFam84, 1), "workspace planes");
constexpr int64_t kImpPartFloats = (int64_t)kImpMaxParts * 32 * imp_geom(32, 32, 16).JP;

struct ImpWs {
    float *wp, *big, *ga, *gb, *t, *part;
};
size_t imp_ws_bytes(int f, int B, bool backward) {
    size_t n = al256(sizeof(float) * kImpPackFloats) + al256(sizeof(float) * imp_conv0_plane(f) * B);
    if (backward) n += 3 * al256(sizeof(float) * imp_res_plane(f) * B) + al256(sizeof(float) * kImpPartFloats);
    return n;
}
ImpWs imp_ws(int f, void* ws, int B, bool backward) {
    const int64_t kImpConv0Plane = imp_conv0_plane(f), kImpResPlane = imp_res_plane(f);
    char* p = static_cast<char*>(ws);
    ImpWs w{};
    w.wp = reinterpret_cast<float*>(p);
    p += al256(sizeof(float) * kImpPackFloats);
    w.big = reinterpret_cast<float*>(p);
    p += al256(sizeof(float) * kImpConv0Plane * B);
    if (backward) {
        w.ga = reinterpret_cast<float*>(p);
        p += al256(sizeof(float) * kImpResPlane * B);
        w.gb = reinterpret_cast<float*>(p);
        p += al256(sizeof(float) * kImpResPlane * B);
        w.t = reinterpret_cast<float*>(p);
        p += al256(sizeof(float) * kImpResPlane * B);
        w.part = reinterpret_cast<float*>(p);
    }
    return w;
}

template <int F, int S, bool POOLED, typename TIN>
void fwd_seq(const TIN* xin, const ImpParams& prm, const float* wp, float* saved, uint8_t* argmax, float* big, float* yout, int B,
             hipStream_t s) {
    constexpr int CI = imp_seq_cin(F, S), C = imp_seq_cout(S), H = imp_seq_h(F, S), HP = imp_half(H), L = 5 * S;
    float* P = saved + imp_saved_offset(F, B, S, 0);
    float* h0 = saved + imp_saved_offset(F, B, S, 1);
    float* x1 = saved + imp_saved_offset(F, B, S, 2);
    float* h1 = saved + imp_saved_offset(F, B, S, 3);
    const float* const* p = prm.p;
    if constexpr (POOLED) {
        convpool<CI, C, H>(xin, wp + imp_pack_offset(L, false), p[2 * L + 1], P, argmax + imp_argmax_offset(F, B, S), B, s);
    } else {
        conv<CI, C, H, false, false>(xin, wp + imp_pack_offset(L, false), p[2 * L + 1], nullptr, nullptr, big, B, s);
        pool_fwd(big, P, argmax + imp_argmax_offset(F, B, S), B, H, C, s);
    }
    conv<C, C, HP, true, false>(P, wp + imp_pack_offset(L + 1, false), p[2 * L + 3], nullptr, nullptr, h0, B, s);
    conv<C, C, HP, true, false>(h0, wp + imp_pack_offset(L + 2, false), p[2 * L + 5], nullptr, P, x1, B, s);
    conv<C, C, HP, true, false>(x1, wp + imp_pack_offset(L + 3, false), p[2 * L + 7], nullptr, nullptr, h1, B, s);
    conv<C, C, HP, true, false>(h1, wp + imp_pack_offset(L + 4, false), p[2 * L + 9], nullptr, x1, yout, B, s);
}

// Backward of sequence S from g_in = dL/d(its output); returns dL/d(its input) (S > 0) in a workspace plane.
template <int F, int S, bool POOLED, typename TIN>
const float* bwd_seq(const TIN* xin, const float* wp, const float* saved, const uint8_t* argmax, const float* g_in, float* const* gr,
                     const ImpWs& w, int B, hipStream_t s) {
    constexpr int CI = imp_seq_cin(F, S), C = imp_seq_cout(S), H = imp_seq_h(F, S), HP = imp_half(H), L = 5 * S;
    const float* P = saved + imp_saved_offset(F, B, S, 0);
    const float* h0 = saved + imp_saved_offset(F, B, S, 1);
    const float* x1 = saved + imp_saved_offset(F, B, S, 2);
    const float* h1 = saved + imp_saved_offset(F, B, S, 3);
    auto other = [&](const float* g) { return g == w.ga ? w.gb : w.ga; };
    float* g1 = other(g_in);
    float* g2 = other(g1);
    // res_block1
    wgrad<C, C, HP, true>(h1, g_in, w.part, gr[2 * L + 8], gr[2 * L + 9], B, s);
    conv<C, C, HP, false, true>(g_in, wp + imp_pack_offset(L + 4, true), nullptr, h1, nullptr, w.t, B, s);
    wgrad<C, C, HP, true>(x1, w.t, w.part, gr[2 * L + 6], gr[2 * L + 7], B, s);
    conv<C, C, HP, false, true>(w.t, wp + imp_pack_offset(L + 3, true), nullptr, x1, g_in, g1, B, s);
    // res_block0
    wgrad<C, C, HP, true>(h0, g1, w.part, gr[2 * L + 4], gr[2 * L + 5], B, s);
    conv<C, C, HP, false, true>(g1, wp + imp_pack_offset(L + 2, true), nullptr, h0, nullptr, w.t, B, s);
    wgrad<C, C, HP, true>(P, w.t, w.part, gr[2 * L + 2], gr[2 * L + 3], B, s);
    conv<C, C, HP, false, true>(w.t, wp + imp_pack_offset(L + 1, true), nullptr, P, g1, g2, B, s);
    // max pool, then the sequence's conv (`pooled`: the pool's backward inside the staging of the conv's two gradient launches)
    const uint8_t* arg = argmax + imp_argmax_offset(F, B, S);
    if constexpr (POOLED) {
        wgrad<CI, C, H, false, true>(xin, g2, w.part, gr[2 * L], gr[2 * L + 1], B, s, arg);
    } else {
        pool_bwd(g2, arg, w.big, B, H, C, s);
        wgrad<CI, C, H, false>(xin, w.big, w.part, gr[2 * L], gr[2 * L + 1], B, s);
    }
    if constexpr (S == 0) {
        return nullptr;
    } else {
        float* gx = other(g2);
        if constexpr (POOLED)
            conv_unpool<C, CI, H>(g2, arg, wp + imp_pack_offset(L, true), gx, B, s);
        else
            conv<C, CI, H, false, true>(w.big, wp + imp_pack_offset(L, true), nullptr, nullptr, nullptr, gx, B, s);
        return gx;
    }
}

int imp_check(int f, const char* fn, int B, int H, int W, int C, int ch0, int ch1, int ch2) {
    MI355_REQUIRE(B > 0, MI355PPO_EINVAL, "%s: B=%d must be positive", fn, B);
    MI355_REQUIRE(H == imp_fam_h(f) && W == imp_fam_h(f) && C == imp_fam_c(f), MI355PPO_EINVAL, "%s: frames %dx%dx%d (only %dx%dx%d)", fn,
                  H, W, C, imp_fam_h(f), imp_fam_h(f), imp_fam_c(f));
    MI355_REQUIRE(ch0 == 16 && ch1 == 32 && ch2 == 32, MI355PPO_EINVAL, "%s: channels [%d, %d, %d] (only [16, 32, 32])", fn, ch0, ch1,
                  ch2);
    return MI355PPO_OK;
}

// The forward / backward of family F on frames of type TIN (f32 for the 64 family, the ring's bytes for the 84 family).
// POOLED (64 family): kernel ICP and the un-pooling gradient launches; the workspace's `big` region stays unused.
template <int F, bool POOLED = false, typename TIN>
int imp_fwd(const char* fn, const TIN* x, const float* const* params, float* y, float* saved, uint8_t* argmax, int B, int H, int W,
            int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes, void* stream) {
    MI355_REQUIRE(x && params && y && saved && argmax, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int st = imp_check(F, fn, B, H, W, C, ch0, ch1, ch2)) return st;
    for (int i = 0; i < kImpParams; ++i) MI355_REQUIRE(params[i], MI355PPO_EINVAL, "%s: null pointer (params[%d])", fn, i);
    MI355_REQUIRE(aligned(x, 4) && aligned(y, 16) && aligned(saved, 16), MI355PPO_EALIGN, "%s: x must be 4-, y / saved 16-byte aligned",
                  fn);
    MI355_REQUIRE(workspace && workspace_bytes >= imp_ws_bytes(F, B, false), MI355PPO_EWORKSPACE, "%s: workspace NULL or < %zu bytes", fn,
                  imp_ws_bytes(F, B, false));
    MI355_REQUIRE(aligned(workspace, 256), MI355PPO_EALIGN, "%s: workspace must be 256-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    ImpParams prm;
    for (int i = 0; i < kImpParams; ++i) prm.p[i] = params[i];
    const ImpWs w = imp_ws(F, workspace, B, false);
    hipLaunchKernelGGL(imp_pack_kernel<F>, dim3(blocks256(kImpPackFloats)), dim3(256), 0, s, prm, w.wp);
    float* y0 = saved + imp_saved_offset(F, B, 0, 4);
    float* y1 = saved + imp_saved_offset(F, B, 1, 4);
    fwd_seq<F, 0, POOLED>(x, prm, w.wp, saved, argmax, w.big, y0, B, s);
    fwd_seq<F, 1, POOLED>((const float*)y0, prm, w.wp, saved, argmax, w.big, y1, B, s);
    fwd_seq<F, 2, POOLED>((const float*)y1, prm, w.wp, saved, argmax, w.big, y, B, s);
    return check_launch(fn);
}

template <int F, bool POOLED = false, typename TIN>
int imp_bwd(const char* fn, const TIN* x, const float* const* params, const float* saved, const uint8_t* argmax, const float* dy,
            float* const* grads, int B, int H, int W, int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes,
            void* stream) {
    MI355_REQUIRE(x && params && saved && argmax && dy && grads, MI355PPO_EINVAL, "%s: null pointer", fn);
    if (int st = imp_check(F, fn, B, H, W, C, ch0, ch1, ch2)) return st;
    for (int i = 0; i < kImpParams; ++i)
        MI355_REQUIRE(params[i] && grads[i], MI355PPO_EINVAL, "%s: null pointer (params / grads[%d])", fn, i);
    MI355_REQUIRE(aligned(x, 4) && aligned(dy, 16) && aligned(saved, 16), MI355PPO_EALIGN, "%s: x must be 4-, dy / saved 16-byte aligned",
                  fn);
    MI355_REQUIRE(!POOLED || aligned(argmax, 16), MI355PPO_EALIGN, "%s: argmax must be 16-byte aligned (its rows are staged by 16-byte loads)", fn);
    MI355_REQUIRE(workspace && workspace_bytes >= imp_ws_bytes(F, B, true), MI355PPO_EWORKSPACE, "%s: workspace NULL or < %zu bytes", fn,
                  imp_ws_bytes(F, B, true));
    MI355_REQUIRE(aligned(workspace, 256), MI355PPO_EALIGN, "%s: workspace must be 256-byte aligned", fn);
    hipStream_t s = as_stream(stream);
    ImpParams prm;
    for (int i = 0; i < kImpParams; ++i) prm.p[i] = params[i];
    const ImpWs w = imp_ws(F, workspace, B, true);
    hipLaunchKernelGGL(imp_pack_kernel<F>, dim3(blocks256(kImpPackFloats)), dim3(256), 0, s, prm, w.wp);
    const float* g = bwd_seq<F, 2, POOLED>(saved + imp_saved_offset(F, B, 1, 4), w.wp, saved, argmax, dy, grads, w, B, s);
    g = bwd_seq<F, 1, POOLED>(saved + imp_saved_offset(F, B, 0, 4), w.wp, saved, argmax, g, grads, w, B, s);
    bwd_seq<F, 0, POOLED>(x, w.wp, saved, argmax, g, grads, w, B, s);
    return check_launch(fn);
}

bool imp_pool_shape(int B, int H, int W, int C) {
    for (int f : {kImpFam64, kImpFam84})
        for (int s = 0; s < kImpSeqs; ++s)
            if (B > 0 && H == W && H == imp_seq_h(f, s) && C == imp_seq_cout(s)) return true;
    return false;
}

}  // namespace
}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int64_t mi355ppo_impala_saved_floats(int B) { return B > 0 ? imp_saved_floats(kImpFam64, B) : 0; }
extern "C" MI355PPO_API int64_t mi355ppo_impala_argmax_bytes(int B) { return B > 0 ? imp_argmax_bytes(kImpFam64, B) : 0; }
extern "C" MI355PPO_API size_t mi355ppo_impala_workspace_bytes(int B, int backward) {
    return B > 0 ? imp_ws_bytes(kImpFam64, B, backward != 0) : 0;
}
extern "C" MI355PPO_API int64_t mi355ppo_impala84_saved_floats(int B) { return B > 0 ? imp_saved_floats(kImpFam84, B) : 0; }
extern "C" MI355PPO_API int64_t mi355ppo_impala84_argmax_bytes(int B) { return B > 0 ? imp_argmax_bytes(kImpFam84, B) : 0; }
extern "C" MI355PPO_API size_t mi355ppo_impala84_workspace_bytes(int B, int backward) {
    return B > 0 ? imp_ws_bytes(kImpFam84, B, backward != 0) : 0;
}

extern "C" MI355PPO_API int mi355ppo_impala_fwd_f32(const float* x, const float* const* params, float* y, float* saved, uint8_t* argmax,
                                                    int B, int H, int W, int C, int ch0, int ch1, int ch2, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
    return imp_fwd<kImpFam64>("mi355ppo_impala_fwd_f32", x, params, y, saved, argmax, B, H, W, C, ch0, ch1, ch2, workspace,
                              workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala_bwd_f32(const float* x, const float* const* params, const float* saved, const uint8_t* argmax,
                                                    const float* dy, float* const* grads, int B, int H, int W, int C, int ch0, int ch1,
                                                    int ch2, void* workspace, size_t workspace_bytes, void* stream) {
    return imp_bwd<kImpFam64>("mi355ppo_impala_bwd_f32", x, params, saved, argmax, dy, grads, B, H, W, C, ch0, ch1, ch2, workspace,
                              workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala_fwd_pooled_f32(const float* x, const float* const* params, float* y, float* saved,
                                                           uint8_t* argmax, int B, int H, int W, int C, int ch0, int ch1, int ch2,
                                                           void* workspace, size_t workspace_bytes, void* stream) {
    return imp_fwd<kImpFam64, true>("mi355ppo_impala_fwd_pooled_f32", x, params, y, saved, argmax, B, H, W, C, ch0, ch1, ch2, workspace,
                                    workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala_bwd_pooled_f32(const float* x, const float* const* params, const float* saved,
                                                           const uint8_t* argmax, const float* dy, float* const* grads, int B, int H, int W,
                                                           int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes,
                                                           void* stream) {
    return imp_bwd<kImpFam64, true>("mi355ppo_impala_bwd_pooled_f32", x, params, saved, argmax, dy, grads, B, H, W, C, ch0, ch1, ch2,
                                    workspace, workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala84_fwd_u8(const uint8_t* x, const float* const* params, float* y, float* saved,
                                                     uint8_t* argmax, int B, int H, int W, int C, int ch0, int ch1, int ch2,
                                                     void* workspace, size_t workspace_bytes, void* stream) {
    return imp_fwd<kImpFam84>("mi355ppo_impala84_fwd_u8", x, params, y, saved, argmax, B, H, W, C, ch0, ch1, ch2, workspace,
                              workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala84_bwd_u8(const uint8_t* x, const float* const* params, const float* saved,
                                                     const uint8_t* argmax, const float* dy, float* const* grads, int B, int H, int W,
                                                     int C, int ch0, int ch1, int ch2, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
    return imp_bwd<kImpFam84>("mi355ppo_impala84_bwd_u8", x, params, saved, argmax, dy, grads, B, H, W, C, ch0, ch1, ch2, workspace,
                              workspace_bytes, stream);
}

extern "C" MI355PPO_API int mi355ppo_impala_maxpool_fwd_f32(const float* x, float* y, uint8_t* argmax, int B, int H, int W, int C,
                                                            void* stream) {
    const char* fn = "mi355ppo_impala_maxpool_fwd_f32";
    MI355_REQUIRE(x && y && argmax, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(imp_pool_shape(B, H, W, C), MI355PPO_EINVAL,
                  "%s: B=%d %dx%dx%d (only the trunks' 64x64x16, 32x32x32, 16x16x32, 84x84x16, 42x42x32, 21x21x32)", fn, B, H, W, C);
    pool_fwd(x, y, argmax, B, H, C, as_stream(stream));
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_impala_maxpool_bwd_f32(const float* dy, const uint8_t* argmax, float* dx, int B, int H, int W, int C,
                                                            void* stream) {
    const char* fn = "mi355ppo_impala_maxpool_bwd_f32";
    MI355_REQUIRE(dy && argmax && dx, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(imp_pool_shape(B, H, W, C), MI355PPO_EINVAL,
                  "%s: B=%d %dx%dx%d (only the trunks' 64x64x16, 32x32x32, 16x16x32, 84x84x16, 42x42x32, 21x21x32)", fn, B, H, W, C);
    pool_bwd(dy, argmax, dx, B, H, C, as_stream(stream));
    return check_launch(fn);
}
