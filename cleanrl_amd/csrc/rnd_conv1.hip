// The normalising one-frame conv1 of RNDModel's predictor / target (cleanrl/ppo_rnd_envpool.py:188-233; gfx950):
//     a1 = leaky(conv(x, W1) + b1),  x[r, p] = (float)clip(((double)u8 - mean[p]) / sd[p], -5, 5)  -- Conv2d(1, 32, 8, stride=4) on 84 x 84,
// forward and weight / bias gradient straight from the u8 rollout rows.  x is rnd_normalize (rnd_rows.h), the row function of
// mi355ppo_rnd_normalize_u8_f32, so the two agree by construction; it never goes to global memory.  Frames are addressed as in rnd.hip
// (row_bytes, pixel_stride, byte_offset, an optional clamped int64 index): nothing outside the frames is read.
//
// Arithmetic: the two-term f16 split (f16split.h).  x under the STATIC scale 2^12 = 2^f16_scale_exp(5.0f) -- |x| <= 5, no amax record, so a
// row's bits do not depend on which other rows share its batch --, W1 (forward) in mi355ppo_fc_pack_f16x2_f32's pack of the (32, 64) matrix
// under its own record, dz1 (gradient) under its amax record; the products hi hi, hi lo, lo hi on v_mfma_f32_32x32x16_f16 with f32 accumulation.
//
// Both kernels: a 4-wave workgroup walks images.  A thread owns pixels tid, tid + 256, ... of every image (28 of them; their mean / sd stay in
// its registers for the life of the kernel), normalises each ONCE per image -- one float64 divide per pixel, not one per tap -- and writes the
// two f16 terms into LDS, where the matrix-instruction operands are read from.
//   forward: LDS planes [84][88] f16 (hi, lo).  Rows of the matrix instruction = 32 consecutive output pixels (13 tiles per image, wave w owns
//     tiles w, w + 4, ..), columns = the 32 channels, the 4 k-steps = tap rows (2 s + lane / 32): a lane's operand is 8 consecutive f16 of one
//     source row.  W1's fragments (32 registers) are loaded once.  Epilogue: * 2^-(12 + e_W) + bias, LeakyReLU as torch defines it, optional
//     (z > 0) mask words (word p = the 32 channels of pixel p) and amax record (one integer atomic max per wave; no float atomics).
//   gradient: kernel P1's roles (conv1p1.hip): rows = the 32 channels (dz1 in two terms), columns = 32 of the 64 taps, the 16 slots = two groups
//     of 8 adjacent output pixels; dW (2 x 16 registers) stays in the accumulators, one partial per wave, folded in a fixed order by
//     conv_wgrad_reduce1/2.  LDS lines as P1's, in f16: line (source row R, x mod 4) holds x = 4 q + t, q = 0 .. 20, in 32 f16; a tap column's 8
//     pixels are 8 consecutive f16 from q = ox0 + kw / 4, read as 5 aligned dwords and shifted by v_alignbit.  The padding f16 are zeroed once
//     (they meet zero dz terms and must be finite).  ONE staged image, between two barriers -- not P1's double buffer.  Two split images
//     (2 x 43 KB = 86 KB) would fit gfx950's 160 KB of LDS; what is missing is registers: P1 hides its staging by holding the next image's
//     dwords in registers across the steps, and this kernel already stands at 256 VGPRs + 38 AGPRs (the 56 statistics doubles), one wave per
//     SIMD, one workgroup per CU.  So nothing covers the staging here: normalising and the matrix steps run in turn, and the launch takes about
//     twice the time of kernel P on the agent's four-frame rows at 4,096 images.  Halving the statistics' registers (a two-pass walk over pixel halves) is the open lever.
#include "common.h"
#include "f16split.h"
#include "leaky_rows.h"
#include "rnd_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

typedef float n1_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned n1_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kN1XExp = 12;                                   // f16_scale_exp(bits of 5.0f): 5 * 2^12 = 20,480 in [2^14, 2^15)
constexpr int kN1PerThread = (kRndPixels + 255) / 256;        // 28 pixels of an image per thread (the last one of threads 0 .. 143 only)
constexpr int kN1Pitch = 88, kN1Plane = 84 * kN1Pitch;        // forward: f16 per staged source row (84 payload, 176 bytes) / per plane
constexpr int kN1Line = 32, kN1RowLds = 4 * kN1Line;          // gradient: f16 per (R, t) line (q = 0 .. 20 payload) / per source row
constexpr int kN1PlaneW = 84 * kN1RowLds;                     // 10,752 f16 = 21,504 bytes per plane
constexpr int kN1Tiles = 13;                                  // 32-pixel tiles of the 400 output pixels (the last one half empty)

// the thread's statistics, once per kernel
struct N1Stats {
    double mu[kN1PerThread], sd[kN1PerThread];
    __device__ __forceinline__ void load(const double* __restrict__ mean, const double* __restrict__ sdev, int tid) {
#pragma unroll
        for (int k = 0; k < kN1PerThread; ++k) {
            const int p = tid + 256 * k;
            mu[k] = p < kRndPixels ? mean[p] : 0.0;
            sd[k] = p < kRndPixels ? sdev[p] : 1.0;
        }
    }
};

// pixel p of the frame -> the two f16 terms of 2^12 x
template <int STRIDE>
__device__ __forceinline__ void n1_split(const unsigned char* row, int p, int off, double mu, double sd, _Float16& hi, _Float16& lo) {
    const float v = rnd_normalize(rnd_pixel<STRIDE>(row, p, off), mu, sd) * f16_pow2(kN1XExp);
    hi = (_Float16)v;
    lo = (_Float16)(v - (float)hi);
}

template <int STRIDE, bool BITS>
__global__ __launch_bounds__(256) void rnd_conv1_fwd_kernel(const unsigned char* __restrict__ src, int64_t B, int64_t row_bytes, int off,
                                                            const int64_t* __restrict__ idx, const double* __restrict__ mean,
                                                            const double* __restrict__ sdev, const unsigned char* __restrict__ pack,
                                                            const float* __restrict__ bias, float* __restrict__ dst, unsigned* __restrict__ bits,
                                                            unsigned* __restrict__ amax, int M, float slope) {
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][kN1Plane];            // 29,568 bytes
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    // W1's fragments: [k-step][hi, lo][64 lanes][8 f16] behind the pack's header (gemmz.hip, zpack_h_kernel); the same for every tile
    const int ew = f16_scale_exp(*reinterpret_cast<const unsigned*>(pack));
    s_f16x8 Wh[4], Wl[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        Wh[s] = *reinterpret_cast<const s_f16x8*>(pack + kF16PackHeader + (2 * s) * 1024 + 16 * lane);
        Wl[s] = *reinterpret_cast<const s_f16x8*>(pack + kF16PackHeader + (2 * s + 1) * 1024 + 16 * lane);
    }
    const float un = f16_unscale(kN1XExp, ew), bias_r = bias[li];
    N1Stats st;
    st.load(mean, sdev, tid);
    float cmax = 0.0f;
    for (int img = blockIdx.x; img < M; img += gridDim.x) {                      // (grid <= M; uniform over the workgroup)
        const unsigned char* const row = src + rnd_clamp_index(idx ? idx[img] : (int64_t)img, B) * row_bytes;
#pragma unroll
        for (int k = 0; k < kN1PerThread; ++k) {
            const int p = tid + 256 * k;
            if (p < kRndPixels) {
                _Float16 h, l;
                n1_split<STRIDE>(row, p, off, st.mu[k], st.sd[k], h, l);
                const int R = p / 84, c = p - 84 * R;
                xs[0][R * kN1Pitch + c] = h;
                xs[1][R * kN1Pitch + c] = l;
            }
        }
        __syncthreads();
        for (int tile = wave; tile < kN1Tiles; tile += 4) {
            const int p = 32 * tile + li, pc = p < 400 ? p : 399;                // (pixels past 400 read the last pixel: results dropped)
            const int oy = pc / 20, ox = pc - 20 * oy;
            n1_f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // tap row 2 s + lh of the lane's pixel: 8 consecutive f16 of source row 4 oy + 2 s + lh from column 4 ox (8-byte aligned)
                const int o = (4 * oy + 2 * s + lh) * kN1Pitch + 4 * ox;
                const uint2 h0 = *reinterpret_cast<const uint2*>(&xs[0][o]), h1 = *reinterpret_cast<const uint2*>(&xs[0][o + 4]);
                const uint2 l0 = *reinterpret_cast<const uint2*>(&xs[1][o]), l1 = *reinterpret_cast<const uint2*>(&xs[1][o + 4]);
                const s_f16x8 Ah = __builtin_bit_cast(s_f16x8, (n1_u32x4){h0.x, h0.y, h1.x, h1.y});
                const s_f16x8 Al = __builtin_bit_cast(s_f16x8, (n1_u32x4){l0.x, l0.y, l1.x, l1.y});
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Wh[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Wl[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Wh[s], acc, 0, 0, 0);
            }
            // accumulator row e of the lane is pixel (e & 3) + 8 (e >> 2) + 4 lh of the tile, column = channel li
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int pp = 32 * tile + (e & 3) + 8 * (e >> 2) + 4 * lh;
                const bool live = pp < 400;
                const float z = acc[e] * un + bias_r;
                const float o = leaky_fwd(z, slope);
                const size_t pix = (size_t)img * 400 + (size_t)pp;
                if (live) {
                    dst[pix * 32 + li] = o;
                    cmax = __builtin_fmaxf(cmax, __builtin_fabsf(o));             // (a NaN is not recorded)
                }
                if constexpr (BITS) {      // ballot lanes 0..31: the 32 channels of the lower half-wave's pixel; lanes 32..63: of that pixel + 4
                    const unsigned long long bal = __builtin_amdgcn_ballot_w64(z > 0.0f);
                    if (li == 0 && live) bits[pix] = lh ? (unsigned)(bal >> 32) : (unsigned)bal;
                }
            }
        }
        __syncthreads();                                                         // this image's readers are done before the next one is staged
    }
    if (amax) amax_commit(amax, __float_as_uint(cmax), blockIdx.x * 4 + wave, lane);      // (uniform; all lanes are here)
}

// ---- weight + bias gradient: kernel P1's walk (conv1p1.hip) with the split x as the staged operand
constexpr int kN1RowsPerWave = 5, kN1Steps = 8, kN1Groups = 15;
__host__ __device__ constexpr int n1_row(int g) { return g < kN1Groups ? g / 3 : kN1RowsPerWave - 1; }
__host__ __device__ constexpr int n1_ox0(int g) { return g < kN1Groups ? 8 * (g % 3) : 16; }
__host__ __device__ constexpr int n1_nv(int g) { return g < kN1Groups ? ((g % 3) < 2 ? 8 : 4) : 0; }

template <int STRIDE>
__global__ __launch_bounds__(256) void rnd_conv1_wgrad_kernel(const unsigned char* __restrict__ src, int64_t B, int64_t row_bytes, int off,
                                                              const int64_t* __restrict__ idx, const double* __restrict__ mean,
                                                              const double* __restrict__ sdev, const float* __restrict__ dz,
                                                              float* __restrict__ part_w,      // [grid * 4][32][64]
                                                              float* __restrict__ part_b,      // [grid * 4][32]
                                                              int images, const unsigned* __restrict__ dz_amax) {
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][kN1PlaneW];           // 43,008 bytes
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int ez = f16_scale_exp(amax_load(dz_amax, lane));
    const float sdz = f16_pow2(ez), un = f16_unscale(ez, kN1XExp);
    const int kw = li & 7, khl = li >> 3;                                // tap column; tap row within the column tile
    const unsigned shb = 16u * (unsigned)(kw >> 2);                      // tap columns 4..7 read one q further: a 16-bit funnel shift

    n1_f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    float bsum = 0.0f;
    N1Stats st;
    st.load(mean, sdev, tid);
    // every f16 of both planes is finite before the first read: the padding (q = 21 .. 31 of a line) is never written again
    for (int i = tid; i < 2 * kN1PlaneW / 2; i += 256) reinterpret_cast<unsigned*>(&xs[0][0])[i] = 0u;

    float ring[8];
    auto dz_fetch = [&](const float* gd, auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int g0 = 2 * s, g1 = 2 * s + 1;
        const int row = lh ? n1_row(g1) : n1_row(g0), ox0 = lh ? n1_ox0(g1) : n1_ox0(g0), nv = lh ? n1_nv(g1) : n1_nv(g0);
        const float* const p = gd + (row * 20 + ox0) * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j) ring[j] = j < nv ? p[j * 32] : 0.0f;      // (pixels past the row's end: zero, never loaded)
    };
    auto dz_of = [&](int im) { return dz + ((long long)im * 400 + wave * (kN1RowsPerWave * 20)) * 32 + li; };

    int img = blockIdx.x;
    if (img >= images) return;                                           // (grid <= images: never taken; uniform over the workgroup)
    dz_fetch(dz_of(img), std::integral_constant<int, 0>{});
    for (; img < images; img += gridDim.x) {
        const int nimg = img + (int)gridDim.x;
        const bool more = nimg < images;                                 // (uniform over the workgroup)
        __syncthreads();                                                 // the previous image's readers (and the zero fill) are done
        const unsigned char* const row = src + rnd_clamp_index(idx ? idx[img] : (int64_t)img, B) * row_bytes;
#pragma unroll
        for (int k = 0; k < kN1PerThread; ++k) {
            const int p = tid + 256 * k;
            if (p < kRndPixels) {
                _Float16 h, l;
                n1_split<STRIDE>(row, p, off, st.mu[k], st.sd[k], h, l);
                const int R = p / 84, c = p - 84 * R;
                const int o = R * kN1RowLds + (c & 3) * kN1Line + (c >> 2);
                xs[0][o] = h;
                xs[1][o] = l;
            }
        }
        __syncthreads();
        const float* const gd = dz_of(img);
        const float* const gdn = dz_of(more ? nimg : img);               // clamped: past the end the prefetch is never consumed

        auto step = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            constexpr int g0 = 2 * s, g1 = 2 * s + 1;
            // ---- dz operand: two f16 terms of the 8 prefetched values; bias sum
            unsigned a_hi[4], a_lo[4];
#pragma unroll
            for (int J = 0; J < 4; ++J) {
                bsum += ring[2 * J];
                bsum += ring[2 * J + 1];
                const s_f32x2 v = s_f32x2{ring[2 * J], ring[2 * J + 1]} * sdz;
                const unsigned h = __builtin_bit_cast(unsigned, __builtin_convertvector(v, s_f16x2));
                const s_f32x2 r = {f16_resid_lo(v[0], h), f16_resid_hi(v[1], h)};
                a_hi[J] = h;
                a_lo[J] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, s_f16x2));
            }
            const s_f16x8 Ah = __builtin_bit_cast(s_f16x8, (n1_u32x4){a_hi[0], a_hi[1], a_hi[2], a_hi[3]});
            const s_f16x8 Al = __builtin_bit_cast(s_f16x8, (n1_u32x4){a_lo[0], a_lo[1], a_lo[2], a_lo[3]});
            if constexpr (s + 1 < kN1Steps) dz_fetch(gd, std::integral_constant<int, s + 1>{});
            else dz_fetch(gdn, std::integral_constant<int, 0>{});
            // ---- x operand per column tile + 3 MFMAs: 10 f16 from q = ox0 (16-byte aligned) of line (4 oy + kh, kw % 4), shifted by kw / 4
            const int rw = lh ? n1_row(g1) : n1_row(g0), ox0 = lh ? n1_ox0(g1) : n1_ox0(g0);
            const int oy = wave * kN1RowsPerWave + rw;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int o = (4 * oy + 4 * t + khl) * kN1RowLds + (kw & 3) * kN1Line + ox0;
                s_f16x8 Bx[2];
#pragma unroll
                for (int term = 0; term < 2; ++term) {
                    const n1_u32x4 w = *reinterpret_cast<const n1_u32x4*>(&xs[term][o]);
                    const unsigned w4 = *reinterpret_cast<const unsigned*>(&xs[term][o + 8]);
                    Bx[term] = __builtin_bit_cast(s_f16x8, (n1_u32x4){__builtin_amdgcn_alignbit(w.y, w.x, shb), __builtin_amdgcn_alignbit(w.z, w.y, shb),
                                                                      __builtin_amdgcn_alignbit(w.w, w.z, shb), __builtin_amdgcn_alignbit(w4, w.w, shb)});
                }
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bx[0], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bx[1], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bx[0], acc[t], 0, 0, 0);
            }
        };
        step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{}); step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{}); step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
        step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});
    }

    float* pw = part_w + (size_t)(blockIdx.x * 4 + wave) * (32 * 64);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) pw[(size_t)((e & 3) + 8 * (e >> 2) + 4 * lh) * 64 + t * 32 + li] = acc[t][e] * un;
    const float both = bsum + __shfl_xor(bsum, 32, 64);
    if (lh == 0) part_b[(size_t)(blockIdx.x * 4 + wave) * 32 + li] = both;
}

// Launches the gradient kernel with `grid` workgroups (<= images): grid * 4 partials for conv_wgrad_reduce1/2 (conv.hip).
int rnd_conv1_wgrad_launch(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride, int off, const int64_t* idx, const double* mean,
                           const double* sd, const float* dz, float* part_w, float* part_b, int images, int grid, hipStream_t s,
                           const unsigned* dz_amax) {
    if (pixel_stride == 4)
        hipLaunchKernelGGL(rnd_conv1_wgrad_kernel<4>, dim3(grid), dim3(256), 0, s, src, B, row_bytes, off, idx, mean, sd, dz, part_w, part_b, images, dz_amax);
    else
        hipLaunchKernelGGL(rnd_conv1_wgrad_kernel<1>, dim3(grid), dim3(256), 0, s, src, B, row_bytes, off, idx, mean, sd, dz, part_w, part_b, images, dz_amax);
    return check_launch("rnd_conv1_wgrad_kernel");
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API int mi355ppo_rnd_conv1_fwd_f16x2(const unsigned char* src, int64_t B, int64_t row_bytes, int pixel_stride,
                                                         int64_t byte_offset, const int64_t* idx, const double* mean, const double* sd,
                                                         const void* pack, const float* bias, float* dst, uint32_t* mask_bits, uint32_t* dst_amax,
                                                         int M, double slope, void* stream) {
    const char* fn = "mi355ppo_rnd_conv1_fwd_f16x2";
    if (int rc = rnd_frame_args(fn, src, B, row_bytes, pixel_stride, byte_offset)) return rc;
    MI355_REQUIRE(mean && sd && pack && bias && dst, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(M > 0 && M <= (1 << 22) && (idx || M <= B), MI355PPO_EINVAL, "%s: M=%d must be in 1..4194304 and, without an index, at most B=%lld", fn,
                  M, (long long)B);
    MI355_REQUIRE(aligned(mean, 8) && aligned(sd, 8) && aligned(idx, 8) && aligned(pack, 16) && aligned(bias, 4) && aligned(dst, 4) &&
                  aligned(mask_bits, 4) && aligned(dst_amax, 64), MI355PPO_EALIGN,
                  "%s: mean / sd / idx must be 8-byte aligned, the pack 16-byte aligned, the amax record 64-byte aligned", fn);
    long long wgs = (long long)cu_count();                      // one 4-wave workgroup per CU (registers: a thread's 28 (mean, sd) pairs)
    if (wgs > M) wgs = M;
    const float sl = (float)slope;
    const unsigned char* const pk = static_cast<const unsigned char*>(pack);
#define MI355_N1_FWD(STRIDE_, BITS_)                                                                                                              \
    hipLaunchKernelGGL((rnd_conv1_fwd_kernel<STRIDE_, BITS_>), dim3((unsigned)wgs), dim3(256), 0, as_stream(stream), src, B, row_bytes,           \
                       (int)byte_offset, idx, mean, sd, pk, bias, dst, mask_bits, dst_amax, M, sl)
    if (pixel_stride == 4) {
        if (mask_bits) MI355_N1_FWD(4, true);
        else MI355_N1_FWD(4, false);
    } else {
        if (mask_bits) MI355_N1_FWD(1, true);
        else MI355_N1_FWD(1, false);
    }
#undef MI355_N1_FWD
    return check_launch(fn);
}
