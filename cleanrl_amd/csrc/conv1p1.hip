// Kernel P1 -- kernel P's F16 mode (conv1p.hip) on ONE-channel uint8 frames: weight + bias gradient of Conv2d(1, 32, 8, stride=4), the first
// layer of cleanrl/pqn_atari_envpool_lstm.py's network (gfx950).
//
// dW1[n][kh][kw] = sum over images and output pixels p = (oy, ox) of dz1[p][n] * frame[4 oy + kh][4 ox + kw]  (the 1 / 255 is applied once to
// the reduced sum), db1[n] = sum dz1[p][n].  Arithmetic class of kernel P's F16 mode and nothing looser: dz in two f16 terms under its amax
// record's power-of-two scale (f16split.h), the frame bytes zero-extended to subnormal f16 (0x00vv = v * 2^-24, multiplied exactly by gfx950's
// f16 MFMA), f32 accumulation; the wave takes the factor s * 2^-24 (a power of two) off when it stores its partial.
//
// Roles in one v_mfma_f32_32x32x16_f16: rows = the 32 output channels, columns = 32 of the 64 taps (column tile t: kh = 4 t + li / 8,
// kw = li % 8), the 16 reduction slots = two groups of 8 horizontally adjacent output pixels (slots 0-7 from the lower half-wave's group, 8-15
// from the upper one's).  2 column tiles x 2 terms = 4 matrix instructions per 16 pixels; dW (2 x 16 VGPRs) stays in the wave's accumulators
// for the life of the kernel.
//
// A workgroup walks images; wave w owns output rows 5 w .. 5 w + 4 of each (kernel P's partition): 15 pixel groups (3 per output row: pixels
// 0-7, 8-15, 16-19 + 4 padding slots whose dz is forced to zero) in 8 steps.  The frame operand of a tap over 8 adjacent output pixels is a
// stride-4 byte sequence of an 84-byte row, so the workgroup stages the image in LDS split by x mod 4: line (source row R, t) holds the bytes of
// x = 4 q + t, q = 0 .. 20 (21 bytes of payload in a 32-byte line), and pixels ox0 .. ox0 + 7 of tap column kw are 8 consecutive bytes starting at
// q = ox0 + kw / 4 of line (4 oy + kh, kw % 4).  Two LDS images: the next image's dwords are requested in front of the current image's steps and
// written into the other buffer behind them, one barrier per image; a lane's dz (8 coalesced dword loads per step) is requested one step ahead.
// The frame is read as aligned dwords (7,056 bytes = 1,764 dwords), nothing outside it.  Padding bytes of a line are never initialised: every
// byte pattern is a finite f16 subnormal and meets a zero dz term.
// Partials: one (32 x 64) matrix + 32 bias sums per wave, folded in a fixed order by conv_wgrad_reduce1/2 (conv.hip): no float atomics.
#include "common.h"
#include "f16split.h"

#pragma clang fp contract(off)

namespace mi355ppo {

typedef float p1_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int p1_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kP1Img = 84 * 84, kP1Dwords = kP1Img / 4;                     // bytes / dwords per frame
constexpr int kP1Line = 32;                                                // bytes per (R, t) line: q = 0..20 payload (+ slack for the shifted read)
constexpr int kP1RowLds = 4 * kP1Line;                                     // 128 bytes of LDS per source row
constexpr int kP1ImgLds = 84 * kP1RowLds;                                  // 10,752 bytes per staged image
constexpr int kP1RowsPerWave = 5, kP1Steps = 8, kP1Groups = 15;

// group g of a wave's 5 output rows -> (output row, first pixel, valid pixels); g = 15 is the empty 16th slot
__host__ __device__ constexpr int p1_row(int g) { return g < kP1Groups ? g / 3 : kP1RowsPerWave - 1; }
__host__ __device__ constexpr int p1_ox0(int g) { return g < kP1Groups ? 8 * (g % 3) : 16; }
__host__ __device__ constexpr int p1_nv(int g) { return g < kP1Groups ? ((g % 3) < 2 ? 8 : 4) : 0; }

__global__ __launch_bounds__(256) void conv1p1_wgrad_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ inds,
                                                            const float* __restrict__ dz,
                                                            float* __restrict__ part_w,      // [grid * 4][32][64]
                                                            float* __restrict__ part_b,      // [grid * 4][32]
                                                            int images, const unsigned* __restrict__ dz_amax) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[2][kP1ImgLds];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int ez = f16_scale_exp(amax_load(dz_amax, lane));
    const float sdz = f16_pow2(ez), un = f16_pow2(24 - ez);              // ez in [-100, 60]: 2^-36 .. 2^124
    const int kw = li & 7, khl = li >> 3;                                // tap column; tap row within the column tile
    const unsigned sh = (unsigned)(kw >> 2);                             // tap columns 4..7 read one q further
    // v_perm selectors (0x0c = the constant byte 0): elements (sh, sh + 1) and (sh + 2, sh + 3) of an 8-byte window, zero-extended
    const unsigned sel0 = 0x0c000c00u | ((sh + 1u) << 16) | sh, sel1 = 0x0c000c00u | ((sh + 3u) << 16) | (sh + 2u);

    p1_f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    float bsum = 0.0f;

    auto row_of = [&](int img) { return inds ? inds[img] : (long long)img; };
    // the whole workgroup: frame (aligned dwords = pixels x = 4 q .. 4 q + 3 of a source row) -> registers -> the four lines of that row.  The loads
    // of the NEXT image are issued in front of the current image's steps and written behind them, so their latency is not waited out.
    constexpr int kStageRegs = (kP1Dwords + 255) / 256;                  // 7 dwords per thread (the last one of threads 0 .. 227 only)
    unsigned st[kStageRegs];
    auto stage_load = [&](long long simg) {
        const unsigned* __restrict__ g = reinterpret_cast<const unsigned*>(src + simg * (long long)kP1Img);
#pragma unroll
        for (int k = 0; k < kStageRegs; ++k) {
            const int i = tid + 256 * k;
            st[k] = i < kP1Dwords ? g[i] : 0u;
        }
    };
    auto stage_store = [&](unsigned char* buf) {
#pragma unroll
        for (int k = 0; k < kStageRegs; ++k) {
            const int i = tid + 256 * k;
            if (i < kP1Dwords) {
                const int R = i / 21, q = i - 21 * R;
                unsigned char* const base = buf + R * kP1RowLds + q;
#pragma unroll
                for (int t = 0; t < 4; ++t) base[t * kP1Line] = (unsigned char)(st[k] >> (8 * t));
            }
        }
    };
    // dz of step s of the image at gd: the lane's channel over its group's 8 pixels, one step ahead of its use (pixels past the row's end:
    // zero, never loaded -- nothing is read outside the image)
    float ring[8];
    auto dz_fetch = [&](const float* gd, auto sc) {
        constexpr int s = decltype(sc)::value;
        constexpr int g0 = 2 * s, g1 = 2 * s + 1;
        const int row = lh ? p1_row(g1) : p1_row(g0), ox0 = lh ? p1_ox0(g1) : p1_ox0(g0), nv = lh ? p1_nv(g1) : p1_nv(g0);
        const float* const p = gd + (row * 20 + ox0) * 32;
#pragma unroll
        for (int j = 0; j < 8; ++j) ring[j] = j < nv ? p[j * 32] : 0.0f;
    };
    auto dz_of = [&](int im) { return dz + ((long long)im * 400 + wave * (kP1RowsPerWave * 20)) * 32 + li; };

    int img = blockIdx.x;
    if (img >= images) return;                                           // (grid <= images: never taken; uniform over the workgroup)
    stage_load(row_of(img));
    stage_store(stage[0]);
    __syncthreads();
    dz_fetch(dz_of(img), std::integral_constant<int, 0>{});
    int cur = 0;
    for (; img < images; img += gridDim.x) {
        const int nimg = img + (int)gridDim.x;
        const bool more = nimg < images;                                 // (uniform over the workgroup)
        if (more) stage_load(row_of(nimg));
        const unsigned char* const tt = stage[cur];
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
            const p1_u32x4 ah = {a_hi[0], a_hi[1], a_hi[2], a_hi[3]}, al = {a_lo[0], a_lo[1], a_lo[2], a_lo[3]};
            const s_f16x8 Ah = __builtin_bit_cast(s_f16x8, ah), Al = __builtin_bit_cast(s_f16x8, al);
            // prefetch the next step's dz (the next image's first step at the end)
            if constexpr (s + 1 < kP1Steps) dz_fetch(gd, std::integral_constant<int, s + 1>{});
            else dz_fetch(gdn, std::integral_constant<int, 0>{});
            // ---- frame operand per column tile + 2 MFMAs: 12 bytes at q = ox0 (8-byte aligned) of line (4 oy + kh, kw % 4), shifted by kw / 4
            const int row = lh ? p1_row(g1) : p1_row(g0), ox0 = lh ? p1_ox0(g1) : p1_ox0(g0);
            const int oy = wave * kP1RowsPerWave + row;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned char* const lp = tt + (4 * oy + 4 * t + khl) * kP1RowLds + (kw & 3) * kP1Line + ox0;
                const uint2 w01 = *reinterpret_cast<const uint2*>(lp);
                const unsigned w2 = *reinterpret_cast<const unsigned*>(lp + 8);
                const p1_u32x4 bz = {__builtin_amdgcn_perm(w01.y, w01.x, sel0), __builtin_amdgcn_perm(w01.y, w01.x, sel1),
                                     __builtin_amdgcn_perm(w2, w01.y, sel0), __builtin_amdgcn_perm(w2, w01.y, sel1)};
                const s_f16x8 Bz = __builtin_bit_cast(s_f16x8, bz);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah, Bz, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al, Bz, acc[t], 0, 0, 0);
            }
        };
        step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{}); step(std::integral_constant<int, 2>{});
        step(std::integral_constant<int, 3>{}); step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
        step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});
        if (more) stage_store(stage[cur ^ 1]);                           // (the other buffer's last readers passed the previous barrier)
        __syncthreads();                                                 // the next image is staged; this one's readers are done
        cur ^= 1;
    }

    float* pw = part_w + (size_t)(blockIdx.x * 4 + wave) * (32 * 64);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) pw[(size_t)((e & 3) + 8 * (e >> 2) + 4 * lh) * 64 + t * 32 + li] = acc[t][e] * un;
    const float both = bsum + __shfl_xor(bsum, 32, 64);
    if (lh == 0) part_b[(size_t)(blockIdx.x * 4 + wave) * 32 + li] = both;
}

// Launches kernel P1 with `grid` workgroups (<= images): grid * 4 partials, the factor 1 / 255 left for the reduction.
int conv1p1_launch(const unsigned char* src, const int64_t* inds, const float* dz, float* part_w, float* part_b, int images, int grid,
                   hipStream_t s, const unsigned* dz_amax) {
    hipLaunchKernelGGL(conv1p1_wgrad_kernel, dim3(grid), dim3(256), 0, s, src, inds, dz, part_w, part_b, images, dz_amax);
    return check_launch("conv1p1_wgrad_kernel");
}

}  // namespace mi355ppo
