// Kernel Q1 -- kernel Q (conv1q.hip) on ONE-channel uint8 frames: conv1(frames[inds] / 255) + bias of Conv2d(1, 32, 8, stride=4) on the
// integer matrix pipe (gfx950).  PRE: the pre-activation a LayerNorm follows, the first layer of cleanrl/pqn_atari_envpool_lstm.py's network;
// otherwise kernel Q's ReLU epilogue (ReLU, optional mask bits, amax record), the first layer of cleanrl/ppo_atari_lstm.py's.
//
// The arithmetic contract is kernel Q's, so the result is defined to the bit: weights as four signed radix-256 digits of a 31-bit fixed-point
// number on the output channel's scale (conv1q1_pack.h), inputs as v - 128 with the 128 * sum digit offsets added to the exact int32
// accumulators (|D_j| <= 64 * 128 * 128), the Horner chain over the four digit sums, * 2^(E_n-6)/255, + bias (ma_q_finish_pre / ma_q_finish, the
// functions the host twins call).  The accumulation is exact, so every summation order gives the same bits.
//
// What differs is the operand geometry.  A pixel has K = 64 bytes: 8 tap rows of 8 bytes, tap row r at byte (4 gy + r) * 84 + 4 gx of its image --
// 4-byte aligned and never more, so a row is loaded as two dwords.  One v_mfma_i32_32x32x32_i8 consumes four tap rows: a lane's 16 operand bytes
// are tap rows 4 g + 2 lh and 4 g + 2 lh + 1 of its pixel.  A 32-pixel tile is 2 x 4 matrix instructions, the digit matrices 8 KB of LDS.  The
// last tap row of the last pixel of an image ends on the image's last byte: no load reaches past it (pixels past P re-read the tile's first
// pixel).  Structure as kernel Q: persistent 4-wave workgroups, a wave owns 32-pixel x 32-channel tiles, the next tile's rows are requested
// while the current ones are consumed, the tile base travels in the stores' vector offset so that pixels past P are dropped by the buffer's
// range check.  The launch is bound by its 51,200 written bytes per image (7,056 read).
#include "common.h"
#include "conv1q1_pack.h"
#include "f16split.h"
#include "ma_atari_rows.h"

#pragma clang fp contract(off)

namespace mi355ppo {

typedef int q1_i32x4 __attribute__((ext_vector_type(4)));
typedef int q1_i32x16 __attribute__((ext_vector_type(16)));
typedef unsigned q1_u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void conv1q1_pack_kernel(const float* __restrict__ W, unsigned char* __restrict__ pack) {
    conv1q1_pack_body(W, pack);
}

// lane `l` of w := the wave-uniform value x (conv1q.hip's q_writelane)
__device__ __forceinline__ int q1_writelane(int w, unsigned x, int l) {
    asm("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(w) : "s"(x), "i"(l));      // (s_nop: two wait states behind the v_cmp that wrote x)
    return w;
}

// PRE: acc * scale + bias without the ReLU; no mask bits and no amax record (only the LayerNorm kernel reads it).
// BITS: also writes (dst > 0) as one bit per element -- word p = the 32 channels of pixel p -- as kernel Q does.
template <int NW, bool PRE, bool BITS>
__global__ __launch_bounds__(64 * NW) void conv1q1_fwd_kernel(const unsigned char* __restrict__ src, const int64_t* __restrict__ inds,
                                                              const unsigned char* __restrict__ pack, const float* __restrict__ bias,
                                                              float* __restrict__ dst, unsigned* __restrict__ bits, unsigned P, int ntiles,
                                                              unsigned dst_bytes, unsigned* __restrict__ amax) {
    static_assert(!PRE || !BITS, "the pre-activation has no ReLU mask");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    __shared__ q1_i32x4 Bl[kQ1Groups][kQDigits][64];            // digit matrices in operand layout
    {
        const q1_i32x4* __restrict__ p4 = reinterpret_cast<const q1_i32x4*>(pack);
        for (int e = tid; e < kQ1Groups * kQDigits * 64; e += 64 * NW) (&Bl[0][0][0])[e] = p4[e];
    }
    __shared__ int Cl[kQDigits + 2][32];                         // digit offsets, scale, bias per channel
    if (tid < 32) {
#pragma unroll
        for (int d = 0; d < kQDigits; ++d) Cl[d][tid] = reinterpret_cast<const int*>(pack + kQ1AccOff)[d * 32 + tid];
        Cl[kQDigits][tid] = reinterpret_cast<const int*>(pack + kQ1ScaleOff)[tid];
        Cl[kQDigits + 1][tid] = __float_as_int(bias[tid]);
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rsrc_dst = __builtin_amdgcn_make_buffer_rsrc(dst, 0, (int)dst_bytes, kQRsrcWord3);
    // word p at byte 4 p of a range of 4 P bytes: the words of pixels past P are dropped by the range check
    const __amdgpu_buffer_rsrc_t rsrc_bits = __builtin_amdgcn_make_buffer_rsrc(bits, 0, BITS ? (int)(dst_bytes >> 5) : 0, kQRsrcWord3);
    const int nwv = gridDim.x * NW;

    // pointer to tap row 2 lh of the lane's pixel of `tile` (pixels past P and tiles past the end read the first pixel of a live tile: results
    // dropped).  A 32-pixel tile touches at most two images: their rows are looked up with scalar loads, as in kernel Q.
    auto setup = [&](int tile) -> const unsigned char* {
        const int tu = __builtin_amdgcn_readfirstlane(tile);
        const bool live = tu < ntiles;
        const unsigned p0 = live ? (unsigned)tu * 32u : 0u;
        const unsigned img0 = p0 / (unsigned)kQPerImg;
        const unsigned last = (P - 1u) / (unsigned)kQPerImg;
        const unsigned img1 = img0 < last ? img0 + 1u : img0;
        const long long s0 = inds ? inds[img0] : (long long)img0;
        const long long s1 = inds ? inds[img1] : (long long)img1;
        const unsigned p = p0 + (unsigned)li;
        const unsigned pp = (live && p < P) ? p : p0;
        const unsigned img = pp / (unsigned)kQPerImg, rem = pp - img * (unsigned)kQPerImg;
        const unsigned gy = rem / (unsigned)kQG, gx = rem - gy * (unsigned)kQG;
        const long long simg = img == img0 ? s0 : s1;
        return src + simg * (long long)kQ1Img + (long long)((gy * 4u + 2u * (unsigned)lh) * (unsigned)kQ1Pitch + gx * 4u);
    };
    // the lane's two tap rows of group g: 2 x 2 dwords at 4-byte alignment, inside [row start, row start + 8)
    auto rows = [&](const unsigned char* base, int g) -> q1_u32x4 {
        const unsigned* r0 = reinterpret_cast<const unsigned*>(base + g * (4 * kQ1Pitch));
        const unsigned* r1 = reinterpret_cast<const unsigned*>(base + g * (4 * kQ1Pitch) + kQ1Pitch);
        return q1_u32x4{r0[0], r0[1], r1[0], r1[1]};
    };
    const unsigned lanebase = (unsigned)(512 * lh + 4 * li);
    unsigned vmax = 0u;                    // bits of the largest value this lane stored (>= 0 after the ReLU): dst's amax record (f16split.h)
    q1_u32x4 ring[kQ1Groups];
    int wg = blockIdx.x;                   // a contiguous range of tile groups per XCD, as kernel Q deals them
    if ((gridDim.x & 7u) == 0u) wg = (int)((blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3));
    int tile = wg * NW + wave;
    const unsigned char* nxt = setup(tile + nwv);
    {
        const unsigned char* cur = setup(tile);
#pragma unroll
        for (int g = 0; g < kQ1Groups; ++g) ring[g] = rows(cur, g);
    }
    // (kernel Q's loop entry: the first tile's rows are waited for here, so the loop's top waits for loads and not for the stores behind them)
#pragma unroll
    for (int g = 0; g < kQ1Groups; ++g) asm volatile("" : "+v"(ring[g]));

    for (; tile < ntiles; tile += nwv) {
        q1_i32x16 acc[kQDigits];
#pragma unroll
        for (int d = 0; d < kQDigits; ++d)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[d][e] = 0;
#pragma unroll
        for (int g = 0; g < kQ1Groups; ++g) {
            const q1_u32x4 t = ring[g] ^ 0x80808080u;                     // v - 128 as int8
            const q1_i32x4 a = {(int)t.x, (int)t.y, (int)t.z, (int)t.w};
#pragma unroll
            for (int d = 0; d < kQDigits; ++d) acc[d] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, Bl[g][d][lane], acc[d], 0, 0, 0);
            ring[g] = rows(nxt, g);                                       // the same rows of the wave's next tile
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue: accumulator row e of the lane is pixel (e & 3) + 8 (e >> 2) + 4 lh of the tile, column = channel li
        int acc0[kQDigits];
#pragma unroll
        for (int d = 0; d < kQDigits; ++d) acc0[d] = Cl[d][li];
        const float scale = __int_as_float(Cl[kQDigits][li]), bias_r = __int_as_float(Cl[kQDigits + 1][li]);
        // byte offset = (4096 tile + 512 lh + 4 li) + 128 ((e & 3) + 8 (e >> 2)); pixels past P lie past dst_bytes = 128 P: the buffer drops them
        const unsigned tl = (unsigned)__builtin_amdgcn_readfirstlane(tile) * 4096u + lanebase;
        int wv = 0;                                                       // BITS: lane L (< 32) collects the mask word of pixel L of the tile
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const unsigned off = tl + (unsigned)(128 * ((e & 3) + 8 * (e >> 2)));
            const int D[kQDigits] = {acc[0][e] + acc0[0], acc[1][e] + acc0[1], acc[2][e] + acc0[2], acc[3][e] + acc0[3]};
            float v;
            if constexpr (PRE) v = ma_q_finish_pre(D, scale, bias_r);
            else {
                v = ma_q_finish(D, scale, bias_r);
                vmax = __float_as_uint(v) > vmax ? __float_as_uint(v) : vmax;     // (pixels past P re-read the tile's first pixel: real values)
            }
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc_dst, off, 0, MI355_AUX_STREAM_ST);
            if constexpr (BITS) {      // ballot lanes 0..31: the 32 channels of pixel (e & 3) + 8 (e >> 2); lanes 32..63: of that pixel + 4
                const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.0f);
                wv = q1_writelane(wv, (unsigned)bal, (e & 3) + 8 * (e >> 2));
                wv = q1_writelane(wv, (unsigned)(bal >> 32), (e & 3) + 8 * (e >> 2) + 4);
            }
        }
        if constexpr (BITS)            // lane L < 32 holds the word of pixel 32 tile + L: byte 4 (32 tile + L), past 4 P dropped; lanes 32.. store nothing
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)wv, rsrc_bits, lh == 0 ? (unsigned)__builtin_amdgcn_readfirstlane(tile) * 128u + 4u * (unsigned)li : kQOob, 0, 0);
        nxt = setup(tile + 2 * nwv);
    }
    if constexpr (!PRE)
        if (amax) amax_commit(amax, vmax, blockIdx.x * NW + wave, lane);      // (uniform; one atomic per wave of the persistent grid)
}

}  // namespace mi355ppo

using namespace mi355ppo;

extern "C" MI355PPO_API size_t mi355ppo_cnn_conv1q1_pack_bytes(void) { return (size_t)kQ1PackBytes; }

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_pack(const float* W, void* pack, void* stream) {
    const char* fn = "mi355ppo_cnn_conv1q1_pack";
    MI355_REQUIRE(W && pack, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(aligned(W, 4) && aligned(pack, 16), MI355PPO_EALIGN, "%s: pack must be 16-byte aligned", fn);
    hipLaunchKernelGGL(conv1q1_pack_kernel, dim3(1), dim3(256), 0, as_stream(stream), W, static_cast<unsigned char*>(pack));
    return check_launch(fn);
}

// pre: the pre-activation; otherwise the ReLU forward (+ mask bits when given, + amax record when given)
static int conv1q1_fwd_impl(const char* fn, const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                            unsigned* bits, int64_t images, void* stream, unsigned* amax, bool pre) {
    MI355_REQUIRE(src_u8 && pack && bias && dst, MI355PPO_EINVAL, "%s: null pointer", fn);
    MI355_REQUIRE(images > 0 && images <= (1 << 22), MI355PPO_EINVAL, "%s: images=%lld out of range (1..4194304)", fn, (long long)images);
    MI355_REQUIRE(aligned(src_u8, 4) && aligned(pack, 16) && aligned(dst, 128) && aligned(inds, 8) && aligned(bias, 4) && aligned(bits, 4),
                  MI355PPO_EALIGN, "%s: src must be 4-byte aligned, pack 16-byte aligned, dst 128-byte aligned", fn);
    const long long P = (long long)images * kQPerImg, dstb = P * 128;
    MI355_REQUIRE(dstb <= (1LL << 32) - 8192, MI355PPO_EINVAL, "%s: destination of %lld bytes exceeds the 32-bit buffer range", fn, dstb);
    const int ntiles = (int)((P + 31) / 32);
    constexpr int NW = 4;
    long long wgs = (long long)cu_count() * 3;                  // kernel Q's grid at rollout sizes: three 4-wave workgroups per CU
    if (wgs * NW > ntiles) wgs = (ntiles + NW - 1) / NW;
#define MI355_Q1_LAUNCH(PRE_, BITS_)                                                                                                            \
    hipLaunchKernelGGL((conv1q1_fwd_kernel<NW, PRE_, BITS_>), dim3((unsigned)wgs), dim3(64 * NW), 0, as_stream(stream),                         \
                       static_cast<const unsigned char*>(src_u8), inds, static_cast<const unsigned char*>(pack), bias, dst, bits, (unsigned)P,  \
                       ntiles, (unsigned)dstb, amax)
    if (pre) MI355_Q1_LAUNCH(true, false);
    else if (bits) MI355_Q1_LAUNCH(false, true);
    else MI355_Q1_LAUNCH(false, false);
#undef MI355_Q1_LAUNCH
    return check_launch(fn);
}

extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_pre_fwd(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                         int64_t images, void* stream) {
    return conv1q1_fwd_impl("mi355ppo_cnn_conv1q1_pre_fwd", src_u8, inds, pack, bias, dst, nullptr, images, stream, nullptr, true);
}

// relu(conv1(src[inds] / 255) + bias) and (dst > 0) as bits: kernel Q's mi355ppo_cnn_conv1q_fwd_bits on one-channel frames.
extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_bits(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                          uint32_t* mask_bits, int64_t images, void* stream) {
    const char* fn = "mi355ppo_cnn_conv1q1_fwd_bits";
    MI355_REQUIRE(mask_bits, MI355PPO_EINVAL, "%s: null pointer", fn);
    return conv1q1_fwd_impl(fn, src_u8, inds, pack, bias, dst, mask_bits, images, stream, nullptr, false);
}

// The same (mask_bits may be null) that also folds the stored activations into `dst_amax`, dst's amax record (MI355PPO_AMAX_WORDS uint32,
// zeroed by the caller): what the f16x2 forward of layer 2 scales its A operand by.
extern "C" MI355PPO_API int mi355ppo_cnn_conv1q1_fwd_amax(const void* src_u8, const int64_t* inds, const void* pack, const float* bias, float* dst,
                                                          uint32_t* mask_bits, int64_t images, uint32_t* dst_amax, void* stream) {
    const char* fn = "mi355ppo_cnn_conv1q1_fwd_amax";
    MI355_REQUIRE(dst_amax && aligned(dst_amax, 64), MI355PPO_EINVAL, "%s: amax record missing or not 64-byte aligned", fn);
    return conv1q1_fwd_impl(fn, src_u8, inds, pack, bias, dst, mask_bits, images, stream, dst_amax, false);
}
