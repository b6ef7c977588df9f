// Kernel RS -- the layer-2 forward of the NatureCNN (cleanrl/ppo_atari_multigpu.py:141) with the source of an image group STREAMED through LDS by
// stride-parity class (round 7).  Kernel R's structure (convr.hip: the source split once into f16 hi / lo records in LDS, every fragment one
// ds_read_b128 at the lane's window origin + a compile-time offset, the weights from the f16x2 pack through the workgroup's two-buffer LDS ring by
// LDS-DMA, kernel Z's epilogue) with the geometry of convrs_geom.h:
//   * the k-steps run in kernel R's ORDER 2 -- four phases of 8 k-steps, phase g = the taps of row parity g >> 1 and column parity g & 1 --, and a stride-2
//     tap reads only pixels of its own parity: phase g needs only CLASS g of the source, one quarter.  Two class buffers of 43.6 KB replace the 121 KB
//     of kernel R's whole two-image source: phase g multiplies from buffer g & 1 while the waves split class g + 1 and write it into the other buffer,
//     one round (16 bytes per lane) in each of five of the phase's eight k-steps, and request class g + 2 into the registers the round has just freed
//     (20 registers in flight).  The pipeline runs across the group boundary -- class 0 of the next group is written during phase 3 --, so there is
//     no fill phase: a group begins with its first class resident;
//   * THREE images per group: 243 rows in eight 32-row tiles (95 % of the slots; kernel R: 162 rows in six tiles, 84 %), eight waves -- two per
//     SIMD --, each one row tile against both column tiles: 2 pixel + 4 weight fragment reads per 6 matrix instructions (kernel R: 4 per 3);
//   * per group, every 128-byte line of a1 is still read exactly once: a class row is ten 128-byte pieces at a 256-byte stride.
// Arithmetic: kernel R's, i.e. kernel Z's SPLIT = 1 instance's -- every output element sees the same k-steps in the same order, per step hi hi, hi lo,
// lo hi into one accumulator, the same split under the same scale, the same epilogue: bit-identical output, mask words and amax record
// (tests/test_gpu_conv2_stream.py).  Which slot a row sits in does not enter the result.
#include "conv_resident.h"
#include "convrs_geom.h"

#pragma clang fp contract(off)

namespace mi355ppo {

// one unit of a class into its record: hi half at `addr`, lo half 64 bytes on (ds_write2_b64).  In assembly on purpose: behind a compiler-visible LDS store the
// compiler waits for every LDS-DMA piece in flight (it cannot tell the ring from the class buffers) -- the weight ring's one slot of distance would be gone.  The
// stores are counted by the explicit lgkmcnt(0) in front of every barrier; an LDS operation the compiler does not know of only makes its own counted waits stricter.
__device__ __forceinline__ void rs_put16(unsigned addr, unsigned long long hi, unsigned long long lo) {
    asm volatile("ds_write2_b64 %0, %1, %2 offset1:8" : : "v"(addr), "v"(hi), "v"(lo) : "memory");
}

struct RSArgs {
    const float* A;             // a1 (images, 20, 20, 32)
    unsigned a_bytes;
    const unsigned char* pack;  // f16x2 pack of the weights (header + [k-step][tile][hi, lo][lane][8 f16])
    const float* bias;
    unsigned* bits_out;         // BITS: the ReLU mask of a2, one bit per element
    float* C;                   // a2 (images, 9, 9, 64)
    unsigned c_bytes;
    long long images;
    int groups;
    const unsigned* a_amax;     // amax record of a1
    unsigned* c_amax;           // amax record of a2 to fold into, or null
};

// vector loads a wave issues behind the LDS-DMA pieces of ring slot `slot` + 1 (requested at the slot's first step, in front of that step's source round) and in
// front of its wait (top of the slot's last step): the source rounds of the slot's steps but the last (convr.hip's r_dma_younger)
constexpr int rs_dma_younger(int slot) {
    using RG = RSGeom;
    int n = 0;
    for (int r = 0; r < RG::NI; ++r) {
        const int w = RG::round_step(r), lo = (slot * RG::SS) % RG::PSTEPS;
        n += (w >= lo && w < lo + RG::SS - 1) ? 1 : 0;
    }
    return n;
}

template <bool BITS>
__global__ __launch_bounds__(RSGeom::THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void rs_kernel(RSArgs a) {
    using RG = RSGeom;
    constexpr int NT = RG::NT, NW = RG::NW, NI = RG::NI, THREADS = RG::THREADS, SS = RG::SS, NSLOT = RG::KSTEPS / SS, PSTEPS = RG::PSTEPS;
    constexpr int kPieces = SS * NT * 2;                  // KiB pieces of a ring slot: (step h of the slot, tile j, term t), x = (h NT + j) 2 + t
    constexpr int kShare = kPieces / NW;                  // every wave moves kShare pieces of a slot
    static_assert(kPieces % NW == 0 && NSLOT % 2 == 0, "whole pieces per wave; the next group's slot 0 goes to buffer 0 while the last slot is read from buffer 1");
    __shared__ __attribute__((aligned(16))) unsigned char lds[RG::LDSB];
    unsigned char* const ring = lds + RG::ABYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;

    const int ea = f16_scale_exp(amax_load(a.a_amax, lane));
    const int eb = f16_scale_exp(*reinterpret_cast<const unsigned*>(a.pack));
    const float sa = f16_pow2(ea), un = f16_unscale(ea, eb);

    // ---- rows of a group.  Slot wave 32 + x holds row table.row[...] of the group (empty slots repeat a row of their sixteen-lane set: the same values
    // stored twice).  A-fragment reads: lane -> slot x = lane % 32.  Epilogue: accumulator e -> slot x = (e & 3) + 8 (e >> 2) + 4 lh; `roff[e >> 1]` =
    // two 16-bit byte offsets of those rows' first channel in C from the group's base (+ the lane's channel; a group's C is 62,208 bytes).
    constexpr RRowTable<RG> table{};
    auto row_pixel = [&](int slot, int& gi, int& gy, int& gx) __attribute__((always_inline)) {
        const int rc = table.src[slot];
        gi = rc / RG::OP;
        const int pp = rc - gi * RG::OP;
        gy = pp / RG::OW; gx = pp - gy * RG::OW;
    };
    constexpr unsigned kGroupC = RG::G * RG::OP * 32 * NT * 4;      // bytes of C per group
    static_assert(kGroupC < 65536, "two row offsets per register");
    const unsigned char* win;                             // window origin of the lane's fragment row in class buffer 0 (+ the lane half's 8 channels)
    unsigned roff[8], rword;                              // rword: C offset of slot row li (mask words out)
    {
        int gi, gy, gx;
        row_pixel(wave * 32 + li, gi, gy, gx);
        win = lds + (gi * RG::IP + RG::pidx(gy, gx)) * RG::PIX + 16 * lh;
        rword = (unsigned)((gi * RG::OP + gy * RG::OW + gx) * (32 * NT)) * 4u;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            row_pixel(wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh, gi, gy, gx);
            const unsigned o = (unsigned)((gi * RG::OP + gy * RG::OW + gx) * (32 * NT)) * 4u + 4u * (unsigned)li;
            roff[e >> 1] = (e & 1) ? (roff[e >> 1] | (o << 16)) : o;
        }
    }
    const unsigned char* const ring_r = ring + 16 * lane;

    // ---- the source, class by class: unit u = 16 bytes = 4 channels of a class pixel; thread tid takes units r THREADS + tid of every class (round r).
    // usrc: the unit's byte offset in the group's a1 for class 0 (class (py, px): + (py IW + px) 128, an immediate); udst: the byte offset of its hi
    // half in a class buffer (lo: + RG::LO).  Units past the class (round 4, threads 352 ..): loaded from nowhere (zeros), written to the spare record.
    unsigned usrc[NI], udst[NI];
#pragma unroll
    for (int r = 0; r < NI; ++r) {
        const int u = r * THREADS + tid;
        const int c4 = u % RG::UPP, j = (u / RG::UPP) % RG::CW, i = (u / (RG::UPP * RG::CW)) % RG::CH, img = u / (RG::UPP * RG::CW * RG::CH);
        const bool ok = u < RG::CUNITS;
        usrc[r] = ok ? (unsigned)(img * RG::IMG_SRC + (2 * i * RG::IW + 2 * j) * (RG::IC * 4) + c4 * 16) : kResOob;
        udst[r] = ok ? (unsigned)((img * RG::IP + i * RG::RP + j) * RG::PIX + c4 * 8) : (unsigned)(RG::SPARE * RG::PIX + c4 * 8);
    }
    // a1's descriptor of a group starts AT the group: the per-unit offsets are then lane constants + an immediate; the range shrinks with the base, so units of
    // images past the batch fall out of it and load zeros without touching memory (their rows are never stored), and a group past the last has no range at all --
    // the loads are issued unconditionally (loads behind a branch leave the compiler without a count of the outstanding ones: convr.hip)
    auto rsrc_a_of = [&](int g) __attribute__((always_inline)) {
        const bool ok = g < a.groups;
        const unsigned gb = (unsigned)g * (unsigned)RG::GROUP_SRC;
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>(const_cast<float*>(a.A)) + (ok ? gb : 0u), 0, ok ? (int)(a.a_bytes - gb) : 0, kResRsrcWord3);
    };
    const unsigned lds_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;      // LDS byte address of class buffer 0
    static_assert(RG::LO == 64, "rs_put16: the lo half one ds_write2_b64 stride (8 x 8 bytes) behind the hi half");
    s_u32x4 pre[NI];                                      // round r of the class after the one being written
    auto get = [&](const __amdgpu_buffer_rsrc_t ra, int cls, int r) __attribute__((always_inline)) {
        pre[r] = __builtin_bit_cast(s_u32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, usrc[r] + (unsigned)(((cls >> 1) * RG::IW + (cls & 1)) * (RG::IC * 4)), 0, MI355_AUX_STREAM_LD));
    };
    auto put = [&](int buf, int r) __attribute__((always_inline)) {
        unsigned hi[2], lo[2];
        f16_split4(pre[r], sa, hi, lo);
        rs_put16(lds_base + (unsigned)(buf * RG::BUFB) + udst[r], ((unsigned long long)hi[1] << 32) | hi[0], ((unsigned long long)lo[1] << 32) | lo[0]);
    };

    // ---- epilogue constants
    // C's descriptor of a group starts AT the group: the per-value offsets are lane constants + an immediate, and rows of images past the batch fall out of its
    // range -- stores dropped (a scalar offset would not be checked)
    auto rsrc_c_of = [&](unsigned gbase) __attribute__((always_inline)) {
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>(a.C) + gbase, 0, (int)(a.c_bytes - gbase), kResRsrcWord3);
    };
    const __amdgpu_buffer_rsrc_t rsrc_b = __builtin_amdgcn_make_buffer_rsrc(BITS ? a.bits_out : nullptr, 0, BITS ? (int)(a.c_bytes >> 5) : 0, kResRsrcWord3);
    float bj[NT];                                         // the lane's bias element per column tile
#pragma unroll
    for (int j = 0; j < NT; ++j) bj[j] = a.bias[32 * j + li];
    float cmax = 0.0f;

    // ---- the weights' ring (convr.hip): slot s = the visited k-steps SS s .. SS s + SS - 1, two buffers, filled by LDS-DMA.  Slot s + 1 is requested at the first
    // step of slot s into the buffer every wave read for the last time before the barrier of slot s - 1; slot NSLOT = the next group's slot 0.  The issuing wave
    // waits for ITS pieces in front of the barrier at the last step of slot s (the last slot: in front of the epilogue; the barrier is the next group's first):
    // vmcnt counts in order, so "all but the rs_dma_younger(s) source rounds issued behind the pieces".
    const __amdgpu_buffer_rsrc_t rsrc_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.pack), 0, kF16PackHeader + RG::KSTEPS * RG::STEPB, kResRsrcWord3);
    auto dma_slot = [&](int slot) __attribute__((always_inline)) {                       // -> buffer slot & 1
#pragma unroll
        for (int u = 0; u < kShare; ++u) {
            const int x = wave * kShare + u, h = x / (NT * 2), jt = x - h * (NT * 2);
            res_dma16(rsrc_p, ring + (slot & 1) * RG::SLOTB + x * 1024, 16u * (unsigned)lane, kF16PackHeader + r_kstep<RG>(SS * (slot % NSLOT) + h) * RG::STEPB + jt * 1024);
        }
    };

    res_f32x16 acc[NT];
    int wv = 0;                                           // BITS: lane L (< 32) collects the mask word of slot row L of the tile in flight
    s_u32x4 pa[2][2], wb[2][NT][2];                       // [k-step parity]: pixel fragment [hi, lo]; weight fragments [tile][hi, lo]
    auto read_a = [&](int par, int v) __attribute__((always_inline)) {
        const int off = (rs_class(v) & 1) * RG::BUFB + rs_tapoff(r_kstep<RG>(v));
        pa[par][0] = *reinterpret_cast<const s_u32x4*>(win + off);
        pa[par][1] = *reinterpret_cast<const s_u32x4*>(win + off + RG::LO);
    };
    auto read_b = [&](int par, int v) __attribute__((always_inline)) {                   // step v = step v % SS of slot v / SS
        const int buf = (v / SS) & 1, h = v % SS;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int t = 0; t < 2; ++t) wb[par][j][t] = *reinterpret_cast<const s_u32x4*>(ring_r + buf * RG::SLOTB + ((h * NT + j) * 2 + t) * 1024);
    };
    // ---- epilogue (kernel Z's), one value: accumulator e of column tile j = row slot (e & 3) + 8 (e >> 2) + 4 lh, channel 32 j + li.  Values of one j come
    // in the order e = 0 .. 15 (the mask word is assembled across them).
    auto epi_elem = [&](int j, int e, unsigned gbase, const __amdgpu_buffer_rsrc_t rc) __attribute__((always_inline)) {
        asm volatile("" : "+v"(roff[e >> 1]));            // (opaque in place: the store's column-tile offset stays an immediate -- convr.hip)
        const unsigned rpk = roff[e >> 1];
        const unsigned ro = ((e & 1) ? rpk >> 16 : rpk & 0xffffu) + (unsigned)(128 * j);
        float v = __builtin_fmaf(acc[j][e], un, bj[j]);                       // (un is a power of two: the product is exact, the fused form rounds as mul + add did)
        v = v < 0.0f ? 0.0f : v;                                              // (a NaN stays a NaN, as kernel Z's SPLIT epilogue)
        cmax = __builtin_fmaxf(cmax, __builtin_fabsf(v));                     // (rows past the batch: relu(bias) of a real channel, or a value some real row has)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, ro, 0, MI355_AUX_STREAM_ST);
        if constexpr (BITS) {                             // lanes 0..31 of the ballot: the 32 channels of slot row (e & 3) + 8 (e >> 2); 32..63: of that row + 4
            if (e == 0) wv = 0;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(v > 0.0f);
            wv = res_writelane(wv, (unsigned)bal, (e & 3) + 8 * (e >> 2));
            wv = res_writelane(wv, (unsigned)(bal >> 32), (e & 3) + 8 * (e >> 2) + 4);
            if (e == 15) __builtin_amdgcn_raw_buffer_store_b32((unsigned)wv, rsrc_b, lh == 0 ? (gbase + rword + (unsigned)(128 * j)) >> 5 : kResOob, 0, 0);
        }
    };
    static_assert(RG::round_step(NI - 1) < PSTEPS - 1, "a class is written before the barrier at its phase's last step");
    auto group = [&](int grp) __attribute__((always_inline)) {
        const unsigned gbase = (unsigned)grp * kGroupC;
        const __amdgpu_buffer_rsrc_t ra_cur = rsrc_a_of(grp), ra_next = rsrc_a_of(grp + (int)gridDim.x);
        // every wave is done with the previous group's last class buffer and ring slot; class 0 and ring slot 0 of this group have been written
        res_ring_barrier();
        read_a(0, 0);
        read_b(0, 0);
#pragma unroll
        for (int v = 0; v < RG::KSTEPS; ++v) {
            const int q = v & 1, slot = v / SS, h = v % SS, g = v / PSTEPS, w = v % PSTEPS;
            // the operands of step v + 1 are requested before the matrix instructions of step v go out
            if (h == SS - 1) res_wait_vmcnt(rs_dma_younger(slot));      // this wave's pieces of slot + 1 have landed
            if (v + 1 < RG::KSTEPS) {
                if (h == SS - 1) res_ring_barrier();          // ... everybody's; phase ends (w == PSTEPS - 1): class g + 1 is written, nobody reads class g - 1's buffer any more
                read_b(q ^ 1, v + 1);
                read_a(q ^ 1, v + 1);
            }
            if (h == 0) {
                dma_slot(slot + 1);
                __builtin_amdgcn_sched_barrier(0);        // (rs_dma_younger assumes the pieces are issued in front of this step's source round)
            }
            // the source: round r of class g + 1 (phase 3: class 0 of the workgroup's next group) leaves its registers for the buffer phase g does not read, and
            // round r of class g + 2 is requested into them -- one round per step keeps the request rate near what arrives (convr.hip, pre_lo)
#pragma unroll
            for (int r = 0; r < NI; ++r)
                if (w == RG::round_step(r)) {
                    put((g + 1) & 1, r);
                    get(g + 2 < RG::PHASES ? ra_cur : ra_next, (g + 2) % RG::PHASES, r);
                }
            __builtin_amdgcn_sched_barrier(0);
            // hi hi, hi lo (weights), lo hi (pixels): kernel Z's order of the three term pairs, tiles innermost
#pragma unroll
            for (int pi = 0; pi < 3; ++pi)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    if (v == 0 && pi == 0) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;      // (the MFMA's inline zero)
                    }
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(s_f16x8, pa[q][pi == 2 ? 1 : 0]),
                                                                    __builtin_bit_cast(s_f16x8, wb[q][j][pi == 1 ? 1 : 0]), acc[j], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the group's values (kernel Z's epilogue order for the forward's mask words: tiles outermost).  The source rounds in flight (class 1 of the next group) are
        // older than the stores: their waits count the stores as younger and do not wait for them.
        const __amdgpu_buffer_rsrc_t rc = rsrc_c_of(gbase);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) epi_elem(j, e, gbase, rc);
    };

    int grp = blockIdx.x;
    if (grp < a.groups) {                                 // (every workgroup of the launch: grid <= groups)
        const __amdgpu_buffer_rsrc_t ra = rsrc_a_of(grp);
#pragma unroll
        for (int r = 0; r < NI; ++r) get(ra, 0, r);
        dma_slot(0);
        __builtin_amdgcn_s_waitcnt(kResWaitVm0);
#pragma unroll
        for (int r = 0; r < NI; ++r) {
            put(0, r);
            get(ra, 1, r);
        }
        // (the loop is entered as the back edge enters it in one respect: no round is in flight that has FEWER loads and stores behind it than on the back edge --
        //  the compiler's wait for a round is counted for the worse of the two entries, and "five loads behind class 1's first round" there would make every group
        //  wait at its first step until all but five of the previous group's stores are acknowledged.  One trip to memory per workgroup and launch.)
        __builtin_amdgcn_s_waitcnt(kResWaitVm0);
    }
    for (; grp < a.groups; grp += gridDim.x) group(grp);
    if (a.c_amax) amax_commit(a.c_amax, __float_as_uint(cmax), blockIdx.x * NW + (unsigned)wave, lane);
}

// Which sizes kernel RS takes from kernel R's layer-2 forward (MI355PPO_CONV_RS through common.h::kernel_switch: 0 = never, min:<n> = from n images on).
bool convrs_takes(long long images) { return kernel_switch("MI355PPO_CONV_RS", images, MI355_RS_MIN_IMAGES); }

int convrs_fwd2(const char* fn, const float* src, unsigned src_bytes, const void* pack, const float* bias, float* dst, unsigned dst_bytes, unsigned* bits,
                long long images, const unsigned* src_amax, unsigned* dst_amax, hipStream_t st) {
    RSArgs a = res_args<RSArgs>(src, src_bytes, pack, dst, dst_bytes, images, src_amax, dst_amax);
    a.bias = bias; a.bits_out = bits;
    return res_launch(bits ? rs_kernel<true> : rs_kernel<false>, a, RSGeom::G, 1, RSGeom::THREADS, st, fn);
}

}  // namespace mi355ppo
