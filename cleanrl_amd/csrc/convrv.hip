// Kernel RV -- the layer-3 data gradient of the NatureCNN (the backward of cleanrl/ppo_atari_multigpu.py:142, `loss.backward()` :358) with SEVEN
// images per group and the rows of a group dealt to tiles BY VERTICAL BORDER CLASS (round 8).  Kernel R's structure (convr.hip: the group's dz3
// resident in LDS as f16 hi / lo records, split once; weights from the f16x2 pack through the workgroup's two-buffer LDS ring; kernel Z's
// epilogue) and kernel RB's shape of a wave (convrb.hip) with the geometry of convrv_geom.h:
//   * a tile holds rows of ONE output row class (y = 0 | 1 | 2..6 | 7 | 8), so no tap it multiplies reads above or below its image: the source
//     has no zero lines, only two zero records in front of every line of seven pixels -- 443 records, 120,496 B, for seven images;
//   * 567 rows in 18 tiles; a ring slot is one tap, and a tile multiplies only the tap rows its class can see: 3,024 matrix instructions per
//     seven images, 432 per image against kernel R's 576 -- the skipped products are exact zeros in kernel R / Z;
//   * 8 waves: SIMD s = wave % 4 holds c tiles 2 s, 2 s + 1 and a pair of border tiles with complementary tap rows ({d, a}: SIMDs 0, 1; {e, b}:
//     SIMDs 2, 3), its two waves take column tile 0 / column tile 1 of those, and one of the two also takes its column half of c tile 8 + s / 2
//     (kernel template parameter XC, chosen per wave at the top of the kernel: the whole persistent loop exists in both forms).  In every k-step a
//     wave with the extra half issues 4 tiles x 3 term pairs = 12 matrix instructions (kernel RB's shape: 80 accumulator registers), its partner
//     9: 21 per SIMD and k-step on all four SIMDs;
//   * the border accumulators: code is the same for all waves -- accumulator 2 in ring slots 0 .. 5, accumulator 3 in slots 6 .. 8, which is
//     {d, a}'s schedule; the {e, b} waves SWAP the two in front of slots 3 and 6 (kernel RB's device: 2 x 32 register moves per group);
//   * nine ring slots: the buffer a slot lives in alternates from group to group (`gpar`), the lane's two ring addresses change places;
//   * pixel fragments single-buffered (a pair of tiles' fragments for step v + 1 is requested right behind that pair's matrix instructions of
//     step v), weight fragments double-buffered, the epilogue's row offsets from a 2.25-KB table in LDS -- as kernel RB.
// Arithmetic: per accumulator the products of kernel Z's SPLIT = 1 instance in its order (k-steps ascending, per step hi hi, hi lo, lo hi) minus
// products of tap rows outside the image (zero operands): bit-identical results (tests/test_gpu_conv3_dgrad_classes.py).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 216 VGPRs, no AGPRs, 80 SGPRs, no scratch, no spills, 155,568 B of LDS, two waves per SIMD.
// Measured: profiles/r08_conv3_dgrad_classes_ab.txt (479 -> 403 us per launch at 32,768 images).
#include "conv_resident.h"
#include "convrv_geom.h"

#pragma clang fp contract(off)

namespace mi355ppo {

struct RVArgs {
    const float* A;             // dz3 (images, 7, 7, 64)
    unsigned a_bytes;
    const unsigned char* pack;  // f16x2 pack of the flipped taps (header + [k-step][column tile][hi, lo][lane][8 f16])
    const unsigned* bits_in;    // ReLU mask of a2, one bit per element of (images, 9, 9, 64)
    float* C;                   // da2 (images, 9, 9, 64)
    unsigned c_bytes;
    long long images;
    int groups;
    int grid;                   // workgroups of the launch (the group stride)
    const unsigned* a_amax;     // amax record of dz3
    unsigned* c_amax;           // amax record of da2 to fold into, or null
};

// the persistent loop of one wave; XC = 1: the wave also holds its column half of c tile 8 + simd / 2 (accumulator 4)
template <int XC>
__device__ __forceinline__ void rv_wave(const RVArgs& a, unsigned char* const lds, const int tid, const int wave) {
    using RG = RVGeom;
    constexpr int NT = RG::NT, NW = RG::NW, NI = RG::NI, THREADS = RG::THREADS, SS = RG::SS, NSLOT = RG::NSLOT;
    constexpr int MT = 4 + XC, NWM = (MT + 1) / 2;        // accumulator tiles; registers of mask words (64 wave rows each)
    constexpr int kPieces = SS * NT * 2;                  // KiB pieces of a ring slot: (step h of the slot, column tile j, term t), x = (h NT + j) 2 + t
    constexpr int kShare = kPieces / NW;                  // every wave moves kShare pieces of a slot
    static_assert(kPieces % NW == 0, "whole pieces per wave");
    unsigned char* const ring = lds + RG::ABYTES;
    unsigned* const rofft = reinterpret_cast<unsigned*>(lds + RG::ABYTES + 2 * RG::SLOTB);
    const int lane = tid & 63, li = lane & 31, lh = lane >> 5;
    const int simd = wave & 3, jc = wave >> 2;             // RG::simd_of, RG::col_of (wave-uniform)
    auto tile_of = [&](int i) __attribute__((always_inline)) -> int {      // RG::wave_tile
        return i < 2 ? 2 * simd + i : (i == 2 ? 10 + simd : (i == 3 ? 14 + simd : 8 + (simd >> 1)));
    };

    const int ea = f16_scale_exp(amax_load(a.a_amax, lane));
    const int eb = f16_scale_exp(*reinterpret_cast<const unsigned*>(a.pack));
    const float sa = f16_pow2(ea), un = f16_unscale(ea, eb);

    // ---- rows: LDS byte offset of the lane's fragment row's window origin (+ the lane half's 8 channels).  c tiles: tap row 0's; the border pair: one per
    // tap row, of the tile that tap row belongs to (RG::border_tile: tile 10 + simd while its class sees the tap row, then tile 14 + simd)
    constexpr RVRowTable table{};
    auto origin = [&](int tile, int ty) __attribute__((always_inline)) -> unsigned {
        const int id = table.src[tile * 32 + li];
        const int gi = id / RG::OP, p = id - gi * RG::OP, y = p / RG::OW, x = p - y * RG::OW;
        return (unsigned)(rv_origin(gi, y, x, ty) * RG::PIX + 16 * lh);
    };
    unsigned winc[2 + XC], winb[3];
    winc[0] = origin(tile_of(0), 0);
    winc[1] = origin(tile_of(1), 0);
    if constexpr (XC) winc[2] = origin(tile_of(4), 0);
    const bool eb_pair = simd >= 2;                        // {e, b}: tile 10 + simd sees tap row 0 only; {d, a}: tap rows 0, 1
    winb[0] = origin(10 + simd, 0);
    winb[1] = origin(eb_pair ? 14 + simd : 10 + simd, 1);
    winb[2] = origin(14 + simd, 2);

    // ---- the group's source: unit u = 16 bytes = 4 channels of a pixel; thread tid takes units it * THREADS + tid
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A), 0, (int)a.a_bytes, kResRsrcWord3);
    unsigned udst[(NI + 1) / 2];                          // LDS byte address / 8 of two units' hi halves (lo: + LO), 16 bits each; 0xffff: no such unit
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int u = it * THREADS + tid;
        const int pix = u / RG::UPP, c4 = u - pix * RG::UPP, img = pix / (RG::IH * RG::IW), q = pix - img * (RG::IH * RG::IW), qy = q / RG::IW, qx = q - qy * RG::IW;
        const unsigned d = u < RG::UNITS ? (unsigned)(RG::rec(img, qy, qx) * RG::PIX + c4 * 8) >> 3 : 0xffffu;
        udst[it >> 1] = (it & 1) ? (udst[it >> 1] | (d << 16)) : d;
    }
    // the next group's source: two loads per k-step from the second step on (res_prefetch), filled at the top of the group (res_fill_packed)
    static_assert(rv_pre_lo(RG::KSTEPS) == NI, "the next group's source is requested inside one k-loop");
    s_u32x4 pre[NI];

    // ---- epilogue constants: C's descriptor of a group starts AT the group (+ the wave's column tile): offsets are table words + the lane's channel
    const unsigned col_off = (unsigned)(jc * 32 * 4);
    float cmax = 0.0f;

    // ---- the weights' ring by LDS-DMA (kernel R's): slot s = k-steps SS s .. SS s + SS - 1 = one tap, two buffers.  Slot s + 1 is requested at the first step of
    // slot s into the buffer every wave read for the last time before the barrier of slot s - 1; the issuing wave waits for ITS pieces (vmcnt counts in order:
    // rv_dma_younger = the vector loads it issued behind them) in front of the barrier at the last step of slot s.  NSLOT is odd: slot s of a group lives in
    // buffer (s & 1) ^ gpar, gpar alternating from group to group (slot NSLOT = the next group's slot 0 goes where slot NSLOT - 2 was).
    const __amdgpu_buffer_rsrc_t rsrc_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.pack), 0, kF16PackHeader + RG::KSTEPS * RG::STEPB, kResRsrcWord3);
    const unsigned lane16 = 16u * (unsigned)lane;
    int gpar = 0;
    unsigned rbuf[2] = {(unsigned)(RG::ABYTES + 16 * lane + jc * 2048), (unsigned)(RG::ABYTES + RG::SLOTB + 16 * lane + jc * 2048)};      // the lane's address in the buffer of this group's even / odd slots
    auto dma_slot = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < kShare; ++u) {
            const int x = wave * kShare + u, h = x / (NT * 2), jt = x - h * (NT * 2);
            res_dma16(rsrc_p, ring + ((slot & 1) ^ gpar) * RG::SLOTB + x * 1024, lane16, kF16PackHeader + (SS * (slot % NSLOT) + h) * RG::STEPB + jt * 1024);
        }
    };

    res_f32x16 acc[MT];
    unsigned wm[NWM];                                     // lane L of wm[k]: the mask word of wave row 64 k + L = slot L % 32 of the wave's tile 2 k + L / 32 (this wave's column tile)
    s_u32x4 pa[4][2], wb[2][2];                           // pixel fragments of the step's tiles [position][hi, lo]; weight fragments [k-step parity][hi, lo]
    auto read_a = [&](int pos, unsigned w, int off) __attribute__((always_inline)) {
        pa[pos][0] = *reinterpret_cast<const s_u32x4*>(lds + w + off);
        pa[pos][1] = *reinterpret_cast<const s_u32x4*>(lds + w + off + RG::LO);
    };
    auto read_c = [&](int pos, int i, int v) __attribute__((always_inline)) { read_a(pos, winc[i], rv_tapoff_c(v)); };       // c tile i (2: the extra half) of k-step v
    auto read_bd = [&](int pos, int v) __attribute__((always_inline)) { read_a(pos, winb[v / RG::SPR], rv_tapoff_b(v)); };   // the border tile of k-step v's tap row
    auto read_b = [&](int par, int v) __attribute__((always_inline)) {
        const int h = v % SS;
#pragma unroll
        for (int t = 0; t < 2; ++t) wb[par][t] = *reinterpret_cast<const s_u32x4*>(lds + rbuf[(v / SS) & 1] + (h * NT * 2 + t) * 1024);
    };
    // mask words in: the C offset of slot x of a tile is table word (lane half (x >> 2) & 1, value (x & 3) + 4 (x >> 3)) of that tile
    unsigned mword[NWM];
#pragma unroll
    for (int k = 0; k < NWM; ++k) {
        const int t = (2 * k + 1 < MT && lh) ? tile_of(2 * k + 1) : tile_of(2 * k);
        mword[k] = (unsigned)((t * 2 + ((li >> 2) & 1)) * 16 + (li & 3) + 4 * (li >> 3));
    }
    auto load_masks = [&](unsigned gbase, const __amdgpu_buffer_rsrc_t rb) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < NWM; ++k) {
            const bool have = 2 * k + 1 < MT || lh == 0;   // (an odd number of tiles: lanes 32 .. 63 of the last register hold nothing)
            const unsigned ro = rofft[mword[k]];
            wm[k] = __builtin_amdgcn_raw_buffer_load_b32(rb, have ? (gbase + ro) >> 5 : kResOob, 0, 0);
        }
    };
    auto mfma3 = [&](int q, int t, int p, int pi, bool z) __attribute__((always_inline)) {
        if (pi == 0 && z) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;                       // (the MFMA's inline zero)
        }
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(s_f16x8, pa[p][pi == 2 ? 1 : 0]), __builtin_bit_cast(s_f16x8, wb[q][pi == 1 ? 1 : 0]), acc[t], 0, 0, 0);
    };
    auto pair = [&](int q, int t0, int p0, bool z0, int t1, int p1, bool z1) __attribute__((always_inline)) {
#pragma unroll
        for (int pi = 0; pi < 3; ++pi) {
            mfma3(q, t0, p0, pi, z0);
            if (t1 >= 0) mfma3(q, t1, p1, pi, z1);
        }
    };

    auto group = [&](int grp) __attribute__((always_inline)) {
        const unsigned gbase = (unsigned)grp * (unsigned)RG::GROUPC + col_off;
        const __amdgpu_buffer_rsrc_t rb_cur = res_rsrc_b_of(a.bits_in, a.c_bytes, grp >= 0 && grp < a.groups);
        // every wave is done with the previous group's records and ring slots
        res_ring_barrier();
        res_fill_packed<RG>(lds, pre, udst, sa);
        __builtin_amdgcn_sched_barrier(0);
        res_ring_barrier();                               // the records are written (slot 0 landed before the previous epilogue / the prologue's wait)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[3][e] = 0.0f;
        read_b(0, 0);
        read_c(0, 0, 0); read_c(1, 1, 0); read_bd(2, 0);
        if constexpr (XC) read_c(3, 2, 0);
#pragma unroll
        for (int v = 0; v < RG::KSTEPS; ++v) {
            const int q = v & 1, slot = v / SS, h = v % SS;
            if (v + 1 < RG::KSTEPS) {
                if (h == SS - 1) {
                    res_wait_vmcnt(rv_dma_younger(slot));      // this wave's pieces of slot + 1 have landed
                    res_ring_barrier();
                }
                read_b(q ^ 1, v + 1);
            }
            if (h == 0) {
                dma_slot(slot + 1);                       // (slot NSLOT = the next group's slot 0; the last group fetches it for nobody)
                __builtin_amdgcn_sched_barrier(0);        // (rv_dma_younger assumes the pieces are issued in front of this step's round)
            }
            if (rv_pre_lo(v + 1) > rv_pre_lo(v)) res_prefetch<RG>(pre, rsrc_a, a.groups, tid, grp + a.grid, rv_pre_lo(v), rv_pre_lo(v + 1) - rv_pre_lo(v));
            if (v == RG::KSTEPS - 3) load_masks(gbase, rb_cur);          // (inside the last slot, behind its first step: no ring wait follows)
            if (h == 0 && (slot == 3 || slot == 6) && eb_pair) {          // {e, b}: the border accumulators change places
                const res_f32x16 t = acc[2];
                acc[2] = acc[3];
                acc[3] = t;
            }
            __builtin_amdgcn_sched_barrier(0);
            pair(q, 0, 0, v == 0, 1, 1, v == 0);
            __builtin_amdgcn_sched_barrier(0);
            if (v + 1 < RG::KSTEPS) { read_c(0, 0, v + 1); read_c(1, 1, v + 1); }
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (XC) pair(q, 2 + (slot >= 6 ? 1 : 0), 2, v == 0 && slot < 6, 4, 3, v == 0);
            else pair(q, 2 + (slot >= 6 ? 1 : 0), 2, v == 0 && slot < 6, -1, 0, false);
            __builtin_amdgcn_sched_barrier(0);
            if (v + 1 < RG::KSTEPS) {
                read_bd(2, v + 1);
                if constexpr (XC) read_c(3, 2, v + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // every load in flight -- the next group's source, its first ring slot, this group's mask words -- is waited for in front of the
        // epilogue's stores (vmcnt counts loads and stores in one in-order queue: convr.hip)
        __builtin_amdgcn_s_waitcnt(kResWaitVm0);
        __builtin_amdgcn_sched_barrier(0);
        const __amdgpu_buffer_rsrc_t rc = res_rsrc_c_of(a.C, a.c_bytes, grp >= 0 && grp < a.groups, gbase);
#pragma unroll
        for (int i = 0; i < MT; ++i) res_masked_tile(acc[i], i, rofft + (tile_of(i) * 2 + lh) * 16, wm, un, cmax, rc, li);
        // the ring's buffers change places for the next group (nine slots)
        gpar ^= 1;
        const unsigned t = rbuf[0];
        rbuf[0] = rbuf[1];
        rbuf[1] = t;
    };

    int grp = blockIdx.x;
    if (grp < a.groups) {
        res_prefetch<RG>(pre, rsrc_a, a.groups, tid, grp, 0, NI);
        dma_slot(0);
        __builtin_amdgcn_s_waitcnt(kResWaitVm0);
    }
    for (; grp < a.groups; grp += a.grid) group(grp);
    if (a.c_amax) amax_commit(a.c_amax, __float_as_uint(cmax), blockIdx.x * NW + (unsigned)wave, lane);
}

__global__ __launch_bounds__(RVGeom::THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void rv_kernel(RVArgs a) {
    using RG = RVGeom;
    __shared__ __attribute__((aligned(16))) unsigned char lds[RG::LDSB];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the zero records (and everything else, once); the epilogue's table: word (tile 2 + lane half) 16 + e = C offset, from the group's first byte, of the row
    // in slot (e & 3) + 8 (e >> 2) + 4 (lane half) of the tile.  (Read after the first group's barriers.)
    for (int o = tid * 16; o < RG::ABYTES; o += RG::THREADS * 16) *reinterpret_cast<s_u32x4*>(lds + o) = (s_u32x4){0u, 0u, 0u, 0u};
    constexpr RVRowTable table{};
    unsigned* const rofft = reinterpret_cast<unsigned*>(lds + RG::ABYTES + 2 * RG::SLOTB);
    for (int w = tid; w < RG::TILES * 32; w += RG::THREADS) {
        const int t = w >> 5, h = (w >> 4) & 1, e = w & 15;
        rofft[w] = (unsigned)table.src[t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h] * (unsigned)(32 * RG::NT * 4);
    }
    if (RG::extra(wave)) rv_wave<1>(a, lds, tid, wave);
    else rv_wave<0>(a, lds, tid, wave);
}

// Which sizes kernel RV takes from kernel R's layer-3 data gradient (MI355PPO_CONV_RV through common.h::kernel_switch: 0 = never, min:<n> = from n images on).
bool convrv_takes(long long images) { return kernel_switch("MI355PPO_CONV_RV", images, MI355_RV_MIN_IMAGES); }

int convrv_dgrad3(const char* fn, const float* dz, unsigned dz_bytes, const void* pack, const unsigned* bits, float* dsrc, unsigned dsrc_bytes,
                  long long images, const unsigned* dz_amax, unsigned* dsrc_amax, hipStream_t st) {
    RVArgs a = res_args<RVArgs>(dz, dz_bytes, pack, dsrc, dsrc_bytes, images, dz_amax, dsrc_amax);
    a.bits_in = bits;
    return res_launch(rv_kernel, a, RVGeom::G, 1, RVGeom::THREADS, st, fn);
}

}  // namespace mi355ppo
