// Kernel RB -- the layer-2 data gradient of the NatureCNN (the backward of cleanrl/ppo_atari_multigpu.py:141, `loss.backward()` :358) with the
// rows of an image group dealt to tiles BY BORDER CLASS (round 6).  Kernel R's structure (convr.hip: the group's dz2 resident in LDS as f16
// hi / lo records, split once; weights from the f16x2 pack through the workgroup's two-buffer LDS ring; kernel Z's epilogue) with the
// geometry of convrb_geom.h:
//   * THREE images per group (padded lines share their border record: 117 records per image), 300 rows in ten 32-row tiles;
//   * six interior tiles walk all 16 k-steps, the four rim tiles (bottom / top line, right / left column of the 10 x 10 grid of window
//     origins) only the 8 k-steps of the two taps that can lie inside the image -- the skipped products are exact zeros in kernel R / Z;
//   * 8 waves = 4 stride-parity classes (one column tile each) x 2 row-waves; a wave holds 3 interior + 2 rim accumulator tiles (80
//     registers) and issues, in every k-step, 4 tiles x 3 term pairs = 12 matrix instructions (kernel R: 2 x 2 x 3): 192 per group of
//     THREE images where kernel R issues 192 per group of two;
//   * pixel fragments single-buffered: a pair of tiles' fragments for step v + 1 is requested right behind that pair's matrix instructions
//     of step v (six matrix instructions of distance), weight fragments double-buffered as in kernel R;
//   * the epilogue's row offsets (5 tiles x 16 values per lane half) come from a 1.25-KB table in LDS instead of 80 registers.
// Arithmetic: per accumulator the products of kernel Z's SPLIT = 1 instance in its order (k-steps ascending, per step hi hi, hi lo, lo hi)
// minus products with a zero-border operand: bit-identical results (tools/conv_traffic hashes, tests/test_gpu_f16x2.py).
#include "conv_resident.h"
#include "convrb_geom.h"

#pragma clang fp contract(off)

namespace mi355ppo {

struct RBArgs {
    const float* A;             // dz2 (images, 9, 9, 64)
    unsigned a_bytes;
    const unsigned char* pack;  // f16x2 pack of the class matrices (header + [k-step][class][hi, lo][lane][8 f16])
    const unsigned* bits_in;    // ReLU mask of a1, one bit per element of (images, 20, 20, 32)
    float* C;                   // da1 (images, 20, 20, 32)
    unsigned c_bytes;
    long long images;
    int groups;
    int grid;                   // workgroups of the launch (the group stride)
    const unsigned* a_amax;     // amax record of dz2
    unsigned* c_amax;           // amax record of da1 to fold into, or null
};

__global__ __launch_bounds__(RBGeom::THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void rb_kernel(RBArgs a) {
    using RG = RBGeom;
    constexpr int NT = RG::NT, MT = RG::MT, NW = RG::NW, NI = RG::NI, THREADS = RG::THREADS, SS = RG::SS, NSLOT = RG::NSLOT, NI3 = RG::NI3;
    constexpr int kPieces = SS * NT * 2;                  // KiB pieces of a ring slot: (step h of the slot, class j, term t), x = (h NT + j) 2 + t
    constexpr int kShare = kPieces / NW;                  // every wave moves kShare pieces of a slot
    static_assert(kPieces % NW == 0 && NSLOT % 2 == 0, "whole pieces per wave; the next group's slot 0 goes to buffer 0 while the last slot is read from buffer 1");
    __shared__ __attribute__((aligned(16))) unsigned char lds[RG::LDSB];
    unsigned char* const ring = lds + RG::ABYTES;
    unsigned* const rofft = reinterpret_cast<unsigned*>(lds + RG::ABYTES + 2 * RG::SLOTB);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int rw = wave & 1, jg = wave >> 1;               // row-wave; class (wave-uniform)

    const int ea = f16_scale_exp(amax_load(a.a_amax, lane));
    const int eb = f16_scale_exp(*reinterpret_cast<const unsigned*>(a.pack));
    const float sa = f16_pow2(ea), un = f16_unscale(ea, eb);

    // ---- rows.  C offset of row (image gi of the group, window origin (gy, gx)) for class 0: pixel (2 gy, 2 gx) of the (20, 20, 32) image
    constexpr RBRowTable table{};
    auto row_coff = [](int id) __attribute__((always_inline)) -> unsigned {
        const int gi = id / 100, gy = (id % 100) / 10, gx = id % 10;
        return (unsigned)(((gi * 20 + 2 * gy) * 20 + 2 * gx) * 32) * 4u;
    };
    unsigned win[NI3], winr[NSLOT];                       // LDS byte offset of the lane's fragment row's window origin (+ the lane half's 8 channels): interior tiles; the rim tile of ring slot s
    auto win_of = [&](int tile) __attribute__((always_inline)) -> unsigned {
        const int id = table.src[(rw * MT + tile) * 32 + li];
        return (unsigned)((id / 100) * RG::IMGB + RG::pidx((id % 100) / 10, id % 10) * RG::PIX + 16 * lh);
    };
#pragma unroll
    for (int i = 0; i < NI3; ++i) win[i] = win_of(i);
    {
        const unsigned w3 = win_of(NI3), w4 = win_of(NI3 + 1);
#pragma unroll
        for (int sl = 0; sl < NSLOT; ++sl) winr[sl] = (rw == 0 ? (sl >> 1) : (sl & 1)) ? w4 : w3;      // RG::rim_of
    }
    // the epilogue's table: word ((rw MT + i) 2 + lh) 16 + e = C offset of the row in slot (e & 3) + 8 (e >> 2) + 4 lh of tile i
    if (tid < RG::RW * MT * 32) {
        const int t = tid >> 5, h = (tid >> 4) & 1, e = tid & 15;          // t = rw MT + i
        rofft[tid] = row_coff(table.src[t * 32 + (e & 3) + 8 * (e >> 2) + 4 * h]);
    }
    unsigned char* const ring_l = ring + 16 * lane;
    const unsigned char* const ring_r = ring_l + jg * 2048;                // this wave's class of a k-step

    // ---- the group's source: unit u = 16 bytes = 4 channels of a pixel; thread tid takes units it * THREADS + tid
    const __amdgpu_buffer_rsrc_t rsrc_a = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A), 0, (int)a.a_bytes, kResRsrcWord3);
    unsigned udst[NI / 2];                                // LDS byte address / 8 of two units' hi halves (lo: + LO), 16 bits each; 0xffff: no such unit
#pragma unroll
    for (int it = 0; it < NI; ++it) {
        const int u = it * THREADS + tid;
        const int pix = u / RG::UPP, c4 = u - pix * RG::UPP, img = pix / (RG::IH * RG::IW), q = pix - img * (RG::IH * RG::IW), qy = q / RG::IW, qx = q - qy * RG::IW;
        const unsigned d = u < RG::UNITS ? (unsigned)(img * RG::IMGB + RG::pidx(qy + 1, qx + 1) * RG::PIX + c4 * 8) >> 3 : 0xffffu;
        udst[it >> 1] = (it & 1) ? (udst[it >> 1] | (d << 16)) : d;
    }
    // the next group's source: two loads per k-step from the second step on (res_prefetch), filled at the top of the group (res_fill_packed)
    constexpr auto pre_lo = [](int v) constexpr -> int { return res_pre_lo(v, NI); };
    static_assert(pre_lo(RG::KSTEPS) == NI, "the next group's source is requested inside one k-loop");
    s_u32x4 pre[NI];
    // the zero border (and everything else, once)
    for (int o = tid * 16; o < RG::ABYTES; o += THREADS * 16) *reinterpret_cast<s_u32x4*>(lds + o) = (s_u32x4){0u, 0u, 0u, 0u};

    // ---- epilogue constants: C's descriptor of a group starts AT the group (+ the wave's class): offsets are table words + the lane's channel
    constexpr unsigned kGroupC = RG::G * 4 * RG::OP * 32 * 4;             // bytes of da1 per group
    const unsigned cls_off = (unsigned)(((jg >> 1) * 20 + (jg & 1)) * 32 * 4);
    float cmax = 0.0f;

    // ---- the weights' ring by LDS-DMA (kernel R's: slot s = k-steps SS s .. SS s + SS - 1 = one tap, two buffers): a piece = one wave instruction, global -> LDS
    // without registers.  Slot s + 1 is requested at the first step of slot s into the buffer every wave read for the last time before the barrier of slot s - 1;
    // the issuing wave waits for ITS pieces (vmcnt counts in order: res_pre_younger = the vector loads it issued behind them) in front of the barrier at the last
    // step of slot s.
    const __amdgpu_buffer_rsrc_t rsrc_p = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(a.pack), 0, kF16PackHeader + RG::KSTEPS * RG::STEPB, kResRsrcWord3);
    const unsigned lane16 = 16u * (unsigned)lane;
    auto dma_slot = [&](int slot) __attribute__((always_inline)) {                       // -> buffer slot & 1
#pragma unroll
        for (int u = 0; u < kShare; ++u) {
            const int x = wave * kShare + u, h = x / (NT * 2), jt = x - h * (NT * 2);
            res_dma16(rsrc_p, ring + (slot & 1) * RG::SLOTB + x * 1024, lane16, kF16PackHeader + (SS * (slot % NSLOT) + h) * RG::STEPB + jt * 1024);
        }
    };

    res_f32x16 acc[MT];
    unsigned wm[3];                                       // lane L of wm[k]: the mask word of wave row 64 k + L (this wave's class)
    s_u32x4 pa[4][2], wb[2][2];                           // pixel fragments of the step's four tiles [pair position][hi, lo]; weight fragments [k-step parity][hi, lo]
    auto read_a = [&](int pos, int tile, int v) __attribute__((always_inline)) {         // tile's fragment of k-step v -> position pos (tile NI3: the step's rim tile)
        const int off = rb_tapoff(v);
        const unsigned w = tile < NI3 ? win[tile] : winr[v / SS];
        pa[pos][0] = *reinterpret_cast<const s_u32x4*>(lds + w + off);
        pa[pos][1] = *reinterpret_cast<const s_u32x4*>(lds + w + off + RG::LO);
    };
    auto read_b = [&](int par, int v) __attribute__((always_inline)) {
        const int buf = (v / SS) & 1, h = v % SS;
#pragma unroll
        for (int t = 0; t < 2; ++t) wb[par][t] = *reinterpret_cast<const s_u32x4*>(ring_r + buf * RG::SLOTB + (h * NT * 2 + t) * 1024);
    };
    // mask words in: lane L of wm[k] takes wave row 64 k + L = slot x = L % 32 of tile 2 k + L / 32, whose C offset is table word (lane half (x >> 2) & 1,
    // value (x & 3) + 4 (x >> 3)) of that tile; wave rows 160 .. 191 do not exist
    const unsigned mword = (unsigned)((rw * MT * 2 + ((li >> 2) & 1)) * 16 + (li & 3) + 4 * (li >> 3) + 32 * lh);
    auto load_masks = [&](unsigned gbase, const __amdgpu_buffer_rsrc_t rb) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const unsigned ro = rofft[mword + (k < 2 || lh == 0 ? 64 * k : 0)];
            wm[k] = __builtin_amdgcn_raw_buffer_load_b32(rb, (k < 2 || lh == 0) ? (gbase + ro) >> 5 : kResOob, 0, 0);
        }
    };
    // six matrix instructions of a pair of tiles: (hi hi, hi lo, lo hi) interleaved over the two tiles (a tile's three are dependent)
    auto pair = [&](int q, int t0, int p0, bool z0, int t1, int p1, bool z1) __attribute__((always_inline)) {
#pragma unroll
        for (int pi = 0; pi < 3; ++pi) {
            if (pi == 0 && z0) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t0][e] = 0.0f;                  // (the MFMA's inline zero)
            }
            acc[t0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(s_f16x8, pa[p0][pi == 2 ? 1 : 0]), __builtin_bit_cast(s_f16x8, wb[q][pi == 1 ? 1 : 0]), acc[t0], 0, 0, 0);
            if (pi == 0 && z1) {
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t1][e] = 0.0f;
            }
            acc[t1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(s_f16x8, pa[p1][pi == 2 ? 1 : 0]), __builtin_bit_cast(s_f16x8, wb[q][pi == 1 ? 1 : 0]), acc[t1], 0, 0, 0);
        }
    };

    // The rim accumulator a ring slot feeds is the same in both row-waves' code -- tile 3 in slots 0, 1, tile 4 in slots 2, 3: row-wave 0's bottom, bottom,
    // top, top.  Row-wave 1 (right, left, right, left) SWAPS the two accumulators in front of slots 1 and 3 (tile 4 zeroed at the group's start): slot 0
    // right -> tile 3; swap; slot 1 left -> tile 3, slot 2 right -> tile 4; swap; slot 3 left -> tile 4.  32 register moves per group in place of two
    // copies of the k-loop (which left the register allocator spilling the prefetched source inside the second copy) or of branches around the matrix
    // instructions (whose accumulators the compiler then merged with copies behind every branch).
    auto group = [&](int grp) __attribute__((always_inline)) {
        const unsigned gbase = (unsigned)grp * kGroupC + cls_off;
        const __amdgpu_buffer_rsrc_t rb_cur = res_rsrc_b_of(a.bits_in, a.c_bytes, grp >= 0 && grp < a.groups);
        // every wave is done with the previous group's records and ring slots
        res_ring_barrier();
        res_fill_packed<RG>(lds, pre, udst, sa);
        __builtin_amdgcn_sched_barrier(0);
        res_ring_barrier();                               // the records are written (slot 0 landed before the previous epilogue / the prologue's wait)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[NI3 + 1][e] = 0.0f;
        read_b(0, 0);
        read_a(0, 0, 0); read_a(1, 1, 0); read_a(2, 2, 0); read_a(3, NI3, 0);
#pragma unroll
        for (int v = 0; v < RG::KSTEPS; ++v) {
            const int q = v & 1, slot = v / SS, h = v % SS;
            if (v + 1 < RG::KSTEPS) {
                if (h == SS - 1) {
                    // this wave's pieces of slot + 1: everything but the vector loads issued behind them (the prefetch rounds of steps SS slot + 1 .. v - 1)
                    static_assert(pre_lo(SS - 1) - pre_lo(1) == 4 && pre_lo(2 * SS - 1) - pre_lo(SS) == 2 && pre_lo(2 * SS) == NI, "the counted waits: 4, 2, 0, 0");
                    res_wait_vmcnt(res_pre_younger(slot, SS, NI));
                    res_ring_barrier();
                }
                read_b(q ^ 1, v + 1);
            }
            if (h == 0) {
                dma_slot(slot + 1);                       // (slot NSLOT = the next group's slot 0; the last group fetches it for nobody)
                __builtin_amdgcn_sched_barrier(0);        // (the counts above assume the pieces are issued in front of this step's prefetch round)
            }
            if (pre_lo(v + 1) > pre_lo(v)) res_prefetch<RG>(pre, rsrc_a, a.groups, tid, grp + a.grid, pre_lo(v), pre_lo(v + 1) - pre_lo(v));
            if (v == RG::KSTEPS - 4) load_masks(gbase, rb_cur);
            if (h == 0 && (slot & 1) && rw != 0) {          // row-wave 1: the rim accumulators change places
                const res_f32x16 t = acc[NI3];
                acc[NI3] = acc[NI3 + 1];
                acc[NI3 + 1] = t;
            }
            __builtin_amdgcn_sched_barrier(0);
            pair(q, 0, 0, v == 0, 1, 1, v == 0);
            __builtin_amdgcn_sched_barrier(0);
            if (v + 1 < RG::KSTEPS) { read_a(0, 0, v + 1); read_a(1, 1, v + 1); }
            __builtin_amdgcn_sched_barrier(0);
            pair(q, 2, 2, v == 0, NI3 + (slot >> 1), 3, v == 0);
            __builtin_amdgcn_sched_barrier(0);
            if (v + 1 < RG::KSTEPS) { read_a(2, 2, v + 1); read_a(3, NI3, v + 1); }
            __builtin_amdgcn_sched_barrier(0);
        }
        // every load in flight -- the next group's source, its first two ring slots, this group's mask words -- is waited for in front of the
        // epilogue's stores (vmcnt counts loads and stores in one in-order queue: convr.hip)
        __builtin_amdgcn_s_waitcnt(kResWaitVm0);
        __builtin_amdgcn_sched_barrier(0);
        const __amdgpu_buffer_rsrc_t rc = res_rsrc_c_of(a.C, a.c_bytes, grp >= 0 && grp < a.groups, gbase);
        const unsigned* const rt = rofft + ((rw * MT) * 2 + lh) * 16;
#pragma unroll
        for (int i = 0; i < MT; ++i) res_masked_tile(acc[i], i, rt + i * 32, wm, un, cmax, rc, li);
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

// Which sizes kernel RB takes from kernel R's RDgrad2: one persistent workgroup per CU with three images each -- from 3,072 images on every CU
// has at least four groups (MI355PPO_CONV_RB through common.h::kernel_switch: 0 = never, min:<n> = from n images on).
bool convrb_takes(long long images) { return kernel_switch("MI355PPO_CONV_RB", images, MI355_RB_MIN_IMAGES); }

int convrb_dgrad2(const char* fn, const float* dz, unsigned dz_bytes, const void* pack, const unsigned* bits, float* dsrc, unsigned dsrc_bytes,
                  long long images, const unsigned* dz_amax, unsigned* dsrc_amax, hipStream_t st) {
    RBArgs a = res_args<RBArgs>(dz, dz_bytes, pack, dsrc, dsrc_bytes, images, dz_amax, dsrc_amax);
    a.bits_in = bits;
    return res_launch(rb_kernel, a, RBGeom::G, 1, RBGeom::THREADS, st, fn);
}

}  // namespace mi355ppo
