// What the input-resident convolution family shares -- kernels R (convr.hip), RB (convrb.hip), RS (convrs.hip) and RV (convrv.hip): the source of a GROUP of
// images held in LDS as f16 hi / lo records, the weights through a two-buffer LDS ring filled by LDS-DMA, kernel Z's epilogue, one persistent workgroup per CU.
// Each file keeps what differs -- geometry, wave schedule, the k-loop body; everything here is inlined into its kernels (the instruction streams are those of
// the four files written out).
#pragma once
#include "common.h"
#include "f16split.h"
#include "conv_resident_geom.h"

namespace mi355ppo {

typedef float res_f32x16 __attribute__((ext_vector_type(16)));

constexpr unsigned kResOob = 0xFFFFF000u;             // buffer offset out of range for every tensor < 4 GiB - 4 KiB
constexpr int kResRsrcWord3 = 0x00020000;             // raw buffer, 32-bit elements
constexpr int kResWaitVm0 = 0x0F70;                   // s_waitcnt vmcnt(0) (gfx9 encoding: expcnt 7, lgkmcnt 15 = no wait)

// lane `l` of w := the wave-uniform value x; x where bit (lane) of {hi, lo} is set, else 0 (gemmz.hip's z_writelane / z_keep_where: the
// s_nop covers the two wait states a VALU read of an SGPR needs behind the VALU write the compiler cannot see inside the asm)
__device__ __forceinline__ int res_writelane(int w, unsigned x, int l) {
    asm("s_nop 1\n\tv_writelane_b32 %0, %1, %2" : "+v"(w) : "s"(x), "i"(l));
    return w;
}
__device__ __forceinline__ float res_keep_where(float x, unsigned lo, unsigned hi) {
    const unsigned long long m = ((unsigned long long)hi << 32) | lo;
    float r;
    asm("s_nop 1\n\tv_cndmask_b32_e64 %0, 0, %1, %2" : "=v"(r) : "v"(x), "s"(m));
    return r;
}

// one LDS-DMA piece: 16 bytes per lane from the buffer (per-lane offset `voff`, wave-uniform `soff`) to LDS at `dst` + 16 lane (buffer_load_dwordx4 ... lds).
// (A plain function on purpose: with the builtin inside a kernel TEMPLATE the host pass drops the kernels' launch stubs without a diagnostic.)
__device__ __forceinline__ void res_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned char* dst, unsigned voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)dst, 16, voff, soff, 0, 0);
}

// the ring's barrier (a bare s_barrier: __syncthreads' fence would drain vmcnt -- source loads, the previous group's stores -- while an LDS-DMA may be pending)
__device__ __forceinline__ void res_ring_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}
// s_waitcnt vmcnt(n): an immediate -- the chain folds once the k-loop around the call is unrolled.  vmcnt counts in order, so a wave that waits for ITS pieces
// of a ring slot waits for "all but the n vector loads issued behind the pieces".
__device__ __forceinline__ void res_wait_vmcnt(int n) {
#define RES_VMCNT_CASE(k) if (n == k) asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory");
    RES_VMCNT_CASE(0) RES_VMCNT_CASE(1) RES_VMCNT_CASE(2) RES_VMCNT_CASE(3) RES_VMCNT_CASE(4) RES_VMCNT_CASE(5) RES_VMCNT_CASE(6) RES_VMCNT_CASE(7)
    RES_VMCNT_CASE(8) RES_VMCNT_CASE(9) RES_VMCNT_CASE(10) RES_VMCNT_CASE(11) RES_VMCNT_CASE(12)
#undef RES_VMCNT_CASE
    if (n < 0 || n > 12) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (never more than a few rounds per slot: a full wait is always correct)
}

// ---- the next group's source (kernels R, RB, RV): unit u = 16 bytes = 4 channels of a pixel; thread tid takes units it * THREADS + tid; rounds it0 .. it0 + n - 1.
// (Issued unconditionally -- past the last group with out-of-range offsets, which load zeros without touching memory: loads behind a
//  branch leave the compiler without a count of the outstanding ones, and every later wait for a weight piece became "all of them".
//  Units past the tensor (last group) load zeros: their rows are never stored.)
template <class RG>
__device__ __forceinline__ void res_prefetch(s_u32x4 (&pre)[RG::NI], const __amdgpu_buffer_rsrc_t rsrc_a, int groups, int tid, int grp, int it0, int n) {
    const bool any = grp < groups;
    const unsigned base = (unsigned)grp * (unsigned)(RG::UNITS * 16);
#pragma unroll
    for (int it = it0; it < it0 + n && it < RG::NI; ++it) {
        const int u = it * RG::THREADS + tid;
        pre[it] = __builtin_bit_cast(s_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc_a, (any && u < RG::UNITS) ? base + (unsigned)u * 16u : kResOob, 0, MI355_AUX_STREAM_LD));
    }
}
// ... split and stored at the top of the group.  udst[it]: LDS byte address of the unit's hi half (lo: + RG::LO); ~0u: no such unit
template <class RG>
__device__ __forceinline__ void res_fill(unsigned char* lds, const s_u32x4 (&pre)[RG::NI], const unsigned (&udst)[RG::NI], float sa) {
#pragma unroll
    for (int it = 0; it < RG::NI; ++it) {
        unsigned hi[2], lo[2];
        f16_split4(pre[it], sa, hi, lo);
        if (udst[it] != ~0u) {
            *reinterpret_cast<uint2*>(lds + udst[it]) = make_uint2(hi[0], hi[1]);
            *reinterpret_cast<uint2*>(lds + udst[it] + RG::LO) = make_uint2(lo[0], lo[1]);
        }
    }
}
// ... with two 16-bit offsets per register (kernels RB, RV): LDS byte address / 8 of two units' hi halves; 0xffff: no such unit
template <class RG>
__device__ __forceinline__ void res_fill_packed(unsigned char* lds, const s_u32x4 (&pre)[RG::NI], unsigned (&udst)[(RG::NI + 1) / 2], float sa) {
    static_assert(RG::ABYTES / 8 < 0xffff, "two 16-bit record offsets per register");
#pragma unroll
    for (int it = 0; it < RG::NI; ++it) {
        unsigned hi[2], lo[2];
        f16_split4(pre[it], sa, hi, lo);
        // (the packed word is made opaque in place: unpacked outside the group loop the eight addresses cost registers the k-loop does not have,
        //  and a scratch reload here waits -- vmcnt is one in-order queue -- for the previous group's stores)
        if ((it & 1) == 0) asm volatile("" : "+v"(udst[it >> 1]));
        const unsigned d = (it & 1) ? udst[it >> 1] >> 16 : udst[it >> 1] & 0xffffu;
        if ((it + 1) * RG::THREADS <= RG::UNITS || d != 0xffffu) {
            *reinterpret_cast<uint2*>(lds + 8u * d) = make_uint2(hi[0], hi[1]);
            *reinterpret_cast<uint2*>(lds + 8u * d + RG::LO) = make_uint2(lo[0], lo[1]);
        }
    }
}

// ---- the buffer descriptors of a group (kernels RB, RV; kernel R writes them out; ok: the group is one of the launch's -- otherwise no range at all).  C's starts AT the group
// (gbase: + the wave's column tiles): the per-value offsets are then lane constants + an immediate, no address arithmetic per store; the range shrinks with the
// base, so rows of images past the batch still fall out of it (a scalar offset would not be checked).  The mask words': one bit per element of C.
// (`ok` comes from the caller: computed in here from the group's number, the kernels' instruction streams changed.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t res_rsrc_c_of(float* C, unsigned c_bytes, bool ok, unsigned gbase) {
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<unsigned char*>(C) + (ok ? gbase : 0u), 0, ok ? (int)(c_bytes - gbase) : 0, kResRsrcWord3);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t res_rsrc_b_of(const void* bits, unsigned c_bytes, bool ok) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(bits), 0, ok ? (int)(c_bytes >> 5) : 0, kResRsrcWord3);
}

// ---- the masked-gradient epilogue of a wave's tile i (kernels RB, RV): `rt` = the tile's 16 words of the row-offset table in LDS for this lane half (word e:
// C offset, from the group's base, of the row in slot (e & 3) + 8 (e >> 2) + 4 lh), lane L of wm[k] = the mask word of wave row 64 k + L.
// (The matrix instructions of a tile pair -- `pair` in convrb.hip / convrv.hip -- stay in their files: as a shared function they were allocated other registers.)
template <int NWM>
__device__ __forceinline__ void res_masked_tile(const res_f32x16& acc, int i, const unsigned* rt, const unsigned (&wm)[NWM], float un, float& cmax,
                                                const __amdgpu_buffer_rsrc_t rc, int li) {
    unsigned ro[16];
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
        const s_u32x4 w = *reinterpret_cast<const s_u32x4*>(rt + 4 * e4);
        ro[4 * e4] = w[0]; ro[4 * e4 + 1] = w[1]; ro[4 * e4 + 2] = w[2]; ro[4 * e4 + 3] = w[3];
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int wr = 32 * i + (e & 3) + 8 * (e >> 2);                 // wave row of lanes 0 .. 31's value; lanes 32 .. 63: + 4
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)wm[wr >> 6], wr & 63);
        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)wm[(wr + 4) >> 6], (wr + 4) & 63);
        const float v = res_keep_where(acc[e] * un, lo, hi);            // lanes 0..31 (lh = 0): bit li of `lo`, lanes 32..63: of `hi`
        cmax = __builtin_fmaxf(cmax, __builtin_fabsf(v));
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rc, ro[e] + 4u * (unsigned)li, 0, MI355_AUX_STREAM_ST);
    }
    __builtin_amdgcn_sched_barrier(0);            // (one tile's offsets in registers at a time: hoisted together they are 80)
}

// ---- host side
// the argument fields every kernel of the family has
template <class Args>
static Args res_args(const float* A, unsigned a_bytes, const void* pack, float* C, unsigned c_bytes, long long images, const unsigned* a_amax, unsigned* c_amax) {
    Args a{};
    a.A = A; a.a_bytes = a_bytes; a.pack = static_cast<const unsigned char*>(pack); a.C = C; a.c_bytes = c_bytes;
    a.images = images; a.a_amax = a_amax; a.c_amax = c_amax;
    return a;
}
// The launch: groups of `g` images on persistent workgroups, `wgs` per CU at the most (Args with a `grid` field take the group stride from it).
template <class Args>
static int res_launch(void (*kernel)(Args), Args a, int g, int wgs, int threads, hipStream_t s, const char* what) {
    a.groups = (int)((a.images + g - 1) / g);
    const int cap = cu_count() * wgs, grid = a.groups < cap ? a.groups : cap;
    if constexpr (requires { a.grid; }) a.grid = grid;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3((unsigned)threads), 0, s, a);
    return check_launch(what);
}

}  // namespace mi355ppo
