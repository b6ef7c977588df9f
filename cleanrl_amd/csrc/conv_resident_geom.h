// What the compile-time geometries of the input-resident convolution family share (convr_geom.h, convrb_geom.h, convrs_geom.h, convrv_geom.h): the
// sixteen-lane sets of a fragment read, the pass that gives empty row slots a row to compute, and the schedule of the next group's source loads.
// Plain constexpr C++ -- no device code -- so that the host checks (tests/host/*_geom_check.cpp) compile it with g++.
#pragma once

#if defined(__HIPCC__)
#define RES_GEOM_FN __device__ __forceinline__ constexpr
#else
#define RES_GEOM_FN inline constexpr
#endif

namespace mi355ppo {

// Base of the row tables (RRowTable, RBRowTable, RVRowTable).  A fragment read (ds_read_b128, lane = row) is served in sets of 16 lanes -- {0-3, 12-15,
// 20-27} and {4-11, 16-19, 28-31} of each wave half; set s of a table = tile s / 2, the first set when s is even.
struct ResRowSets {
    static constexpr bool first_set(int l) { return l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28); }
    // `src`: the row a slot computes -- its own, or (empty slots, row < 0) a row of the SAME sixteen-lane set: the same address as that lane's, a broadcast,
    // where row 0 would be one more record on some bank; an empty slot computes and stores that row's values a second time.
    template <int SLOTS>
    static constexpr void fill_empty(const short (&row)[SLOTS], short (&src)[SLOTS]) {
        for (int s = 0; s < SLOTS / 16; ++s) {
            const int base = (s >> 1) * 32;
            int have = 0;                                   // (a set without any row: all sixteen lanes on row 0, one address)
            for (int l = 0; l < 32; ++l)
                if (first_set(l) == ((s & 1) == 0) && row[base + l] >= 0) { have = row[base + l]; break; }
            for (int l = 0; l < 32; ++l)
                if (first_set(l) == ((s & 1) == 0)) src[base + l] = row[base + l] >= 0 ? row[base + l] : (short)have;
        }
    }
};

// Loads of the next group's source issued before k-step v: rounds [res_pre_lo(v), res_pre_lo(v + 1)) of the `ni` go out in step v.  Two per step from the
// second step on (the small sources of the data gradients: 38 - 42 KB are in flight at once without holding anybody), or -- span > 0, the forwards'
// 104 KB -- evenly over steps 1 .. span: a CU takes in ~11 bytes per cycle from HBM when every CU asks, so 24 KB per step (12 waves x 2 loads) is
// five times what arrives, the queue fills within two steps and every wave then waits AT ITS NEXT LOAD until the 104 KB have drained --
// s_memtime: k-steps 2 .. 7 of the layer-2 forward took 11,200 ticks instead of 2,000 (profiles/r05_kernel_r_trace.txt).  One round
// every ~3 steps asks for what arrives.
RES_GEOM_FN int res_pre_lo(int v, int ni, int span = 0) {
    const int n = span > 0 ? ((v - 1) * ni + span - 1) / span : (v - 1) * 2;
    return v < 1 ? 0 : (n > ni ? ni : n);
}
// of those, the loads a wave issues behind the LDS-DMA pieces of ring slot `slot` + 1 (requested at the slot's first step, in front of that step's
// round) and in front of its wait (top of the slot's last step): the rounds of the slot's steps but the last (ss k-steps per slot)
RES_GEOM_FN int res_pre_younger(int slot, int ss, int ni, int span = 0) { return res_pre_lo(ss * slot + ss - 1, ni, span) - res_pre_lo(ss * slot, ni, span); }

}  // namespace mi355ppo
