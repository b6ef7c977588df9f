// Kernel RV's compile-time geometry (convrv.hip): the layer-3 data gradient with SEVEN images per group and the rows of a group dealt to tiles
// BY VERTICAL BORDER CLASS.  Plain constexpr C++ -- no device code -- so that the host can check it (tests/test_kernel_rv_geometry.py compiles
// tests/host/convrv_geom_check.cpp against this header with g++).
//
// The GEMM of an image (kernel R's RDgrad3, convr_geom.h): rows = the 9 x 9 pixels of da2, k = (tap row ty, tap column tx, 64 channels of dz3) of
// a 3 x 3 window over the 7 x 7 dz3 bordered by two zero pixels = 36 k-steps in ascending order (ks = 12 ty + 4 tx + chunk), columns = 64 input
// channels in two 32-column tiles.  Output row y reads dz3 rows y + ty - 2: by y the tap rows that can touch the image are
//     class a: y = 0      ty {2}          class b: y = 1      ty {1, 2}       class c: y = 2 .. 6   ty {0, 1, 2}
//     class d: y = 7      ty {0, 1}       class e: y = 8      ty {0}
// -- 441 of kernel R's 729 tap-rows per image when the horizontal border is counted too, 567 of 729 by the vertical one alone, which is what is
// skipped here.  A tile whose 32 rows all lie in ONE class never reads above or below its image, so the source needs no zero LINES:
//   * records (kernel R's: 128 B hi | 128 B lo | 16 B pad) in lines of NINE -- two zero records, then the line's seven pixels; the two zero
//     records of the next line (of the next image's first line; two trailing records behind the group) are a line's right border:
//     7 x 63 + 2 = 443 records = 120,496 B for SEVEN images (kernel R: three);
//   * 7 x 81 = 567 rows in 18 class-pure tiles: c 315 rows in ten tiles, a, b, d, e 63 rows in two tiles each;
//   * a ring slot is one tap (SS = 4), and a tile multiplies only the taps of its class: 10 x 9 + 2 x (3 + 6 + 6 + 3) = 126 tile-taps per group,
//     x 2 column tiles x 4 k-steps x 3 term pairs = 3,024 matrix instructions per seven images: 432 per image against kernel R's 576;
//   * in every tap row 14 row tiles are active (ten c; ty 0: d, e; ty 1: b, d; ty 2: a, b) = 28 (row tile, column tile) units = 7 per SIMD:
//     SIMD s holds the c tiles 2 s, 2 s + 1 and the pair with complementary tap rows -- {d, a} on SIMDs 0, 1, {e, b} on SIMDs 2, 3 --, its two
//     waves (s and s + 4) take column tile 0 and column tile 1 of those, and ONE of the two also takes its column half of c tile 8 + s / 2.
#pragma once

#include "conv_resident_geom.h"

namespace mi355ppo {

struct RVGeom {
    static constexpr int IH = 7, IW = 7, IC = 64, OH = 9, OW = 9, OP = OH * OW, KH = 3, KW = 3, HL = 2;      // dz3 image; da2 image; taps; border
    static constexpr int G = 7, NW = 8, NT = 2, TILES = 18, CT = 10;                     // images per group; waves; column tiles; row tiles (the first CT: class c)
    static constexpr int RP = 9, IPIX = IH * RP, RECS = G * IPIX + 2;                    // records per line (two zero records first); per image; per group
    static constexpr int PIX = 4 * IC + 16, LO = 2 * IC, C16 = IC / 16;                  // record: 128 B hi | 128 B lo | 16 B pad (17 sixteen-byte slots: odd)
    static constexpr int KSTEPS = KH * KW * C16, SS = 4, NSLOT = KSTEPS / SS, SPR = KW * C16;      // k-steps; per ring slot (= one tap); slots; k-steps per tap row
    static constexpr int ABYTES = RECS * PIX;
    static constexpr int STEPB = NT * 2048, SLOTB = SS * STEPB;
    static constexpr int ROWS = G * OP, SLOTS = 32 * TILES;
    static constexpr int UPP = IC / 4, UNITS = G * IH * IW * UPP, THREADS = 64 * NW, NI = (UNITS + THREADS - 1) / THREADS;
    static constexpr int ROFFB = TILES * 2 * 16 * 4;                                     // the epilogue's row offsets: [tile][lane half][value] words
    static constexpr int LDSB = ABYTES + 2 * SLOTB + ROFFB;
    static constexpr int GROUPC = G * OP * 32 * NT * 4;                                  // bytes of da2 per group
    // record of dz3 pixel (qy, qx) of image gi; qx = -2, -1 and 7, 8 are zero records (this line's, the next line's)
    static constexpr int rec(int gi, int qy, int qx) { return gi * IPIX + qy * RP + HL + qx; }
    // vertical class of output row y: 0 = a .. 4 = e; its first and last valid tap row
    static constexpr int cls_of(int y) { return y == 0 ? 0 : y == 1 ? 1 : y <= 6 ? 2 : y == 7 ? 3 : 4; }
    static constexpr int ty_first(int cls) { return cls == 0 ? 2 : cls == 1 ? 1 : 0; }
    static constexpr int ty_last(int cls) { return cls == 3 ? 1 : cls == 4 ? 0 : 2; }
    // Tiles: 0 .. 9 class c; 10 + s the border tile SIMD s multiplies FIRST (d, d, e, e); 14 + s the one it multiplies second (a, a, b, b).
    static constexpr int tile_cls(int t) { return t < CT ? 2 : t < 12 ? 3 : t < 14 ? 4 : t < 16 ? 0 : 1; }
    static constexpr int slot_first(int t) { return 3 * ty_first(tile_cls(t)); }          // a tile's first and last active ring slot (slot = 3 ty + tx)
    static constexpr int slot_last(int t) { return 3 * ty_last(tile_cls(t)) + 2; }
    static constexpr bool active(int t, int slot) { return slot >= slot_first(t) && slot <= slot_last(t); }
    // Waves: wave w sits on SIMD w % 4 and takes column tile w / 4.  Its accumulators: 0, 1 = c tiles 2 s, 2 s + 1; 2 = tile 10 + s; 3 = tile 14 + s;
    // 4 (waves with extra(w) only) = c tile 8 + s / 2.
    static constexpr int simd_of(int w) { return w & 3; }
    static constexpr int col_of(int w) { return w >> 2; }
    static constexpr bool extra(int w) { return (simd_of(w) & 1) == col_of(w); }
    static constexpr int ntiles(int w) { return extra(w) ? 5 : 4; }
    static constexpr int wave_tile(int w, int i) { return i < 2 ? 2 * simd_of(w) + i : i == 2 ? 10 + simd_of(w) : i == 3 ? 14 + simd_of(w) : 8 + (simd_of(w) >> 1); }
    // the border tile a wave multiplies in tap row ty: its accumulator 2 in the tap rows of tile 10 + s, accumulator 3 in the others
    static constexpr int border_tile(int w, int ty) { return ty <= ty_last(tile_cls(10 + simd_of(w))) ? 10 + simd_of(w) : 14 + simd_of(w); }
};

static_assert(RVGeom::LDSB <= 160 * 1024 && (RVGeom::PIX / 16) % 2 == 1 && RVGeom::ROWS <= RVGeom::SLOTS && RVGeom::KSTEPS % RVGeom::SS == 0, "LDS, odd pitch, row slots, whole ring slots");
static_assert(RVGeom::ABYTES / 8 < 0xffff, "two 16-bit record offsets per register");

// Byte offset of k-step ks' hi fragment from the lane's window origin.  c tiles: the origin is the record of dz3 pixel (y - 2, x - 2) -- tap row 0;
// border tiles keep one origin PER TAP ROW (the record of pixel (y + ty - 2, x - 2): a class's first valid tap row is folded into the origin), so
// their offsets carry the tap column only and no immediate is negative.
RES_GEOM_FN int rv_tapoff_c(int ks) {
    const int ty = ks / RVGeom::SPR, us = ks - ty * RVGeom::SPR, tx = us / RVGeom::C16, chunk = us - tx * RVGeom::C16;
    return (ty * RVGeom::RP + tx) * RVGeom::PIX + chunk * 32;
}
RES_GEOM_FN int rv_tapoff_b(int ks) {
    const int us = ks % RVGeom::SPR, tx = us / RVGeom::C16, chunk = us - tx * RVGeom::C16;
    return tx * RVGeom::PIX + chunk * 32;
}
// record of the window origin of row (gi, y, x) for tap row ty (pixel (y + ty - 2, x - 2): a zero record of line y + ty - 2 when x < 2)
RES_GEOM_FN int rv_origin(int gi, int y, int x, int ty) { return RVGeom::rec(gi, y + ty - RVGeom::HL, x - RVGeom::HL); }

// Which row of the group sits in which lane: slot tile 32 + lane % 32 -> row id = image 81 + y 9 + x (`row`: -1 = an empty slot; `src`: the row the
// slot computes, ResRowSets::fill_empty).  A fragment read (ds_read_b128, lane = row) is served in sets of 16 lanes and is conflict-free when the 16 window
// origins differ mod 16 (record pitch 17 slots).  As RRowTable does, the rows of a class are dealt to the sets of the class's tiles by the
// residue of their window origin -- a set takes a residue twice only when no other set of the class can take it (the border classes: a
// class's 63 origins 63 gi + x fall on 15 residues, up to seven rows each, for four sets).
struct RVRowTable : ResRowSets {
    short row[RVGeom::SLOTS], src[RVGeom::SLOTS];
    constexpr RVRowTable() : row{}, src{} {
        using RG = RVGeom;
        constexpr int NSET = RG::SLOTS / 16;
        int fill[NSET] = {};
        bool has[NSET][16] = {};
        int slot_of[NSET][16] = {};                        // k-th lane (0..15) of set s -> slot; sets 2 t, 2 t + 1 belong to tile t
        for (int s = 0; s < NSET; ++s) {
            int k = 0;
            for (int l = 0; l < 32; ++l)
                if (first_set(l) == ((s & 1) == 0)) slot_of[s][k++] = (s >> 1) * 32 + l;
        }
        for (int i = 0; i < RG::SLOTS; ++i) row[i] = -1;
        bool done[RG::ROWS] = {};
        for (int cls = 0; cls < 5; ++cls) {
            int sets[2 * RG::CT] = {}, ns = 0;             // the sets of the class's tiles
            for (int t = 0; t < RG::TILES; ++t)
                if (RG::tile_cls(t) == cls) { sets[ns++] = 2 * t; sets[ns++] = 2 * t + 1; }
            int next = 0;
            for (int pass = 0; pass < 2; ++pass)           // pass 0: conflict-free placements only; pass 1: whatever is left, anywhere in the class
                for (int r = 0; r < RG::ROWS; ++r) {
                    const int gi = r / RG::OP, p = r - gi * RG::OP, y = p / RG::OW, x = p - y * RG::OW;
                    if (RG::cls_of(y) != cls || done[r]) continue;
                    const int c = rv_origin(gi, y, x, RG::ty_first(cls)) & 15;
                    bool placed = false;
                    for (int t = 0; t < ns && !placed; ++t) {
                        const int k = (next + t) % ns, s = sets[k];
                        if (fill[s] < 16 && (pass == 1 || !has[s][c])) {
                            row[slot_of[s][fill[s]++]] = (short)r;
                            has[s][c] = true;
                            placed = true;
                            done[r] = true;
                            next = k + 1;
                        }
                    }
                }
        }
        fill_empty(row, src);
    }
};

// the next group's source: two 16-byte loads per k-step from the second step on, NI in all; those a wave issues behind a ring slot's LDS-DMA pieces
RES_GEOM_FN int rv_pre_lo(int v) { return res_pre_lo(v, RVGeom::NI); }
RES_GEOM_FN int rv_dma_younger(int slot) { return res_pre_younger(slot, RVGeom::SS, RVGeom::NI); }

}  // namespace mi355ppo
