// Kernel RS's compile-time geometry (convrs.hip): the layer-2 forward with the source of an image group STREAMED through LDS by stride-parity class.
// Plain constexpr C++ -- no device code -- so that the host can check it (tests/test_kernel_rs_geometry.py compiles
// tests/host/convrs_geom_check.cpp against this header with g++).
//
// The GEMM of a group is kernel R's RConv2 (convr_geom.h): rows = the 9 x 9 outputs of G images, K = 4 x 4 taps x 32 channels in 32 k-steps of 16,
// visited in ORDER 2 (r_kstep): four phases of 8 k-steps, phase g = the taps of row parity g >> 1 and column parity g & 1.  A stride-2 tap (ty, tx)
// of output (gy, gx) reads pixel (2 gy + ty, 2 gx + tx): a pixel of CLASS (ty & 1, tx & 1) = g.  So a phase touches one quarter of the source, and
// only that quarter has to be in LDS while the phase is multiplied:
//   * class (py, px) of an image = the 10 x 10 grid of pixels (2 i + py, 2 j + px); record of class pixel (i, j) of image `img` of the group =
//     img IP + i RP + j (records are kernel R's: 64 B hi | 64 B lo | 16 B pad = 144 B = 9 sixteen-byte slots);
//   * tap (ty, tx) of output (gy, gx) = record origin(gy, gx) + (ty >> 1) RP + (tx >> 1) with origin = img IP + gy RP + gx: additive, the SAME
//     origin in every class, so the lane's window origin is one register and every tap a compile-time offset;
//   * two class buffers: phase g multiplies from buffer g & 1 while class g + 1 (of the next group after phase 3) is split and written into the other;
//   * THREE images per group: 243 rows in eight 32-row tiles (kernel R: 162 rows in six).  RP = 10, IP = 101: no residue mod 16 of the 243
//     origins occurs more than 16 times, and RRowTable deals them to the 16 sixteen-lane sets without a conflict.
#pragma once

#include "convr_geom.h"

namespace mi355ppo {

struct RSGeom {
    static constexpr int IH = 20, IW = 20, IC = 32, KH = 4, KW = 4, S = 1, OH = 9, OW = 9, NT = 2, G = 3, NW = 8, MT = 1, ORDER = 2, SS = 4, WGS = 1;
    static constexpr int NTW = NT, RW = NW;                                         // every wave: one 32-row tile against both column tiles
    static constexpr int PIX = 4 * IC + 16, LO = 2 * IC, C16 = IC / 16, UPP = IC / 4;      // bytes per pixel record: 2 IC hi | 2 IC lo | 16 pad; chunks / 16-byte units per pixel
    static constexpr int CH = IH / 2, CW = IW / 2;                                  // a class of an image: CH x CW pixels
    static constexpr int RP = 10, IP = 101, IPIX = IP;                              // records per class row; per image of a class buffer (one spare: the origins' residues)
    static constexpr int SPARE = CH * RP;                                           // image 0's spare record: no window reaches it (the threads without a unit write there)
    static constexpr int OP = OH * OW, ROWS = G * OP, SLOTS = 32 * MT * NW;
    static constexpr int KSTEPS = KH * KW * C16, SPR = KW * C16, PHASES = 4, PSTEPS = KSTEPS / PHASES;      // k-steps; per tap row; phases = classes; k-steps per phase
    static constexpr int BUFB = G * IP * PIX, ABYTES = 2 * BUFB;                    // one class buffer; both
    static constexpr int STEPB = NT * 2048, SLOTB = SS * STEPB;                     // one k-step of the pack; ring slot
    static constexpr int LDSB = ABYTES + 2 * SLOTB;
    static constexpr int THREADS = 64 * NW;
    static constexpr int CUNITS = G * CH * CW * UPP, NI = (CUNITS + THREADS - 1) / THREADS;      // 16-byte units of a group's class; rounds per thread and class
    static constexpr int IMG_SRC = IH * IW * IC * 4, GROUP_SRC = G * IMG_SRC;       // bytes of a1 per image / group
    // RRowTable's view: record index of the window origin of output (gy, gx) (S = 1: pidx(gy, gx)), the same in all four classes
    static constexpr int pidx(int y, int x) { return y * RP + x; }
    // class unit u (0 .. CUNITS - 1) = (image, class row i, class column j, 4-channel chunk c4), c4 fastest: a class row is CW pieces of 128 contiguous bytes
    // at a 256-byte stride in memory.  -> byte offset in the group's source for class `cls`; byte offset of the unit's hi half in a class buffer
    static constexpr int unit_src(int cls, int u) {
        const int c4 = u % UPP, j = (u / UPP) % CW, i = (u / (UPP * CW)) % CH, img = u / (UPP * CW * CH);
        return img * IMG_SRC + ((2 * i + (cls >> 1)) * IW + 2 * j + (cls & 1)) * (IC * 4) + c4 * 16;
    }
    static constexpr int unit_dst(int u) {
        const int c4 = u % UPP, j = (u / UPP) % CW, i = (u / (UPP * CW)) % CH, img = u / (UPP * CW * CH);
        return (img * IP + i * RP + j) * PIX + c4 * 8;
    }
    // rounds of a class go out / are written in these k-steps of a phase (behind the ring's LDS-DMA pieces of steps 0 and SS: convrs.hip)
    static constexpr int round_step(int r) { return r < 3 ? r : r + 1; }
    static_assert((PIX / 16) % 2 == 1 && KSTEPS % (PHASES * SS) == 0 && PSTEPS == 2 * SS && ROWS <= SLOTS && NI == 5, "odd record pitch; whole ring slots per phase");
    static_assert((G - 1) * IP + (CH - 1) * RP + CW <= G * IP && RP >= CW && IP >= CH * RP && SPARE < IP && (OH - 1 + 1) * RP + OW - 1 + 1 < SPARE, "class records inside the buffer");
    static_assert(LDSB <= 160 * 1024, "LDS");
};

// visited step v -> the class buffer it reads (= its phase's class, mod 2) and the byte offset of the step's hi fragment from the lane's window origin
RES_GEOM_FN int rs_class(int v) { return v / RSGeom::PSTEPS; }
RES_GEOM_FN int rs_tapoff(int ks) {
    const int ty = ks / RSGeom::SPR, us = ks - ty * RSGeom::SPR, tx = us / RSGeom::C16, chunk = us - tx * RSGeom::C16;
    return ((ty >> 1) * RSGeom::RP + (tx >> 1)) * RSGeom::PIX + chunk * 32;
}

}  // namespace mi355ppo
