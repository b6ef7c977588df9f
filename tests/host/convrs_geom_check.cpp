// Host-side check of kernel RS's compile-time geometry (cleanrl_amd/csrc/convrs_geom.h), compiled with g++ by tests/test_kernel_rs_geometry.py.
// Prints one JSON object; exits non-zero on the first violated property.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "convrs_geom.h"

using namespace mi355ppo;
using RG = RSGeom;

#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        if (!(cond)) {                                       \
            std::fprintf(stderr, "RSGeom: ");                \
            std::fprintf(stderr, __VA_ARGS__);               \
            std::fprintf(stderr, "\n");                      \
            std::exit(1);                                    \
        }                                                    \
    } while (0)

// the 16-lane sets a ds_read_b128 is served in (MI355X_MICROARCH.md, LDS): per wave half {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}
static bool first_set(int l) { return l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28); }

// record of class pixel (i, j) of image img in a class buffer -- the definition the kernel's offsets are checked against
static int record(int img, int i, int j) { return img * RG::IP + i * RG::RP + j; }

int main() {
    static constexpr RRowTable<RG> table{};
    // ---- every row of a group sits in exactly one slot; the other slots are empty
    std::vector<int> seen(RG::ROWS, 0);
    int empty = 0;
    for (int i = 0; i < RG::SLOTS; ++i) {
        const int r = table.row[i];
        if (r < 0) { ++empty; continue; }
        REQUIRE(r < RG::ROWS, "slot %d holds row %d of %d", i, r, RG::ROWS);
        ++seen[r];
    }
    for (int r = 0; r < RG::ROWS; ++r) REQUIRE(seen[r] == 1, "row %d sits in %d slots", r, seen[r]);
    REQUIRE(empty == RG::SLOTS - RG::ROWS, "%d empty slots, %d expected", empty, RG::SLOTS - RG::ROWS);
    // ---- fragment reads: the 16 lanes of a set start in 16 different sixteen-byte slots of the 256-byte bank row (odd record pitch: the residues of
    // the window origins decide; every tap adds the same offset to all lanes; an empty slot repeats a row of its own set: the same address, a broadcast)
    const int pitch = RG::PIX / 16;
    REQUIRE(pitch % 2 == 1, "record pitch of %d sixteen-byte slots is even", pitch);
    int conflicts = 0, sets = 0;
    for (int tile = 0; tile < RG::SLOTS / 32; ++tile)
        for (int half = 0; half < 2; ++half) {
            std::set<long> at[16];
            for (int l = 0; l < 32; ++l) {
                if (first_set(l) != (half == 0)) continue;
                const int r = table.src[tile * 32 + l];
                REQUIRE(r >= 0 && r < RG::ROWS && (table.row[tile * 32 + l] < 0 || table.row[tile * 32 + l] == r), "slot %d computes row %d", tile * 32 + l, r);
                const int gi = r / RG::OP, p = r - gi * RG::OP, gy = p / RG::OW, gx = p - gy * RG::OW;
                const long rec = (long)gi * RG::IPIX + RG::pidx(RG::S * gy, RG::S * gx);
                REQUIRE(rec == record(gi, gy, gx), "row %d: origin record %ld", r, rec);
                at[(rec * pitch) & 15].insert(rec);
            }
            ++sets;
            for (int c = 0; c < 16; ++c) conflicts += at[c].size() > 1 ? (int)at[c].size() - 1 : 0;
        }
    REQUIRE(conflicts == 0, "%d bank conflicts in the fragment reads of %d sixteen-lane sets", conflicts, sets);
    // ---- (origin) + (tap offset) = the record of pixel (2 gy + ty, 2 gx + tx) in the class (ty & 1, tx & 1), for all rows and taps; inside the buffer
    for (int r = 0; r < RG::ROWS; ++r) {
        const int gi = r / RG::OP, p = r - gi * RG::OP, gy = p / RG::OW, gx = p - gy * RG::OW;
        for (int k = 0; k < RG::KSTEPS; ++k) {
            const int ty = k / RG::SPR, us = k - ty * RG::SPR, tx = us / RG::C16, chunk = us - tx * RG::C16;
            const int y = 2 * gy + ty, x = 2 * gx + tx;
            REQUIRE(y < RG::IH && x < RG::IW, "row %d tap (%d, %d) leaves the image", r, ty, tx);
            const int want = record(gi, y >> 1, x >> 1) * RG::PIX + chunk * 32;      // pixel (y, x) = class pixel (y >> 1, x >> 1) of class (y & 1, x & 1) = (ty & 1, tx & 1)
            const int got = (gi * RG::IPIX + RG::pidx(gy, gx)) * RG::PIX + rs_tapoff(k);
            REQUIRE(want == got, "row %d, k-step %d: record offset %d, origin + tap offset gives %d", r, k, want, got);
            REQUIRE(got + RG::LO + 32 <= RG::BUFB, "row %d, k-step %d reads past the class buffer", r, k);
        }
    }
    // ---- the visited sequence is r_kstep<RConv2>'s, a permutation, and phase g holds only taps of class g
    std::set<int> ks;
    for (int v = 0; v < RG::KSTEPS; ++v) {
        const int k = r_kstep<RG>(v);
        REQUIRE(k == r_kstep<RConv2>(v), "visited step %d -> k-step %d, kernel R's layer-2 forward visits %d", v, k, r_kstep<RConv2>(v));
        REQUIRE(k >= 0 && k < RG::KSTEPS, "visited step %d -> k-step %d", v, k);
        ks.insert(k);
        const int ty = k / RG::SPR, tx = (k % RG::SPR) / RG::C16;
        REQUIRE(rs_class(v) == (ty & 1) * 2 + (tx & 1), "visited step %d (phase %d) reads tap (%d, %d)", v, rs_class(v), ty, tx);
    }
    REQUIRE((int)ks.size() == RG::KSTEPS && RConv2::KSTEPS == RG::KSTEPS, "the visited order repeats a k-step");
    // ---- every 16-byte unit of a group's source is assigned to exactly one (class, round, thread); its LDS place is its pixel's record
    std::map<int, int> src_seen;
    for (int cls = 0; cls < RG::PHASES; ++cls) {
        std::set<int> dst_seen;
        for (int it = 0; it < RG::NI; ++it)
            for (int t = 0; t < RG::THREADS; ++t) {
                const int u = it * RG::THREADS + t;
                if (u >= RG::CUNITS) continue;
                const int s = RG::unit_src(cls, u), d = RG::unit_dst(u);
                REQUIRE(s >= 0 && s % 16 == 0 && s + 16 <= RG::GROUP_SRC, "class %d unit %d: source offset %d", cls, u, s);
                ++src_seen[s];
                const int img = s / RG::IMG_SRC, q = (s % RG::IMG_SRC) / (RG::IC * 4), y = q / RG::IW, x = q % RG::IW, c4 = (s % (RG::IC * 4)) / 16;
                REQUIRE((y & 1) * 2 + (x & 1) == cls, "class %d unit %d is pixel (%d, %d)", cls, u, y, x);
                REQUIRE(d == record(img, y >> 1, x >> 1) * RG::PIX + c4 * 8, "class %d unit %d: LDS offset %d", cls, u, d);
                REQUIRE(d + 8 <= RG::LO + (d / RG::PIX) * RG::PIX && d + RG::LO + 8 <= RG::BUFB, "class %d unit %d leaves its record", cls, u);
                REQUIRE(dst_seen.insert(d).second, "class %d: two units share LDS offset %d", cls, d);
            }
    }
    REQUIRE((int)src_seen.size() == RG::GROUP_SRC / 16, "%d of %d source units assigned", (int)src_seen.size(), RG::GROUP_SRC / 16);
    for (const auto& kv : src_seen) REQUIRE(kv.second == 1, "source unit at %d assigned %d times", kv.first, kv.second);
    // ---- the rounds of a phase are written before the phase's last k-step (its barrier) and in ascending steps
    for (int r = 0; r < RG::NI; ++r) REQUIRE(RG::round_step(r) < RG::PSTEPS - 1 && (r == 0 || RG::round_step(r) > RG::round_step(r - 1)), "round %d in step %d", r, RG::round_step(r));
    // ---- sizes the kernel relies on
    REQUIRE(RG::LDSB <= 160 * 1024, "LDS: %d bytes", RG::LDSB);
    std::printf("{\"instance\": \"RSGeom\", \"rows\": %d, \"slots\": %d, \"ksteps\": %d, \"sets\": %d, \"conflicts\": %d, \"lds_bytes\": %d, \"rounds_per_thread\": %d, \"class_units\": %d}\n",
                RG::ROWS, RG::SLOTS, RG::KSTEPS, sets, conflicts, RG::LDSB, RG::NI, RG::CUNITS);
    return 0;
}
