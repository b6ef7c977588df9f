// Host-side check of kernel RV's compile-time geometry (cleanrl_amd/csrc/convrv_geom.h), compiled with g++ by tests/test_kernel_rv_geometry.py.
// Prints one JSON object; exits non-zero on the first violated property.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <vector>

#include "convrv_geom.h"

using namespace mi355ppo;
using RG = RVGeom;

#define REQUIRE(cond, ...)                                   \
    do {                                                     \
        if (!(cond)) {                                       \
            std::fprintf(stderr, "RVGeom: ");                \
            std::fprintf(stderr, __VA_ARGS__);               \
            std::fprintf(stderr, "\n");                      \
            std::exit(1);                                    \
        }                                                    \
    } while (0)

// the 16-lane sets a ds_read_b128 is served in: per wave half {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}
static bool first_set(int l) { return l < 4 || (l >= 12 && l < 16) || (l >= 20 && l < 28); }

// is record `idx` of a group one the kernel never writes a pixel to (the two in front of every line, the two behind the group)?
static bool zero_record(int idx) { return idx >= RG::G * RG::IPIX ? idx < RG::RECS : (idx % RG::IPIX) % RG::RP < RG::HL; }

struct Row { int gi, y, x; };
static Row row_of(int r) { return {r / RG::OP, (r % RG::OP) / RG::OW, r % RG::OW}; }

int main() {
    static constexpr RVRowTable table{};
    // ---- every row of a group sits in exactly one slot, in a tile of its own class; an empty slot computes a row of its own sixteen-lane set
    std::vector<int> seen(RG::ROWS, 0);
    int empty = 0;
    for (int i = 0; i < RG::SLOTS; ++i) {
        const int r = table.row[i], s = table.src[i], tile = i / 32;
        REQUIRE(s >= 0 && s < RG::ROWS && (r < 0 || r == s), "slot %d computes row %d (holds %d)", i, s, r);
        REQUIRE(RG::cls_of(row_of(s).y) == RG::tile_cls(tile), "slot %d of tile %d (class %d) computes row %d of class %d", i, tile, RG::tile_cls(tile), s, RG::cls_of(row_of(s).y));
        if (r < 0) {
            ++empty;
            bool same_set = false;
            for (int l = 0; l < 32; ++l) same_set = same_set || (first_set(l) == first_set(i % 32) && table.row[tile * 32 + l] == s);
            REQUIRE(same_set, "empty slot %d repeats row %d of another sixteen-lane set", i, s);
            continue;
        }
        REQUIRE(r < RG::ROWS, "slot %d holds row %d of %d", i, r, RG::ROWS);
        ++seen[r];
    }
    for (int r = 0; r < RG::ROWS; ++r) REQUIRE(seen[r] == 1, "row %d sits in %d slots", r, seen[r]);
    REQUIRE(empty == RG::SLOTS - RG::ROWS, "%d empty slots, %d expected", empty, RG::SLOTS - RG::ROWS);
    // ---- each tile's active ring slots are exactly the taps of its class's valid tap rows
    for (int t = 0; t < RG::TILES; ++t)
        for (int slot = 0; slot < RG::NSLOT; ++slot) {
            const int ty = slot / RG::KW, cls = RG::tile_cls(t);
            REQUIRE(RG::active(t, slot) == (ty >= RG::ty_first(cls) && ty <= RG::ty_last(cls)), "tile %d (class %d), slot %d", t, cls, slot);
        }
    for (int y = 0; y < RG::OH; ++y)
        for (int ty = 0; ty < RG::KH; ++ty) {
            const bool inside = y + ty - RG::HL >= 0 && y + ty - RG::HL < RG::IH, listed = ty >= RG::ty_first(RG::cls_of(y)) && ty <= RG::ty_last(RG::cls_of(y));
            REQUIRE(inside == listed, "output row %d, tap row %d: inside the image %d, in its class's list %d", y, ty, (int)inside, (int)listed);
        }
    // ---- the waves' schedule: which (row tile, column tile) a wave multiplies in which k-step, as the kernel's loop does
    std::map<std::pair<int, int>, std::vector<int>> visited;        // (tile, column tile) -> k-steps in the order they are multiplied
    std::map<std::pair<int, int>, int> owner;
    long mfma_total = 0;
    int max_imm = 0, simd_step = 0;
    for (int ks = 0; ks < RG::KSTEPS; ++ks) {
        const int slot = ks / RG::SS, ty = ks / RG::SPR, tx = (ks % RG::SPR) / RG::C16, chunk = ks % RG::C16;
        REQUIRE(slot == ty * RG::KW + tx, "k-step %d: ring slot %d is not tap (%d, %d)", ks, slot, ty, tx);
        int per_simd[4] = {};
        for (int w = 0; w < RG::NW; ++w) {
            std::vector<int> tiles = {RG::wave_tile(w, 0), RG::wave_tile(w, 1), RG::border_tile(w, ty)};
            if (RG::extra(w)) tiles.push_back(RG::wave_tile(w, 4));
            REQUIRE(tiles[2] == RG::wave_tile(w, 2) || tiles[2] == RG::wave_tile(w, 3), "wave %d: border tile %d of tap row %d is not one of its accumulators", w, tiles[2], ty);
            for (size_t n = 0; n < tiles.size(); ++n) {
                const int t = tiles[n];
                REQUIRE(RG::active(t, slot), "wave %d multiplies tile %d in slot %d, which its class does not see", w, t, slot);
                const auto key = std::make_pair(t, RG::col_of(w));
                REQUIRE(owner.emplace(key, w).first->second == w, "tile %d, column tile %d is multiplied by waves %d and %d", t, RG::col_of(w), owner[key], w);
                visited[key].push_back(ks);
                per_simd[RG::simd_of(w)] += 3;
                mfma_total += 3;
                // the records its 32 lanes read: origin + offset = the record of dz3 pixel (y + ty - 2, x + tx - 2) of the row's own image, or a zero record
                const bool border = n == 2;
                const int off = border ? rv_tapoff_b(ks) : rv_tapoff_c(ks);
                REQUIRE(off >= 0, "negative immediate %d", off);
                max_imm = off + RG::LO > max_imm ? off + RG::LO : max_imm;
                for (int l = 0; l < 32; ++l) {
                    const Row r = row_of(table.src[t * 32 + l]);
                    const int byte = rv_origin(r.gi, r.y, r.x, border ? ty : 0) * RG::PIX + off;
                    REQUIRE(byte >= 0 && byte + RG::LO + 32 <= RG::ABYTES, "tile %d lane %d k-step %d reads at %d, outside the records", t, l, ks, byte);
                    REQUIRE(byte % RG::PIX == chunk * 32, "tile %d lane %d k-step %d: offset %d inside the record", t, l, ks, byte % RG::PIX);
                    const int idx = byte / RG::PIX, qy = r.y + ty - RG::HL, qx = r.x + tx - RG::HL;
                    REQUIRE(qy >= 0 && qy < RG::IH, "tile %d lane %d k-step %d: dz3 line %d", t, l, ks, qy);
                    if (qx >= 0 && qx < RG::IW) REQUIRE(idx == RG::rec(r.gi, qy, qx) && !zero_record(idx), "tile %d lane %d k-step %d: record %d, pixel (%d, %d) of image %d is %d", t, l, ks, idx, qy, qx, r.gi, RG::rec(r.gi, qy, qx));
                    else REQUIRE(zero_record(idx), "tile %d lane %d k-step %d: record %d of a border tap is not a zero record", t, l, ks, idx);
                }
            }
        }
        REQUIRE(per_simd[0] == per_simd[1] && per_simd[1] == per_simd[2] && per_simd[2] == per_simd[3], "k-step %d: %d / %d / %d / %d matrix instructions on the four SIMDs", ks,
                per_simd[0], per_simd[1], per_simd[2], per_simd[3]);
        REQUIRE(ks == 0 || per_simd[0] == simd_step, "k-step %d: %d matrix instructions per SIMD, %d before", ks, per_simd[0], simd_step);
        simd_step = per_simd[0];
    }
    REQUIRE(mfma_total == 3024, "%ld matrix instructions per group", mfma_total);
    REQUIRE((int)visited.size() == RG::TILES * RG::NT, "%d of %d (tile, column tile) units are multiplied", (int)visited.size(), RG::TILES * RG::NT);
    // ---- per unit (hence per row) the visited k-steps are exactly the class's valid-tap-row ones, ascending
    for (const auto& kv : visited) {
        const int cls = RG::tile_cls(kv.first.first);
        std::vector<int> want;
        for (int ks = 0; ks < RG::KSTEPS; ++ks)
            if (ks / RG::SPR >= RG::ty_first(cls) && ks / RG::SPR <= RG::ty_last(cls)) want.push_back(ks);
        REQUIRE(kv.second == want, "tile %d, column tile %d: %d k-steps visited, %d valid", kv.first.first, kv.first.second, (int)kv.second.size(), (int)want.size());
    }
    // ---- every 16-byte unit of a group's source goes to its pixel's record; no two share a place; none lands in a zero record
    std::set<int> dst_seen;
    for (int u = 0; u < RG::UNITS; ++u) {
        const int pix = u / RG::UPP, c4 = u % RG::UPP, img = pix / (RG::IH * RG::IW), q = pix % (RG::IH * RG::IW);
        const int idx = RG::rec(img, q / RG::IW, q % RG::IW), d = idx * RG::PIX + c4 * 8;
        REQUIRE(!zero_record(idx) && idx < RG::RECS && d % 8 == 0 && d / 8 < 0xffff && d + RG::LO + 8 <= RG::ABYTES, "unit %d: record %d, offset %d", u, idx, d);
        REQUIRE(dst_seen.insert(d).second, "two units share LDS offset %d", d);
    }
    REQUIRE(RG::NI * RG::THREADS >= RG::UNITS && RG::NI == 11, "%d rounds of %d threads for %d units", RG::NI, RG::THREADS, RG::UNITS);
    // ---- fragment reads: rows of one sixteen-lane set that share a bank slot (odd record pitch: the residues of the window origins decide)
    int conflicts = 0, conflicts_c = 0, sets = 0;
    for (int tile = 0; tile < RG::TILES; ++tile)
        for (int half = 0; half < 2; ++half) {
            std::set<int> at[16];
            for (int l = 0; l < 32; ++l) {
                if (first_set(l) != (half == 0)) continue;
                const Row r = row_of(table.src[tile * 32 + l]);
                const int rec = rv_origin(r.gi, r.y, r.x, RG::ty_first(RG::tile_cls(tile)));
                at[rec & 15].insert(rec);
            }
            ++sets;
            for (int c = 0; c < 16; ++c) {
                const int n = at[c].size() > 1 ? (int)at[c].size() - 1 : 0;
                conflicts += n;
                if (tile < RG::CT) conflicts_c += n;
            }
        }
    // ---- the hand-counted waits: loads issued behind a slot's ring pieces; sizes the kernel relies on
    int rounds = 0;
    for (int slot = 0; slot < RG::NSLOT; ++slot) {
        REQUIRE(rv_dma_younger(slot) >= 0 && rv_dma_younger(slot) <= 6, "slot %d: %d loads behind its pieces", slot, rv_dma_younger(slot));
        rounds += rv_pre_lo(RG::SS * slot + RG::SS) - rv_pre_lo(RG::SS * slot);
    }
    REQUIRE(rounds == RG::NI && rv_pre_lo(RG::KSTEPS - 3) == RG::NI, "%d of %d rounds requested in the k-loop, all before the mask words", rounds, RG::NI);
    REQUIRE(RG::LDSB <= 160 * 1024, "LDS: %d bytes", RG::LDSB);
    REQUIRE(max_imm + 16 <= 65535, "ds_read immediate %d", max_imm);
    REQUIRE((RG::TILES * 32 * 4) == RG::ROFFB && RG::ABYTES % 16 == 0 && RG::GROUPC == RG::ROWS * 256, "table, alignment, group size");
    std::printf("{\"instance\": \"RVGeom\", \"rows\": %d, \"slots\": %d, \"tiles\": %d, \"ksteps\": %d, \"mfma_per_group\": %ld, \"mfma_per_simd_step\": %d, \"sets\": %d, \"conflicts\": %d, "
                "\"conflicts_c\": %d, \"lds_bytes\": %d, \"source_bytes\": %d, \"max_immediate\": %d, \"rounds_per_thread\": %d}\n",
                RG::ROWS, RG::SLOTS, RG::TILES, RG::KSTEPS, mfma_total, simd_step, sets, conflicts, conflicts_c, RG::LDSB, RG::ABYTES, max_imm, RG::NI);
    return 0;
}
