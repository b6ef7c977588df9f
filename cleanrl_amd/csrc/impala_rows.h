// Geometry and row math of the fused IMPALA-CNN trunk kernels (impala.hip) and of their host-pointer twins (host_twins.hip):
// one definition, compiled for both sides without FMA contraction, so the twins run the device kernels' own arithmetic.
//
// The trunk (cleanrl/ppo_procgen.py:86-124, cleanrl/ppg_procgen.py:123-165), on channels-last f32 activations:
//   3 x [ conv3x3(pad 1) -> max_pool2d(3, stride 2, pad 1) -> 2 x ( x + conv1(relu(conv0(relu(x)))) ) ]
// with (C_in, C_out, H = W) = (3, 16, 64), (16, 32, 32), (32, 32, 16) for the three sequences' first convolutions; the residual
// convolutions run at half that size.  Layer l = 5 s + i of sequence s: i = 0 the sequence's conv, 1 / 2 res_block0.conv0 / conv1,
// 3 / 4 res_block1.conv0 / conv1; parameter 2 l is its (C_out, C_in, 3, 3) weight, 2 l + 1 its bias (the state_dict order).
//
// Convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32, whose result is bit for bit a k-ordered fmaf chain:
//   out[p][n] = epilogue( sum_k a[p][k] * Wt[k][n] ),  the sum an fmaf chain from 0.0f in ascending k,
//   k = tap * CP + ci, tap = 3 ky + kx, CP = C_in rounded up to 4 (padded channels: a = 0, Wt = 0, still part of the chain).
//   a[p][k] = input pixel (y + ky - 1, x + kx - 1), channel ci (ReLU'd when the layer's input is), 0 outside the image.
//   Forward:        Wt[k][n] = W[n][ci][tap];            epilogue (acc + bias[n]) (+ residual[p][n]).
//   Data gradient:  the same conv over dY (C_out channels, k = tap * C_out + co) with the taps flipped (imp_wt_dgrad);
//                   epilogue (mask[p][n] > 0 ? acc : 0) (+ residual gradient[p][n]), the mask being the saved tensor the
//                   forward ReLU'd (x > 0 exactly when relu(x) > 0).
//   Weight / bias gradient: dW[n][j] = sum over pixels p of dY[p][n] * a[p][j] (j = k above; column j = 9 CP holds 1.0, the
//                   bias gradient), one fmaf chain per (n, j) in ascending pixel order inside a PART (a fixed run of bands,
//                   imp_part_range); the parts are then folded in a fixed order: kImpFoldGroups runs of consecutive parts
//                   (imp_fold_range), each added in ascending order from 0.0f, then the run sums in ascending order from 0.0f.
//                   No atomics: deterministic.
// Every output pixel's chain reads only its own image, so forward and data-gradient results do not depend on the batch.
//
// Max pool (3, stride 2, pad 1) tie rule -- ATen's: the window is scanned in row-major order over its VALID positions only
// (padding is never chosen), starting from value -inf at the first valid position; a position replaces the running maximum
// when its value is greater, or is NaN.  So the FIRST maximum wins an exact tie.  The argmax byte is the window-relative
// index 3 (iy - (2 oy - 1)) + (ix - (2 ox - 1)) in 0..8.
// Max-pool backward: input pixel (iy, ix) sums, from 0.0f, the gradients of the outputs whose recorded argmax it is, in
// row-major OUTPUT order (oy ascending, then ox) -- the order ATen's CPU kernel adds them in, so the result equals torch's.
#pragma once
#include "common.h"
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace mi355ppo {

constexpr int kImpH = 64;                 // procgen frames: 64 x 64 x 3 (the 64 family)
constexpr int kImpC = 3;
constexpr int kImpFam64 = 0;              // frame family of a trunk: 64 x 64 x 3 f32 frames, planes 64 -> 32 -> 16 -> 8
constexpr int kImpFam84 = 1;              // 84 x 84 x 4 u8 Atari stacks, planes 84 -> 42 -> 21 -> 11 (the pool's (h + 1) / 2)
constexpr int kImpSeqs = 3;
constexpr int kImpLayers = 15;
constexpr int kImpParams = 30;
constexpr int kImpThreads = 256;          // 4 waves per workgroup in every conv launch
constexpr int kImpMaxParts = 512;         // weight-gradient partials per layer (fewer when there are fewer bands)

MI355_HD constexpr int imp_fam_h(int f) { return f == kImpFam84 ? 84 : kImpH; }
MI355_HD constexpr int imp_fam_c(int f) { return f == kImpFam84 ? 4 : kImpC; }
MI355_HD constexpr int imp_half(int h) { return (h + 1) / 2; }                  // max_pool2d(3, stride 2, pad 1)'s output size
MI355_HD constexpr int imp_seq_cin(int f, int s) { return s == 0 ? imp_fam_c(f) : (s == 1 ? 16 : 32); }
MI355_HD constexpr int imp_seq_cout(int s) { return s == 0 ? 16 : 32; }
MI355_HD constexpr int imp_seq_h(int f, int s) {                                // input size of sequence s
    int h = imp_fam_h(f);
    for (int i = 0; i < s; ++i) h = imp_half(h);
    return h;
}
MI355_HD constexpr int imp_layer_cin(int f, int l) { return l % 5 == 0 ? imp_seq_cin(f, l / 5) : imp_seq_cout(l / 5); }
MI355_HD constexpr int imp_layer_cout(int l) { return imp_seq_cout(l / 5); }
MI355_HD constexpr int imp_cpad(int c) { return (c + 3) & ~3; }

// One conv launch's tiling for (input channels CI, output channels CO, size H = W):
//   a wave owns MT 16-pixel tiles x NT 16-channel tiles (4 accumulators); a workgroup (4 waves) owns PIX = 64 MT consecutive
//   output pixel SLOTS: a band of R = min(h, PIX / h) whole rows of NI images (NI > 1 only at 8 x 8, where R = h).  The LDS
//   input tile holds NI x (R + 2) rows x (H + 2) columns with a zero halo, S floats per pixel (CP + 4: the 16 pixels x 4
//   channels of one MFMA operand fall in 64 distinct banks).  An image has BPI = ceil(h / R) bands.
// Ragged bands (the 84 family; in the 64 family R h NI = PIX and R divides h, so nothing below is ever dead): slots at or
//   beyond LIVE = NI R h, and rows at or beyond h in an image's last band, are DEAD.  A dead slot reads a valid LDS cell (slot
//   0's, or the zero rows staged below the image) and is never stored.  In the weight gradient a band's live pixels are its
//   first npix = (live rows) h slots; the chain advances four pixels per MFMA, so a band whose npix is no multiple of 4 ends
//   with 4 - npix % 4 dead steps that enter every chain of the part as fmaf(0.0f, 0.0f, acc) (NOT skipped: the twin adds the
//   same steps; their only effect is that a -0.0f sum becomes +0.0f).
struct ImpGeom {
    int CP, S, KP, KS, NT, MT, PIX, R, NI, COLS, ROWS, LDS_IN, LDS_W, JP, BPI, LIVE;
};
MI355_HD constexpr ImpGeom imp_geom(int ci, int co, int h) {
    ImpGeom g{};
    g.CP = imp_cpad(ci);
    g.S = g.CP == 4 ? 4 : g.CP + 4;
    g.KP = 9 * g.CP;
    g.KS = g.KP / 4;
    g.NT = co / 16;
    g.MT = 4 / g.NT;
    g.PIX = 64 * g.MT;
    g.R = h < g.PIX / h ? h : g.PIX / h;
    g.NI = g.PIX / (g.R * h);
    g.COLS = h + 2;
    g.ROWS = g.NI * (g.R + 2);
    g.LDS_IN = g.ROWS * g.COLS * g.S;
    g.LDS_W = g.KP * co;
    g.JP = (g.KP + 1 + 15) / 16 * 16;     // weight-gradient columns: KP taps x channels, the bias column, zero padding
    g.BPI = (h + g.R - 1) / g.R;
    g.LIVE = g.NI * g.R * h;
    return g;
}

// Bands (one workgroup's PIX pixels) of a batch, and band b's first image / first row.
MI355_HD int64_t imp_bands(const ImpGeom& g, int h, int B) {
    return g.NI == 1 ? (int64_t)B * g.BPI : ((int64_t)B + g.NI - 1) / g.NI;
}
MI355_HD void imp_band(const ImpGeom& g, int h, int64_t b, int64_t* img0, int* y0) {
    if (g.NI == 1) {
        *img0 = b / g.BPI;
        *y0 = (int)(b % g.BPI) * g.R;
    } else {
        *img0 = b * g.NI;
        *y0 = 0;
    }
}
// Live pixels of the band at (img0, y0): whole rows, of the images that exist.
MI355_HD int imp_band_pixels(const ImpGeom& g, int h, int64_t img0, int y0, int B) {
    if (g.NI > 1) return (int)(B - img0 < g.NI ? B - img0 : g.NI) * g.R * h;
    return (h - y0 < g.R ? h - y0 : g.R) * h;
}
MI355_HD int imp_parts(int64_t bands) { return bands < kImpMaxParts ? (int)bands : kImpMaxParts; }
constexpr int kImpFoldGroups = 16;       // runs of consecutive parts folded side by side, then in order
MI355_HD void imp_fold_range(int parts, int g, int* q0, int* q1) {
    *q0 = parts * g / kImpFoldGroups;
    *q1 = parts * (g + 1) / kImpFoldGroups;
}
MI355_HD void imp_part_range(int64_t bands, int parts, int q, int64_t* b0, int64_t* b1) {
    *b0 = bands * q / parts;
    *b1 = bands * (q + 1) / parts;
}

// The layer input as the convolution reads it.
MI355_HD float imp_relu(float v) { return v > 0.0f ? v : 0.0f; }
// A frame byte of the 84 family as layer 0 reads it: torch's ``x / 255.0`` on a u8 tensor (an f32 division, rounded once).
MI355_HD float imp_u8(uint8_t b) { return (float)b / 255.0f; }

// Wt[k][n] of the forward: W (co, ci, 3, 3) with ci < cin, zero for the padded channels.
MI355_HD float imp_wt_fwd(const float* w, int cin, int k, int n) {
    const int cp = imp_cpad(cin), tap = k / cp, ci = k % cp;
    return ci < cin ? w[((size_t)n * cin + ci) * 9 + tap] : 0.0f;
}
// Wt[k][n] of the data gradient dX = conv(dY, Wt): k = tap * cout + co over dY's channels, n = the forward's input channel,
// the kernel flipped (tap -> 8 - tap): dX[y][x][n] = sum dY[y + ky - 1][x + kx - 1][co] W[co][n][2 - ky][2 - kx].
MI355_HD float imp_wt_dgrad(const float* w, int cin, int cout, int k, int n) {
    const int tap = k / cout, co = k % cout;
    return w[((size_t)co * cin + n) * 9 + 8 - tap];
}

// Epilogues (acc: the fmaf chain).
MI355_HD float imp_epi_fwd(float acc, float bias, const float* res) { float v = acc + bias; return res ? v + *res : v; }
MI355_HD float imp_epi_dgrad(float acc, const float* mask, const float* res) {
    float v = mask ? (*mask > 0.0f ? acc : 0.0f) : acc;
    return res ? v + *res : v;
}

// Max pool of output (oy, ox) of one channel: src points at channel c of pixel (0, 0) of the image, pixels C floats apart.
MI355_HD float imp_pool_window(const float* src, int h, int c_stride, int oy, int ox, uint8_t* arg) {
    const int y0 = 2 * oy - 1, x0 = 2 * ox - 1;
    const int ya = y0 < 0 ? 0 : y0, yb = y0 + 3 < h ? y0 + 3 : h;
    const int xa = x0 < 0 ? 0 : x0, xb = x0 + 3 < h ? x0 + 3 : h;
    float best = -INFINITY;
    int bi = (ya - y0) * 3 + (xa - x0);
    for (int y = ya; y < yb; ++y)
        for (int x = xa; x < xb; ++x) {
            const float v = src[((size_t)y * h + x) * c_stride];
            if (v > best || v != v) {
                best = v;
                bi = (y - y0) * 3 + (x - x0);
            }
        }
    *arg = (uint8_t)bi;
    return best;
}

// Max-pool backward of input pixel (iy, ix) of one channel: g / arg point at channel c of output pixel (0, 0), ho = imp_half(h).
MI355_HD float imp_pool_grad(const float* g, const uint8_t* arg, int ho, int c_stride, int iy, int ix) {
    float s = 0.0f;
    const int oya = iy / 2, oyb = (iy + 1) / 2 < ho - 1 ? (iy + 1) / 2 : ho - 1;
    const int oxa = ix / 2, oxb = (ix + 1) / 2 < ho - 1 ? (ix + 1) / 2 : ho - 1;
    for (int oy = oya; oy <= oyb; ++oy)
        for (int ox = oxa; ox <= oxb; ++ox) {
            const size_t o = ((size_t)oy * ho + ox) * c_stride;
            if (arg[o] == (iy - (2 * oy - 1)) * 3 + (ix - (2 * ox - 1))) s = s + g[o];
        }
    return s;
}

// Saved-activation layout (floats, one plane of B images each, in this order): per sequence s the pooled output P (= res
// block 0's input), res block 0's conv0 output h0, its output x1, res block 1's conv0 output h1, and for s < 2 its output y
// (the next sequence's input; the last sequence's output is the caller's y).  Argmax bytes: one plane per sequence.
// Every plane of both families is a multiple of 4 floats, so each starts 16-byte aligned for any B.
MI355_HD constexpr int64_t imp_plane(int f, int s) { const int hp = imp_half(imp_seq_h(f, s)); return (int64_t)hp * hp * imp_seq_cout(s); }
MI355_HD constexpr int64_t imp_saved_floats(int f, int B) {
    int64_t n = 0;
    for (int s = 0; s < kImpSeqs; ++s) n += (s < 2 ? 5 : 4) * imp_plane(f, s);
    return n * B;
}
MI355_HD constexpr int64_t imp_saved_offset(int f, int B, int s, int which) {    // which: 0 P, 1 h0, 2 x1, 3 h1, 4 y
    int64_t n = 0;
    for (int t = 0; t < s; ++t) n += (t < 2 ? 5 : 4) * imp_plane(f, t);
    return (n + which * imp_plane(f, s)) * B;
}
MI355_HD constexpr int64_t imp_argmax_bytes(int f, int B) { return (imp_plane(f, 0) + imp_plane(f, 1) + imp_plane(f, 2)) * B; }
MI355_HD constexpr int64_t imp_argmax_offset(int f, int B, int s) {
    int64_t n = 0;
    for (int t = 0; t < s; ++t) n += imp_plane(f, t);
    return n * B;
}
static_assert(imp_saved_floats(kImpFam84, 1) == 227168 && imp_argmax_bytes(kImpFam84, 1) == 46208, "84 family: 887 KiB saved per image");

}  // namespace mi355ppo

namespace mi355ppo {

// Packed conv weights (the workspace's first region): one piece per launch that reads weights -- the 15 forward convolutions,
// then the data gradients of layers 1 .. 14 (layer 0's input, the frames, needs none).  A piece is in MFMA fragment order:
// float (ks NT + nt) 64 + lane = Wt[4 ks + lane / 16][16 nt + lane % 16], so a lane's B operand is one linear LDS read.
// The pieces do not depend on the frame family: 3 and 4 frame channels both pad to CP = 4, and layer 0 has no data gradient.
MI355_HD constexpr int imp_pack_floats(int l, bool dgrad) {
    return dgrad ? 9 * imp_layer_cout(l) * imp_layer_cin(kImpFam64, l) : 9 * imp_cpad(imp_layer_cin(kImpFam64, l)) * imp_layer_cout(l);
}
MI355_HD constexpr int imp_pack_offset(int l, bool dgrad) {
    int n = 0;
    for (int i = 0; i < (dgrad ? kImpLayers : l); ++i) n += imp_pack_floats(i, false);
    if (dgrad)
        for (int i = 1; i < l; ++i) n += imp_pack_floats(i, true);
    return n;
}
constexpr int kImpPackFloats = imp_pack_offset(kImpLayers, true);

}  // namespace mi355ppo
