// Row / element math of the Atari DQN / C51 kernels (dqn_atari.hip: dqn_atari.py, c51_atari.py) and their host twins
// (host_twins.hip): one definition compiled for both sides, so a twin returns the device's bits.  td_target, the softmax, the
// projection, the loss elements, the categorical row and the argmax are dqn_rows.h's; op_mac / op_clamp are offpolicy_rows.h's.  The
// frame words and the host gather serve Rainbow's two rings too (rainbow_rows.h, rainbow_twins.hip).
//
// * The frame ring is ONE u8 array (slots, n_envs, 84, 84, 4), channels-last, as the reference's memory-optimised ReplayBuffer keeps
//   one observation array: a step's obs goes to slot pos, its next_obs to slot (pos + 1) % slots; a sample's next_obs is the frame at
//   (batch_inds + 1) % slots.  Every offset into it is 64-bit: the default ring is 28.2 GB.
// * The head is Linear(512, J), J = n_actions * n_atoms, on the post-ReLU h of Linear(3136, 512).  Every dot product starts at 0.0f and
//   adds its products in ascending index order through op_mac, then adds the bias.
// * Only the taken action's n_atoms logits carry gradient: dz of a row is n_atoms wide.  dh[r, k] adds dz[r, j] * W[a_r * n_atoms + j, k]
//   over ascending j; dW[a * n_atoms + j, k] adds dz[r, j] * h[r, k] over the rows r with a_r == a in ascending r, db likewise; the rows
//   of an action no batch row took are zeros.
#pragma once
#include <string.h>

#include "dqn_rows.h"

namespace mi355ppo {

constexpr int kDaH = 512;            // hidden width: Linear(3136, 512)
constexpr int kDaPix = 84 * 84;      // pixels of a frame; a pixel is 4 bytes (the stack's 4 planes, channels-last)
constexpr int kDaPlanes = 4;
constexpr int kDaMaxOut = 1024;      // n * n_atoms
constexpr int kDaMaxRows = 1024;     // batch rows of an update

MI355_HD bool da_limits(int hidden, int n, int na) {
    return hidden == kDaH && n >= 2 && n <= kDqMaxAct && na >= 1 && na <= kDqMaxAtoms && n * na <= kDaMaxOut;
}
// host-side argument check of the head entry points and of their twins
inline int da_shape(const char* fn, int M, int hidden, int n, int na) {
    MI355_REQUIRE(M >= 1 && M <= kDaMaxRows && da_limits(hidden, n, na), MI355PPO_EINVAL,
                  "%s: rows=%d hidden=%d n_actions=%d n_atoms=%d: the fused Q heads take 1 <= rows <= %d, hidden == %d, 2 <= n_actions <= %d, "
                  "1 <= n_atoms <= %d, n_actions * n_atoms <= %d", fn, M, hidden, n, na, kDaMaxRows, kDaH, kDqMaxAct, kDqMaxAtoms, kDaMaxOut);
    return MI355PPO_OK;
}
// host-side argument check of the ring entry points and of their twins
inline int da_ring_shape(const char* fn, int64_t slots, int N) {
    MI355_REQUIRE(slots > 0 && N > 0, MI355PPO_EINVAL, "%s: slots=%lld n_envs=%d must be positive", fn, (long long)slots, N);
    return MI355PPO_OK;
}

// word (= pixel) offset of frame (slot, env) inside the ring
MI355_HD int64_t da_frame(int64_t slot, int e, int N) { return (slot * N + e) * (int64_t)kDaPix; }
// the slot a sample's next_obs lives in
MI355_HD int64_t da_next_slot(int64_t slot, int64_t slots) { return (slot + 1) % slots; }
// one pixel channels-last: plane c of an (4, 84, 84) stack becomes byte c of the word
MI355_HD uint32_t da_pack(const uint8_t* stack, int p) {
    return (uint32_t)stack[p] | ((uint32_t)stack[kDaPix + p] << 8) | ((uint32_t)stack[2 * kDaPix + p] << 16) | ((uint32_t)stack[3 * kDaPix + p] << 24);
}

// qh_gather_kernel (qhead_wg.h) on the host: sample m's frame to row m, its next frame to row M + m, and the row's scalars.  aliased:
// the next frame is ring_a's at da_next_slot; otherwise ring_b's at the same slot.  ei == nullptr: env 0.
inline void da_gather_host(const uint8_t* ring_a, const uint8_t* ring_b, const int64_t* ring_actions, const float* ring_rewards,
                           const float* ring_dones, const int64_t* bi, const int64_t* ei, int64_t slots, int N, bool aliased, uint8_t* frames,
                           int64_t* actions, float* rewards, float* dones, int M) {
    const size_t fb = (size_t)4 * kDaPix;
    for (int m = 0; m < M; ++m) {
        const int64_t slot = op_clamp(bi[m], slots);
        const int e = ei ? (int)op_clamp(ei[m], N) : 0;
        memcpy(frames + (size_t)m * fb, ring_a + 4 * da_frame(slot, e, N), fb);
        memcpy(frames + (size_t)(M + m) * fb, aliased ? ring_a + 4 * da_frame(da_next_slot(slot, slots), e, N) : ring_b + 4 * da_frame(slot, e, N), fb);
        actions[m] = ring_actions[slot * N + e];
        rewards[m] = ring_rewards[slot * N + e];
        dones[m] = ring_dones[slot * N + e];
    }
}

// z[j] = b[j] + sum_k h[k] * W[j, k]
MI355_HD float da_dot(const float* h, const float* w, float b) {
    float acc = 0.0f;
    for (int k = 0; k < kDaH; ++k) acc = op_mac(acc, h[k], w[k]);
    return acc + b;
}
// dh[k] of one row: the taken action's rows of W (wa = W + a * n_atoms * 512), ascending atom
MI355_HD float da_dh(const float* dz, int na, const float* wa, int k) {
    float acc = 0.0f;
    for (int j = 0; j < na; ++j) acc = op_mac(acc, dz[j], wa[(int64_t)j * kDaH + k]);
    return acc;
}
// dW[a * n_atoms + j, k] (h != nullptr) or db[a * n_atoms + j] (h == nullptr): the rows that took action a, ascending
MI355_HD float da_wgrad(const int* act, const float* dz, int na, int M, int a, int j, const float* h, int k) {
    float acc = 0.0f;
    for (int r = 0; r < M; ++r)
        if (act[r] == a) acc = h ? op_mac(acc, dz[(int64_t)r * na + j], h[(int64_t)r * kDaH + k]) : acc + dz[(int64_t)r * na + j];
    return acc;
}

}  // namespace mi355ppo
