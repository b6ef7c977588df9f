// Stand-alone driver of the Rainbow host twins (cleanrl_amd/csrc/rainbow_twins.hip) for the address and undefined-behaviour
// sanitizers: its own main, every buffer a heap allocation of exactly the size the C ABI names, capacities 1, 3 and 37 (no level,
// leaves at two depths, several levels), batches 1, 5 and 32 with duplicate and out-of-range indices.  It checks what it can without a
// reference: the rings hold the last transition written to each slot, every inner node is the f32 sum of its children, sampled
// indices lie in the ring, the largest weight is 1.  Then the noisy layers, the dueling head at (rows, actions, atoms) = (5, 6, 5) -- both
// pmfs of every row sum to 1 -- and the gather on its own.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/rainbow_host_check.cpp \
//       cleanrl_amd/csrc/rainbow_twins.hip cleanrl_amd/csrc/api.hip -o tools/rainbow_host_check && tools/rainbow_host_check
//
// (without the three -Xarch_host flags: the plain build that tests/test_rainbow_twins.py runs).  Never loaded into python.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mi355ppo.h"

namespace {

constexpr int kPix = 84 * 84, kFrame = 4 * kPix;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
double rnd01() { return (rnd() & 0xFFFFFF) / (double)(1 << 24); }

#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            fprintf(stderr, "%s:%d: slots=%d B=%d: %s\n", __FILE__, __LINE__, (int)slots, B, #cond); \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int run(int64_t slots, int B, double alpha) {
    std::vector<uint8_t> ring_obs((size_t)slots * kFrame), ring_next((size_t)slots * kFrame), obs(kFrame), nxt(kFrame);
    std::vector<int64_t> ring_act(slots), size(1, 0), idx(B), act_out(B), action(1);
    std::vector<float> ring_rew(slots), ring_done(slots), tree(2 * slots - 1, 0.0f), state{1.0f, 0.4f}, w(B), loss(B), rew_out(B), done_out(B),
        reward(1), done(1);
    std::vector<double> u(B);
    std::vector<uint8_t> frames((size_t)2 * B * kFrame), last_obs((size_t)slots * kFrame), last_next((size_t)slots * kFrame);
    for (int64_t s = 0; s < slots + 2; ++s) {
        const int64_t pos = s % slots;
        for (int i = 0; i < kFrame; ++i) obs[i] = (uint8_t)rnd(), nxt[i] = (uint8_t)rnd();
        action[0] = rnd() % 18, reward[0] = (float)rnd01(), done[0] = (float)(rnd() & 1);
        CHECK(mi355ppo_rainbow_per_add_u8_cpu(obs.data(), nxt.data(), action.data(), reward.data(), done.data(), ring_obs.data(), ring_next.data(),
                                              ring_act.data(), ring_rew.data(), ring_done.data(), tree.data(), state.data(), size.data(), pos, slots,
                                              alpha) == 0);
        for (int p = 0; p < kPix; ++p)
            for (int c = 0; c < 4; ++c) {
                last_obs[(size_t)pos * kFrame + 4 * p + c] = obs[(size_t)c * kPix + p];
                last_next[(size_t)pos * kFrame + 4 * p + c] = nxt[(size_t)c * kPix + p];
            }
        CHECK(ring_act[pos] == action[0] && ring_rew[pos] == reward[0] && ring_done[pos] == done[0]);
    }
    CHECK(ring_obs == last_obs && ring_next == last_next && size[0] == slots);
    for (int round = 0; round < 3; ++round) {
        for (int i = 0; i < B; ++i) u[i] = rnd01();
        state[1] = 0.4f + 0.3f * round;
        CHECK(mi355ppo_rainbow_per_sample_cpu(u.data(), tree.data(), state.data(), size.data(), slots, idx.data(), w.data(), B) == 0);
        float wmax = 0.0f;
        for (int i = 0; i < B; ++i) {
            CHECK(idx[i] >= 0 && idx[i] < slots && w[i] > 0.0f && w[i] <= 1.0f);
            wmax = w[i] > wmax ? w[i] : wmax;
        }
        CHECK(wmax == 1.0f);
        for (int i = 0; i < B; ++i) loss[i] = (float)((rnd01() - 0.5) * (round == 1 ? 8.0 : 0.5));
        if (round == 1 && B >= 5) idx[0] = slots + 3, idx[1] = -2, idx[B - 1] = idx[2];          // clamped, and a duplicate
        CHECK(mi355ppo_rainbow_per_update_cpu(idx.data(), loss.data(), tree.data(), state.data(), slots, alpha, 1e-6, B) == 0);
        for (int64_t p = 0; p + 1 < slots; ++p) CHECK(tree[p] == tree[2 * p + 1] + tree[2 * p + 2]);
        CHECK(state[0] >= 1.0f);
    }
    CHECK(mi355ppo_rainbow_per_gather_u8_cpu(ring_obs.data(), ring_next.data(), ring_act.data(), ring_rew.data(), ring_done.data(), idx.data(), slots,
                                             frames.data(), act_out.data(), rew_out.data(), done_out.data(), B) == 0);
    for (int m = 0; m < B; ++m) {
        const int64_t s = idx[m] < 0 ? 0 : (idx[m] >= slots ? slots - 1 : idx[m]);
        for (int i = 0; i < kFrame; ++i) {
            CHECK(frames[(size_t)m * kFrame + i] == ring_obs[(size_t)s * kFrame + i]);
            CHECK(frames[(size_t)(B + m) * kFrame + i] == ring_next[(size_t)s * kFrame + i]);
        }
        CHECK(act_out[m] == ring_act[s] && rew_out[m] == ring_rew[s] && done_out[m] == ring_done[s]);
    }
    return 0;
}

int run_noisy(int n, int na) {
    const int64_t slots = 0;
    const int B = 0;
    const int64_t E = mi355ppo_rainbow_noisy_count(n, na, 0), P = mi355ppo_rainbow_noisy_count(n, na, 1);
    CHECK(E > 0 && P == 2 * E);
    std::vector<float> params(P), eps(E), eff(E), g(E), grads(P);
    for (auto& v : params) v = (float)(rnd01() - 0.5);
    for (auto& v : eps) v = (float)(rnd01() - 0.5);
    for (auto& v : g) v = (float)(rnd01() - 0.5);
    CHECK(mi355ppo_rainbow_noisy_compose_f32_cpu(params.data(), eps.data(), eff.data(), n, na) == 0);
    CHECK(mi355ppo_rainbow_noisy_grad_f32_cpu(g.data(), eps.data(), grads.data(), n, na) == 0);
    // the first layer's weight: params = mu | sigma | ..., eps and the effective buffer both start with it
    const int64_t W = (int64_t)512 * 3136;
    for (int64_t i = 0; i < W; i += 997) CHECK(eff[i] == params[i] + params[W + i] * eps[i] && grads[i] == g[i] && grads[W + i] == g[i] * eps[i]);
    return 0;
}

// the dueling head's twins on heap buffers of exactly the ABI's sizes: rows that are done and not, rewards past both clamps
int run_head(int M, int n, int na) {
    const int64_t slots = 0;
    const int B = M;
    const int J = (n + 1) * na, H2 = 1024, HID = 512;
    std::vector<float> h((size_t)M * H2), hn(h.size()), hnt(h.size()), w((size_t)J * HID), b(J), wt(w.size()), bt(J), support(na), rew(M), done(M),
        wts(M), dh(h.size()), dw(w.size()), db(J), sc(2), lps(M), npm((size_t)M * na), tpm((size_t)M * na), q((size_t)M * n);
    std::vector<int64_t> actions(M), best(M), greedy(M);
    for (auto* v : {&h, &hn, &hnt}) for (auto& x : *v) x = (float)rnd01();
    for (auto* v : {&w, &b, &wt, &bt}) for (auto& x : *v) x = (float)(rnd01() - 0.5) * 0.1f;
    for (int k = 0; k < na; ++k) support[k] = -10.0f + 20.0f * k / (na - 1);
    for (int r = 0; r < M; ++r) actions[r] = r == 0 ? n + 2 : rnd() % n, rew[r] = (float)(rnd01() - 0.5) * 60.0f, done[r] = (float)(r & 1), wts[r] = 0.1f + (float)rnd01();
    CHECK(mi355ppo_rainbow_head_act_f32_cpu(h.data(), w.data(), b.data(), support.data(), greedy.data(), q.data(), M, n, na) == 0);
    CHECK(mi355ppo_rainbow_head_fwd_bwd_f32_cpu(h.data(), hn.data(), hnt.data(), w.data(), b.data(), wt.data(), bt.data(), support.data(), actions.data(),
                                                rew.data(), done.data(), wts.data(), 0.970299, -10.0, 10.0, dh.data(), dw.data(), db.data(), sc.data(),
                                                lps.data(), best.data(), npm.data(), tpm.data(), M, n, na) == 0);
    for (int r = 0; r < M; ++r) {
        float sn = 0.0f, st = 0.0f;
        for (int k = 0; k < na; ++k) sn += npm[(size_t)r * na + k], st += tpm[(size_t)r * na + k];
        CHECK(sn > 0.9999f && sn < 1.0001f && st > 0.9999f && st < 1.0001f);       // the projection keeps the mass
        CHECK(greedy[r] >= 0 && greedy[r] < n && best[r] >= 0 && best[r] < n && lps[r] > 0.0f);
    }
    CHECK(sc[0] > 0.0f && sc[1] == sc[1]);
    return 0;
}

// the gather twin on its own: two slots, indices on both sides of the ring
int run_gather() {
    const int64_t slots = 2;
    const int B = 3;
    std::vector<uint8_t> ring_obs((size_t)slots * kFrame), ring_next(ring_obs.size()), frames((size_t)2 * B * kFrame);
    for (auto& v : ring_obs) v = (uint8_t)rnd();
    for (auto& v : ring_next) v = (uint8_t)rnd();
    std::vector<int64_t> ring_act{3, 7}, idx{1, 5, -3}, act_out(B);
    std::vector<float> ring_rew{0.5f, -1.0f}, ring_done{0.0f, 1.0f}, rew_out(B), done_out(B);
    CHECK(mi355ppo_rainbow_per_gather_u8_cpu(ring_obs.data(), ring_next.data(), ring_act.data(), ring_rew.data(), ring_done.data(), idx.data(), slots,
                                             frames.data(), act_out.data(), rew_out.data(), done_out.data(), B) == 0);
    const int64_t want[3] = {1, 1, 0};
    for (int m = 0; m < B; ++m) {
        CHECK(std::equal(frames.begin() + (size_t)m * kFrame, frames.begin() + (size_t)(m + 1) * kFrame, ring_obs.begin() + (size_t)want[m] * kFrame));
        CHECK(std::equal(frames.begin() + (size_t)(B + m) * kFrame, frames.begin() + (size_t)(B + m + 1) * kFrame,
                         ring_next.begin() + (size_t)want[m] * kFrame));
        CHECK(act_out[m] == ring_act[want[m]] && rew_out[m] == ring_rew[want[m]] && done_out[m] == ring_done[want[m]]);
    }
    return 0;
}

}  // namespace

int main() {
    const int64_t caps[3] = {1, 3, 37};
    const int batches[3] = {1, 5, 32};
    for (int64_t slots : caps)
        for (int B : batches)
            for (double alpha : {0.5, 0.6})
                if (run(slots, B, alpha)) return 1;
    if (run_noisy(2, 2) || run_noisy(6, 5) || run_noisy(9, 101)) return 1;
    if (run_head(5, 6, 5) || run_gather()) return 1;
    printf("rainbow host check: ok\n");
    return 0;
}
