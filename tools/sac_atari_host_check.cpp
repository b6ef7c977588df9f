// Stand-alone driver of the discrete-SAC host twins (cleanrl_amd/csrc/sac_atari_twins.hip) for the address and undefined-behaviour
// sanitizers: its own main, every buffer a heap allocation of exactly the size the C ABI names.  Rings of 1, 3 and 7 slots with 1 and
// 2 envs, written past a wrap and gathered with out-of-range indices; the three head twins at (rows, actions) = (1, 2), (5, 6) and
// (64, 18) with an out-of-range action, a done row, an infinite reward and a row whose logits span a gap of 120.  It checks what it
// can without a reference: the rings hold the last transition written to each slot, probabilities sum to 1, sampled actions lie in
// range, the gradient rows of an action nobody took are zero, the dense actor gradient's bias row sums to zero.
//
//   hipcc -x hip --cuda-host-only -std=c++20 -ffp-contract=off -g -O1 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Icleanrl_amd/csrc tools/sac_atari_host_check.cpp \
//       cleanrl_amd/csrc/sac_atari_twins.hip cleanrl_amd/csrc/api.hip -o tools/sac_atari_host_check && tools/sac_atari_host_check
//
// (without the three -Xarch_host flags: the plain build that tests/test_sac_atari_twins.py runs).  Never loaded into python.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "mi355ppo.h"

namespace {

constexpr int kPix = 84 * 84, kFrame = 4 * kPix, kHid = 512;

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}
double rnd01() { return (rnd() & 0xFFFFFF) / (double)(1 << 24); }

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "%s:%d: a=%d b=%d: %s\n", __FILE__, __LINE__, ca, cb, #cond); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int run_ring(int slots, int N) {
    const int ca = slots, cb = N;
    const size_t ring_bytes = (size_t)slots * N * kFrame;
    std::vector<uint8_t> ring_a(ring_bytes), ring_b(ring_bytes), last_a(ring_bytes), last_b(ring_bytes), obs((size_t)N * kFrame), nxt((size_t)N * kFrame);
    std::vector<int64_t> ring_act((size_t)slots * N), action(N);
    std::vector<float> ring_rew((size_t)slots * N), ring_done((size_t)slots * N), reward(N), done(N);
    for (int s = 0; s < slots + 3; ++s) {
        const int64_t pos = s % slots;
        for (auto& v : obs) v = (uint8_t)rnd();
        for (auto& v : nxt) v = (uint8_t)rnd();
        for (int e = 0; e < N; ++e) action[e] = rnd() % 18, reward[e] = (float)rnd01(), done[e] = (float)(rnd() & 1);
        CHECK(mi355ppo_replay_add2_u8_cpu(obs.data(), nxt.data(), action.data(), reward.data(), done.data(), ring_a.data(), ring_b.data(),
                                          ring_act.data(), ring_rew.data(), ring_done.data(), pos, slots, N) == 0);
        for (int e = 0; e < N; ++e) {
            const size_t f = ((size_t)pos * N + e) * kFrame;
            for (int p = 0; p < kPix; ++p)
                for (int c = 0; c < 4; ++c) {
                    last_a[f + 4 * p + c] = obs[(size_t)e * kFrame + (size_t)c * kPix + p];
                    last_b[f + 4 * p + c] = nxt[(size_t)e * kFrame + (size_t)c * kPix + p];
                }
            CHECK(ring_act[pos * N + e] == action[e] && ring_rew[pos * N + e] == reward[e] && ring_done[pos * N + e] == done[e]);
        }
    }
    CHECK(ring_a == last_a && ring_b == last_b);
    CHECK(mi355ppo_replay_add2_u8_cpu(obs.data(), nxt.data(), action.data(), reward.data(), done.data(), ring_a.data(), ring_b.data(), ring_act.data(),
                                      ring_rew.data(), ring_done.data(), slots, slots, N) == MI355PPO_EINVAL);
    const int M = 5;
    std::vector<int64_t> bi{0, slots - 1, slots + 4, -3, slots / 2}, ei{0, N - 1, N + 2, -1, 0}, act_out(M);
    std::vector<float> rew_out(M), done_out(M);
    std::vector<uint8_t> frames((size_t)2 * M * kFrame);
    CHECK(mi355ppo_replay_gather2_u8_cpu(ring_a.data(), ring_b.data(), ring_act.data(), ring_rew.data(), ring_done.data(), bi.data(), ei.data(), slots, N,
                                         frames.data(), act_out.data(), rew_out.data(), done_out.data(), M) == 0);
    for (int m = 0; m < M; ++m) {
        const int64_t s = bi[m] < 0 ? 0 : (bi[m] >= slots ? slots - 1 : bi[m]), e = ei[m] < 0 ? 0 : (ei[m] >= N ? N - 1 : ei[m]);
        const size_t f = ((size_t)s * N + e) * kFrame;
        for (int i = 0; i < kFrame; ++i) {
            CHECK(frames[(size_t)m * kFrame + i] == ring_a[f + i]);
            CHECK(frames[(size_t)(M + m) * kFrame + i] == ring_b[f + i]);
        }
        CHECK(act_out[m] == ring_act[s * N + e] && rew_out[m] == ring_rew[s * N + e] && done_out[m] == ring_done[s * N + e]);
    }
    return 0;
}

int run_heads(int M, int n) {
    const int ca = M, cb = n;
    const size_t hw = (size_t)M * kHid, ww = (size_t)n * kHid;
    std::vector<std::vector<float>> h(6, std::vector<float>(hw)), w(5, std::vector<float>(ww)), b(5, std::vector<float>(n));
    for (auto& v : h) for (auto& x : v) x = (float)rnd01();
    for (auto& v : w) for (auto& x : v) x = (float)(rnd01() - 0.5) * 0.12f;
    for (auto& v : b) for (auto& x : v) x = (float)(rnd01() - 0.5) * 0.2f;
    // the actor is w[2]: hidden column 0 feeds actions 0 and 1 with +-60 on the last row alone
    for (int j = 0; j < n; ++j) w[2][(size_t)j * kHid] = j == 0 ? 60.0f : (j == 1 ? -60.0f : 0.0f);
    for (int which : {2, 5})
        for (int r = 0; r < M; ++r) h[which][(size_t)r * kHid] = r == M - 1 ? 1.0f : 0.0f;
    std::vector<int64_t> actions(M), sampled(M);
    std::vector<float> rew(M), done(M), alpha{0.2f}, noise((size_t)M * n), probs((size_t)M * n);
    for (int r = 0; r < M; ++r) actions[r] = r == 0 ? n + 2 : rnd() % (n - 1), rew[r] = (float)(rnd01() - 0.5) * 6.0f, done[r] = (float)(r & 1);
    if (M > 2) rew[2] = std::numeric_limits<float>::infinity();
    for (auto& x : noise) x = (float)(-std::log(1.0 - rnd01()) + 1e-6);
    CHECK(mi355ppo_sacd_head_act_f32_cpu(h[5].data(), w[2].data(), b[2].data(), noise.data(), sampled.data(), probs.data(), M, kHid, n) == 0);
    for (int r = 0; r < M; ++r) {
        float s = 0.0f;
        for (int a = 0; a < n; ++a) s += probs[(size_t)r * n + a];
        CHECK(s > 0.9999f && s < 1.0001f && sampled[r] >= 0 && sampled[r] < n);
    }
    CHECK(probs[(size_t)(M - 1) * n + 1] == 0.0f);
    std::vector<float> dh1(hw), dh2(hw), dw1(ww), db1(n), dw2(ww), db2(n), sc(4), V(M), y(M);
    CHECK(mi355ppo_sacd_critic_fwd_bwd_f32_cpu(h[0].data(), h[1].data(), h[2].data(), h[3].data(), h[4].data(), w[0].data(), b[0].data(), w[1].data(),
                                               b[1].data(), w[2].data(), b[2].data(), w[3].data(), b[3].data(), w[4].data(), b[4].data(),
                                               actions.data(), rew.data(), done.data(), alpha.data(), 0.99, dh1.data(), dh2.data(), dw1.data(),
                                               db1.data(), dw2.data(), db2.data(), sc.data(), V.data(), y.data(), M, kHid, n) == 0);
    for (int r = 0; r < M; ++r) CHECK(std::isfinite(V[r]) && (std::isfinite(y[r]) || r == 2));
    bool last_taken = false;
    for (int r = 0; r < M; ++r) last_taken |= (actions[r] >= n - 1);           // row 0's out-of-range action is clamped onto n - 1
    if (!last_taken)
        for (int k = 0; k < kHid; ++k) CHECK(dw1[(size_t)(n - 1) * kHid + k] == 0.0f && dw2[(size_t)(n - 1) * kHid + k] == 0.0f);
    CHECK(mi355ppo_sacd_critic_fwd_bwd_f32_cpu(h[0].data(), h[1].data(), h[2].data(), h[3].data(), h[4].data(), w[0].data(), b[0].data(), w[1].data(),
                                               b[1].data(), w[2].data(), b[2].data(), w[3].data(), b[3].data(), w[4].data(), b[4].data(),
                                               actions.data(), rew.data(), done.data(), alpha.data(), 0.99, dh1.data(), dh2.data(), dw1.data(),
                                               db1.data(), dw2.data(), db2.data(), sc.data(), nullptr, nullptr, M, kHid, n) == 0);
    std::vector<float> dh(hw), dw(ww), db(n), er(M), loss(1);
    CHECK(mi355ppo_sacd_actor_fwd_bwd_f32_cpu(h[5].data(), h[0].data(), h[1].data(), w[2].data(), b[2].data(), w[0].data(), b[0].data(), w[1].data(),
                                              b[1].data(), alpha.data(), 0.89 * std::log((double)n), dh.data(), dw.data(), db.data(), er.data(),
                                              loss.data(), M, kHid, n) == 0);
    double sum_db = 0.0;
    for (int j = 0; j < n; ++j) sum_db += db[j];
    CHECK(std::isfinite(loss[0]) && std::fabs(sum_db) < 1e-5);                 // a softmax's logit gradients sum to zero in every row
    for (int r = 0; r < M; ++r) CHECK(std::isfinite(er[r]));
    CHECK(mi355ppo_sacd_actor_fwd_bwd_f32_cpu(h[5].data(), h[0].data(), h[1].data(), w[2].data(), b[2].data(), w[0].data(), b[0].data(), w[1].data(),
                                              b[1].data(), alpha.data(), 1.0, dh.data(), dw.data(), db.data(), er.data(), loss.data(), M, kHid,
                                              19) == MI355PPO_EINVAL);
    return 0;
}

}  // namespace

int main() {
    for (int slots : {1, 3, 7})
        for (int N : {1, 2})
            if (run_ring(slots, N)) return 1;
    if (run_heads(1, 2) || run_heads(5, 6) || run_heads(64, 18)) return 1;
    printf("sac_atari host check: ok\n");
    return 0;
}
