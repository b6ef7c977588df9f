"""The host twins of the Atari DQN / C51 kernels (csrc/dqn_atari.hip): the frame ring against the reference buffer's rules, the wide
heads against the reference's ops -- bit for bit where the reference is an exact recipe (argmax, td_target, the projection), within
twice the f32 reference's own error against float64 autograd plus 2e-6 everywhere else (DESIGN.md section 3.11's bar)."""
import ctypes

import pytest
import torch

import bounds_cases as B
import dqn_atari_cases as A
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")


# ================================================================================================== ring
@pytest.mark.parametrize("slots", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 3])
def test_ring_follows_the_reference_buffers_rules(slots, N):
    """Enough adds that the ring wraps and an episode is truncated: truncated episodes leave a ``final_observation`` in slot pos + 1 that the next add overwrites,
    and with one slot next_obs is what stays."""
    steps = A.ring_steps(slots, N, max(slots + 3, 8))
    ring, ref, (bi, ei), out = A.run_ring(H, CPU, slots, N, steps)
    assert torch.equal(ring[0], ref.frames_hwc())
    assert torch.equal(ring[1], torch.from_numpy(ref.actions)) and torch.equal(ring[2], torch.from_numpy(ref.rewards))
    assert torch.equal(ring[3], torch.from_numpy(ref.dones))
    obs, nxt, act, rew, done = ref.get(bi, ei)
    M = len(bi)
    hwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    assert torch.equal(out[0][:M], hwc(obs)) and torch.equal(out[0][M:], hwc(nxt))
    assert torch.equal(out[1], torch.from_numpy(act)) and torch.equal(out[2], torch.from_numpy(rew)) and torch.equal(out[3], torch.from_numpy(done))
    assert (bi == slots - 1).any()                                           # whose next frame is slot 0
    assert not torch.equal(steps[4][1], steps[5][0])                         # the quirk: step 4's final_observation did not survive step 5's add


def test_ring_entry_points_refuse_bad_arguments():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mi355ppo_replay_add_u8_cpu(p, p, p, p, p, p, p, p, p, 2, 2, 1) == -1
    assert lib.mi355ppo_replay_add_u8(p, p, p, p, p, p, p, p, p, 0, 0, 1, None) == -1
    assert lib.mi355ppo_replay_add_u8(p, p, p, p, p, None, p, p, p, 0, 4, 1, None) == -1
    assert lib.mi355ppo_replay_gather_u8(p, p, p, p, p, p, 4, 1, p, p, p, p, 1025, None) == -1
    assert lib.mi355ppo_replay_gather_u8_cpu(p, p, p, p, p, p, 4, 0, p, p, p, p, 8) == -1


# ================================================================================================== heads
def _refs(c):
    return A.reference_head(c, torch.float64), A.reference_head(c, torch.float32)


@pytest.mark.parametrize("M,n,na", A.HEAD_GRID)
def test_heads_against_the_reference(M, n, na):
    c = A.make_head_case(M, n, na)
    got = A.run_heads(H, c, CPU)
    r64, r32 = _refs(c)
    # exact recipes, given the twin's own target side
    assert torch.equal(got["act"], torch.argmax(got["q"], dim=1))
    if na == 1:
        target_max, _ = got["aux_a"].max(dim=1)
        assert torch.equal(got["aux_b"], c.rewards + c.gamma * target_max * (1 - c.dones))
    else:
        want = A.projection(got["aux_a"], c.rewards.reshape(-1, 1), c.dones.reshape(-1, 1), c.atoms, c.gamma, c.v_min, c.v_max)
        assert torch.equal(got["aux_b"], want)
    # everything else: twice the f32 reference's own error against float64, plus 2e-6
    for k in ("q", "aux_a", "aux_b", "scalars", "dh", "dw", "db"):
        ok, err, own = A.within_bar(got[k], r64[k], r32[k])
        print(f"M={M} n={n} atoms={na} {k}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (k, err, own)
    # untaken actions: exact zeros, written
    taken = set(c.actions.tolist())
    for a in range(n):
        if a not in taken:
            assert not got["dw"].view(n, na, -1)[a].any() and not got["db"].view(n, na)[a].any()


@pytest.mark.parametrize("na", [1, 5])
def test_argmax_ties_go_to_the_lowest_index_and_nan_is_the_maximum(na):
    c = A.make_head_case(5, 6, na, tie=True)
    got = A.run_heads(H, c, CPU)
    assert torch.equal(got["q"][:, 0], got["q"][:, 1])
    assert torch.equal(got["act"], torch.argmax(got["q"], dim=1)) and not (got["act"] == 1).any()
    c.h[2, 7] = float("nan")
    got = A.run_heads(H, c, CPU)
    assert got["act"][2] == 0 and torch.equal(got["act"], torch.argmax(got["q"], dim=1))


@pytest.mark.parametrize("n,na", [(6, 5), (18, 51)])
def test_no_gradient_where_the_pmf_clamp_is_active(n, na):
    """Atom 0 of every action sits near e^-30 in the online head: ``clamp(1e-5)`` is active there and passes no gradient."""
    c = A.make_head_case(32, n, na, dead=True)
    got = A.run_heads(H, c, CPU)
    r64, r32 = _refs(c)
    for k in ("scalars", "dh", "dw", "db"):
        ok, err, own = A.within_bar(got[k], r64[k], r32[k])
        assert ok, (k, err, own)
    live = A.run_heads(H, A.make_head_case(32, n, na), CPU)
    assert got["db"].view(n, na)[:, 0].abs().max() < 1e-6 * live["db"].view(n, na)[:, 0].abs().max()


def test_projection_edges_are_reached():
    """The case generator's first rows: b integral inside the support, b = 0, b at the top (l == u there), both clamps, with d = 1 and 0."""
    def b_of(c):
        tz = (c.rewards.reshape(-1, 1) + c.gamma * c.atoms * (1 - c.dones.reshape(-1, 1))).clamp(c.v_min, c.v_max)
        return (tz - c.v_min) / (c.atoms[1] - c.atoms[0])

    c = A.make_head_case(32, 6, 51)
    b = b_of(c)
    top = (b[[2, 3, 5]] - 50).abs().max()                                     # delta_z = 0.4 is inexact: b lands within rounding of the top
    assert (b[[1, 4, 6]] == 0).all() and top < 1e-4
    assert c.dones[:3].eq(1).all() and c.dones[3:5].eq(0).all()
    small = A.make_head_case(8, 2, 5, v_min=-2.0, v_max=2.0)
    b = b_of(small)
    assert (b[0] == 2).all() and (b[1] == 0).all() and (b[2] == 4).all() and (b[3] == 4).all() and (b[4] == 0).all()      # delta_z = 1: b integral, l == u
    got = A.run_heads(H, small, CPU)
    assert torch.equal(got["aux_b"], A.projection(got["aux_a"], small.rewards.reshape(-1, 1), small.dones.reshape(-1, 1), small.atoms, small.gamma, -2.0, 2.0))


@pytest.mark.parametrize("na", [1, 51])
def test_each_row_of_a_batch_is_the_row_alone(na):
    """dh of row r in a batch of 32 is that row's dh alone, times 1 / 32 (the mean; a power of two, so exact)."""
    c = A.make_head_case(32, 6, na)
    full = A.run_heads(H, c, CPU)
    for r in (0, 3, 31):
        one = A.make_head_case(1, 6, na)
        for k in ("h", "h_next", "actions", "rewards", "dones"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in ("w", "b", "wt", "bt"):
            setattr(one, k, getattr(c, k))
        alone = A.run_heads(H, one, CPU)
        assert torch.equal(full["dh"][r], alone["dh"][0] / 32)


def test_two_calls_are_bit_identical():
    c = A.make_head_case(32, 18, 51)
    a, b = A.run_heads(H, c, CPU), A.run_heads(H, c, CPU)
    assert all(A.same(a[k], b[k]) for k in a)


def test_sizes_outside_the_limits_are_refused_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    td = lambda M, hid, n: lib.mi355ppo_dqn_head_td_fwd_bwd_f32(p, p, p, p, p, p, p, p, p, 0.99, p, p, p, p, None, None, M, hid, n, p, 1 << 30, None)  # noqa: E731
    c51 = lambda M, n, na: lib.mi355ppo_c51_head_fwd_bwd_f32(p, p, p, p, p, p, p, p, p, p, 0.99, -10.0, 10.0, p, p, p, p, None, None, M, 512, n, na, p, 1 << 30, None)  # noqa: E731
    assert td(0, 512, 4) == -1 and td(1025, 512, 4) == -1 and td(32, 256, 4) == -1 and td(32, 512, 1) == -1 and td(32, 512, 19) == -1
    assert b"hidden == 512" in lib.mi355ppo_last_error()
    assert c51(32, 4, 1) == -1 and c51(32, 4, 102) == -1 and c51(32, 11, 101) == -1
    assert lib.mi355ppo_dqn_head_act_f32(p, p, p, None, p, None, 1, 512, 4, 51, p, 1 << 30, None) == -1          # atoms missing
    assert lib.mi355ppo_dqn_head_td_fwd_bwd_f32(p, p, p, p, p, p, p, p, p, 0.99, p, p, p, p, None, None, 32, 512, 4, p, 16, None) == -4
    assert lib.mi355ppo_dqn_head_workspace_bytes(32, 18, 51) == (2 * 32 * 918 + 2 * 64 + 32 * 51 + 32) * 4
    assert lib.mi355ppo_dqn_head_workspace_bytes(32, 18, 57) == 0 and lib.mi355ppo_dqn_head_act_workspace_bytes(3, 18, 51) == 3 * 918 * 4
    from cleanrl_amd import ops
    assert ops.dqn_head_limits_ok(18, 51, 32) and not ops.dqn_head_limits_ok(18, 57) and not ops.dqn_head_limits_ok(1, 1)


# ================================================================================================== guard bands
@pytest.mark.parametrize("shape", A.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_twins_stay_inside_their_outputs(shape, monkeypatch):
    B.check(A.bounds_head_case(*shape), H, CPU, monkeypatch)


@pytest.mark.parametrize("shape", A.GUARD_RINGS, ids=lambda s: "-".join(map(str, s)))
def test_ring_twins_stay_inside_the_ring_and_the_batch(shape, monkeypatch):
    B.check(A.bounds_ring_case(*shape), H, CPU, monkeypatch)


def test_frame_offsets_past_2_31_words_are_64_bit():
    """``da_frame`` (the one function the kernels and the twins compile) at slot 400,000: word offset 2.8e9, past 2^31.  The twin is
    handed ring pointers moved back by exactly that slot's offset, so a correct 64-bit offset lands in a two-frame buffer here; an
    ``int`` offset would not come back to it."""
    lib = _lib.load()
    S, fb = 400_000, 84 * 84 * 4
    assert S * 84 * 84 > 1 << 31
    g = torch.Generator().manual_seed(1)
    two = torch.randint(0, 256, (2, 84, 84, 4), dtype=torch.uint8, generator=g)
    act, rew, done = torch.tensor([3, 5]), torch.tensor([0.5, -1.0]), torch.tensor([0.0, 1.0])
    out = (torch.zeros((2, 84, 84, 4), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1), torch.zeros(1))
    bi, ei = torch.tensor([S]), torch.tensor([0])
    P = lambda t, back: ctypes.c_void_p(t.data_ptr() - back)  # noqa: E731
    rc = lib.mi355ppo_replay_gather_u8_cpu(P(two, S * fb), P(act, 8 * S), P(rew, 4 * S), P(done, 4 * S), P(bi, 0), P(ei, 0), S + 2, 1,
                                           P(out[0], 0), P(out[1], 0), P(out[2], 0), P(out[3], 0), 1)
    assert rc == 0 and torch.equal(out[0], two) and out[1].item() == 3 and out[2].item() == 0.5 and out[3].item() == 0.0
    fresh = torch.zeros_like(two)
    obs = two.permute(0, 3, 1, 2).contiguous()
    rc = lib.mi355ppo_replay_add_u8_cpu(P(obs[0:1], 0), P(obs[1:2], 0), P(act, 0), P(rew, 0), P(done, 0), P(fresh, S * fb), P(out[1], 8 * S),
                                        P(out[2], 4 * S), P(out[3], 4 * S), S, S + 2, 1)
    assert rc == 0 and torch.equal(fresh, two)
