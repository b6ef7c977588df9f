"""The Rainbow entry points' host twins (csrc/rainbow_twins.hip) against the reference's recorded buffer, torch and autograd, and
``agents.NoisyDuelingDistributionalNetwork`` against the reference's seeded construction.  No GPU."""
import ctypes
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bounds_cases as B
import rainbow_cases as R
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_entry_point_has_a_twin_and_is_bound():
    for n in ("per_add_u8", "per_sample", "per_gather_u8", "per_update", "noisy_compose_f32", "noisy_grad_f32", "head_act_f32", "head_fwd_bwd_f32"):
        assert f"mi355ppo_rainbow_{n}" in _lib.SIGNATURES and f"mi355ppo_rainbow_{n}_cpu" in _lib.SIGNATURES
        name = "rainbow_" + n.replace("_f32", "")
        assert callable(getattr(ops, name)) and callable(getattr(H, name)) and name in ops.__all__
    assert _lib.load().mi355ppo_version() == 271


# ================================================================================================== the networks
@pytest.mark.parametrize("k", [0, 1])
def test_seeded_networks_equal_the_references_tensor_for_tensor(k):
    """Same seed, same draws in the same order: every parameter and noise buffer at the fixture's stride, after construction and
    after one more ``reset_noise()``."""
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork

    d = R.network_fixture()
    seed, n, na, v_min, v_max = d[f"n{k}_meta"]
    torch.manual_seed(int(seed))
    net = NoisyDuelingDistributionalNetwork(SimpleNamespace(single_action_space=SimpleNamespace(n=int(n))), int(na), int(v_min), int(v_max))
    assert list(net.state_dict().keys()) == list(d[f"n{k}_names"])
    flat = lambda: torch.cat([t.detach().reshape(-1) for t in net.state_dict().values()])[::int(d["stride"])]  # noqa: E731
    assert torch.equal(flat(), torch.from_numpy(d[f"n{k}_init"]))
    net.reset_noise()
    assert torch.equal(flat(), torch.from_numpy(d[f"n{k}_renoised"]))
    assert net.delta_z == (int(v_max) - int(v_min)) / (int(na) - 1) and net.training
    x = torch.randint(0, 256, (3, 4, 84, 84)).float()
    dist = net(x)
    assert dist.shape == (3, int(n), int(na)) and torch.allclose(dist.sum(2), torch.ones(3, int(n)), atol=1e-5)
    net.eval()
    assert not torch.equal(net(x), dist)                                      # eval drops the noise, as the reference's does


# ================================================================================================== the buffer
def _fixture_ids():
    d = R.per_fixture()
    return list(range(int(d["n_cases"])))


@pytest.mark.parametrize("k", _fixture_ids())
def test_buffer_twins_follow_the_references_recorded_buffer(k):
    """Capacities 1, 2, 3, 5, 37, 64 x batches 1, 5, 32, alpha 0.5 / 0.6, four betas, duplicate indices: indices equal, inner nodes
    bit-equal given the leaves, leaves and ``max_priority ** alpha`` within 1 ulp, weights within 4 ulp, max_priority and size equal."""
    c = R.fixture_case(R.per_fixture(), k)
    adds, samples, updates = R.replay_fixture_case(H, CPU, c)
    assert adds >= c.slots + 3 and samples == 5 and updates == 5


def test_the_fixture_covers_what_the_issue_lists():
    d = R.per_fixture()
    cases = [R.fixture_case(d, k) for k in range(int(d["n_cases"]))]
    assert {c.slots for c in cases} == {1, 2, 3, 5, 37, 64} and {c.B for c in cases} == {1, 5, 32} and {c.alpha for c in cases} == {0.5, 0.6}
    assert len({b for c in cases for b in c.beta[c.kind == 1]}) >= 4
    dup = [c for c in cases if any(len(set(c.idx[i])) < c.B for i in np.flatnonzero(c.kind == 2))]
    assert len(dup) >= 10
    assert any(c.maxp[-1] > 1.0 for c in cases)


@pytest.mark.parametrize("slots,B", [(1, 1), (2, 5), (3, 32), (5, 5), (37, 32), (64, 1)])
def test_ring_contents_and_tree_invariants_of_a_free_run(slots, B):
    T = R.per_script(slots, B)
    out = R.run_per(H, CPU, slots, B, T)
    R.check_ring_contents(out, T, slots)
    for k in range(3):
        assert R.same_bits(out[f"tree{k}"], R.rebuild(out[f"tree{k}"], slots))
        assert bool((out[f"indices{k}"] >= 0).all()) and bool((out[f"indices{k}"] < slots).all())
        assert out[f"weights{k}"].max().item() == 1.0
    p = T["loss"].abs().float() + np.float32(R.EPS)
    assert out["state"][0].item() == max(1.0, p.max().item()) and out["state"][1].item() == np.float32(0.7)


def test_duplicate_indices_keep_the_highest_batch_position():
    slots = 5
    buf = ops.rainbow_new_buffer(slots, CPU)
    idx = torch.tensor([3, 1, 3, 3, 1])
    loss = torch.tensor([0.5, 0.25, 2.0, 0.125, 4.0])
    H.rainbow_per_update(buf, idx, loss, 0.5, 0.0)
    leaves = buf[5][slots - 1:]
    assert torch.equal(leaves, torch.tensor([0.0, 2.0, 0.0, 0.125 ** 0.5, 0.0])) and buf[6][0].item() == 4.0
    assert R.same_bits(buf[5], R.rebuild(buf[5], slots))


def test_frame_offsets_past_2_31_words_are_64_bit_in_both_rings():
    """``da_frame`` at slot 400,000 (word offset 2.8e9): the twins are handed ring pointers moved back by exactly that slot's offset,
    so a 64-bit offset lands in the one-frame buffers here; the tree (3.2 MB at this size) is real."""
    lib = _lib.load()
    S, fb = 400_000, 84 * 84 * 4
    slots = S + 2
    assert S * 84 * 84 > 1 << 31
    g = torch.Generator().manual_seed(1)
    a, b = (torch.randint(1, 256, (1, 84, 84, 4), dtype=torch.uint8, generator=g) for _ in range(2))
    act, rew, done = torch.tensor([3]), torch.tensor([0.5]), torch.tensor([1.0])
    out = (torch.zeros((2, 84, 84, 4), dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.zeros(1), torch.zeros(1))
    P = lambda t, back=0: ctypes.c_void_p(t.data_ptr() - back)  # noqa: E731
    at = torch.tensor([S])
    rc = lib.mi355ppo_rainbow_per_gather_u8_cpu(P(a, S * fb), P(b, S * fb), P(act, 8 * S), P(rew, 4 * S), P(done, 4 * S), P(at), slots,
                                                P(out[0]), P(out[1]), P(out[2]), P(out[3]), 1)
    assert rc == 0 and torch.equal(out[0][0], a[0]) and torch.equal(out[0][1], b[0]) and out[1].item() == 3 and out[3].item() == 1.0
    fa, fb_ = torch.zeros_like(a), torch.zeros_like(b)
    tree, state, size = torch.zeros(2 * slots - 1), torch.tensor([1.0, 0.4]), torch.zeros(1, dtype=torch.int64)
    chw = lambda t: t.permute(0, 3, 1, 2).contiguous()  # noqa: E731
    ca, cb = chw(a), chw(b)
    rc = lib.mi355ppo_rainbow_per_add_u8_cpu(P(ca), P(cb), P(act), P(rew), P(done), P(fa, S * fb), P(fb_, S * fb), P(out[1], 8 * S),
                                             P(out[2], 4 * S), P(out[3], 4 * S), P(tree), P(state), P(size), S, slots, 0.5)
    assert rc == 0 and torch.equal(fa, a) and torch.equal(fb_, b)
    assert tree[slots - 1 + S].item() == 1.0 and tree[0].item() == 1.0 and tree.sum().item() == (slots + S).bit_length() and size.item() == 1


def test_refusals_come_before_any_work():
    lib = _lib.load()
    t = torch.zeros(64)
    p = ctypes.c_void_p(t.data_ptr())
    assert lib.mi355ppo_rainbow_per_sample_cpu(p, p, p, p, 4, p, p, 0) == -1 and b"rows" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_rainbow_per_sample_cpu(p, p, p, p, 4, p, p, 1025) == -1
    assert lib.mi355ppo_rainbow_per_sample_cpu(p, p, p, p, 0, p, p, 4) == -1 and b"slots" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_rainbow_per_update_cpu(p, None, p, p, 4, 0.5, 1e-6, 4) == -1 and b"null" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_rainbow_per_add_u8_cpu(*([p] * 13), 4, 4, 0.5) == -1 and b"pos" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_rainbow_per_gather_u8_cpu(*([p] * 6), 4, p, p, p, p, 0) == -1
    for n, na in ((1, 51), (19, 5), (6, 1), (6, 102), (18, 54)):
        assert lib.mi355ppo_rainbow_noisy_compose_f32_cpu(p, p, p, n, na) == -1 and b"n_actions" in lib.mi355ppo_last_error()
        assert lib.mi355ppo_rainbow_noisy_count(n, na, 0) == 0 and not ops.rainbow_noisy_limits_ok(n, na)
        with pytest.raises(ValueError):
            ops.rainbow_noisy_counts(n, na)
    # the device entry points validate before their first HIP call: the same refusals without a device
    assert lib.mi355ppo_rainbow_per_sample(p, p, p, p, 4, p, p, 0, None) == -1
    assert lib.mi355ppo_rainbow_per_update(p, p, p, p, 0, 0.5, 1e-6, 4, None) == -1
    assert lib.mi355ppo_rainbow_per_add_u8(*([p] * 13), -1, 4, 0.5, None) == -1
    assert lib.mi355ppo_rainbow_per_gather_u8(*([p] * 6), 4, p, p, p, p, 1025, None) == -1
    assert lib.mi355ppo_rainbow_noisy_compose_f32(p, p, p, 19, 51, None) == -1 and lib.mi355ppo_rainbow_noisy_grad_f32(p, None, p, 6, 51, None) == -1
    with pytest.raises(TypeError):
        ops.rainbow_per_sample(ops.rainbow_new_buffer(2, CPU), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.int64), torch.zeros(2))


# ================================================================================================== the noisy layers
@pytest.mark.parametrize("n,na", R.NOISY_SHAPES)
def test_compose_and_grad_twins_are_torchs_bits(n, na):
    net = R.make_network(n, na)
    params, eps = R.noisy_flat(net)
    E, P = ops.rainbow_noisy_counts(n, na)
    assert (eps.numel(), params.numel()) == (E, P) == (_lib.load().mi355ppo_rainbow_noisy_count(n, na, 0), _lib.load().mi355ppo_rainbow_noisy_count(n, na, 1))
    g = torch.randn(E, generator=torch.Generator().manual_seed(3))
    want_eff, want_grads = R.reference_noisy(net, g)
    got = R.run_noisy(H, CPU, n, na, dict(params=params, eps=eps, g=g))
    assert R.same_bits(got["effective"], want_eff) and R.same_bits(got["grads"], want_grads)
    # the layout: the value stream's 512 hidden rows, then the advantage stream's; the value stream's n_atoms output rows first
    v0, v2, a0, a2 = net.noisy_layers()
    W_fc = got["effective"][:1024 * 3136].view(1024, 3136)
    assert torch.equal(W_fc[512:], (a0.weight_mu + a0.weight_sigma * a0.weight_epsilon).detach())
    W_out = got["effective"][1024 * 3136 + 1024:][:(n + 1) * na * 512].view((n + 1) * na, 512)
    assert torch.equal(W_out[:na], (v2.weight_mu + v2.weight_sigma * v2.weight_epsilon).detach())


# ================================================================================================== guard bands
@pytest.mark.parametrize("shape", R.GUARD_PER, ids=lambda s: "-".join(map(str, s)))
def test_buffer_twins_stay_inside_their_buffers(shape, monkeypatch):
    B.check(R.bounds_per_case(*shape), H, CPU, monkeypatch)


@pytest.mark.parametrize("shape", R.GUARD_NOISY, ids=lambda s: "-".join(map(str, s)))
def test_noisy_twins_stay_inside_their_buffers(shape, monkeypatch):
    B.check(R.bounds_noisy_case(*shape), H, CPU, monkeypatch)


# ================================================================================================== the sanitizer driver
def test_the_standalone_host_check_builds_and_passes_without_sanitizers(tmp_path):
    """tools/rainbow_host_check.cpp: its own ``main`` over the tree and ring twins at capacities 1, 3 and 37.  Here it is built plain
    and run; the address / undefined-behaviour sanitizer build of the same program is a command in its header (a stand-alone program,
    never under python)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path / "rainbow_host_check")
    csrc = os.path.join(ROOT, "cleanrl_amd", "csrc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++20", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tools", "rainbow_host_check.cpp"), os.path.join(csrc, "rainbow_twins.hip"), os.path.join(csrc, "api.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)


# ================================================================================================== the dueling distributional head
@pytest.mark.parametrize("M,n,na", [(1, 2, 2), (5, 6, 5), (32, 18, 51), (3, 9, 101), (32, 4, 51)])
def test_head_twin_within_the_reference_bar(M, n, na):
    """Against float64 autograd of the reference's lines on the effective layers: twice the f32 reference's own error plus 2e-6.  The
    selected actions are held to the float64 reference where its two best expectations are further apart than that error."""
    c = R.make_head_case(M, n, na)
    got = R.run_heads(H, c, CPU)
    r64, r32 = R.reference_head(c, torch.float64), R.reference_head(c, torch.float32)
    q64 = r64["q"].sort(1).values
    clear = (q64[:, -1] - q64[:, -2]) > 1e-4
    assert clear.any() and torch.equal(got["act"][clear], r64["act"][clear])
    assert torch.equal(got["best"], r64["best"])                             # the same double-Q selection: the targets are comparable
    for k in ("q", "next_pmfs", "target_pmfs", "loss_per_sample", "scalars", "dh", "dw", "db"):
        ok, err, own = R.within_bar(got[k], r64[k], r32[k])
        print(f"M={M} n={n} atoms={na} {k}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (k, err, own)
    assert torch.allclose(got["target_pmfs"].sum(1), torch.ones(M), atol=1e-5)


def test_head_ties_nan_and_inf_follow_the_rules():
    c = R.make_head_case(5, 6, 5, tie=True)
    c.h[2, 7] = float("nan")
    c.rewards[1] = float("inf")
    got = R.run_heads(H, c, CPU)
    assert not (got["act"] == 1).any() and not (got["best"] == 1).any() and got["act"][2] == 0
    assert torch.isfinite(got["loss_per_sample"][[0, 3, 4]]).all()


def test_each_row_of_a_batch_is_that_row_alone_times_its_weight_over_m():
    c = R.make_head_case(32, 6, 51)
    full = R.run_heads(H, c, CPU)
    for r in (0, 7, 31):
        one = R.make_head_case(1, 6, 51)
        for k in ("h", "h_next", "h_next_target", "actions", "rewards", "dones"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in ("w", "b", "wt", "bt"):
            setattr(one, k, getattr(c, k))
        one.weights = torch.ones(1)
        alone = R.run_heads(H, one, CPU)
        assert R.same_bits(full["loss_per_sample"][r], alone["loss_per_sample"][0])
        scale = (c.weights[r] * torch.tensor(1 / 32, dtype=torch.float32)).item()
        assert torch.allclose(full["dh"][r], alone["dh"][0] * scale, rtol=1e-5, atol=1e-9)


def test_head_refusals():
    for n, na, M in ((1, 51, 4), (19, 5, 4), (6, 1, 4), (18, 54, 4), (6, 5, 0), (6, 5, 1025)):
        assert not ops.rainbow_head_limits_ok(n, na, M)
        assert _lib.load().mi355ppo_rainbow_head_workspace_bytes(M, n, na) == 0 and _lib.load().mi355ppo_rainbow_head_act_workspace_bytes(M, n, na) == 0
    c = R.make_head_case(2, 6, 5)
    c.support = torch.linspace(-10, 10, 1)
    with pytest.raises((_lib.Mi355PpoError, ValueError)):
        R.run_heads(H, c, CPU)


@pytest.mark.parametrize("shape", R.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_twins_stay_inside_their_buffers(shape, monkeypatch):
    B.check(R.bounds_head_case(*shape), H, CPU, monkeypatch)
