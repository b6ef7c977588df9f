"""Host twins of the discrete-SAC kernels (csrc/sac_atari.hip, csrc/sac_atari_twins.hip) on the CPU: the C ABI's surface and its
validation, the two frame rings against a numpy model of the reference's plain buffer, the head twins against float64 autograd of
sac_atari.py's lines, the temperature step through the actor kernel's ``e_r`` rows, the sampling rule, the networks' seeded
construction and the stand-alone host check."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import bounds_cases as B
import sac_atari_cases as S
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRY_POINTS = ("mi355ppo_replay_add2_u8", "mi355ppo_replay_gather2_u8", "mi355ppo_sacd_head_act_f32", "mi355ppo_sacd_critic_fwd_bwd_f32",
                       "mi355ppo_sacd_actor_fwd_bwd_f32")


# ================================================================================================== the C ABI
def test_every_new_device_entry_point_has_its_cpu_twin_and_a_header_section():
    hdr = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    lib = _lib.load()
    for name in DEVICE_ENTRY_POINTS:
        assert name in _lib.SIGNATURES and name + "_cpu" in _lib.SIGNATURES
        dev_args, cpu_args = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_cpu"][1]
        tail = dev_args[len(cpu_args):]                                       # the twin: the device signature minus workspace and stream
        assert dev_args[:len(cpu_args)] == cpu_args and tail in ([ctypes.c_void_p], [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])
        assert name + "(" in hdr and name + "_cpu(" in hdr and getattr(lib, name + "_cpu") is not None
    for name in ("mi355ppo_sacd_head_act_workspace_bytes", "mi355ppo_sacd_critic_workspace_bytes", "mi355ppo_sacd_actor_workspace_bytes"):
        assert name in _lib.SIGNATURES
    assert "cleanrl/sac_atari.py" in hdr


def test_validation_is_loud_and_precedes_any_launch():
    """No device is needed: every refusal comes back before the first HIP call, with its code and a message."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(p.value + 2)
    big = 1 << 30

    def critic(M, hidden, n, ws=p, ws_bytes=big, h=p):
        return lib.mi355ppo_sacd_critic_fwd_bwd_f32(h, *[p] * 18, 0.99, *[p] * 9, M, hidden, n, ws, ws_bytes, None)

    def actor(M, hidden, n, ws=p, ws_bytes=big, h=p):
        return lib.mi355ppo_sacd_actor_fwd_bwd_f32(h, *[p] * 9, 1.0, *[p] * 5, M, hidden, n, ws, ws_bytes, None)

    def act(N, hidden, n, ws=p, ws_bytes=big, h=p):
        return lib.mi355ppo_sacd_head_act_f32(h, p, p, p, p, None, N, hidden, n, ws, ws_bytes, None)

    for fn in (critic, actor, act):
        assert fn(4, 512, 6, h=None) == -1 and b"null" in lib.mi355ppo_last_error()
        assert fn(4, 256, 6) == -1 and b"hidden" in lib.mi355ppo_last_error()
        for n in (1, 19):
            assert fn(4, 512, n) == -1 and b"n_actions" in lib.mi355ppo_last_error()
        for M in (0, 1025):
            assert fn(M, 512, 6) == -1 and b"rows" in lib.mi355ppo_last_error()
        assert fn(4, 512, 6, ws_bytes=16) == -4 and b"workspace" in lib.mi355ppo_last_error()
        assert fn(4, 512, 6, ws=None) == -4
        assert fn(4, 512, 6, ws=mis) == -2
    # the twins refuse the same shapes
    assert lib.mi355ppo_sacd_critic_fwd_bwd_f32_cpu(*[p] * 19, 0.99, *[p] * 9, 4, 512, 19) == -1
    assert lib.mi355ppo_sacd_actor_fwd_bwd_f32_cpu(*[p] * 10, 1.0, *[p] * 5, 1025, 512, 6) == -1
    assert lib.mi355ppo_sacd_head_act_f32_cpu(p, p, p, p, p, None, 4, 256, 6) == -1
    # workspace sizes: z of every pass | the row scalars, padded to 64 rows | dz | the taken actions
    assert lib.mi355ppo_sacd_critic_workspace_bytes(5, 6) == (5 * 5 * 6 + 4 * 64 + 2 * 5 + 5) * 4
    assert lib.mi355ppo_sacd_actor_workspace_bytes(5, 6) == (3 * 5 * 6 + 64 + 5 * 6) * 4
    assert lib.mi355ppo_sacd_head_act_workspace_bytes(5, 6) == 5 * 6 * 4
    for f in (lib.mi355ppo_sacd_critic_workspace_bytes, lib.mi355ppo_sacd_actor_workspace_bytes, lib.mi355ppo_sacd_head_act_workspace_bytes):
        assert f(0, 6) == 0 and f(1025, 6) == 0 and f(4, 1) == 0 and f(4, 19) == 0
    # the rings
    add = lambda ring=p, pos=0, slots=2, N=1, obs=p: lib.mi355ppo_replay_add2_u8(obs, p, p, p, p, ring, p, p, p, p, pos, slots, N, None)  # noqa: E731
    assert add(obs=None) == -1 and b"null" in lib.mi355ppo_last_error()
    assert add(ring=mis) == -2 and b"aligned" in lib.mi355ppo_last_error()
    assert add(pos=2) == -1 and add(pos=-1) == -1 and add(slots=0) == -1 and add(N=0) == -1
    gather = lambda ring=p, M=4, slots=2, N=1, out=p: lib.mi355ppo_replay_gather2_u8(ring, p, p, p, p, p, p, slots, N, out, p, p, p, M, None)  # noqa: E731
    assert gather(ring=None) == -1
    assert gather(ring=mis) == -2 and gather(out=mis) == -2
    assert gather(M=0) == -1 and gather(M=1025) == -1 and gather(slots=0) == -1
    assert lib.mi355ppo_replay_add2_u8_cpu(p, p, p, p, p, p, p, p, p, p, 3, 2, 1) == -1
    assert lib.mi355ppo_replay_gather2_u8_cpu(p, p, p, p, p, p, p, 2, 1, p, p, p, p, 0) == -1


# ================================================================================================== the rings
@pytest.mark.parametrize("slots", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 3])
def test_ring_twins_follow_the_plain_buffers_rules(slots, N):
    steps = S.ring_steps(slots, N, max(slots + 3, 8))
    ring, ref, idx, out = S.run_ring(H, CPU, slots, N, steps)
    S.check_ring_against_model(ring, ref, idx, out)
    assert (ref.pos, ref.full) == (max(slots + 3, 8) % slots, True)


def test_frame_offsets_past_2_31_words_are_formed_in_64_bits(tmp_path):
    """``da_frame`` -- the offset both rings' kernels and twins form -- at a slot whose word offset lies past 2^31 (host only: no ring
    of that size is needed)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "frame_offset.cpp"
    src.write_text('#include "sac_atari_rows.h"\n#include <cstdio>\nnamespace mi355ppo { void set_error(const char*, ...) {} }\n'
                   'int main() { printf("%lld %lld\\n", (long long)mi355ppo::da_frame(400000, 2, 3), (long long)mi355ppo::da_frame(999999, 0, 1)); }\n')
    out = str(tmp_path / "frame_offset")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++20", "-I" + os.path.join(ROOT, "cleanrl_amd", "csrc"), str(src), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = map(int, subprocess.run([out], capture_output=True, text=True).stdout.split())
    assert a == (400000 * 3 + 2) * 7056 > 1 << 31 and b == 999999 * 7056 > 1 << 31


# ================================================================================================== the heads
@pytest.mark.parametrize("M,n", S.HEAD_GRID)
def test_head_twins_within_the_reference_bar(M, n):
    """Against float64 autograd of the reference's lines: twice the f32 reference's own error plus 2e-6."""
    c = S.make_head_case(M, n)
    got = S.run_heads(H, c, CPU)
    for ref, keys in ((S.reference_critic, S.CRITIC_OUTS), (S.reference_actor, S.ACTOR_OUTS)):
        r64, r32 = ref(c, torch.float64), ref(c, torch.float32)
        for k in keys:
            ok, err, own = S.within_bar(got[k], r64[k], r32[k])
            print(f"M={M} n={n} {k}: err {err:.3e} reference's own {own:.3e}")
            assert ok, (k, err, own)
    # the case holds what the issue asks of it
    assert c.dones[0] == 1 and (M == 1 or c.actions[0] == c.actions[1]) and not (c.actions == n - 1).any()
    assert not got["dw1"][n - 1].any() and not got["dw2"][n - 1].any() and got["db1"][n - 1] == 0 and got["db2"][n - 1] == 0
    # the gap row: p underflows to exactly 0 in f32, logp stays finite, and nothing downstream turns non-finite
    assert got["probs"][M - 1, 1] == 0 and got["probs"][M - 1, 0] == 1
    z = torch.nn.functional.linear(c.h_pi_next[M - 1], c.w_pi, c.b_pi)
    assert z[0] - z[1] >= S.GAP
    assert all(torch.isfinite(got[k]).all() for k in S.HEAD_OUTS if k != "act")


@pytest.mark.parametrize("M,n", [(5, 6), (64, 18)])
def test_alpha_step_through_the_entropy_rows(M, n):
    """``sac_alpha_`` on ``e_r`` with a target entropy of 0 and eps 1e-4: the reference's ``alpha_loss`` and its gradient at the bar of
    the heads, then twelve Adam steps against ``torch.optim.Adam(eps=1e-4)`` at rtol 1e-5 / atol 1e-7."""
    c = S.make_head_case(M, n)
    got = S.run_heads(H, c, CPU)
    r64, r32 = S.reference_actor(c, torch.float64), S.reference_actor(c, torch.float32)
    la = c.alpha.log().clone()
    st = [la, torch.zeros(1), torch.zeros(1), torch.zeros(1), torch.zeros(1)]
    p = torch.nn.Parameter(la.clone())
    opt = torch.optim.Adam([p], lr=3e-4, eps=1e-4)
    g = torch.Generator().manual_seed(M + n)
    for step in range(1, 13):
        e = got["e_rows"] if step == 1 else torch.randn(M, generator=g) * 10.0 ** float(torch.randint(-4, 1, (1,), generator=g))
        loss = (-p.exp() * e).mean()
        opt.zero_grad()
        loss.backward()
        H.sac_alpha_(e.contiguous(), 0.0, st[0], st[1], st[2], step, 3e-4, st[3], st[4], eps=1e-4)
        if step == 1:
            for k in ("alpha_loss", "alpha_grad"):                            # the loss is its own gradient with respect to log_alpha
                ok, err, own = S.within_bar(st[4], r64[k], r32[k])
                print(f"M={M} n={n} {k}: err {err:.3e} reference's own {own:.3e}")
                assert ok, (k, err, own)
        opt.step()
    assert torch.allclose(st[0], p.detach(), rtol=1e-5, atol=1e-7) and torch.allclose(st[3], p.detach().exp(), rtol=1e-5, atol=1e-7)


def test_act_is_the_argmax_of_probs_over_noise_with_ties_to_the_lowest_index():
    for M, n in S.HEAD_GRID:
        c = S.make_head_case(M, n)
        got = S.run_heads(H, c, CPU)
        assert torch.equal(got["act"], torch.argmax(got["probs"] / c.noise, dim=1))
        assert torch.allclose(got["probs"].sum(1), torch.ones(M), atol=1e-6)
    c = S.make_head_case(5, 6)
    c.w_pi[:] = 0.0                                                           # equal logits and equal noise: every action ties
    c.b_pi[:] = 0.25
    c.noise[:] = 1.0
    c.noise[3] = torch.tensor([2.0, 1.0, 1.0, 2.0, 1.0, 0.5])               # one clear winner
    c.noise[4] = torch.tensor([2.0, 1.0, 1.0, 2.0, 1.0, 1.0])               # a tie between actions 1, 2, 4 and 5
    got = S.run_heads(H, c, CPU)
    assert got["act"].tolist() == [0, 0, 0, 5, 1]


def test_twin_guard_bands(monkeypatch):
    B.check(S.bounds_head_case(5, 6), H, CPU, monkeypatch)
    B.check(S.bounds_ring_case(2, 3), H, CPU, monkeypatch)


# ================================================================================================== the networks
def test_seeded_constructions_match_the_reference():
    from cleanrl_amd.agents import AtariSACActor, AtariSoftQNetwork

    z = np.load(os.path.join(ROOT, "tests", "golden", "sac_atari_network_init.npz"))
    probes = z["probe_index"].tolist()
    for n_actions, seed in ((6, 1), (18, 7)):
        torch.manual_seed(seed)
        env = S.atari_env(n_actions)
        for key, cls in (("actor", AtariSACActor), ("qf1", AtariSoftQNetwork), ("qf2", AtariSoftQNetwork)):
            net = cls(env)
            f = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
            pre = f"n{n_actions}_seed{seed}/{key}"
            assert list(net.state_dict().keys()) == json.loads(bytes(z[pre + "/keys"]).decode())
            assert f.numel() == int(z[pre + "/count"])
            assert f.view(torch.int32).to(torch.int64).sum().item() == int(z[pre + "/bits_checksum"])          # every bit of every element
            assert abs(f.double().abs().sum().item() - float(z[pre + "/abs_checksum"])) <= 1e-9 * float(z[pre + "/abs_checksum"])
            assert np.array_equal(f[probes].numpy(), z[pre + "/probes"])
            assert all(not b.any() for k, b in net.state_dict().items() if k.endswith("bias"))


# ================================================================================================== the stand-alone host check
def test_the_standalone_host_check_builds_and_passes_without_sanitizers(tmp_path):
    """tools/sac_atari_host_check.cpp: its own ``main`` over the ring and head twins.  Here it is built plain and run; the address /
    undefined-behaviour sanitizer build of the same program is a command in its header (a stand-alone program, never under python)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = str(tmp_path / "sac_atari_host_check")
    csrc = os.path.join(ROOT, "cleanrl_amd", "csrc")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++20", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
           os.path.join(ROOT, "tools", "sac_atari_host_check.cpp"), os.path.join(csrc, "sac_atari_twins.hip"), os.path.join(csrc, "api.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([out], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout, r.stderr)
