"""The QDagger drop-in on the GPU: the IMPALA-CNN trunk on Atari stacks (the 84 family of csrc/impala.hip) against its host twin
bit for bit, against float64 autograd of the reference's modules, determinism, batch invariance and graph capture; the QDagger
head (csrc/qdagger.hip) against its twin, the reference's lines and inside guard bands; the learner against float64 autograd and
the minted runs; the script with both fused switches."""
import pytest
import torch

import bounds_cases as B
import impala84_cases as C
import qdagger_cases as Q
from cleanrl_amd import host_ops, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


def _case(kind, B, seed):
    _, params = C.make_params(seed=seed)
    return params, C.make_frames(kind, B, seed=seed), C.upstream(B, seed=seed + 7)


# ------------------------------------------------------------------------------------------------------- trunk
@pytest.mark.parametrize("frames", C.FRAMES)
def test_trunk_device_equals_twin_bit_for_bit(frames):
    params, x, dy = _case(frames, 2, seed=5)
    hy, hs, ha = host_ops.impala84_forward(x, params)
    hg = host_ops.impala84_backward(x, params, hs, ha, dy)
    dp = [p.detach().to(DEV) for p in params]
    y, saved, arg = ops.impala84_forward(x.to(DEV), dp)
    grads = ops.impala84_backward(x.to(DEV), dp, saved, arg, dy.to(DEV))
    assert torch.equal(y.cpu(), hy) and torch.equal(saved.cpu(), hs) and torch.equal(arg.cpu(), ha)
    for i, (g, h) in enumerate(zip(grads, hg)):
        assert torch.equal(g.cpu(), h), f"gradient {i}"


@pytest.mark.parametrize("B", [1, 3, 32])
def test_trunk_against_float64(B):
    params, x, dy = _case("flat" if B == 3 else "noise", B, seed=B)
    dp = [p.detach().to(DEV) for p in params]
    y, saved, arg = ops.impala84_forward(x.to(DEV), dp)
    grads = ops.impala84_backward(x.to(DEV), dp, saved, arg, dy.to(DEV))
    args = C.argmax_planes(arg.cpu(), B)
    C.check_argmax(params, x, args)
    C.check_against_f64(("gpu", B), params, x, dy, y.cpu(), [g.cpu() for g in grads], args, verbose=True)


def test_trunk_maxpool_kernels_equal_twin():
    for B, H, Cc in ((2, 84, 16), (3, 42, 32), (5, 21, 32)):
        g = torch.Generator().manual_seed(H)
        x = torch.randint(0, 3, (B, H, H, Cc), generator=g).float()
        y, arg = ops.impala_maxpool_forward(x.to(DEV))
        hy, ha = host_ops.impala_maxpool_forward(x)
        assert torch.equal(y.cpu(), hy) and torch.equal(arg.cpu(), ha)
        dy = torch.randn(tuple(hy.shape), generator=g)
        assert torch.equal(ops.impala_maxpool_backward(dy.to(DEV), arg, size=H).cpu(), host_ops.impala_maxpool_backward(dy, ha, size=H))


def test_trunk_determinism_and_batch_invariance():
    B = 32
    params, x, dy = _case("noise", B, seed=11)
    dp = [p.detach().to(DEV) for p in params]
    x, dy = x.to(DEV), dy.to(DEV)
    y1, s1, a1 = ops.impala84_forward(x, dp)
    y2, s2, a2 = ops.impala84_forward(x, dp)
    assert torch.equal(y1, y2) and torch.equal(s1, s2) and torch.equal(a1, a2)
    g1 = ops.impala84_backward(x, dp, s1, a1, dy)
    g2 = ops.impala84_backward(x, dp, s2, a2, dy)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    planes = [h * h * c for h, c in C.PLANES]
    for i in (0, 17, 31):
        yi, si, ai = ops.impala84_forward(x[i:i + 1].contiguous(), dp)
        assert torch.equal(yi[0], y1[i])
        for s in range(3):                                          # every saved activation plane and the argmax of image i
            n = planes[s]
            for which in range(5 if s < 2 else 4):
                off = sum((5 if t < 2 else 4) * planes[t] for t in range(s)) + which * n
                assert torch.equal(si[off:off + n], s1[off * B + i * n:off * B + (i + 1) * n])
            assert torch.equal(C.argmax_planes(ai, 1)[s][0], C.argmax_planes(a1, B)[s][i])
        # The data gradients are not an output; they show in the weight gradients.  With dy zero outside image i the batch's
        # other images contribute exact zeros, so the 30 gradients are image i's alone up to the order of the fold (B = 32
        # splits the bands into other parts than B = 1).  Each side is within about 1e-6 (norm-relative) of the exact sum
        # (impala_cases' twin study), so the two are within 4e-6 of each other.
        dyi = torch.zeros_like(dy)
        dyi[i] = dy[i]
        gb = ops.impala84_backward(x, dp, s1, a1, dyi)
        gi = ops.impala84_backward(x[i:i + 1].contiguous(), dp, si, ai, dy[i:i + 1].contiguous())
        for k, (a, b) in enumerate(zip(gb, gi)):
            assert ((a - b).double().norm() / b.double().norm().clamp_min(1e-30)).item() <= 4e-6, f"image {i} gradient {k}"


def test_trunk_graph_capture_of_the_b1_forward_replayed_on_new_bytes():
    params, x, _ = _case("noise", 1, seed=2)
    dp = [p.detach().to(DEV) for p in params]
    buf = x.to(DEV)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.impala84_trunk(buf, dp)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.impala84_trunk(buf, dp)
        new = C.make_frames("flat", 1, seed=9).to(DEV)
        buf.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.impala84_trunk(new, dp)
    assert torch.equal(out, eager)


# -------------------------------------------------------------------------------------------------------- head
@pytest.mark.parametrize("M,n", Q.GPU_HEADS)
def test_head_equals_its_twin_and_repeats(M, n):
    c = Q.make_head_case(M, n, temperature=0.7)
    want = Q.run_heads(host_ops, c, CPU)
    got = {k: v.cpu() for k, v in Q.run_heads(ops, c, DEV).items()}
    for k in want:
        assert Q.same(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())
    again = {k: v.cpu() for k, v in Q.run_heads(ops, c, DEV).items()}
    assert all(Q.same(again[k], got[k]) for k in got)


def test_head_within_the_reference_bar_at_the_scripts_shape():
    """M = 32, 18 actions on the device against float64 autograd: twice the f32 reference's own error plus 2e-6."""
    c = Q.make_head_case(32, 18, temperature=0.7)
    got = Q.run_heads(ops, c, DEV)
    r64, r32 = Q.reference_head(c, torch.float64), Q.reference_head(c, torch.float32)
    for k in ("q", "target_q", "td_target", "scalars", "dh", "dw", "db"):
        ok, err, own = Q.within_bar(got[k], r64[k], r32[k])
        print(f"{k}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (k, err, own)


def test_head_ties_and_non_finite_inputs_follow_the_twin():
    c = Q.make_head_case(5, 6, tie=True)
    c.h[2, 7] = float("nan")
    c.rewards[1] = float("inf")
    want = Q.run_heads(host_ops, c, CPU)
    got = {k: v.cpu() for k, v in Q.run_heads(ops, c, DEV).items()}
    assert all(Q.same(got[k], want[k]) for k in want)
    assert not (got["act"] == 1).any() and got["act"][2] == 0


@pytest.mark.parametrize("shape", Q.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_kernels_stay_inside_their_outputs_and_workspaces(shape, monkeypatch):
    B.check(Q.bounds_head_case(*shape), ops, DEV, monkeypatch)


# ----------------------------------------------------------------------------------------------------- learner
def test_trunk_fc_and_head_together_at_the_scripts_batch(monkeypatch):
    """One update at M = 32 through gather, the fused IMPALA trunk, torch's FC, the teacher's trunk and head, the QDagger head kernels
    and ``h.backward(dh)``, against float64 autograd at DESIGN.md section 4's "trunk + FC" row: forward 5e-5, every gradient
    max(5e-5 x scale, 4 x the error of torch's f32 backward against float64)."""
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    L = Q.make_learner(DEV, "fused", M=32, slots=40, n=6, fill=True)
    assert L.q_network.impala_backend == "fused"
    g = torch.Generator().manual_seed(1)
    bi, ei = torch.randint(0, 40, (32,), generator=g).numpy(), torch.zeros(32, dtype=torch.int64).numpy()
    idx = L._stage_indices(bi, ei)
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    L.update_kernels(idx[0], idx[1], adam=False, distill_coeff=0.37)
    torch.cuda.synchronize()
    assert {"mi355ppo_replay_gather_u8", "mi355ppo_impala84_fwd_u8", "mi355ppo_impala84_bwd_u8", "mi355ppo_dqn_head_act_f32",
            "mi355ppo_qdagger_head_fwd_bwd_f32"} <= set(seen)
    r64, r32 = Q.reference_update(L, bi, ei, torch.float64, 0.37), Q.reference_update(L, bi, ei, torch.float32, 0.37)
    sc = L._sc.cpu().double()
    ferr = (sc - r64["scalars"]).abs().max().item()
    print(f"forward: err {ferr:.3e}")
    assert ferr <= 5e-5 * max(1.0, r64["scalars"].abs().max().item())
    got, off = L.grads.cpu().double(), 0
    for name, p in L.q_network.named_parameters():
        sl = slice(off, off + p.numel())
        off += p.numel()
        ref = r64["grads"][sl]
        err, own = (got[sl] - ref).abs().max().item(), (r32["grads"][sl].double() - ref).abs().max().item()
        bar = max(5e-5 * ref.abs().max().item(), 4 * own)
        print(f"{name}: err {err:.3e} torch f32 {own:.3e} bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("name", ["qdagger", "qdagger_t07"])
def test_goldens_teacher_forced_on_the_hip_path(name, monkeypatch):
    """The minted runs teacher-forced through the fused learner on the device, at the bars DESIGN.md section 4 holds the Atari trunks
    to across Adam steps (the config-B row): loss scalars rtol 1e-3 with an absolute floor of 1e-4, and at the first update the
    pre-Adam flat gradient within 1e-3 of its largest element with 1 - cosine <= 1e-5 against the reference's lines in f32.  The minted runs use a learning rate of 1e-5: at the script's 1e-4 the reference's own float32 lines
    drift 1e-3 from their float64 copy over these 39 Adam steps, the size of this bar (tools/mint_qdagger_goldens.py)."""
    import numpy as np

    import qdagger_replay as R
    from cleanrl_amd.learner_qdagger import QDaggerLearner

    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    first = {}
    orig = QDaggerLearner.update_kernels

    def spy(self, bi, ei, adam=True, aux=None, distill_coeff=1.0):
        if not first:
            want = Q.reference_update(self, bi.cpu().numpy(), ei.cpu().numpy(), torch.float32, distill_coeff)["grads"]
            orig(self, bi, ei, adam=False, distill_coeff=distill_coeff)
            first["got"], first["want"] = self.grads.detach().cpu().clone(), want
        return orig(self, bi, ei, adam=adam, aux=aux, distill_coeff=distill_coeff)

    monkeypatch.setattr(QDaggerLearner, "update_kernels", spy)
    rec = R.replay(name, "fused", DEV)
    g = R.golden_case(name)
    got, want = first["got"].double(), first["want"].double()
    worst = ((got - want).abs().max() / want.abs().max()).item()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=0).item()
    print(f"{name}: first update max|dg|/absmax {worst:.2e}, 1-cosine {1 - cos:.2e}")
    assert worst <= 1e-3 and 1 - cos <= 1e-5
    for k in R.SCALARS:
        for key in (k, "offline_" + k):
            m = ~np.isnan(g[key])
            print(f"{name}: {key} max deviation {np.abs(rec[key][m] - g[key][m]).max():.3e} (reference's own f32-vs-f64 {R.sensitivity(name)[k]:.3e})")
            assert np.allclose(rec[key][m], g[key][m], rtol=1e-3, atol=1e-4), key
            assert np.array_equal(np.isnan(rec[key]), np.isnan(g[key]))


def test_script_runs_fused(tmp_path):
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MI355PPO_OFFPOLICY="fused", MI355PPO_IMPALA="fused", MI355PPO_STANDIN_HORIZON="20")
    env.pop("MI355PPO_TEACHER_MODEL", None)
    out = subprocess.run([sys.executable, os.path.join(root, "cleanrl_amd", "qdagger_dqn_atari_impalacnn.py"), "--teacher-steps", "100",
                          "--offline-steps", "100", "--total-timesteps", "300", "--learning-starts", "120", "--buffer-size", "200",
                          "--teacher-eval-episodes", "2"], capture_output=True, text=True, cwd=tmp_path, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "SPS:" in out.stdout and "nan" not in out.stdout.lower() and "randomly initialised teacher" in out.stderr
