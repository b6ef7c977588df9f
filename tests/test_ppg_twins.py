"""The PPG auxiliary-phase operators (csrc/ppg.hip, cleanrl_amd/ppg_ops.py) on their host twins, without a GPU: the minted cases of
the reference's own lines at the project's numeric rule, the zero-probability row, the accumulate flag, the split optimiser step
against ``clip_adam_``, refusals, the switch, the launch budget, and ``PPGLearner``'s fused branch driven on the CPU."""
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributions as td
from torch.distributions.categorical import Categorical

import ppg_cases as P
from conftest import load_golden
from cleanrl_amd import _lib, host_ops, learner_ppg
from cleanrl_amd import envs as E
from cleanrl_amd.agents import PPGAgent
from cleanrl_amd.learner_ppg import PPGLearner
from cleanrl_amd.learner_smoke import default_args

CPU = torch.device("cpu")
PLAIN = P.plain(CPU)


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when the goldens were minted
    yield
    torch.set_num_threads(n)


# ---------------------------------------------------------------------------------------------- the reference's lines
@pytest.mark.parametrize("name", list(P.GOLDEN_CASES))
def test_twins_on_the_minted_cases_within_the_rule(name):
    c = P.golden_as_case(name)
    got = P.run_aux(host_ops, c, *PLAIN)
    c_old = dict(c, heads=c["heads"], aux_pi=torch.zeros_like(c["aux_pi"]))
    got["aux_pi_rows"] = P.run_old(host_ops, c_old, *PLAIN)
    assert set(got) == set(P.COMPARED) and all(torch.isfinite(v).all() for v in got.values())
    P.assert_within_rule(name, got)


@pytest.mark.parametrize("name", list(P.GOLDEN_CASES))
def test_a_logit_120_below_the_maximum_is_an_exact_zero_term(name):
    """p_old of that action is exactly 0, so its KL term is exactly 0 whatever the logit is: -120, -1e4 and -inf (where
    p_old * (logp_old - logp_new) would be 0 * inf) give the same bits everywhere, and nothing is NaN."""
    c = P.golden_as_case(name)
    t0, c0, j0 = c["low"]
    row = c["aux_pi"][t0, c0]
    assert torch.softmax(row, -1)[j0] == 0.0 and row[j0] <= row.max() - 100.0
    ref = P.run_aux(host_ops, c, *PLAIN)
    assert all(torch.isfinite(v).all() for v in ref.values())
    for low in (-1e4, float("-inf")):
        pi = c["aux_pi"].clone()
        pi[t0, c0, j0] = low
        out = P.run_aux(host_ops, dict(c, aux_pi=pi), *PLAIN)
        for k, v in ref.items():
            assert torch.equal(out[k], v) and not torch.isnan(out[k]).any(), (low, k)


def test_a_zero_new_probability_under_a_positive_old_one_is_inf_as_in_torch():
    c = P.case(1, 1, 2)
    heads = [t.clone() for t in c["heads"]]
    heads[0].zero_()
    heads[1].copy_(torch.tensor([0.0, -200.0]))                 # p_new[1] == 0 in f32
    pi = torch.log(torch.tensor([0.5, 0.5])).expand(1, c["aux_pi"].shape[1], 2).contiguous()
    out = P.run_aux(host_ops, dict(c, heads=heads, aux_pi=pi), *PLAIN)
    want = td.kl_divergence(Categorical(logits=pi[0, :1]), Categorical(logits=heads[1][None])).mean()
    assert torch.isinf(want) and torch.isinf(out["scalars"][0]) and out["scalars"][0] > 0
    assert torch.isfinite(out["dh"]).all() and torch.isfinite(out["scalars"][1:]).all()


# ---------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("T,n,A", [(7, 1, 2), (9, 4, 15), (3, 3, 30)])
def test_accumulate_adds_the_folded_value_once_bit_for_bit(T, n, A):
    c = P.case(T, n, A)
    fresh = P.run_aux(host_ops, c, *PLAIN)
    added = P.run_aux(host_ops, c, *PLAIN, prefill=c["prefill"])
    for k, pre in zip(P.HEADS, c["prefill"]):
        assert torch.equal(added["d_" + k], pre + fresh["d_" + k]), k
    for k in ("scalars", "dh"):
        assert torch.equal(added[k], fresh[k])


# ---------------------------------------------------------------------------------------------- the split optimiser step
@pytest.mark.parametrize("n", [5, 1001, 4100])
def test_clip_adam_split_is_clip_adam_on_each_range(n):
    c = P.adam_case(n)
    head, tail = P.run_plain_adam(host_ops, c, PLAIN[0], 7), P.run_plain_adam(host_ops, c, PLAIN[0], 3)
    for n_split in (n, 0, n // 3, n - 1):
        out = P.run_split(host_ops, c, *PLAIN, n_split, 7, 3)
        for k, (o, h, t) in enumerate(zip(out[:4], head, tail)):
            assert torch.equal(o[:n_split], h[:n_split]) and torch.equal(o[n_split:], t[n_split:]), (n_split, k)
        assert torch.count_nonzero(out[1]) == 0
    same = P.run_split(host_ops, c, *PLAIN, n // 2, 7, 7)             # equal steps: clip_adam_ on the whole buffer
    assert all(torch.equal(o, h) for o, h in zip(same[:4], head))
    want_norm = (c["grads"] * P.ADAM["grad_scale"]).double().norm()
    assert abs(float(same[4]) - float(want_norm)) <= 1e-6 * float(want_norm)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_raise_before_any_call(monkeypatch):
    monkeypatch.setattr(_lib, "call", lambda *a: pytest.fail("the library was called"))
    c = P.case(3, 3, 15)
    H, put, out_of = host_ops, *PLAIN

    def aux(**over):
        return P.run_aux(H, dict(c, **over), put, out_of)

    for A in (1, 31):                                             # A + 2 outputs must fit one 32-output tile
        heads = [torch.zeros(s) for s in P.head_shapes(A)]
        with pytest.raises(ValueError, match="actions"):
            aux(heads=heads, aux_pi=torch.zeros(3, 6, A))
        with pytest.raises(ValueError, match="actions"):
            H.ppg_old_logits_(c["h"], heads[0], heads[1], c["cols"], torch.zeros(3, 6, A))
    with pytest.raises(ValueError, match="hidden width"):
        aux(h=torch.zeros(9, 128))
    with pytest.raises(ValueError, match="hidden width"):
        H.ppg_old_logits_(torch.zeros(9, 512), c["heads"][0], c["heads"][1], c["cols"], torch.zeros(3, 6, 15))
    R = c["aux_pi"].shape[1]
    for bad in (torch.tensor([0, 1, R]), torch.tensor([-1, 1, 2])):
        with pytest.raises(ValueError, match="cols"):
            aux(cols=bad)
        with pytest.raises(ValueError, match="cols"):
            P.run_gather(H, dict(c, cols=bad), put, out_of)
        with pytest.raises(ValueError, match="cols"):
            P.run_old(H, dict(c, cols=bad), put, out_of)
    with pytest.raises(TypeError):
        aux(cols=c["cols"].int())
    with pytest.raises(TypeError):
        aux(h=c["h"].double())
    with pytest.raises(ValueError):
        aux(h=c["h"][:-1].contiguous())                          # not T * n rows
    with pytest.raises(ValueError, match="contiguous"):
        H.ppg_aux_gather(c["aux_obs"].transpose(2, 3), c["cols"])
    with pytest.raises(ValueError):
        P.run_gather(H, dict(c, aux_obs=torch.zeros((3, 6, 5, 3), dtype=torch.uint8)), put, out_of)       # 15-byte rows
    with pytest.raises(TypeError):
        P.run_gather(H, dict(c, aux_obs=c["aux_obs"].float()), put, out_of)
    a = P.adam_case(5)
    for n_split, sh, st in ((6, 1, 1), (-1, 1, 1), (2, 0, 1), (2, 1, 0)):
        with pytest.raises(ValueError):
            P.run_split(H, a, put, out_of, n_split, sh, st)


def test_the_entry_points_refuse_other_sizes_themselves():
    """The C ABI's own checks (MI355PPO_EINVAL = -1), reached past the wrapper: outputs stay untouched."""
    lib = _lib.load()
    ptr = lambda t: t.data_ptr()
    h, w, b, cols, pi = torch.zeros(3, 256), torch.zeros(31, 256), torch.zeros(31), torch.zeros(1, dtype=torch.int64), torch.full((3, 2, 31), 7.0)
    assert lib.mi355ppo_ppg_old_logits_f32_cpu(ptr(h), ptr(w), ptr(b), ptr(cols), ptr(pi), 3, 1, 2, 31, 256) == -1
    assert lib.mi355ppo_ppg_old_logits_f32_cpu(ptr(h), ptr(w), ptr(b), ptr(cols), ptr(pi), 3, 1, 2, 1, 256) == -1
    assert lib.mi355ppo_ppg_old_logits_f32_cpu(ptr(h), ptr(w), ptr(b), ptr(cols), ptr(pi), 3, 1, 2, 15, 128) == -1
    assert b"hidden" in lib.mi355ppo_last_error() and bool((pi == 7.0).all())
    assert lib.mi355ppo_ppg_aux_workspace_bytes(16, 31) == 0 and lib.mi355ppo_ppg_aux_workspace_bytes(0, 15) == 0
    assert lib.mi355ppo_ppg_aux_workspace_bytes(16, 15) == 2 * 3 * 8 + 2 * (32 * 256 + 32) * 4


def test_the_switch_is_read_when_a_learner_is_built(monkeypatch):
    monkeypatch.delenv("MI355PPO_PPG", raising=False)
    assert learner_ppg.ppg_backend() == "torch"
    for v, want in (("fused", "fused"), (" Fused ", "fused"), ("torch", "torch"), ("", "torch")):
        monkeypatch.setenv("MI355PPO_PPG", v)
        assert learner_ppg.ppg_backend() == want
    monkeypatch.setenv("MI355PPO_PPG", "hip")
    with pytest.raises(ValueError, match="MI355PPO_PPG"):
        learner_ppg.ppg_backend()
    with pytest.raises(ValueError, match="MI355PPO_PPG"):
        _learner()
    monkeypatch.setenv("MI355PPO_PPG", "fused")
    assert not _learner().ppg_fused                               # HIP learner only: a host learner stays on its own path


# ---------------------------------------------------------------------------------------------- the learner's fused branch on the CPU
ENVS = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))


def _learner(T=8, N=4, **over):
    kw = dict(num_steps=T, num_minibatches=2, gamma=0.999, clip_coef=0.2, adv_norm_fullbatch=True, e_policy=1, e_auxiliary=2, beta_clone=1.0,
              num_aux_rollouts=2, n_aux_grad_accum=1, aux_batch_rollouts=N, n_iteration=1, learning_rate=5e-4)
    kw.update(over)
    return PPGLearner(PPGAgent(ENVS), default_args(**kw), ENVS.single_observation_space, ENVS.single_action_space, N, CPU)


def _fused_ops():
    from test_hip_branches_on_fake_ops import FakeOps

    class FusedOps(FakeOps):
        ppg_aux_gather = staticmethod(host_ops.ppg_aux_gather)
        ppg_old_logits_ = staticmethod(host_ops.ppg_old_logits_)
        ppg_aux_fwd_bwd = staticmethod(host_ops.ppg_aux_fwd_bwd)
        clip_adam_split_ = staticmethod(host_ops.clip_adam_split_)

    return FusedOps


def _through_the_policy_phase(L, g, fake):
    """Teacher-forced through tests/golden/ppg_phase.npz up to the end of the policy phase, as the GPU golden test drives it."""
    T = L.T
    as_obs = (lambda x: torch.from_numpy(x)) if fake else (lambda x: x)
    F = lambda k: torch.from_numpy(g[k])
    L.observe(0, as_obs(g["frames_u8"][0]), as_obs(g["step_done"][0]))
    torch.manual_seed(int(g["sample_seed"]))
    for step in range(T):
        L.act(step)
        L.actions[step].copy_(F("actions")[step]); L.logprobs[step].copy_(F("logprobs")[step]); L.values[step].copy_(F("values")[step])
        L.store_reward(step, g["rewards"][step])
        L.observe(step + 1, as_obs(g["frames_u8"][step + 1]), as_obs(g["step_done"][step + 1]))
    L.finish_rollout()
    L.returns.copy_(F("returns"))
    L.advantages.copy_(L.returns - L.values)
    np.random.seed(int(g["shuffle_seed"]))
    L.update(float(g["lr"]))


def _pair_after_the_policy_phase(g):
    from test_hip_branches_on_fake_ops import _pair

    host, fake = _pair(lambda: PPGAgent(ENVS), lambda ag: PPGLearner(ag, _learner().args, ENVS.single_observation_space,
                                                                      ENVS.single_action_space, 4, CPU))
    for L in (host, fake):                                        # the golden's initial weights on both (one-thread seeding, as minted)
        torch.manual_seed(int(g["init_seed"]))
        src = PPGAgent(ENVS)
        with torch.no_grad():
            for p, q in zip(L.agent.parameters(), src.parameters()):
                p.copy_(q)
    _through_the_policy_phase(host, g, False)
    _through_the_policy_phase(fake, g, True)
    fake.ops, fake.ppg_fused = _fused_ops(), True
    return host, fake


def _flat(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


def _delta_matches(got_now, init_sub, final_sub, what, frac, rtol=5e-2, atol=2e-5):
    delta, want = got_now - init_sub, final_sub - init_sub
    close = np.isclose(delta, want, rtol=rtol, atol=atol)
    assert close.mean() > frac, f"{what}: only {close.mean():.4f} of sampled parameters moved as the reference's did"


def test_fused_branch_of_the_learner_through_the_golden_phase_against_the_host_learner(one_thread, monkeypatch, capsys):
    """Per minibatch the three losses, per optimiser step the flat gradient before it: the fused branch (on the twins) against the host
    learner's ``aux_phase`` (the reference's lines with autograd), at the project's numeric rule.  The rule needs the deviation a
    correct float32 implementation shows on the same quantity; no float64 run of the learner is recorded, so that role is played
    by the ``torch`` backend of the same HIP branch (the parent's code path), run from the same state against the same host
    learner: the fused branch may deviate from the host learner by at most twice what the ``torch`` backend does, plus 2e-6.  (An
    absolute 2e-6 alone cannot hold for any path: the flat gradient reaches 10, where one float32 ulp is 1e-6, and the two
    learners leave the policy phase 1e-6 apart.)  Then the parameters at the bars of the GPU golden test, and the shuffle stream."""
    monkeypatch.delenv("MI355PPO_PPG", raising=False)
    monkeypatch.delenv("MI355PPO_IMPALA", raising=False)
    g = load_golden("ppg_phase")["ppg_T8_N4"]
    host, fake = _pair_after_the_policy_phase(g)
    _, parent = _pair_after_the_policy_phase(g)
    parent.ppg_fused = False
    assert not host.ppg_fused and fake.hip and fake._stale_grads is not None and torch.equal(fake._stale_grads, parent._stale_grads)
    LOSSES = ("kl_loss", "aux_value_loss", "real_value_loss")
    # the host learner and the torch backend: their losses are locals of aux_phase, read from its frame when it steps
    # (n_aux_grad_accum = 1: every minibatch)
    rec_host, rec_parent, rec_fake, seen = [], [], [], {}
    real_clip = torch.nn.utils.clip_grad_norm_

    def recording_clip(params, max_norm):
        loc = sys._getframe(1).f_locals
        rec_host.append(([float(loc[k].detach()) for k in LOSSES], torch.cat([p.grad.reshape(-1) for p in host.agent.parameters()]).clone()))
        return real_clip(params, max_norm)

    monkeypatch.setattr(learner_ppg.nn.utils, "clip_grad_norm_", recording_clip)
    np.random.seed(4)
    aux_host = host.aux_phase()
    after_host = np.random.random()
    monkeypatch.setattr(learner_ppg.nn.utils, "clip_grad_norm_", real_clip)
    parent_step = parent._aux_step_hip

    def recording_parent_step(lr):
        loc = sys._getframe(1).f_locals
        rec_parent.append(([float(loc[k].detach()) for k in LOSSES], parent.flat.grads.clone()))
        return parent_step(lr)

    parent._aux_step_hip = recording_parent_step
    np.random.seed(4)
    parent.aux_phase()
    # the fused branch: the scalars tensor and the flat gradient as clip_adam_split_ receives them
    ops = fake.ops
    real_loss, real_step = ops.ppg_aux_fwd_bwd, ops.clip_adam_split_

    def recording_loss(*a, **kw):
        out = real_loss(*a, **kw)
        seen["losses"] = out[0].tolist()
        return out

    def recording_step(params, grads, *a, **kw):
        rec_fake.append((seen["losses"], grads.clone()))
        return real_step(params, grads, *a, **kw)

    ops.ppg_aux_fwd_bwd, ops.clip_adam_split_ = staticmethod(recording_loss), staticmethod(recording_step)
    np.random.seed(4)
    aux_fake = fake.aux_phase()
    after_fake = np.random.random()
    assert "aux epoch 2" in capsys.readouterr().out
    assert after_host == after_fake                               # the shuffle stream was consumed exactly as on the host path
    assert len(rec_host) == len(rec_parent) == len(rec_fake) == 4                    # 2 epochs x 2 minibatches
    for k, ((lh, gh), (lp, gp), (lf, gf)) in enumerate(zip(rec_host, rec_parent, rec_fake)):
        dl, bl = max(abs(a - b) for a, b in zip(lh, lf)), 2 * max(abs(a - b) for a, b in zip(lh, lp)) + 2e-6
        dg, bg = float((gh - gf).abs().max()), 2 * float((gh - gp).abs().max()) + 2e-6
        print(f"minibatch {k}: losses {dl:.3e} (bar {bl:.3e}), flat gradient {dg:.3e} (bar {bg:.3e}; |g| max {float(gh.abs().max()):.3e})")
        assert dl <= bl and dg <= bg, (k, dl, bl, dg, bg)
    for k in aux_host:
        assert abs(aux_host[k] - aux_fake[k]) <= 2 * abs(aux_host[k] - parent.last_aux[k]) + 2e-6 and fake.last_aux[k] == aux_fake[k]
    stride = int(g["stride"])
    _delta_matches(_flat(fake.agent)[::stride].numpy(), g["init_params_sub"], g["final_params_sub"], "PPG auxiliary phase (fused)", frac=0.85)
    assert fake._aux_update == 0 and fake._stale_grads is None and fake._aux_tail_step == 4 and fake.flat.step == 2 + 4
    assert torch.count_nonzero(fake.flat.grads) == 0
    fake.flat.check_views()


def _launches_of(source: str, entry: str) -> int:
    """``hipLaunchKernelGGL`` sites in the body of the extern "C" entry point ``entry`` (one branch of an if / else counts once)."""
    src = (Path(_lib.__file__).parent / "csrc" / source).read_text()
    start = src.index(f"int {entry}(")
    body = src[start:src.index("\n}\n", start)]
    return len(re.findall(r"hipLaunchKernelGGL\(", body))


def test_launch_budget_of_the_auxiliary_phase(one_thread, monkeypatch, capsys):
    """Above the trunk and ``encodertop`` an auxiliary minibatch makes at most 3 library calls (gather, loss, step) and at most 6
    launches, an old-policy minibatch 2 calls.  What is counted is the calls on the twins' ``_lib.call``; the launches per call are
    read off the entry points' source."""
    g = load_golden("ppg_phase")["ppg_T8_N4"]
    _, fake = _pair_after_the_policy_phase(g)
    launches = {"mi355ppo_ppg_aux_gather_u8_f32": _launches_of("ppg.hip", "mi355ppo_ppg_aux_gather_u8_f32"),
                "mi355ppo_ppg_old_logits_f32": _launches_of("ppg.hip", "mi355ppo_ppg_old_logits_f32"),
                "mi355ppo_ppg_aux_fwd_bwd_f32": _launches_of("ppg.hip", "mi355ppo_ppg_aux_fwd_bwd_f32"),
                "mi355ppo_clip_adam_split_f32": _launches_of("optim.hip", "mi355ppo_clip_adam_split_f32")}
    assert launches == {"mi355ppo_ppg_aux_gather_u8_f32": 1, "mi355ppo_ppg_old_logits_f32": 1, "mi355ppo_ppg_aux_fwd_bwd_f32": 2,
                        "mi355ppo_clip_adam_split_f32": 2}
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name[:-len("_cpu")]), real(name, *a))[1])
    np.random.seed(4)
    fake.aux_phase()
    capsys.readouterr()
    old, mb = ["mi355ppo_ppg_aux_gather_u8_f32", "mi355ppo_ppg_old_logits_f32"], ["mi355ppo_ppg_aux_gather_u8_f32",
                                                                                     "mi355ppo_ppg_aux_fwd_bwd_f32", "mi355ppo_clip_adam_split_f32"]
    assert seen == old * 2 + mb * 4                               # R / num_aux_rollouts = 2 minibatches; 2 epochs of them
    assert len(mb) <= 3 and sum(launches[k] for k in mb) <= 6 and len(old) == 2
