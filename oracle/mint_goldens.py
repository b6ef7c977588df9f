"""Mint ``tests/golden/*.npz`` by executing the reference's own source lines.

TEST INFRASTRUCTURE.  Run in the build container only (needs ``/root/reference``):

    python -m oracle.mint_goldens

Every array written here is either a seeded synthetic *input* or an *output of the
reference's verbatim lines* (``oracle/ref_extract.py``) under the installed
torch 2.10.0 on CPU (reference pin: torch 2.4.1).  The fixtures are small (a few MB in
total) and are committed; the GPU box has no ``/root/reference`` and only reads them.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import synthetic  # noqa: E402  (input generators only)
from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
torch.set_num_threads(1)
torch.use_deterministic_algorithms(True)


def _np(d):
    out = {}
    for k, v in d.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    return out


def _save(name, cases):
    flat = {}
    for case, d in cases.items():
        for k, v in _np(d).items():
            flat[f"{case}/{k}"] = v
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **flat)
    print(f"{name}: {len(cases)} cases, {os.path.getsize(path) / 1024:.0f} KiB")


# ---------------------------------------------------------------------------------- GAE
def mint_gae():
    cases = {}

    def run(name, script, rewards, dones, values, next_done, next_value, gamma, lam):
        adv, ret = R.run_gae(script, rewards, dones, values, next_done, next_value, gamma, lam)
        cases[name] = dict(rewards=rewards, dones=dones, values=values, next_done=next_done, next_value=next_value,
                           gamma=np.float64(gamma), gae_lambda=np.float64(lam), advantages=adv, returns=ret,
                           script=np.bytes_(script))

    # the shape/distributions of the reference's only numeric test (tests/test_jax_compute_gae.py:66-88)
    g = torch.Generator().manual_seed(42)
    T, N = 123, 7
    run("jaxtest_123x7", "ppo_atari_envpool.py",
        torch.rand(T, N, generator=g) * 2 - 1, torch.randint(0, 2, (T, N), generator=g).float(),
        torch.rand(T, N, generator=g), torch.randint(0, 2, (N,), generator=g).float(), torch.rand(N, generator=g),
        0.99, 0.95)
    # BASELINE.json configs A, B (full), C/D/E (narrow slices of the same generators)
    for name, script, (T, N), A in [
        ("A_128x4", "ppo.py", (128, 4), 2),
        ("B_128x128", "ppo_atari_envpool.py", (128, 128), 4),
        ("C_128x1024", "ppo_atari.py", (128, 1024), 4),
        ("D_128x256", "ppo_atari_multigpu.py", (128, 256), 4),
        ("E_2048x16", "ppo_continuous_action.py", (2048, 16), 4),
    ]:
        s = synthetic.rollout_scalars(T, N, A, seed=1)
        run(name, script, s["rewards"], s["dones"], s["values"], s["next_done"], s["next_value"], 0.99, 0.95)
    # edges: T=1, N=1, ragged N, every step terminal, no terminal, gamma=lambda=1, next_done set
    g = torch.Generator().manual_seed(7)
    for name, (T, N), dmode, gam, lam in [
        ("edge_1x1", (1, 1), "rand", 0.99, 0.95), ("edge_1x5", (1, 5), "rand", 0.99, 0.95),
        ("edge_5x1", (5, 1), "rand", 0.99, 0.95), ("edge_33x67", (33, 67), "rand", 0.99, 0.95),
        ("edge_alldone_16x9", (16, 9), "ones", 0.99, 0.95), ("edge_nodone_16x9", (16, 9), "zeros", 0.99, 0.95),
        ("edge_gamma1_40x13", (40, 13), "rand", 1.0, 1.0), ("edge_g09_l08_40x13", (40, 13), "rand", 0.9, 0.8),
        ("edge_lam0_40x13", (40, 13), "rand", 0.99, 0.0),
    ]:
        rewards = torch.randn(T, N, generator=g)
        values = torch.randn(T, N, generator=g) * 3
        if dmode == "rand":
            dones = (torch.rand(T, N, generator=g) < 0.2).float()
            nd = (torch.rand(N, generator=g) < 0.5).float()
        else:
            dones = torch.ones(T, N) if dmode == "ones" else torch.zeros(T, N)
            nd = torch.ones(N) if dmode == "ones" else torch.zeros(N)
        run(name, "ppo.py", rewards, dones, values, nd, torch.randn(N, generator=g), gam, lam)
    _save("gae", cases)


# ----------------------------------------------------------------------- distributions
def mint_categorical():
    """``Agent.get_action_and_value`` sampling path with the reference's Categorical (torch)."""
    from torch.distributions.categorical import Categorical

    cases = {}
    g = torch.Generator().manual_seed(11)
    for name, B, A, scale in [("B1_A4", 1, 4, 1.0), ("B7_A2", 7, 2, 1.0), ("B1024_A4", 1024, 4, 1.0),
                              ("B1000_A6", 1000, 6, 3.0), ("B513_A18", 513, 18, 1.0),
                              ("B256_A4_peaked", 256, 4, 30.0), ("B256_A9_tiny", 256, 9, 0.01)]:
        logits = torch.randn(B, A, generator=g) * scale
        probs = Categorical(logits=logits)
        torch.manual_seed(1234)
        action = probs.sample()                       # ppo_atari_multigpu.py:158
        torch.manual_seed(1234)
        noise = torch.empty_like(probs.probs).exponential_(1)   # the q of multinomial's one-draw fast path
        assert torch.equal(action, torch.argmax(probs.probs / noise, -1))
        cases[name] = dict(logits=logits, noise_exp1=noise, action=action, logprob=probs.log_prob(action),
                           entropy=probs.entropy(), probs=probs.probs)
    _save("categorical", cases)


def mint_normal():
    from torch.distributions.normal import Normal

    cases = {}
    g = torch.Generator().manual_seed(13)
    for name, B, D in [("B1_D1", 1, 1), ("B64_D6", 64, 6), ("B1000_D17", 1000, 17), ("B333_D3", 333, 3)]:
        mean = torch.randn(B, D, generator=g)
        logstd = torch.randn(1, D, generator=g) * 0.5
        std = torch.exp(logstd.expand_as(mean))       # ppo_continuous_action.py:135-137
        probs = Normal(mean, std)
        torch.manual_seed(99)
        action = probs.sample()
        torch.manual_seed(99)
        z = torch.empty_like(mean).normal_()
        assert torch.equal(action, z * std + mean)
        cases[name] = dict(mean=mean, logstd=logstd.reshape(-1), noise=z, action=action,
                           logprob_sum=probs.log_prob(action).sum(1), entropy_sum=probs.entropy().sum(1))
    _save("normal", cases)


# ------------------------------------------------------------------------------- loss
def _behaviour_batch(g, new_lp, new_value, B):
    """Old-policy tensors around the fresh policy so that ratios land inside AND outside the clip range."""
    s = torch.where(torch.rand(B, generator=g) < 0.5, torch.tensor(0.03), torch.tensor(0.6))
    b_logprobs = (new_lp + torch.randn(B, generator=g) * s).detach()
    sv = torch.where(torch.rand(B, generator=g) < 0.5, torch.tensor(0.05), torch.tensor(0.5))
    b_values = (new_value + torch.randn(B, generator=g) * sv).detach()
    b_advantages = torch.randn(B, generator=g) * 1.7 + 0.3
    b_returns = b_values + b_advantages
    return b_logprobs, b_advantages, b_returns, b_values


def _hooked(module):
    box = {}

    def hook(_m, _inp, out):
        out.retain_grad()
        box["out"] = out

    module.register_forward_hook(hook)
    return box


def mint_loss_categorical():
    cases = {}
    g = torch.Generator().manual_seed(21)
    specs = [
        ("mlp_A2", "ppo.py", (4,), 2, 512, 128, dict(clip_coef=0.2)),
        ("mlp_A2_noadvnorm", "ppo.py", (4,), 2, 512, 128, dict(clip_coef=0.2, norm_adv=False)),
        ("mlp_A2_novclip", "ppo.py", (4,), 2, 512, 128, dict(clip_coef=0.2, clip_vloss=False)),
        ("mlp_A2_plain", "ppo.py", (4,), 2, 512, 128, dict(clip_coef=0.2, clip_vloss=False, norm_adv=False, ent_coef=0.0)),
        ("cnn_A4", "ppo_atari_envpool.py", (4, 84, 84), 4, 256, 64, {}),
        ("cnn_A18", "ppo_atari.py", (4, 84, 84), 18, 96, 32, {}),
        ("cnn_A4_multigpu", "ppo_atari_multigpu.py", (4, 84, 84), 4, 256, 64, {}),
    ]
    for name, script, obs_shape, A, B, M, kw in specs:
        torch.manual_seed(5)
        Agent, _ = R.load_agent_class(script)
        agent = Agent(R.fake_envs(obs_shape, n_actions=A))
        args = R.make_args(**kw)
        if len(obs_shape) == 3:
            b_obs = torch.randint(0, 256, (B,) + obs_shape, generator=g).float()
        else:
            b_obs = torch.randn((B,) + obs_shape, generator=g)
        b_actions = torch.randint(0, A, (B,), generator=g).float()        # stored as f32 (:236)
        with torch.no_grad():
            _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions.long())
        b_logprobs, b_advantages, b_returns, b_values = _behaviour_batch(g, lp_all, v_all.view(-1), B)
        mb_inds = np.random.RandomState(3).permutation(B)[:M]
        actor_last = agent.actor if isinstance(agent.actor, torch.nn.Linear) else agent.actor[-1]
        critic_last = agent.critic if isinstance(agent.critic, torch.nn.Linear) else agent.critic[-1]
        lbox, vbox = _hooked(actor_last), _hooked(critic_last)
        ns = R.run_loss(script, agent, args, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, mb_inds)
        ns["loss"].backward()
        cases[name] = dict(
            new_logits=lbox["out"], new_value=vbox["out"].view(-1), mb_inds=mb_inds.astype(np.int64),
            b_actions=b_actions, b_logprobs=b_logprobs, b_advantages=b_advantages, b_returns=b_returns, b_values=b_values,
            clip_coef=np.float64(args.clip_coef), ent_coef=np.float64(args.ent_coef), vf_coef=np.float64(args.vf_coef),
            norm_adv=np.int32(args.norm_adv), clip_vloss=np.int32(args.clip_vloss),
            loss=ns["loss"], pg_loss=ns["pg_loss"], v_loss=ns["v_loss"], entropy=ns["entropy_loss"],
            old_approx_kl=ns["old_approx_kl"], approx_kl=ns["approx_kl"], clipfrac=np.float32(ns["clipfracs"][0]),
            newlogprob=ns["newlogprob"], dlogits=lbox["out"].grad, dvalue=vbox["out"].grad.view(-1),
            script=np.bytes_(script))
    _save("loss_categorical", cases)


def mint_loss_normal():
    cases = {}
    g = torch.Generator().manual_seed(23)
    script = "ppo_continuous_action.py"
    for name, obs_dim, D, B, M, kw in [
        ("halfcheetah_D6", 17, 6, 1024, 256, dict(clip_coef=0.2, ent_coef=0.0)),
        ("halfcheetah_D6_ent", 17, 6, 1024, 256, dict(clip_coef=0.2, ent_coef=0.01)),
        ("hopper_D3_noadvnorm", 11, 3, 512, 128, dict(clip_coef=0.2, ent_coef=0.0, norm_adv=False)),
        ("d1_novclip", 3, 1, 256, 64, dict(clip_coef=0.2, ent_coef=0.02, clip_vloss=False)),
    ]:
        torch.manual_seed(9)
        Agent, _ = R.load_agent_class(script)
        agent = Agent(R.fake_envs((obs_dim,), action_shape=(D,)))
        with torch.no_grad():
            agent.actor_logstd.copy_(torch.randn(1, D, generator=g) * 0.3)
        args = R.make_args(**kw)
        b_obs = torch.randn(B, obs_dim, generator=g)
        with torch.no_grad():
            mean_all = agent.actor_mean(b_obs)
            b_actions = mean_all + torch.randn(B, D, generator=g) * torch.exp(agent.actor_logstd)
            _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions)
        b_logprobs, b_advantages, b_returns, b_values = _behaviour_batch(g, lp_all, v_all.view(-1), B)
        mb_inds = np.random.RandomState(4).permutation(B)[:M]
        mbox, vbox = _hooked(agent.actor_mean[-1]), _hooked(agent.critic[-1])
        ns = R.run_loss(script, agent, args, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values, mb_inds)
        ns["loss"].backward()
        cases[name] = dict(
            new_mean=mbox["out"], logstd=agent.actor_logstd.detach().reshape(-1), new_value=vbox["out"].view(-1),
            mb_inds=mb_inds.astype(np.int64), b_actions=b_actions, b_logprobs=b_logprobs, b_advantages=b_advantages,
            b_returns=b_returns, b_values=b_values,
            clip_coef=np.float64(args.clip_coef), ent_coef=np.float64(args.ent_coef), vf_coef=np.float64(args.vf_coef),
            norm_adv=np.int32(args.norm_adv), clip_vloss=np.int32(args.clip_vloss),
            loss=ns["loss"], pg_loss=ns["pg_loss"], v_loss=ns["v_loss"], entropy=ns["entropy_loss"],
            old_approx_kl=ns["old_approx_kl"], approx_kl=ns["approx_kl"], clipfrac=np.float32(ns["clipfracs"][0]),
            newlogprob=ns["newlogprob"], dmean=mbox["out"].grad, dlogstd=agent.actor_logstd.grad.reshape(-1),
            dvalue=vbox["out"].grad.view(-1), script=np.bytes_(script))
    _save("loss_normal", cases)


# --------------------------------------------------------------- full update step (a7+a8+a9)
def _flat(params):
    return torch.cat([p.detach().reshape(-1) for p in params])


GRAD_STRIDE = 7


class _GradSpy:
    """Wraps the reference's optimizer object inside the exec'ed update lines: records what ``optimizer.step()`` sees in
    ``.grad`` -- i.e. the gradient after ``loss.backward()``, the collective block (multi-GPU script) and
    ``clip_grad_norm_`` -- for the first ``keep`` steps.  Everything else is forwarded untouched."""

    def __init__(self, optimizer, params, keep=1, keep_steps=None, on_step=None):
        self._opt, self._params, self._keep, self.grads = optimizer, list(params), keep, []
        self._keep_steps, self._on_step, self.n_steps = keep_steps, on_step, 0      # 1-based step numbers to record instead of the first `keep`

    def __getattr__(self, name):
        return getattr(self._opt, name)

    def step(self, *a, **kw):
        self.n_steps += 1
        if (self._keep_steps is None and len(self.grads) < self._keep) or (self._keep_steps is not None and self.n_steps in self._keep_steps):
            self.grads.append(_flat([p.grad for p in self._params]).clone())
        if self._on_step is not None:
            self._on_step(self.n_steps)
        return self._opt.step(*a, **kw)


def _grad_record(prefix, g, params, stride=GRAD_STRIDE):
    """Strided subsample + norms of a flat gradient (the whole vector is 6.7 MB; the subsample estimates the cosine,
    the norms pin the scale globally and per parameter tensor)."""
    sizes = [p.numel() for p in params]
    per = torch.stack([t.double().norm() for t in torch.split(g, sizes)])
    return {f"{prefix}_sub": g[::stride].clone(), f"{prefix}_norm": np.float64(g.double().norm().item()),
            f"{prefix}_tensor_norms": per, f"{prefix}_absmax": np.float64(g.abs().max().item()),
            f"{prefix}_stride": np.int64(stride)}


class _FakeDist:
    """Stand-in for ``torch.distributed`` inside ppo_atari_multigpu.py:360-374: a 2-rank SUM all-reduce
    whose other rank's flat gradient was computed beforehand."""

    class ReduceOp:
        SUM = "sum"

    def __init__(self, other_flat_grad):
        self.other = other_flat_grad

    def all_reduce(self, tensor, op=None):
        tensor.add_(self.other)


def mint_update_step():
    cases = {}
    g = torch.Generator().manual_seed(31)
    # (1) ppo.py MLP: 3 consecutive minibatch updates (loss + backward + clip_grad_norm_ + Adam)
    script = "ppo.py"
    torch.manual_seed(1)
    Agent, _ = R.load_agent_class(script)
    agent = Agent(R.fake_envs((4,), n_actions=2))
    args = R.make_args(clip_coef=0.2)
    opt = R.make_optimizer(agent, 2.5e-4)
    B, M = 512, 128
    b_obs = torch.randn(B, 4, generator=g)
    b_actions = torch.randint(0, 2, (B,), generator=g).float()
    with torch.no_grad():
        _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions.long())
    b_logprobs, b_advantages, b_returns, b_values = _behaviour_batch(g, lp_all, v_all.view(-1), B)
    perm = np.random.RandomState(5).permutation(B)
    d = dict(init_params=_flat(agent.parameters()), b_obs=b_obs, b_actions=b_actions, b_logprobs=b_logprobs,
             b_advantages=b_advantages, b_returns=b_returns, b_values=b_values, perm=perm.astype(np.int64),
             lr=np.float64(2.5e-4), clip_coef=np.float64(0.2), ent_coef=np.float64(0.01), vf_coef=np.float64(0.5),
             max_grad_norm=np.float64(0.5), shapes=np.array([p.numel() for p in agent.parameters()], np.int64))
    losses, gnorm = [], []
    for k in range(3):
        ns = R.run_loss(script, agent, args, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                        perm[k * M:(k + 1) * M], step=True, optimizer=opt)
        losses.append(ns["loss"].item())
        d[f"params_after_{k + 1}"] = _flat(agent.parameters())
    d["losses"] = np.array(losses, np.float32)
    cases["ppo_mlp_3steps"] = d

    # (2) ppo_atari_multigpu.py NatureCNN, world_size=2: flat-grad all-reduce SUM, /world_size, clip, Adam
    script = "ppo_atari_multigpu.py"
    torch.manual_seed(1)
    Agent, _ = R.load_agent_class(script)
    agent = Agent(R.fake_envs((4, 84, 84), n_actions=4))
    args = R.make_args(world_size=2)
    opt = R.make_optimizer(agent, 2.5e-4)
    B, M = 64, 32
    ranks = []
    for r in range(2):
        b_obs = torch.randint(0, 256, (B, 4, 84, 84), generator=g).float()
        b_actions = torch.randint(0, 4, (B,), generator=g).float()
        with torch.no_grad():
            _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions.long())
        ranks.append((b_obs, b_actions) + _behaviour_batch(g, lp_all, v_all.view(-1), B))
    mb = np.random.RandomState(6).permutation(B)[:M]
    # rank 1's local gradient (no step)
    ns1 = R.run_loss(script, agent, args, *ranks[1], mb)
    agent.zero_grad()
    ns1["loss"].backward()
    g1 = _flat([p.grad for p in agent.parameters()]).clone()
    agent.zero_grad()
    init = _flat(agent.parameters()).clone()
    # rank 0 executes :320-377 including the collective block against the fake dist
    ns0 = R.run_loss(script, agent, args, *ranks[0], mb)
    lines = R._read(script)
    lo = R._find(lines, "optimizer.zero_grad()")
    hi = R._find(lines, "optimizer.step()", lo)
    import textwrap
    ns0["dist"] = _FakeDist(g1)
    spy = _GradSpy(opt, agent.parameters())
    ns0["optimizer"] = spy
    exec(textwrap.dedent("\n".join(lines[lo:hi + 1])), ns0)       # ppo_atari_multigpu.py:357-377
    final = _flat(agent.parameters())
    sub = slice(0, None, 53)
    cases["multigpu_cnn_world2"] = dict(
        obs_u8_rank0=ranks[0][0].to(torch.uint8), obs_u8_rank1=ranks[1][0].to(torch.uint8),
        **{f"{k}_rank{r}": ranks[r][i + 1] for r in range(2)
           for i, k in enumerate(["b_actions", "b_logprobs", "b_advantages", "b_returns", "b_values"])},
        mb_inds=mb.astype(np.int64), init_params_sub=init[sub], final_params_sub=final[sub],
        delta_sub=(final - init)[sub], loss_rank0=ns0["loss"].detach(), loss_rank1=ns1["loss"].detach(),
        init_seed=np.int64(1), stride=np.int64(53), lr=np.float64(2.5e-4),
        init_checksum=np.float64(init.double().sum().item()), final_checksum=np.float64(final.double().sum().item()),
        # what optimizer.step() saw: (g0 + g1) / world_size after clip_grad_norm_ (:368-376); g1 = rank 1's local gradient
        **_grad_record("step_grad", spy.grads[0], agent.parameters()), **_grad_record("rank1_grad", g1, agent.parameters()))
    _save("update_step", cases)


# --------------------------------------------------------------- feed-forward Atari script: one whole iteration
def mint_atari_iteration():
    """One whole iteration of ppo_atari_envpool.py (config B's script) on synthetic inputs (T=8, N=4): the reference
    Agent's action logic (:223-232) fills the rollout, then its GAE lines (:251-263) and its flatten + epoch / minibatch
    update lines (:265-322, 2 minibatches x 2 epochs) are executed verbatim."""
    import textwrap

    import torch.nn as nn

    script = "ppo_atari_envpool.py"
    lines = R._read(script)
    T, N, A = 8, 4, 4
    torch.manual_seed(21)
    Agent, _ = R.load_agent_class(script)
    envs = R.fake_envs((4, 84, 84), n_actions=A)
    agent = Agent(envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=2, update_epochs=2, batch_size=T * N, minibatch_size=T * N // 2)
    optimizer = _GradSpy(R.make_optimizer(agent, 2.5e-4), agent.parameters())
    init = _flat(agent.parameters()).clone()
    g = torch.Generator().manual_seed(53)
    frames = torch.randint(0, 256, (T + 1, N, 4, 84, 84), generator=g, dtype=torch.uint8)
    step_done = (torch.rand(T + 1, N, generator=g) < 0.2).float()
    step_done[0] = 0.0
    rewards = torch.randint(-1, 2, (T, N), generator=g).float()
    obs = torch.zeros((T, N, 4, 84, 84))
    actions, logprobs, dones, values = (torch.zeros((T, N)) for _ in range(4))
    torch.manual_seed(23)                                      # the sampler's stream
    for step in range(T):
        obs[step], dones[step] = frames[step].float(), step_done[step]
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(obs[step])
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = frames[T].float(), step_done[T]
    device = torch.device("cpu")
    ns = dict(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs,
              rewards=rewards, dones=dones, values=values, next_obs=next_obs, next_done=next_done, device=device, np=np,
              torch=torch, nn=nn)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    np.random.seed(6)
    exec(textwrap.dedent("\n".join(lines[u0:u1])), ns)
    final = _flat(agent.parameters())
    sub = slice(0, None, 89)
    cases = {"atari_T8_N4": dict(
        frames_u8=frames, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, values=values,
        advantages=ns["advantages"], returns=ns["returns"], init_params_sub=init[sub], final_params_sub=final[sub],
        stride=np.int64(89), init_checksum=np.float64(init.double().sum().item()),
        final_checksum=np.float64(final.double().sum().item()), last_loss=ns["loss"].detach(), last_pg_loss=ns["pg_loss"].detach(),
        last_v_loss=ns["v_loss"].detach(), last_entropy=ns["entropy_loss"].detach(), last_approx_kl=ns["approx_kl"],
        clipfracs=np.array(ns["clipfracs"], np.float32), init_seed=np.int64(21), sample_seed=np.int64(23),
        shuffle_seed=np.int64(6), lr=np.float64(2.5e-4), lines=np.array([g0 + 1, g1 + 1, u0 + 1, u1], np.int64),
        # the clipped gradient the FIRST optimizer.step() of the update saw (minibatch 1 of epoch 1)
        **_grad_record("mb1_grad", optimizer.grads[0], agent.parameters()))}
    _save("atari_iteration", cases)


# --------------------------------------------------------------- config B at its full size: one whole iteration, 16 updates
SCALAR_KEYS = ("loss", "pg_loss", "v_loss", "entropy_loss", "old_approx_kl", "approx_kl")


def mint_atari_iteration_config_b(save=True):
    """BASELINE configs[1] at full size: one whole iteration of ppo_atari_envpool.py with num_envs = 128, num_steps = 128,
    4 minibatches x 4 epochs = 16 updates of 4,096 rows.  The reference Agent's action logic (:223-232) fills the rollout, then
    its GAE lines (:251-263) and its flatten + epoch / minibatch update lines (:265-322) are executed verbatim.  The frames
    (129 x 128 x 4 x 84 x 84 uint8 = 466 MB) come from ``synthetic.atari_frames`` (numpy legacy RandomState: both sides
    regenerate them from the seed; a checksum is stored).  Recorded: the seven scalars of ALL 16 minibatches, the clipped
    flat gradient the optimizer saw at updates 1, 8 and 16 (strided), the parameters after update 16 (strided), the rollout
    tensors (actions, log-probs, values) and the GAE output."""
    import textwrap

    import torch.nn as nn

    script = "ppo_atari_envpool.py"
    lines = R._read(script)
    T, N, A = 128, 128, 4
    frame_seed = 77
    torch.manual_seed(21)
    Agent, _ = R.load_agent_class(script)
    envs = R.fake_envs((4, 84, 84), n_actions=A)
    agent = Agent(envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=4, update_epochs=4, batch_size=T * N, minibatch_size=T * N // 4)
    ns = {}
    scalars = []

    def on_step(k):          # called inside the reference's own loop, right before optimizer.step() of update k
        scalars.append([float(ns[key]) for key in SCALAR_KEYS] + [float(ns["clipfracs"][-1])])

    optimizer = _GradSpy(R.make_optimizer(agent, 2.5e-4), agent.parameters(), keep_steps=(1, 8, 16), on_step=on_step)
    init = _flat(agent.parameters()).clone()
    frames = torch.from_numpy(synthetic.atari_frames((T + 1) * N, seed=frame_seed)).view(T + 1, N, 4, 84, 84)
    rs = np.random.RandomState(frame_seed + 1)
    step_done = torch.from_numpy((rs.random_sample((T + 1, N)) < 1.0 / 50.0).astype(np.float32))
    step_done[0] = 0.0
    rewards = torch.from_numpy(rs.choice(np.array([-1.0, 0.0, 1.0], np.float32), size=(T, N), p=[0.05, 0.9, 0.05]).astype(np.float32))
    obs = torch.zeros((T, N, 4, 84, 84))
    actions, logprobs, dones, values = (torch.zeros((T, N)) for _ in range(4))
    torch.manual_seed(23)                                      # the sampler's stream
    for step in range(T):
        obs[step], dones[step] = frames[step].float(), step_done[step]
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(obs[step])
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = frames[T].float(), step_done[T]
    device = torch.device("cpu")
    ns.update(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs,
              rewards=rewards, dones=dones, values=values, next_obs=next_obs, next_done=next_done, device=device, np=np,
              torch=torch, nn=nn)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    np.random.seed(6)
    exec(textwrap.dedent("\n".join(lines[u0:u1])), ns)
    assert optimizer.n_steps == 16 and len(optimizer.grads) == 3
    final = _flat(agent.parameters())
    sub = slice(0, None, 89)
    d = dict(
        frame_seed=np.int64(frame_seed), frames_checksum=np.int64(frames.sum(dtype=torch.int64).item()),
        frames_first_row=frames[0, 0, 0, 0].clone(), step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs,
        values=values, advantages=ns["advantages"], returns=ns["returns"], init_params_sub=init[sub], final_params_sub=final[sub],
        stride=np.int64(89), init_checksum=np.float64(init.double().sum().item()),
        final_checksum=np.float64(final.double().sum().item()), scalars=np.array(scalars, np.float32),
        scalar_names=np.array(list(SCALAR_KEYS) + ["clipfrac"]), init_seed=np.int64(21), sample_seed=np.int64(23),
        shuffle_seed=np.int64(6), lr=np.float64(2.5e-4), lines=np.array([g0 + 1, g1 + 1, u0 + 1, u1], np.int64))
    for k, gk in zip((1, 8, 16), optimizer.grads):
        d.update(_grad_record(f"mb{k}_grad", gk, agent.parameters(), stride=53))
    if save:
        _save("atari_iteration_cfgB", {"atari_T128_N128": d})
    return _np(d)


# --------------------------------------------------------------- recurrent script: rollout -> GAE -> env-wise update
def mint_lstm_iteration():
    """One whole iteration of ppo_atari_lstm.py on synthetic inputs: the reference Agent's own action logic fills the
    rollout (T=8, N=4), then its GAE lines (:266-283) and its flatten + env-wise minibatch update lines (:285-356) are
    executed verbatim (2 minibatches x 2 epochs)."""
    import textwrap
    from types import SimpleNamespace

    import torch.nn as nn

    script = "ppo_atari_lstm.py"
    lines = R._read(script)
    T, N, A = 8, 4, 4
    torch.manual_seed(7)
    Agent, _ = R.load_agent_class(script)
    envs = R.fake_envs((1, 84, 84), n_actions=A)
    agent = Agent(envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=2, update_epochs=2, batch_size=T * N)
    optimizer = R.make_optimizer(agent, 2.5e-4)
    init = _flat(agent.parameters()).clone()
    g = torch.Generator().manual_seed(41)
    frames = torch.randint(0, 256, (T + 1, N, 1, 84, 84), generator=g, dtype=torch.uint8)
    step_done = (torch.rand(T + 1, N, generator=g) < 0.25).float()
    step_done[0] = 0.0
    rewards = torch.randint(-1, 2, (T, N), generator=g).float()
    obs = torch.zeros((T, N, 1, 84, 84))
    actions, logprobs, dones, values = (torch.zeros((T, N)) for _ in range(4))
    next_lstm_state = (torch.zeros(agent.lstm.num_layers, N, agent.lstm.hidden_size),
                       torch.zeros(agent.lstm.num_layers, N, agent.lstm.hidden_size))
    initial_lstm_state = (next_lstm_state[0].clone(), next_lstm_state[1].clone())
    torch.manual_seed(11)                                     # the sampler's stream (Categorical.sample)
    for step in range(T):                                      # :240-249, the env replaced by the synthetic stream
        next_obs, next_done = frames[step].float(), step_done[step]
        obs[step], dones[step] = next_obs, next_done
        with torch.no_grad():
            action, logprob, _, value, next_lstm_state = agent.get_action_and_value(next_obs, next_lstm_state, next_done)
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = frames[T].float(), step_done[T]
    device = torch.device("cpu")
    ns = dict(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs,
              rewards=rewards, dones=dones, values=values, next_obs=next_obs, next_done=next_done,
              next_lstm_state=next_lstm_state, initial_lstm_state=initial_lstm_state, device=device, np=np, torch=torch, nn=nn)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)              # :266-283
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    np.random.seed(5)                                                   # the env-index shuffle (:302)
    exec(textwrap.dedent("\n".join(lines[u0:u1])), ns)                  # :285-356
    final = _flat(agent.parameters())
    sub = slice(0, None, 97)
    cases = {"lstm_T8_N4": dict(
        frames_u8=frames, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, values=values,
        next_h=next_lstm_state[0], next_c=next_lstm_state[1], advantages=ns["advantages"], returns=ns["returns"],
        init_params_sub=init[sub], final_params_sub=final[sub], stride=np.int64(97),
        init_checksum=np.float64(init.double().sum().item()), final_checksum=np.float64(final.double().sum().item()),
        last_loss=ns["loss"].detach(), last_pg_loss=ns["pg_loss"].detach(), last_v_loss=ns["v_loss"].detach(),
        last_entropy=ns["entropy_loss"].detach(), last_approx_kl=ns["approx_kl"], clipfracs=np.array(ns["clipfracs"], np.float32),
        init_seed=np.int64(7), sample_seed=np.int64(11), shuffle_seed=np.int64(5), lr=np.float64(2.5e-4),
        lines=np.array([g0 + 1, g1 + 1, u0 + 1, u1], np.int64))}
    _save("lstm_iteration", cases)


# --------------------------------------------------------------- procgen: IMPALA-CNN agent, pixel-interleaved frames
def mint_procgen_update():
    """ppo_procgen.py: two consecutive minibatch updates (:259-299 loss + backward + clip_grad_norm_ + Adam) of the
    reference's IMPALA-CNN Agent on (B, 64, 64, 3) frames, plus its GAE lines on the rollout-shaped tensors."""
    script = "ppo_procgen.py"
    torch.manual_seed(9)
    Agent, _ = R.load_agent_class(script)
    agent = Agent(R.fake_envs((64, 64, 3), n_actions=15))
    args = R.make_args(clip_coef=0.2)
    opt = R.make_optimizer(agent, 5e-4)
    g = torch.Generator().manual_seed(43)
    B, M = 48, 16
    b_obs_u8 = torch.randint(0, 256, (B, 64, 64, 3), generator=g, dtype=torch.uint8)
    b_obs = b_obs_u8.float()
    b_actions = torch.randint(0, 15, (B,), generator=g).float()
    with torch.no_grad():
        _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions.long())
    b_logprobs, b_advantages, b_returns, b_values = _behaviour_batch(g, lp_all, v_all.view(-1), B)
    perm = np.random.RandomState(8).permutation(B)
    init = _flat(agent.parameters()).clone()
    sub = slice(0, None, 31)
    d = dict(init_params_sub=init[sub], stride=np.int64(31), init_checksum=np.float64(init.double().sum().item()),
             b_obs_u8=b_obs_u8, b_actions=b_actions, b_logprobs=b_logprobs, b_advantages=b_advantages, b_returns=b_returns,
             b_values=b_values, perm=perm.astype(np.int64), lr=np.float64(5e-4), init_seed=np.int64(9),
             logprob_all=lp_all, value_all=v_all.view(-1))
    losses = []
    for k in range(2):
        ns = R.run_loss(script, agent, args, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                        perm[k * M:(k + 1) * M], step=True, optimizer=opt)
        losses.append(ns["loss"].item())
        d[f"params_sub_after_{k + 1}"] = _flat(agent.parameters())[sub]
    d["losses"] = np.array(losses, np.float32)
    d["final_checksum"] = np.float64(_flat(agent.parameters()).double().sum().item())
    _save("procgen_update", {"impala_2steps": d})


# --------------------------------------------------------------- two-player Atari: 6-channel frames, partial /255
def mint_ma_atari_update():
    """ppo_pettingzoo_ma_atari.py: two consecutive minibatch updates (its loss + backward + clip + Adam lines) of the
    reference Agent on (B, 84, 84, 6) observations whose last two channels are agent-indicator planes."""
    script = "ppo_pettingzoo_ma_atari.py"
    torch.manual_seed(33)
    Agent, _ = R.load_agent_class(script)
    agent = Agent(R.fake_envs((84, 84, 6), n_actions=6))
    args = R.make_args(clip_coef=0.1)
    opt = R.make_optimizer(agent, 2.5e-4)
    g = torch.Generator().manual_seed(61)
    B, M = 32, 16
    frames = torch.randint(0, 256, (B, 84, 84, 4), generator=g, dtype=torch.uint8)
    ind = torch.zeros((B, 84, 84, 2), dtype=torch.uint8)
    ind[0::2, :, :, 0] = 1
    ind[1::2, :, :, 1] = 1
    b_obs_u8 = torch.cat([frames, ind], dim=-1)
    b_obs = b_obs_u8.float()
    b_actions = torch.randint(0, 6, (B,), generator=g).float()
    with torch.no_grad():
        _, lp_all, _, v_all = agent.get_action_and_value(b_obs, b_actions.long())
    b_logprobs, b_advantages, b_returns, b_values = _behaviour_batch(g, lp_all, v_all.view(-1), B)
    perm = np.random.RandomState(9).permutation(B)
    init = _flat(agent.parameters()).clone()
    sub = slice(0, None, 83)
    d = dict(init_params_sub=init[sub], stride=np.int64(83), b_obs_u8=b_obs_u8, b_actions=b_actions, b_logprobs=b_logprobs,
             b_advantages=b_advantages, b_returns=b_returns, b_values=b_values, perm=perm.astype(np.int64), lr=np.float64(2.5e-4),
             init_seed=np.int64(33), logprob_all=lp_all, value_all=v_all.view(-1))
    losses = []
    for k in range(2):
        ns = R.run_loss(script, agent, args, b_obs, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                        perm[k * M:(k + 1) * M], step=True, optimizer=opt)
        losses.append(ns["loss"].item())
        d[f"params_sub_after_{k + 1}"] = _flat(agent.parameters())[sub]
    d["losses"] = np.array(losses, np.float32)
    assert torch.equal(b_obs, b_obs_u8.float()), "the reference must not modify the stored observations"
    _save("ma_atari_update", {"ma_2steps": d})


# --------------------------------------------------------------- PPG: policy phase with full-batch normalisation + auxiliary phase
def mint_ppg_phase():
    """One whole phase of ppg_procgen.py with n_iteration = 1 on synthetic inputs (T=8, N=4): the reference Agent's action
    logic fills the rollout; its GAE lines, its flatten + full-batch advantage normalisation + policy minibatch lines
    (:330-392), its aux-buffer storage lines (:411-414) and its whole auxiliary phase (:416-471, 2 epochs x 2 minibatches of
    2 rollouts) are executed verbatim."""
    import ast
    import textwrap

    import torch.distributions as td
    import torch.nn as nn
    from torch.distributions.categorical import Categorical

    script = "ppg_procgen.py"
    lines = R._read(script)
    tree = ast.parse("\n".join(lines))
    cls_ns = {"np": np, "torch": torch, "nn": nn, "Categorical": Categorical}
    want = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))
            and n.name in ("layer_init_normed", "flatten01", "unflatten01", "ResidualBlock", "ConvSequence", "Agent")]
    exec(compile(ast.Module(body=want, type_ignores=[]), f"<reference:{script}>", "exec"), cls_ns)
    T, N, A = 8, 4, 15
    envs = R.fake_envs((64, 64, 3), n_actions=A)
    torch.manual_seed(27)
    agent = cls_ns["Agent"](envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=2, batch_size=T * N, minibatch_size=T * N // 2, gamma=0.999,
                       clip_coef=0.2, adv_norm_fullbatch=True, e_policy=1, e_auxiliary=2, beta_clone=1.0, num_aux_rollouts=2,
                       n_aux_grad_accum=1, aux_batch_rollouts=N, n_iteration=1, learning_rate=5e-4)
    optimizer = torch.optim.Adam(agent.parameters(), lr=args.learning_rate, eps=1e-8)
    init = _flat(agent.parameters()).clone()
    g = torch.Generator().manual_seed(59)
    frames = torch.randint(0, 256, (T + 1, N, 64, 64, 3), generator=g, dtype=torch.uint8)
    step_done = (torch.rand(T + 1, N, generator=g) < 0.2).float()
    step_done[0] = 0.0
    rewards = torch.rand(T, N, generator=g) * 2.0
    obs = torch.zeros((T, N, 64, 64, 3))
    actions, logprobs, dones, values = (torch.zeros((T, N)) for _ in range(4))
    torch.manual_seed(29)
    for step in range(T):
        obs[step], dones[step] = frames[step].float(), step_done[step]
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(obs[step])
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = frames[T].float(), step_done[T]
    device = torch.device("cpu")
    aux_obs = torch.zeros((T, N, 64, 64, 3), dtype=torch.uint8)
    aux_returns = torch.zeros((T, N))
    ns = dict(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs, rewards=rewards,
              dones=dones, values=values, next_obs=next_obs, next_done=next_done, device=device, np=np, torch=torch, nn=nn, td=td,
              Categorical=Categorical, flatten01=cls_ns["flatten01"], unflatten01=cls_ns["unflatten01"], aux_obs=aux_obs,
              aux_returns=aux_returns, update=1)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    np.random.seed(7)
    exec(textwrap.dedent("\n".join(lines[u0:u1])), ns)                  # policy phase update
    after_policy = _flat(agent.parameters()).clone()
    policy_loss = ns["loss"].detach().clone()                           # the auxiliary phase reuses the name `loss`
    s0 = R._find(lines, "# PPG Storage", u1) + 1
    exec(textwrap.dedent("\n".join(lines[s0:s0 + 3])), ns)
    a0 = R._find(lines, "# AUXILIARY PHASE", s0) + 1
    a1 = R._find(lines, 'writer.add_scalar("losses/aux/kl_loss"', a0)
    exec(textwrap.dedent("\n".join(lines[a0:a1])), ns)                  # auxiliary phase
    final = _flat(agent.parameters())
    sub = slice(0, None, 61)
    cases = {"ppg_T8_N4": dict(
        frames_u8=frames, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, values=values,
        returns=ns["returns"], b_advantages=ns["b_advantages"], init_params_sub=init[sub], policy_params_sub=after_policy[sub],
        final_params_sub=final[sub], stride=np.int64(61), final_checksum=np.float64(final.double().sum().item()),
        policy_loss=policy_loss, kl_loss=ns["kl_loss"].detach(), aux_value_loss=ns["aux_value_loss"].detach(),
        real_value_loss=ns["real_value_loss"].detach(), aux_pi=ns["aux_pi"], init_seed=np.int64(27), sample_seed=np.int64(29),
        shuffle_seed=np.int64(7), lr=np.float64(5e-4), lines=np.array([u0 + 1, u1, s0 + 1, a0 + 1, a1], np.int64))}
    _save("ppg_phase", cases)


# --------------------------------------------------------------- RND: two value streams, intrinsic reward, distillation loss
def mint_rnd_iteration():
    """One whole iteration of ppo_rnd_envpool.py on synthetic inputs (T=8, N=4): the reference Agent / RNDModel fill the
    rollout following :345-371, then its lines from the intrinsic-reward scaling through both GAE streams, the flatten,
    the observation-statistics update and the minibatch loop (:390-524) are executed verbatim (2 minibatches x 1 epoch).
    ``RunningMeanStd`` is gym 0.23.1's (pyproject.toml:17), which is not installed: the restatement in
    cleanrl_amd/learner_rnd.py of its published algorithm stands in; ``RewardForwardFilter`` is the reference's own class."""
    import ast
    import textwrap

    import torch.nn as nn
    import torch.nn.functional as F
    from torch.distributions.categorical import Categorical

    from cleanrl_amd.learner_rnd import RunningMeanStd

    script = "ppo_rnd_envpool.py"
    lines = R._read(script)
    tree = ast.parse("\n".join(lines))
    cls_ns = {"np": np, "torch": torch, "nn": nn, "Categorical": Categorical}
    want = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))
            and n.name in ("layer_init", "Agent", "RNDModel", "RewardForwardFilter")]
    exec(compile(ast.Module(body=want, type_ignores=[]), f"<reference:{script}>", "exec"), cls_ns)
    T, N, A = 8, 4, 6
    envs = R.fake_envs((4, 84, 84), n_actions=A)
    torch.manual_seed(13)
    agent = cls_ns["Agent"](envs)
    rnd_model = cls_ns["RNDModel"](4, A)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=2, update_epochs=1, batch_size=T * N, minibatch_size=T * N // 2,
                       gamma=0.999, int_gamma=0.99, clip_coef=0.1, ent_coef=0.001, update_proportion=0.25, int_coef=1.0,
                       ext_coef=2.0, learning_rate=1e-4)
    combined_parameters = list(agent.parameters()) + list(rnd_model.predictor.parameters())
    optimizer = torch.optim.Adam(combined_parameters, lr=args.learning_rate, eps=1e-5)
    init = _flat(combined_parameters).clone()
    g = torch.Generator().manual_seed(47)
    frames = torch.randint(0, 256, (T + 1, N, 4, 84, 84), generator=g, dtype=torch.uint8)
    step_done = (torch.rand(T + 1, N, generator=g) < 0.2).float()
    step_done[0] = 0.0
    rewards = torch.randint(-1, 2, (T, N), generator=g).float()
    reward_rms, obs_rms = RunningMeanStd(), RunningMeanStd(shape=(1, 1, 84, 84))
    obs_rms.update(torch.randint(0, 256, (64, 1, 84, 84), generator=g).double().numpy())       # stands for the init phase
    obs_mean0, obs_var0, obs_count0 = obs_rms.mean.copy(), obs_rms.var.copy(), obs_rms.count
    discounted_reward = cls_ns["RewardForwardFilter"](args.int_gamma)
    device = torch.device("cpu")
    obs = torch.zeros((T, N, 4, 84, 84))
    actions, logprobs, curiosity_rewards, dones, ext_values, int_values = (torch.zeros((T, N)) for _ in range(6))
    torch.manual_seed(17)                                      # the sampler's stream
    for step in range(T):                                       # :345-371 with the env replaced by the synthetic stream
        obs[step], dones[step] = frames[step].float(), step_done[step]
        with torch.no_grad():
            value_ext, value_int = agent.get_value(obs[step])
            ext_values[step], int_values[step] = value_ext.flatten(), value_int.flatten()
            action, logprob, _, _, _ = agent.get_action_and_value(obs[step])
        actions[step], logprobs[step] = action, logprob
        next_obs, next_done = frames[step + 1].float(), step_done[step + 1]
        rnd_next_obs = (((next_obs[:, 3, :, :].reshape(N, 1, 84, 84) - torch.from_numpy(obs_rms.mean).to(device))
                         / torch.sqrt(torch.from_numpy(obs_rms.var).to(device))).clip(-5, 5)).float()
        target_next_feature = rnd_model.target(rnd_next_obs)
        predict_next_feature = rnd_model.predictor(rnd_next_obs)
        curiosity_rewards[step] = ((target_next_feature - predict_next_feature).pow(2).sum(1) / 2).data
    raw_curiosity = curiosity_rewards.clone()
    ns = dict(args=args, agent=agent, rnd_model=rnd_model, optimizer=optimizer, combined_parameters=combined_parameters,
              envs=envs, obs=obs, actions=actions, logprobs=logprobs, rewards=rewards, curiosity_rewards=curiosity_rewards,
              dones=dones, ext_values=ext_values, int_values=int_values, next_obs=next_obs, next_done=next_done,
              reward_rms=reward_rms, obs_rms=obs_rms, discounted_reward=discounted_reward, device=device, np=np, torch=torch,
              nn=nn, F=F)
    u0 = R._find(lines, "curiosity_reward_per_env = np.array(")
    u1 = R._find(lines, "# TRY NOT TO MODIFY: record rewards for plotting purposes", u0)
    np.random.seed(5)
    torch.manual_seed(19)                                      # the distillation mask's stream (torch.rand, :472)
    exec(textwrap.dedent("\n".join(lines[u0:u1])), ns)          # :390-524
    final = _flat(combined_parameters)
    sub = slice(0, None, 211)
    cases = {"rnd_T8_N4": dict(
        frames_u8=frames, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, ext_values=ext_values,
        int_values=int_values, raw_curiosity=raw_curiosity, scaled_curiosity=ns["curiosity_rewards"],
        obs_mean0=obs_mean0, obs_var0=obs_var0, obs_count0=np.float64(obs_count0),
        obs_mean1=obs_rms.mean, obs_var1=obs_rms.var, reward_var=np.float64(reward_rms.var),
        ext_advantages=ns["ext_advantages"], int_advantages=ns["int_advantages"], ext_returns=ns["ext_returns"],
        int_returns=ns["int_returns"], b_advantages=ns["b_advantages"],
        init_params_sub=init[sub], final_params_sub=final[sub], stride=np.int64(211),
        init_checksum=np.float64(init.double().sum().item()), final_checksum=np.float64(final.double().sum().item()),
        last_loss=ns["loss"].detach(), last_pg_loss=ns["pg_loss"].detach(), last_v_loss=ns["v_loss"].detach(),
        last_entropy=ns["entropy_loss"].detach(), last_fwd_loss=ns["forward_loss"].detach(), last_approx_kl=ns["approx_kl"],
        init_seed=np.int64(13), sample_seed=np.int64(17), shuffle_seed=np.int64(5), mask_seed=np.int64(19), lr=np.float64(1e-4),
        n_actions=np.int64(A), lines=np.array([u0 + 1, u1], np.int64))}
    _save("rnd_iteration", cases)


def mint_ppo_iteration():
    """BASELINE configs[0]'s script (cleanrl/ppo.py, CartPole-shaped: obs 4, 2 actions, the MLP Agent), one whole iteration on
    synthetic inputs (T = 16, N = 4): the reference Agent fills the rollout (:122-126 through torch's Categorical, seeded), then
    the script's GAE lines and its flatten + epoch / minibatch update lines (4 minibatches x 4 epochs = sixteen Adam steps,
    the script's defaults: clip 0.2, ent 0.01) are exec'd verbatim.  Recorded as in ``mint_continuous_iteration``."""
    import textwrap

    import torch.nn as nn

    script = "ppo.py"
    lines = R._read(script)
    T, N, OBS, A = 16, 4, 4, 2
    torch.manual_seed(41)
    Agent, _ = R.load_agent_class(script)
    envs = R.fake_envs((OBS,), n_actions=A)
    agent = Agent(envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=4, update_epochs=4, batch_size=T * N, minibatch_size=T * N // 4,
                       clip_coef=0.2, ent_coef=0.01, learning_rate=2.5e-4)
    scalars = []
    keys = ("loss", "pg_loss", "v_loss", "entropy_loss", "old_approx_kl", "approx_kl")
    optimizer = _GradSpy(R.make_optimizer(agent, 2.5e-4), agent.parameters())
    init = _flat(agent.parameters()).clone()
    g = torch.Generator().manual_seed(59)
    obs_seq = torch.randn(T + 1, N, OBS, generator=g) * 0.5
    step_done = (torch.rand(T + 1, N, generator=g) < 0.15).float()
    step_done[0] = 0.0
    rewards = torch.ones(T, N)                                 # CartPole pays 1 per step
    obs = torch.zeros((T, N, OBS))
    actions, logprobs, dones, values = (torch.zeros((T, N)) for _ in range(4))
    torch.manual_seed(43)                                      # the sampler's stream
    for step in range(T):
        obs[step], dones[step] = obs_seq[step], step_done[step]
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(obs[step])
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = obs_seq[T], step_done[T]
    device = torch.device("cpu")
    ns = dict(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs,
              rewards=rewards, dones=dones, values=values, next_obs=next_obs, next_done=next_done, device=device, np=np,
              torch=torch, nn=nn)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    body = lines[u0:u1]
    k = max(i for i, ln in enumerate(body) if "optimizer.step()" in ln)
    indent = body[k][:len(body[k]) - len(body[k].lstrip())]
    body.insert(k + 1, indent + "_record(loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl)")
    ns["_record"] = lambda *v: scalars.append(torch.stack([x.detach().reshape(()) for x in v]))
    np.random.seed(10)
    exec(textwrap.dedent("\n".join(body)), ns)
    final = _flat(agent.parameters())
    assert len(scalars) == 16
    cases = {"cartpole_T16_N4": dict(
        obs_seq=obs_seq, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, values=values,
        advantages=ns["advantages"], returns=ns["returns"], init_params=init, final_params=final,
        scalars=torch.stack(scalars), scalar_names=np.array(keys), clipfracs=np.array(ns["clipfracs"], np.float32),
        init_seed=np.int64(41), sample_seed=np.int64(43), shuffle_seed=np.int64(10), lr=np.float64(2.5e-4),
        lines=np.array([g0 + 1, g1 + 1, u0 + 1, u1], np.int64),
        **_grad_record("mb1_grad", optimizer.grads[0], agent.parameters(), stride=1))}
    _save("ppo_iteration", cases)


def mint_continuous_iteration():
    """BASELINE configs[4]'s script, one whole iteration on synthetic inputs (T = 16, N = 4, obs 17 / act 6 = HalfCheetah's
    shapes): the reference Agent of ppo_continuous_action.py fills the rollout through its own ``get_action_and_value``
    (:134-141, torch's Normal sampler seeded), then the script's GAE lines (:232-246) and its flatten + epoch / minibatch
    update lines (:248-309; 2 minibatches x 3 epochs = six Adam steps; clip 0.2, ent 0.0, the script's defaults) are exec'd
    verbatim.  Recorded: the rollout, GAE outputs, every minibatch's loss scalars, the clipped gradient of the first step,
    ``actor_logstd`` after every step (the shared parameter the Normal loss twin / kernel sums its gradient for) and the
    parameters at the end."""
    import textwrap

    import torch.nn as nn

    script = "ppo_continuous_action.py"
    lines = R._read(script)
    T, N, OBS, ACT = 16, 4, 17, 6
    torch.manual_seed(31)
    Agent, _ = R.load_agent_class(script)
    envs = R.fake_envs((OBS,), action_shape=(ACT,))
    agent = Agent(envs)
    args = R.make_args(num_steps=T, num_envs=N, num_minibatches=2, update_epochs=3, batch_size=T * N, minibatch_size=T * N // 2,
                       clip_coef=0.2, ent_coef=0.0, learning_rate=3e-4)
    logstd_trace, scalars = [], []
    keys = ("loss", "pg_loss", "v_loss", "entropy_loss", "old_approx_kl", "approx_kl")

    optimizer = _GradSpy(R.make_optimizer(agent, 3e-4), agent.parameters())
    init = _flat(agent.parameters()).clone()
    g = torch.Generator().manual_seed(57)
    obs_seq = torch.randn(T + 1, N, OBS, generator=g)
    step_done = (torch.rand(T + 1, N, generator=g) < 0.15).float()
    step_done[0] = 0.0
    rewards = torch.randn(T, N, generator=g)
    obs = torch.zeros((T, N, OBS))
    actions = torch.zeros((T, N, ACT))
    logprobs, dones, values = (torch.zeros((T, N)) for _ in range(3))
    torch.manual_seed(37)                                      # the sampler's stream
    for step in range(T):
        obs[step], dones[step] = obs_seq[step], step_done[step]
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(obs[step])
            values[step] = value.flatten()
        actions[step], logprobs[step] = action, logprob
    next_obs, next_done = obs_seq[T], step_done[T]
    device = torch.device("cpu")
    ns = dict(args=args, agent=agent, optimizer=optimizer, envs=envs, obs=obs, actions=actions, logprobs=logprobs,
              rewards=rewards, dones=dones, values=values, next_obs=next_obs, next_done=next_done, device=device, np=np,
              torch=torch, nn=nn)
    g0 = R._find(lines, "# bootstrap value if not done") + 1
    g1 = R._find(lines, "returns = advantages + values", g0)
    exec(textwrap.dedent("\n".join(lines[g0:g1 + 1])), ns)
    u0 = R._find(lines, "# flatten the batch", g1) + 1
    u1 = R._find(lines, "y_pred, y_true = b_values.cpu().numpy()", u0)
    body = lines[u0:u1]
    # record every minibatch's scalars: one statement appended after `optimizer.step()` at its own indentation
    k = max(i for i, ln in enumerate(body) if "optimizer.step()" in ln)
    indent = body[k][:len(body[k]) - len(body[k].lstrip())]
    body.insert(k + 1, indent + "_record(loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl)")

    def _record(*v):                                           # runs right after `optimizer.step()` of every minibatch
        scalars.append(torch.stack([x.detach().reshape(()) for x in v]))
        logstd_trace.append(agent.actor_logstd.detach().clone().reshape(-1))

    ns["_record"] = _record
    np.random.seed(9)
    exec(textwrap.dedent("\n".join(body)), ns)
    final = _flat(agent.parameters())
    assert len(scalars) == 6 and len(logstd_trace) == 6
    cases = {"mujoco_T16_N4": dict(
        obs_seq=obs_seq, step_done=step_done, rewards=rewards, actions=actions, logprobs=logprobs, values=values,
        advantages=ns["advantages"], returns=ns["returns"], init_params=init, final_params=final,
        scalars=torch.stack(scalars), scalar_names=np.array(keys), logstd_after_step=torch.stack(logstd_trace),
        clipfracs=np.array(ns["clipfracs"], np.float32), init_seed=np.int64(31), sample_seed=np.int64(37), shuffle_seed=np.int64(9),
        lr=np.float64(3e-4), lines=np.array([g0 + 1, g1 + 1, u0 + 1, u1], np.int64),
        **_grad_record("mb1_grad", optimizer.grads[0], agent.parameters(), stride=1))}
    _save("continuous_iteration", cases)


CLI_SCRIPTS = ["ppo", "ppo_atari", "ppo_atari_envpool", "ppo_atari_multigpu", "ppo_continuous_action", "ppo_atari_lstm", "ppo_procgen",
               "ppo_rnd_envpool", "ppg_procgen"]


def mint_cli_surface():
    """tests/golden/cli_surface.json: the reference's command-line surface as data -- every field of each script's ``Args`` with its
    default (``exp_name`` left out), and every ``parser.add_argument`` of ppo_pettingzoo_ma_atari.py with its default (``exp_name``:
    computed from the file name, left out).  tests/test_cli_scripts.py and tests/test_ma_atari_script.py check against it."""
    import ast
    import json

    args = {}
    for script in CLI_SCRIPTS:
        tree = ast.parse("\n".join(R._read(script + ".py")))
        (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args"]
        ref = {}
        for b in cls.body:
            if isinstance(b, ast.AnnAssign) and b.target.id != "exp_name":
                try:
                    ref[b.target.id] = ast.literal_eval(b.value)
                except ValueError:
                    v = b.value
                    if isinstance(v, ast.Call) and getattr(v.func, "id", "") == "int" and len(v.args) == 1:
                        ref[b.target.id] = int(ast.literal_eval(v.args[0]))      # `int(25e6)` (ppo_procgen.py)
                    else:
                        ref[b.target.id] = []          # field(default_factory=lambda: [])
        args[script] = ref
    argparse_defaults = {}
    for node in ast.walk(ast.parse("\n".join(R._read("ppo_pettingzoo_ma_atari.py")))):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            flag = ast.literal_eval(node.args[0])
            default = [k.value for k in node.keywords if k.arg == "default"][0]
            try:
                argparse_defaults[flag.lstrip("-").replace("-", "_")] = ast.literal_eval(default)
            except ValueError:
                pass                                                   # exp_name: os.path.basename(__file__).rstrip(".py")
    path = os.path.join(OUT, "cli_surface.json")
    with open(path, "w") as fh:
        json.dump({"args": args, "ppo_pettingzoo_ma_atari_argparse": argparse_defaults}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"cli_surface: {len(args)} Args classes, {len(argparse_defaults)} argparse flags")


def main():
    assert R.available(), "needs /root/reference (build container only)"
    os.makedirs(OUT, exist_ok=True)
    if len(sys.argv) > 1:                     # python -m oracle.mint_goldens atari_iteration_config_b ...: only these
        for name in sys.argv[1:]:
            globals()["mint_" + name]()
        return
    for script in ["ppo.py", "ppo_atari.py", "ppo_atari_envpool.py", "ppo_atari_multigpu.py", "ppo_continuous_action.py", "ppo_procgen.py"]:
        print(script, R.line_ranges(script))
    mint_gae()
    mint_categorical()
    mint_normal()
    mint_loss_categorical()
    mint_loss_normal()
    mint_update_step()
    mint_atari_iteration()
    mint_atari_iteration_config_b()
    mint_lstm_iteration()
    mint_procgen_update()
    mint_rnd_iteration()
    mint_ppg_phase()
    mint_ma_atari_update()
    mint_continuous_iteration()
    mint_ppo_iteration()
    mint_cli_surface()


if __name__ == "__main__":
    main()
