"""The Random-Network-Distillation PPO learner of ``ppo_rnd_envpool.py`` on the storage, kernels and update machinery of
``PPOLearner``.

What RND adds to the feed-forward path (reference: cleanrl/ppo_rnd_envpool.py):

====================================  ==========================================================
reference                              here
====================================  ==========================================================
:301-303  reward / observation stats   ``reward_rms``, ``obs_rms`` (``RunningMeanStd``), ``discounted_reward``
:310-314  second value stream          ``int_values``, ``curiosity_rewards`` (+ ``int_advantages`` / ``int_returns``)
:347-355  action logic, two values     ``act``                (K5 convert, network, K2 sample kernel)
:363-371  intrinsic reward             ``curiosity``          (normalised newest frame -> target / predictor nets)
:390-400  intrinsic-reward scaling     ``finish_rollout``     (forward filter per env, running variance; host numpy)
:402-432  TWO GAE streams              ``finish_rollout``     (K1 twice: extrinsic with the dones at gamma, intrinsic
                                                               non-episodic -- all-zero dones -- at int_gamma)
:444      combined advantage           ``update``             ``int_coef * A_int + ext_coef * A_ext``
:446,451  observation statistics       ``update``
:461-521  minibatch update             ``_minibatch_*``       (K5 gather, network forward, K3 fused loss on the combined
                                                               advantage and the clipped EXTRINSIC value; the unclipped
                                                               intrinsic value loss and the masked distillation loss are
                                                               two small torch terms; autograd; fused clip + Adam over
                                                               agent + predictor parameters in one flat buffer)
====================================  ==========================================================

``MI355PPO_RND=fused`` (HIP learner only; the default ``torch`` is the table above) moves what surrounds the two RND networks onto
the kernels of csrc/rnd.hip: ``curiosity`` = normalise kernel + networks + intrinsic-reward kernel with device copies
of the observation statistics; ``finish_rollout`` = one reward-filter launch on a device (mean, var, count) triple, no host round
trip; ``update`` = exact integer observation moments of the u8 batch (one 113 KB read-back), the RND input of each minibatch
normalised straight from the u8 rollout rows, and one loss kernel for the distillation and intrinsic-value terms.

``MI355PPO_RND_TRUNK=fused`` (with ``MI355PPO_RND=fused`` only; default ``torch``) moves the three NatureCNN stacks of a
minibatch onto the library as well: the agent's trunk through ``RNDAgent.heads3_u8``, the predictor's and the target's one-frame
LeakyReLU stacks through ``leaky_cnn.LeakyNatureTrunk`` -- all three read the u8 rollout rows, so neither the K5 conversion nor the
``rnd_normalize`` launch runs and no f32 frame tensor is allocated.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

from . import host_ops
from .learner import PPOLearner
from .rnd_ops import RND_PIXELS, rnd_mean_var


class RunningMeanStd:
    """``gym.wrappers.normalize.RunningMeanStd`` of gym 0.23.1 (the reference's pin, pyproject.toml:17; imported at
    ppo_rnd_envpool.py:16; not installed in this image): running mean / variance with Chan et al.'s parallel update."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, "float64")
        self.var = np.ones(shape, "float64")
        self.count = epsilon

    def update(self, x):
        self.update_from_moments(np.mean(x, axis=0), np.var(x, axis=0), x.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        tot_count = self.count + batch_count
        new_mean = self.mean + delta * batch_count / tot_count
        m2 = self.var * self.count + batch_var * batch_count + np.square(delta) * self.count * batch_count / tot_count
        self.mean, self.var, self.count = new_mean, m2 / tot_count, tot_count


class RewardForwardFilter:
    """ppo_rnd_envpool.py:236-246."""

    def __init__(self, gamma):
        self.rewems = None
        self.gamma = gamma

    def update(self, rews):
        if self.rewems is None:
            self.rewems = rews
        else:
            self.rewems = self.rewems * self.gamma + rews
        return self.rewems


def rnd_backend() -> str:
    """``MI355PPO_RND``: ``torch`` (the default) or ``fused`` (csrc/rnd.hip, HIP learner only); read when a learner is built."""
    v = os.environ.get("MI355PPO_RND", "torch").strip().lower() or "torch"
    if v not in ("torch", "fused"):
        raise ValueError(f"MI355PPO_RND={v!r}: expected 'torch' or 'fused'")
    return v


def rnd_trunk_backend() -> str:
    """``MI355PPO_RND_TRUNK``: ``torch`` (the default) or ``fused`` -- the three NatureCNN stacks of a minibatch straight from the u8
    rollout rows: the agent's trunk on the kernels of cleanrl_amd/cnn.py (``RNDAgent.heads3_u8``), the predictor's and the target's
    one-frame LeakyReLU stacks on cleanrl_amd/leaky_cnn.py (csrc/rnd_conv1.hip, csrc/leaky.hip).  HIP learner with
    ``MI355PPO_RND=fused`` only; read when a learner is built."""
    v = os.environ.get("MI355PPO_RND_TRUNK", "torch").strip().lower() or "torch"
    if v not in ("torch", "fused"):
        raise ValueError(f"MI355PPO_RND_TRUNK={v!r}: expected 'torch' or 'fused'")
    return v


class DeviceRunningMeanStd:
    """``reward_rms`` of the fused backend: the (mean, var, count) float64 triple lives on the device, where the reward-filter
    kernel updates it.  Reading an attribute synchronises (only then); assigning one writes the device triple."""

    def __init__(self, device, epsilon=1e-4):
        self.stats = torch.tensor([0.0, 1.0, epsilon], dtype=torch.float64, device=device)

    @property
    def mean(self):
        return float(self.stats[0].item())

    @mean.setter
    def mean(self, value):
        self.stats[0].fill_(float(value))

    @property
    def var(self):
        return float(self.stats[1].item())

    @var.setter
    def var(self, value):
        self.stats[1].fill_(float(value))

    @property
    def count(self):
        return float(self.stats[2].item())

    @count.setter
    def count(self, value):
        self.stats[2].fill_(float(value))


class _Combined(nn.Module):
    """agent parameters followed by the predictor's: the order of ``combined_parameters`` (:295)."""

    def __init__(self, agent, predictor):
        super().__init__()
        self.agent, self.predictor = agent, predictor


class RNDPPOLearner(PPOLearner):
    def __init__(self, agent, rnd_model, args, obs_space, act_space, num_envs, device, world_size: int = 1,
                 sample_seed: int = 0):
        super().__init__(agent, args, obs_space, act_space, num_envs, device, world_size=world_size, sample_seed=sample_seed)
        assert self.image and tuple(obs_space.shape) == (4, 84, 84), "RND reads the newest of 4 stacked 84x84 frames"
        self.rnd_model = rnd_model
        self.combined_parameters = list(agent.parameters()) + list(rnd_model.predictor.parameters())     # :295
        if self.hip:
            from .flat import FlatParams

            self.flat = FlatParams(_Combined(agent, rnd_model.predictor))    # one flat buffer for the fused clip + Adam
            n_upd = self._scalars.shape[0]
            self._extra = torch.zeros((n_upd, 2), device=device)             # intrinsic value loss, distillation loss
            self._zeros_TN = torch.zeros((self.T, self.N), device=device)
            self._zeros_N = torch.zeros(self.N, device=device)
        else:
            self.optimizer = optim.Adam(self.combined_parameters, lr=args.learning_rate, eps=1e-5)        # :296-300
        T, N = self.T, self.N
        self.int_values = torch.zeros((T, N), device=device)
        self.curiosity_rewards = torch.zeros((T, N), device=device)
        self.int_advantages = torch.zeros((T, N), device=device)
        self.int_returns = torch.zeros((T, N), device=device)
        self.reward_rms = RunningMeanStd()
        self.obs_rms = RunningMeanStd(shape=(1, 1, 84, 84))
        self.discounted_reward = RewardForwardFilter(args.int_gamma)
        self.last_fwd_loss = float("nan")
        self.rnd_fused = False
        if self.hip and rnd_backend() == "fused":
            self.init_rnd_fused()
        self.rnd_trunk_fused = False
        self.select_rnd_trunk()

    def select_rnd_trunk(self) -> None:
        """``MI355PPO_RND_TRUNK`` on the HIP learner (the host learner ignores it, as it ignores ``MI355PPO_RND``)."""
        if self.hip and rnd_trunk_backend() == "fused":
            if not self.rnd_fused:
                raise ValueError("MI355PPO_RND_TRUNK=fused needs MI355PPO_RND=fused: it reads the u8 NHWC rollout rows and the device "
                                 "copies of the observation statistics that backend keeps")
            self.init_rnd_trunk_fused()

    def init_rnd_trunk_fused(self) -> None:
        """The state of ``MI355PPO_RND_TRUNK=fused``: the agent's ``cnn.NatureTrunk`` and the predictor's / target's
        ``leaky_cnn.LeakyNatureTrunk``, each with cached weight packs.  ``optimizer_step_hip`` bumps the ``weights_version`` of the two
        trained ones after every step, which writes the parameters through raw pointers; the target's packs are derived once."""
        assert self.rnd_fused and self.nhwc, "MI355PPO_RND_TRUNK=fused runs on the u8 NHWC rollout rows of MI355PPO_RND=fused"
        from .leaky_cnn import LeakyNatureTrunk

        self.agent._nature_trunk().bufs.cache_weights = True
        self._rnd_pred = LeakyNatureTrunk(self.rnd_model.predictor, head=True)
        self._rnd_pred_tail = self.rnd_model.predictor[9:]              # Linear, ReLU, Linear: torch modules on the node's (M, 512)
        self._rnd_targ = LeakyNatureTrunk(self.rnd_model.target, head=False)
        self._rnd_x_step = None                                         # no normalised f32 frames under the switch
        self.rnd_trunk_fused = True

    def _rnd_features(self, rows, idx=None):
        """(predictor, target) features of the newest frame of ``rows[idx]``, from the u8 rows (``MI355PPO_RND_TRUNK=fused``)."""
        predict = self._rnd_pred_tail(self._rnd_pred(rows, idx, self._rnd_mean, self._rnd_sd))
        return predict, self._rnd_targ(rows, idx, self._rnd_mean, self._rnd_sd)

    def optimizer_step_hip(self, lr: float) -> None:
        super().optimizer_step_hip(lr)
        if self.rnd_trunk_fused:                    # the kernel rewrote the predictor's parameters through raw pointers too
            self._rnd_pred.bufs.weights_version += 1

    def _heads3_rows(self, rows, idx=None):
        """``agent.heads3`` of the u8 rollout rows ``rows[idx]``: the trunk kernels under ``MI355PPO_RND_TRUNK=fused``, else K5 + torch."""
        if self.rnd_trunk_fused:
            return self.agent.heads3_u8(rows, idx)
        if idx is None:
            return self.agent.heads3(self._features(rows))
        if self._x_mb is None or self._x_mb.shape[0] != idx.numel():
            self._x_mb = torch.empty((idx.numel(),) + self.obs_shape, device=self.device)
        return self.agent.heads3(self.ops.obs_u8_to_f32(rows, idx, self._x_mb).permute(0, 3, 1, 2))

    def init_rnd_fused(self) -> None:
        """The state of ``MI355PPO_RND=fused``: device copies of the observation statistics, the filter state and the reward
        statistics on the device (``discounted_reward`` is not used), the buffers the kernels write."""
        assert self.hip and self.nhwc, "MI355PPO_RND=fused runs on the HIP learner's u8 NHWC rollout storage"
        dev, P = self.device, RND_PIXELS
        self.rnd_fused = True
        self._rnd_mean = torch.zeros(P, dtype=torch.float64, device=dev)
        self._rnd_sd = torch.ones(P, dtype=torch.float64, device=dev)
        self._rnd_sums = torch.zeros((2, P), dtype=torch.int64, device=dev)
        self._rnd_rewems = torch.zeros(self.T, device=dev)              # all zero == the reference's "first call returns rews"
        self._rnd_x_step = torch.empty((self.N, 1, 84, 84), device=dev)
        self._rnd_x_mb = None
        self.reward_rms = DeviceRunningMeanStd(dev)
        self.refresh_obs_stats()

    def refresh_obs_stats(self) -> None:
        """Upload ``obs_rms.mean`` and ``sqrt(obs_rms.var)`` (float64, formed once here) to the device copies the normalise kernel
        reads.  Runs by itself at the first ``curiosity`` of a rollout and in ``update``; call it after overwriting ``obs_rms``
        anywhere else."""
        self._rnd_mean.copy_(torch.from_numpy(np.ascontiguousarray(self.obs_rms.mean, dtype=np.float64).reshape(-1)))
        self._rnd_sd.copy_(torch.from_numpy(np.sqrt(np.asarray(self.obs_rms.var, dtype=np.float64)).reshape(-1)))

    # ------------------------------------------------------------------ rollout
    def _newest_frame(self, rows):
        """The last of the 4 stacked frames of observation rows, as (B, 1, 84, 84) f32 (0..255): ``x[:, 3, :, :]``."""
        if self.nhwc:
            return rows[..., 3].reshape(-1, 1, 84, 84).float()
        return rows[:, 3, :, :].reshape(-1, 1, 84, 84).float()

    def _rnd_input(self, rows):
        """:363-368 / :453-458: ((newest frame - obs_rms.mean) / sqrt(obs_rms.var)).clip(-5, 5).float()"""
        mean = torch.from_numpy(self.obs_rms.mean).to(self.device)
        var = torch.from_numpy(self.obs_rms.var).to(self.device)
        return ((self._newest_frame(rows) - mean) / torch.sqrt(var)).clip(-5, 5).float()

    @torch.no_grad()
    def act(self, step: int):
        if self.hip:
            logits, v_ext, v_int = self._heads3_rows(self.obs[step])
            seed, off = self.agent.rng.next()
            a64, _, _, _ = self.ops.categorical_sample(logits.contiguous(), seed=seed, offset=off,
                                                       action_f32_out=self.actions[step], logprob_out=self.logprobs[step],
                                                       want_entropy=False)
            self.values[step].copy_(v_ext.view(-1))
            self.int_values[step].copy_(v_int.view(-1))
            return a64
        value_ext, value_int = self.agent.get_value(self.obs[step])                       # :348-352
        self.values[step], self.int_values[step] = value_ext.flatten(), value_int.flatten()
        action, logprob, _, _, _ = self.agent.get_action_and_value(self.obs[step])         # :353
        self.actions[step] = action
        self.logprobs[step] = logprob
        return action

    @torch.no_grad()
    def curiosity(self, step: int):
        """Intrinsic reward of the transition into the observation stored in slot ``step + 1`` (:363-371)."""
        rows, _ = self._slot(step + 1)
        if self.rnd_fused:
            if step == 0:
                self.refresh_obs_stats()
            if self.rnd_trunk_fused:
                predict, target = self._rnd_features(rows)
                self.ops.rnd_intrinsic_reward(target.contiguous(), predict.contiguous(), out=self.curiosity_rewards[step])
                return self.curiosity_rewards[step]
            x = self.ops.rnd_normalize(rows, self._rnd_mean, self._rnd_sd, out=self._rnd_x_step)
            self.ops.rnd_intrinsic_reward(self.rnd_model.target(x).contiguous(), self.rnd_model.predictor(x).contiguous(),
                                          out=self.curiosity_rewards[step])
            return self.curiosity_rewards[step]
        rnd_next_obs = self._rnd_input(rows)
        target_next_feature = self.rnd_model.target(rnd_next_obs)
        predict_next_feature = self.rnd_model.predictor(rnd_next_obs)
        self.curiosity_rewards[step] = (target_next_feature - predict_next_feature).pow(2).sum(1) / 2
        return self.curiosity_rewards[step]

    @torch.no_grad()
    def finish_rollout(self) -> None:
        a = self.args
        if self.rnd_fused:  # :390-400 in one launch: filter along the env axis, running variance, division -- nothing leaves the device
            self.ops.rnd_reward_filter_(self.curiosity_rewards, self._rnd_rewems, self.reward_rms.stats, a.int_gamma)
        else:
            # :390-400 intrinsic-reward scaling -- (T, N) floats through the host, as the reference
            curiosity_reward_per_env = np.array(
                [self.discounted_reward.update(reward_per_step) for reward_per_step in self.curiosity_rewards.cpu().data.numpy().T])
            mean, std, count = (np.mean(curiosity_reward_per_env), np.std(curiosity_reward_per_env), len(curiosity_reward_per_env))
            self.reward_rms.update_from_moments(mean, std**2, count)
            self.curiosity_rewards /= np.sqrt(self.reward_rms.var)
        if self.hip:
            _, v_ext, v_int = self._heads3_rows(self.boot_obs)
            self.ops.gae(self.rewards, self.dones, self.values, self.boot_done, v_ext.reshape(-1).contiguous(),
                         a.gamma, a.gae_lambda, self.advantages, self.returns)
            # the intrinsic stream is non-episodic (int_nextnonterminal = 1.0, :413,418): K1 with all-zero dones
            self.ops.gae(self.curiosity_rewards, self._zeros_TN, self.int_values, self._zeros_N,
                         v_int.reshape(-1).contiguous(), a.int_gamma, a.gae_lambda, self.int_advantages, self.int_returns)
        else:
            next_value_ext, next_value_int = self.agent.get_value(self.boot_obs)
            adv, ret = host_ops.gae(self.rewards, self.dones, self.values, self.boot_done, next_value_ext.reshape(1, -1),
                                    a.gamma, a.gae_lambda)
            self.advantages.copy_(adv)
            self.returns.copy_(ret)
            zeros = torch.zeros_like(self.dones)
            adv, ret = host_ops.gae(self.curiosity_rewards, zeros, self.int_values, torch.zeros_like(self.boot_done),
                                    next_value_int.reshape(1, -1), a.int_gamma, a.gae_lambda)
            self.int_advantages.copy_(adv)
            self.int_returns.copy_(ret)

    # ------------------------------------------------------------------ update
    def update(self, lr: float) -> dict:
        a = self.args
        B, M = self.batch_size, self.minibatch_size
        b_inds = np.arange(B)
        b_obs = self.obs.reshape((-1,) + self.obs_shape)
        b_actions = self.actions.reshape(-1)
        b_logprobs = self.logprobs.reshape(-1)
        b_ext_returns, b_int_returns = self.returns.reshape(-1), self.int_returns.reshape(-1)
        b_ext_values = self.values.reshape(-1)
        b_advantages = self.int_advantages.reshape(-1) * a.int_coef + self.advantages.reshape(-1) * a.ext_coef     # :444
        if self.rnd_fused:  # :446 from exact integer moments of the u8 rows; :453-458 per minibatch, straight from the rollout rows
            mean, var = rnd_mean_var(self.ops.rnd_obs_moments(b_obs, self._rnd_sums), B)
            self.obs_rms.update_from_moments(mean.reshape(1, 1, 84, 84), var.reshape(1, 1, 84, 84), B)
            self.refresh_obs_stats()
            rnd_next_obs = None
        else:
            newest = self._newest_frame(b_obs)
            if self.hip:        # statistics of np.mean / np.var over the batch axis, on the device in f64
                d = newest.double()
                self.obs_rms.update_from_moments(d.mean(0).cpu().numpy(), d.var(0, unbiased=False).cpu().numpy(), d.shape[0])
                del d
            else:
                self.obs_rms.update(newest.cpu().numpy())                                                          # :446
            mean = torch.from_numpy(self.obs_rms.mean).to(self.device)
            var = torch.from_numpy(self.obs_rms.var).to(self.device)
            rnd_next_obs = ((newest - mean) / torch.sqrt(var)).clip(-5, 5).float()                                   # :453-458
            del newest
        k = 0
        clipfracs = []
        last = None
        for epoch in range(int(a.update_epochs)):
            np.random.shuffle(b_inds)
            if self.hip:
                inds_dev = self.upload_permutation(epoch, b_inds)
            for start in range(0, B, M):
                end = start + M
                if self.hip:
                    self._minibatch_rnd_hip(inds_dev[start:end], b_obs, rnd_next_obs, b_actions, b_logprobs, b_advantages,
                                            b_ext_returns, b_int_returns, b_ext_values, lr, k)
                else:
                    last = self._minibatch_rnd_host(b_inds[start:end], b_obs, rnd_next_obs, b_actions, b_logprobs, b_advantages,
                                                    b_ext_returns, b_int_returns, b_ext_values, lr)
                    clipfracs.append(last[6].item())
                k += 1
            if a.target_kl is not None:
                approx_kl = (self._scalars[k - 1, 5] if self.hip else last[5]).item()
                if approx_kl > a.target_kl:
                    break
        if self.hip:
            sc, ex = self._scalars[:k].cpu().numpy(), self._extra[:k].cpu().numpy()
            last_np, clipfrac = sc[-1].copy(), float(np.mean(sc[:, 6]))
            int_v, fwd = float(ex[-1, 0]), float(ex[-1, 1])
            last_np[2] += int_v                                            # v_loss = ext_v_loss + int_v_loss (:513)
            last_np[0] += int_v * a.vf_coef + fwd                          # the K3 scalar holds the terms it computed
        else:
            last_np, clipfrac, fwd = last.numpy(), float(np.mean(clipfracs)), float(last[7])
        self.last_fwd_loss = fwd
        return dict(loss=float(last_np[0]), policy_loss=float(last_np[1]), value_loss=float(last_np[2]),
                    entropy=float(last_np[3]), old_approx_kl=float(last_np[4]), approx_kl=float(last_np[5]),
                    clipfrac=clipfrac, fwd_loss=fwd, num_updates=k)

    def _forward_loss(self, rnd_rows):
        """:467-476: per-sample distillation error, averaged over a random ``update_proportion`` of the minibatch."""
        predict_next_state_feature, target_next_state_feature = self.rnd_model(rnd_rows)
        forward_loss = F.mse_loss(predict_next_state_feature, target_next_state_feature.detach(), reduction="none").mean(-1)
        mask = torch.rand(len(forward_loss), device=self.device)
        mask = (mask < self.args.update_proportion).type(torch.FloatTensor).to(self.device)
        return (forward_loss * mask).sum() / torch.max(mask.sum(), torch.tensor([1], device=self.device, dtype=torch.float32))

    def _minibatch_rnd_hip(self, idx, b_obs, rnd_next_obs, b_actions, b_logprobs, b_advantages, b_ext_returns, b_int_returns,
                           b_ext_values, lr, k):
        a, ops = self.args, self.ops
        if self.rnd_fused:
            return self._minibatch_rnd_fused(idx, b_obs, b_actions, b_logprobs, b_advantages, b_ext_returns, b_int_returns, b_ext_values,
                                             lr, k)
        forward_loss = self._forward_loss(rnd_next_obs.index_select(0, idx))
        if self._x_mb is None or self._x_mb.shape[0] != idx.numel():
            self._x_mb = torch.empty((idx.numel(),) + self.obs_shape, device=self.device)
        x = ops.obs_u8_to_f32(b_obs, idx, self._x_mb).permute(0, 3, 1, 2)               # K5: b_obs[mb_inds] ; x / 255.0
        logits, v_ext, v_int = self.agent.heads3(x)
        v_ext, v_int = v_ext.view(-1), v_int.view(-1)
        # K3 on the combined advantage and the (clipped) extrinsic value: pg_loss - ent_coef*entropy + vf_coef*ext_v_loss
        _, dlogits, dv_ext = ops.ppo_loss_categorical(logits.detach().contiguous(), v_ext.detach().contiguous(), idx, b_actions,
                                                      b_logprobs, b_advantages, b_ext_returns, b_ext_values, a.clip_coef,
                                                      a.ent_coef, a.vf_coef, a.norm_adv, a.clip_vloss,
                                                      scalars_out=self._scalars[k])
        int_v_loss = 0.5 * ((v_int - b_int_returns.index_select(0, idx)) ** 2).mean()                         # :512
        self._extra[k, 0], self._extra[k, 1] = int_v_loss.detach(), forward_loss.detach().view(())
        rest = int_v_loss * a.vf_coef + forward_loss.view(())
        torch.autograd.backward([logits, v_ext, rest], [dlogits, dv_ext, None])                               # :518
        if self.world_size > 1:
            dist.all_reduce(self.flat.grads, op=dist.ReduceOp.SUM)
        self.optimizer_step_hip(lr)                                                                           # :519-524

    def _minibatch_rnd_fused(self, idx, b_obs, b_actions, b_logprobs, b_advantages, b_ext_returns, b_int_returns, b_ext_values, lr, k):
        """``_minibatch_rnd_hip`` with the RND input normalised from the u8 rows and the two extra loss terms in one kernel."""
        a, ops = self.args, self.ops
        M = idx.numel()
        if self.rnd_trunk_fused:
            predict, target = self._rnd_features(b_obs, idx)                                                  # :453-458, :463 from the u8 rows
        else:
            if self._rnd_x_mb is None or self._rnd_x_mb.shape[0] != M:
                self._rnd_x_mb = torch.empty((M, 1, 84, 84), device=self.device)
            predict, target = self.rnd_model(ops.rnd_normalize(b_obs, self._rnd_mean, self._rnd_sd, idx=idx, out=self._rnd_x_mb))   # :453-458, :463
        u = torch.rand(M, device=self.device)                                                                 # :467
        logits, v_ext, v_int = self._heads3_rows(b_obs, idx)               # K5 gather + torch, or the trunk kernels on the u8 rows
        v_ext, v_int = v_ext.view(-1), v_int.view(-1)
        _, dlogits, dv_ext = ops.ppo_loss_categorical(logits.detach().contiguous(), v_ext.detach().contiguous(), idx, b_actions,
                                                      b_logprobs, b_advantages, b_ext_returns, b_ext_values, a.clip_coef,
                                                      a.ent_coef, a.vf_coef, a.norm_adv, a.clip_vloss,
                                                      scalars_out=self._scalars[k])
        _, d_predict, d_v_int = ops.rnd_loss_fwd_bwd(predict.detach().contiguous(), target.detach().contiguous(), u, a.update_proportion,
                                                     v_int.detach().contiguous(), b_int_returns, idx, a.vf_coef, scalars=self._extra[k])
        torch.autograd.backward([logits, v_ext, v_int, predict], [dlogits, dv_ext, d_v_int, d_predict])       # :518
        if self.world_size > 1:
            dist.all_reduce(self.flat.grads, op=dist.ReduceOp.SUM)
        self.optimizer_step_hip(lr)                                                                           # :519-524

    def _minibatch_rnd_host(self, mb_inds, b_obs, rnd_next_obs, b_actions, b_logprobs, b_advantages, b_ext_returns,
                            b_int_returns, b_ext_values, lr):
        """The reference's minibatch body on CPU tensors (:461-524).  Returns the 7 scalars of K3's host-pointer twin with
        ``v_loss = ext + int`` and ``loss`` including the distillation term, followed by the distillation loss."""
        a = self.args
        self.optimizer.param_groups[0]["lr"] = lr
        forward_loss = self._forward_loss(rnd_next_obs[mb_inds])
        # the network's three outputs (get_action_and_value's forward, :478-480), then K3 through the C ABI's host-pointer twin on
        # the combined advantage and the (clipped) extrinsic value -- the seam the HIP branch crosses (_minibatch_rnd_hip); the
        # intrinsic value loss and the distillation term are added outside
        logits, new_ext_values, new_int_values = self.agent.heads3(self.agent._normalise(b_obs[mb_inds]))
        ext_loss, sc = host_ops.ppo_loss_categorical(logits, new_ext_values, torch.as_tensor(mb_inds, dtype=torch.int64), b_actions,
                                                     b_logprobs, b_advantages, b_ext_returns, b_ext_values, a.clip_coef, a.ent_coef,
                                                     a.vf_coef, a.norm_adv, a.clip_vloss)
        int_v_loss = 0.5 * ((new_int_values.view(-1) - b_int_returns[mb_inds]) ** 2).mean()
        loss = ext_loss + int_v_loss * a.vf_coef + forward_loss.view(())
        self.optimizer.zero_grad()
        loss.backward()
        if a.max_grad_norm:
            nn.utils.clip_grad_norm_(self.combined_parameters, a.max_grad_norm)
        self.optimizer.step()
        sc = sc.clone()
        sc[0], sc[2] = loss.detach(), sc[2] + int_v_loss.detach()
        return torch.cat([sc, forward_loss.detach().view(1)])
