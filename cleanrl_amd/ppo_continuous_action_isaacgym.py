"""Drop-in for ``cleanrl/ppo_continuous_action_isaacgym/ppo_continuous_action_isaacgym.py`` (thousands of device-resident
environments, two 256-256 tanh networks, Normal policy).

    MI355PPO_MLP256=fused python cleanrl_amd/ppo_continuous_action_isaacgym.py --env-id Ant --seed 1

``isaacgymenvs`` does not exist on ROCm; where it imports it is used as the reference uses it, otherwise an Ant-shaped
(obs 60, act 8) stand-in task is stepped on the device (``envs.DeviceLinearContinuousVecEnv``; with ``--no-cuda`` the host task
``envs.SyntheticContinuousVecEnv``).  With ``MI355PPO_MLP256=fused`` both networks run on the K8 kernels (csrc/mlp256.hip): rollout step, bootstrap value and
the minibatch forward / backward; the default ``torch`` keeps them on library GEMMs behind the HIP sampling / loss kernels.
The epoch permutation is ``torch.randperm`` on the device, as the reference's (:331).
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import IsaacGymAgent as Agent  # noqa: E402
from cleanrl_amd.learner import PPOLearner  # noqa: E402


@dataclass
class Args:
    exp_name: str = os.path.basename(__file__)[: -len(".py")]
    """the name of this experiment"""
    seed: int = 1
    """seed of the experiment"""
    torch_deterministic: bool = True
    """sets `torch.backends.cudnn.deterministic`"""
    cuda: bool = True
    """use the GPU (HIP kernels) when one is present; `--no-cuda` selects the CPU host path"""
    track: bool = False
    """track the run with Weights and Biases (needs the `wandb` package)"""
    wandb_project_name: str = "cleanRL"
    """W&B project"""
    wandb_entity: str = None
    """W&B entity (team)"""
    capture_video: bool = False
    """record videos of the agent (needs isaacgymenvs)"""

    # Algorithm specific arguments
    env_id: str = "Ant"
    """the id of the environment"""
    total_timesteps: int = 30000000
    """total timesteps of the experiment"""
    learning_rate: float = 0.0026
    """Adam learning rate"""
    num_envs: int = 4096
    """number of parallel environments"""
    num_steps: int = 16
    """steps per environment per rollout"""
    anneal_lr: bool = False
    """linearly anneal the learning rate to 0 over the run"""
    gamma: float = 0.99
    """discount factor"""
    gae_lambda: float = 0.95
    """lambda of generalised advantage estimation"""
    num_minibatches: int = 2
    """minibatches per epoch"""
    update_epochs: int = 4
    """epochs over the rollout per policy update"""
    norm_adv: bool = True
    """normalise advantages per minibatch"""
    clip_coef: float = 0.2
    """surrogate clipping coefficient"""
    clip_vloss: bool = False
    """clip the value loss as in the PPO paper's implementation"""
    ent_coef: float = 0.0
    """entropy bonus coefficient"""
    vf_coef: float = 2
    """value-loss coefficient"""
    max_grad_norm: float = 1
    """global gradient-norm clip"""
    target_kl: float = None
    """stop the epoch loop early when approx_kl exceeds this"""
    reward_scaler: float = 1
    """declared by the reference and never read; kept for the flag surface"""
    record_video_step_frequency: int = 1464
    """video recording period in steps (needs isaacgymenvs)"""

    # to be filled in runtime
    batch_size: int = 0
    """rollout batch size (computed at run time)"""
    minibatch_size: int = 0
    """minibatch size (computed at run time)"""
    num_iterations: int = 0
    """number of rollout/update iterations (computed at run time)"""


class _TensorEnv:
    """A stand-in task behind isaacgymenvs' calling convention: ``reset() -> obs``, ``step(action) -> (obs, reward, done, info)``, all
    tensors on ``device``.  ``env``: the device-resident task (its own tensors) or the host task (numpy arrays, converted here)."""

    def __init__(self, env, device):
        self.env, self.device, self.num_envs = env, device, env.num_envs
        self.observation_space, self.action_space = env.single_observation_space, env.single_action_space
        self.on_device = hasattr(env, "obs")

    def _t(self, x):
        return torch.as_tensor(np.asarray(x, np.float32), device=self.device)

    def reset(self):
        return self.env.obs() if self.on_device else self._t(self.env.reset()[0])

    def step(self, action):
        if self.on_device:
            obs, reward, done = self.env.step(action)
            return obs, reward, done, {}
        obs, reward, terminated, truncated, _ = self.env.step(action.cpu().numpy())
        return self._t(obs), self._t(reward), self._t(np.logical_or(terminated, truncated)), {}

    def close(self):
        self.env.close()


class RecordEpisodeStatisticsTorch:
    """Episode returns / lengths of every env as device tensors.  A rewrite of what the reference's wrapper of the same name does (:115-146),
    not a copy of it: each step adds the reward and one step to the running totals, publishes a snapshot of them as ``info["r"]`` /
    ``info["l"]`` (so the step that ends an episode reports the whole episode), then clears the totals of the envs that finished."""

    def __init__(self, env, device):
        self.env, self.device, self.num_envs = env, device, getattr(env, "num_envs", 1)
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self.returns = self.lengths = None

    def reset(self, **kwargs):
        self.returns = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
        self.lengths = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        return self.env.reset(**kwargs)

    def step(self, action):
        obs, rewards, dones, infos = self.env.step(action)
        infos["r"], infos["l"] = self.returns + rewards, self.lengths + 1
        running = dones == 0
        self.returns, self.lengths = infos["r"] * running, infos["l"] * running
        return obs, rewards, dones, infos

    def close(self):
        self.env.close()


class _ObsKey:
    """isaacgymenvs returns ``{"obs": tensor}``: hand the tensor on (the reference's ExtractObsWrapper)."""

    def __init__(self, env):
        self.env, self.num_envs = env, env.num_envs
        self.observation_space, self.action_space = env.observation_space, env.action_space

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)["obs"]

    def step(self, action):
        obs, r, d, info = self.env.step(action)
        return obs["obs"], r, d, info

    def close(self):
        pass


def make_envs(args, device):
    try:
        import isaacgymenvs
    except Exception:
        isaacgymenvs = None
    if isaacgymenvs is not None:
        on = device.type == "cuda"
        envs = isaacgymenvs.make(seed=args.seed, task=args.env_id, num_envs=args.num_envs, sim_device="cuda:0" if on else "cpu",
                                 rl_device="cuda:0" if on else "cpu", graphics_device_id=0 if on else -1, headless=not on, multi_gpu=False,
                                 virtual_screen_capture=args.capture_video, force_render=False)
        return _ObsKey(envs)
    print("[cleanrl_amd] isaacgymenvs not installed: using the Ant-shaped (obs 60, act 8) stand-in task", file=sys.stderr)
    if device.type == "cuda":
        return _TensorEnv(E.DeviceLinearContinuousVecEnv(args.num_envs, device, seed=args.seed, obs_dim=60, act_dim=8), device)
    return _TensorEnv(E.SyntheticContinuousVecEnv(args.num_envs, seed=args.seed, obs_dim=60, act_dim=8), device)


def main(argv=None):
    args = cli.parse(Args, argv)
    args.batch_size = int(args.num_envs * args.num_steps)
    args.minibatch_size = int(args.batch_size // args.num_minibatches)
    args.num_iterations = args.total_timesteps // args.batch_size
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)
    envs = RecordEpisodeStatisticsTorch(make_envs(args, device), device)
    envs.single_action_space, envs.single_observation_space = envs.action_space, envs.observation_space
    assert not hasattr(envs.single_action_space, "n"), "only continuous action space is supported"

    agent = Agent(envs).to(device)
    learner = PPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, args.num_envs, device, sample_seed=args.seed)
    learner.device_randperm = True                                      # :331
    print(f"[cleanrl_amd] 256-256 networks on {'the K8 kernels (MI355PPO_MLP256=fused)' if learner.mlp256 is not None else 'torch modules'}",
          file=sys.stderr)

    global_step = 0
    start_time = time.time()
    next_obs = envs.reset()
    learner.observe(0, next_obs, torch.zeros(args.num_envs, device=device))
    metrics = {}
    for iteration in range(1, args.num_iterations + 1):
        lrnow = args.learning_rate
        if args.anneal_lr:
            lrnow = (1.0 - (iteration - 1.0) / args.num_iterations) * args.learning_rate
        for step in range(0, args.num_steps):
            global_step += args.num_envs
            action = learner.act(step)
            next_obs, reward, next_done, info = envs.step(action)
            learner.store_reward(step, reward)
            learner.observe(step + 1, next_obs, next_done)
            if 0 <= step <= 2:                                          # :291-302: the first finished env of the rollout's first steps
                hit = torch.nonzero(next_done)
                if hit.numel():
                    idx = int(hit[0, 0])
                    episodic_return = info["r"][idx].item()
                    print(f"global_step={global_step}, episodic_return={episodic_return}")
                    writer.add_scalar("charts/episodic_return", episodic_return, global_step)
                    writer.add_scalar("charts/episodic_length", info["l"][idx].item(), global_step)
                    if "consecutive_successes" in info:
                        writer.add_scalar("charts/consecutive_successes", info["consecutive_successes"].item(), global_step)
        learner.finish_rollout()
        metrics = learner.update(lrnow)
        learner.start_iteration()
        writer.add_scalar("charts/learning_rate", lrnow, global_step)
        writer.add_scalar("losses/value_loss", metrics["value_loss"], global_step)
        writer.add_scalar("losses/policy_loss", metrics["policy_loss"], global_step)
        writer.add_scalar("losses/entropy", metrics["entropy"], global_step)
        writer.add_scalar("losses/old_approx_kl", metrics["old_approx_kl"], global_step)
        writer.add_scalar("losses/approx_kl", metrics["approx_kl"], global_step)
        writer.add_scalar("losses/clipfrac", metrics["clipfrac"], global_step)
        print("SPS:", int(global_step / (time.time() - start_time)))
        writer.add_scalar("charts/SPS", int(global_step / (time.time() - start_time)), global_step)
    learner.last_metrics = metrics
    envs.close()
    writer.close()
    return learner


if __name__ == "__main__":
    main()
