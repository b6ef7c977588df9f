"""Drop-in for ``cleanrl/sac_atari.py``: discrete Soft Actor-Critic on Atari frame stacks.

    python cleanrl_amd/sac_atari.py --env-id BeamRiderNoFrameskip-v4 --seed 1 [--no-cuda]

Same flags, defaults, stdout lines and scalar tags as the reference.  ``AtariSACActor`` and ``AtariSoftQNetwork`` (cleanrl_amd/agents.py)
are the reference's ``Actor`` and ``SoftQNetwork``; ``SACAtariLearner`` (cleanrl_amd/learner_sac_atari.py) holds the replay buffer and runs
the action logic, the training step and the target update.  ``MI355PPO_OFFPOLICY=fused`` keeps the frames as bytes in two device rings,
runs the five trunks on this library's kernels and the heads, both losses and the head backwards on csrc/sac_atari.hip, with ``alpha`` in
device memory; ``torch`` runs the reference's ops.  With gymnasium the reference's wrapper stack
(cleanrl_amd/atari_wrappers.py) is used, without it the built-in stand-in.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import AtariSACActor as Actor, AtariSoftQNetwork as SoftQNetwork  # noqa: E402
from cleanrl_amd.learner_sac_atari import SACAtariLearner  # noqa: E402


@dataclass
class Args:
    exp_name: str = os.path.basename(__file__)[: -len(".py")]
    """the name of this experiment"""
    seed: int = 1
    """seed of the experiment"""
    torch_deterministic: bool = True
    """if toggled, `torch.backends.cudnn.deterministic=False`"""
    cuda: bool = True
    """if toggled, cuda will be enabled by default"""
    track: bool = False
    """if toggled, this experiment will be tracked with Weights and Biases"""
    wandb_project_name: str = "cleanRL"
    """the wandb's project name"""
    wandb_entity: str = None
    """the entity (team) of wandb's project"""
    capture_video: bool = False
    """whether to capture videos of the agent performances (check out `videos` folder)"""

    # Algorithm specific arguments
    env_id: str = "BeamRiderNoFrameskip-v4"
    """the id of the environment"""
    total_timesteps: int = 5000000
    """total timesteps of the experiments"""
    buffer_size: int = int(1e6)
    """the replay memory buffer size"""
    gamma: float = 0.99
    """the discount factor gamma"""
    tau: float = 1.0
    """target smoothing coefficient (default: 1)"""
    batch_size: int = 64
    """the batch size of sample from the reply memory"""
    learning_starts: int = 2e4
    """timestep to start learning"""
    policy_lr: float = 3e-4
    """the learning rate of the policy network optimizer"""
    q_lr: float = 3e-4
    """the learning rate of the Q network network optimizer"""
    update_frequency: int = 4
    """the frequency of training updates"""
    target_network_frequency: int = 8000
    """the frequency of updates for the target networks"""
    alpha: float = 0.2
    """Entropy regularization coefficient."""
    autotune: bool = True
    """automatic tuning of the entropy coefficient"""
    target_entropy_scale: float = 0.89
    """coefficient for scaling the autotune entropy target"""


def make_envs(args, run_name, seeds):
    if E.have_gymnasium():
        import gymnasium as gym

        from cleanrl_amd.atari_wrappers import ClipRewardEnv, EpisodicLifeEnv, FireResetEnv, MaxAndSkipEnv, NoopResetEnv

        def make_env(env_id, seed, idx, capture_video):
            def thunk():
                if capture_video and idx == 0:
                    env = gym.make(env_id, render_mode="rgb_array")
                    env = gym.wrappers.RecordVideo(env, f"videos/{run_name}")
                else:
                    env = gym.make(env_id)
                env = gym.wrappers.RecordEpisodeStatistics(env)
                env = NoopResetEnv(env, noop_max=30)
                env = MaxAndSkipEnv(env, skip=4)
                env = EpisodicLifeEnv(env)
                if "FIRE" in env.unwrapped.get_action_meanings():
                    env = FireResetEnv(env)
                env = ClipRewardEnv(env)
                env = gym.wrappers.ResizeObservation(env, (84, 84))
                env = gym.wrappers.GrayScaleObservation(env)
                env = gym.wrappers.FrameStack(env, 4)
                env.action_space.seed(seed)
                return env

            return thunk

        envs = gym.vector.SyncVectorEnv([make_env(args.env_id, s, i, args.capture_video) for i, s in enumerate(seeds)])
        assert isinstance(envs.single_action_space, gym.spaces.Discrete), "only discrete action space is supported"
        return envs
    print(f"[cleanrl_amd] gymnasium not installed: using the synthetic Atari stand-in for {args.env_id}", file=sys.stderr)
    horizon = os.environ.get("MI355PPO_STANDIN_HORIZON")
    return E.AtariReplayVecEnv(len(seeds), seed=args.seed, horizon=int(horizon) if horizon else None)



def main(argv=None):
    args = cli.parse(Args, argv)
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args, run_name, [args.seed])
    actor = Actor(envs).to(device)
    qf1 = SoftQNetwork(envs).to(device)
    qf2 = SoftQNetwork(envs).to(device)
    qf1_target = SoftQNetwork(envs).to(device)
    qf2_target = SoftQNetwork(envs).to(device)
    qf1_target.load_state_dict(qf1.state_dict())
    qf2_target.load_state_dict(qf2.state_dict())
    learner = SACAtariLearner(actor, qf1, qf2, qf1_target, qf2_target, args, envs, device)
    start_time = time.time()

    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.total_timesteps):
        actions = learner.act(obs, global_step)
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)

        if "final_info" in infos:
            for info in infos["final_info"]:
                if not info or "episode" not in info:
                    continue
                print(f"global_step={global_step}, episodic_return={info['episode']['r']}")
                writer.add_scalar("charts/episodic_return", info["episode"]["r"], global_step)
                writer.add_scalar("charts/episodic_length", info["episode"]["l"], global_step)
                break

        real_next_obs = next_obs.copy()
        for idx, trunc in enumerate(truncations):
            if trunc:
                real_next_obs[idx] = infos["final_observation"][idx]
        learner.store(obs, real_next_obs, actions, rewards, terminations)
        obs = next_obs

        if global_step > args.learning_starts:
            if global_step % args.update_frequency == 0:
                learner.train_step()
            if global_step % args.target_network_frequency == 0:
                learner.sync_target()
            if global_step % 100 == 0 and learner.last is not None:
                m = learner.metrics()
                writer.add_scalar("losses/qf1_values", m["qf1_values"], global_step)
                writer.add_scalar("losses/qf2_values", m["qf2_values"], global_step)
                writer.add_scalar("losses/qf1_loss", m["qf1_loss"], global_step)
                writer.add_scalar("losses/qf2_loss", m["qf2_loss"], global_step)
                writer.add_scalar("losses/qf_loss", m["qf_loss"] / 2.0, global_step)
                writer.add_scalar("losses/actor_loss", m["actor_loss"], global_step)
                writer.add_scalar("losses/alpha", m["alpha"], global_step)
                print("SPS:", int(global_step / (time.time() - start_time)))
                writer.add_scalar("charts/SPS", int(global_step / (time.time() - start_time)), global_step)
                if args.autotune:
                    writer.add_scalar("losses/alpha_loss", m["alpha_loss"], global_step)

    envs.close()
    writer.close()
    return learner


if __name__ == "__main__":
    main()
