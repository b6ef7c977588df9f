"""Drop-in for ``cleanrl/sac_continuous_action.py``: SAC (twin soft critics, a tanh-Gaussian policy, a tuned entropy coefficient).

    python cleanrl_amd/sac_continuous_action.py --env-id Hopper-v4 --seed 1 [--no-cuda] [--no-autotune]

Same flags, defaults, stdout lines and scalar tags as the reference.  ``SoftActor`` / ``SoftQNetwork`` (cleanrl_amd/agents.py) are the
reference's networks; ``SACLearner`` (cleanrl_amd/learner_sac.py) holds the replay buffer and runs the action logic and the training
step.  ``MI355PPO_OFFPOLICY=fused`` keeps the buffer and ``alpha`` in device memory and runs a step in 8 launches, 20 with the policy
update (csrc/sac.hip, csrc/offpolicy.hip); ``torch`` runs the reference's ops.  Without gymnasium the built-in continuous stand-in is
used.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import SoftActor as Actor, SoftQNetwork  # noqa: E402
from cleanrl_amd.learner_sac import SACLearner  # noqa: E402


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
    env_id: str = "Hopper-v4"
    """the environment id of the task"""
    total_timesteps: int = 1000000
    """total timesteps of the experiments"""
    num_envs: int = 1
    """the number of parallel game environments"""
    buffer_size: int = int(1e6)
    """the replay memory buffer size"""
    gamma: float = 0.99
    """the discount factor gamma"""
    tau: float = 0.005
    """target smoothing coefficient (default: 0.005)"""
    batch_size: int = 256
    """the batch size of sample from the reply memory"""
    learning_starts: int = 5e3
    """timestep to start learning"""
    policy_lr: float = 3e-4
    """the learning rate of the policy network optimizer"""
    q_lr: float = 1e-3
    """the learning rate of the Q network network optimizer"""
    policy_frequency: int = 2
    """the frequency of training policy (delayed)"""
    target_network_frequency: int = 1  # Denis Yarats' implementation delays this by 2.
    """the frequency of updates for the target nerworks"""
    alpha: float = 0.2
    """Entropy regularization coefficient."""
    autotune: bool = True
    """automatic tuning of the entropy coefficient"""


def make_envs(args, run_name, seeds):
    if E.have_gymnasium():
        import gymnasium as gym

        def make_env(env_id, seed, idx, capture_video):
            def thunk():
                if capture_video and idx == 0:
                    env = gym.make(env_id, render_mode="rgb_array")
                    env = gym.wrappers.RecordVideo(env, f"videos/{run_name}")
                else:
                    env = gym.make(env_id)
                env = gym.wrappers.RecordEpisodeStatistics(env)
                env.action_space.seed(seed)
                return env

            return thunk

        envs = gym.vector.SyncVectorEnv([make_env(args.env_id, s, i, args.capture_video) for i, s in enumerate(seeds)])
        assert isinstance(envs.single_action_space, gym.spaces.Box), "only continuous action space is supported"
        return envs
    print(f"[cleanrl_amd] gymnasium not installed: using the built-in continuous stand-in for {args.env_id}", file=sys.stderr)
    return E.SyntheticReplayVecEnv(len(seeds), seed=args.seed, horizon=int(os.environ.get("MI355PPO_STANDIN_HORIZON", "1000")))


def main(argv=None):
    args = cli.parse(Args, argv)
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args, run_name, [args.seed + i for i in range(args.num_envs)])
    actor = Actor(envs).to(device)
    qf1 = SoftQNetwork(envs).to(device)
    qf2 = SoftQNetwork(envs).to(device)
    qf1_target = SoftQNetwork(envs).to(device)
    qf2_target = SoftQNetwork(envs).to(device)
    qf1_target.load_state_dict(qf1.state_dict())
    qf2_target.load_state_dict(qf2.state_dict())
    learner = SACLearner(actor, qf1, qf2, qf1_target, qf2_target, args, envs, device)
    start_time = time.time()

    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.total_timesteps):
        actions = learner.act(obs, global_step)
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)

        if "final_info" in infos:
            for info in infos["final_info"]:
                if info is not None:
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
            learner.train_step(policy_update=global_step % args.policy_frequency == 0,
                               target_update=global_step % args.target_network_frequency == 0)
            if global_step % 100 == 0:
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
