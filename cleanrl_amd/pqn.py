"""Drop-in for ``cleanrl/pqn.py``: PQN (parallelised Q-learning with Q(lambda) targets, a LayerNorm MLP and RAdam), classic control.

    python cleanrl_amd/pqn.py --env-id CartPole-v1 --num-envs 4 --num-steps 128 --seed 1 [--no-cuda]

Same flags, defaults, stdout lines and scalar tags as the reference.  ``QNetwork`` (cleanrl_amd/agents.py) is the reference's
network; ``PQNLearner`` (cleanrl_amd/learner_pqn.py) runs the rollout, Q(lambda) and the update.  ``MI355PPO_PQN=fused`` (the
default on a GPU) runs each rollout step as one launch and each minibatch as two, plus two for clip + RAdam (csrc/pqn.hip);
``torch`` runs the reference's ops.  Without gymnasium the built-in numpy CartPole-v1 is used.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import QNetwork  # noqa: E402
from cleanrl_amd.learner_pqn import PQNLearner  # noqa: E402


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
    env_id: str = "CartPole-v1"
    """the id of the environment"""
    total_timesteps: int = 500000
    """total timesteps of the experiments"""
    learning_rate: float = 2.5e-4
    """the learning rate of the optimizer"""
    num_envs: int = 4
    """the number of parallel game environments"""
    num_steps: int = 128
    """the number of steps to run for each environment per update"""
    num_minibatches: int = 4
    """the number of mini-batches"""
    update_epochs: int = 4
    """the K epochs to update the policy"""
    anneal_lr: bool = True
    """Toggle learning rate annealing"""
    gamma: float = 0.99
    """the discount factor gamma"""
    start_e: float = 1
    """the starting epsilon for exploration"""
    end_e: float = 0.05
    """the ending epsilon for exploration"""
    exploration_fraction: float = 0.5
    """the fraction of `total_timesteps` it takes from start_e to end_e"""
    max_grad_norm: float = 10.0
    """the maximum norm for the gradient clipping"""
    q_lambda: float = 0.65
    """the lambda for Q(lambda)"""


def make_envs(args, run_name):
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

        return gym.vector.SyncVectorEnv([make_env(args.env_id, args.seed + i, i, args.capture_video) for i in range(args.num_envs)])
    if args.env_id != "CartPole-v1":
        raise SystemExit(f"gymnasium is not installed and the built-in environments only cover CartPole-v1, not {args.env_id}")
    print("[cleanrl_amd] gymnasium not installed: using the built-in numpy CartPole-v1", file=sys.stderr)
    return E.CartPoleVecEnv(args.num_envs, seed=args.seed)


def main(argv=None):
    args = cli.parse(Args, argv)
    args.batch_size = int(args.num_envs * args.num_steps)
    args.minibatch_size = int(args.batch_size // args.num_minibatches)
    args.num_iterations = args.total_timesteps // args.batch_size
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args, run_name)
    assert hasattr(envs.single_action_space, "n"), "only discrete action space is supported"
    q_network = QNetwork(envs).to(device)
    learner = PQNLearner(q_network, args, envs.single_observation_space.shape, envs.single_action_space.n, args.num_envs, device)

    start_time = time.time()
    next_obs, _ = envs.reset(seed=args.seed)
    learner.reset(next_obs)
    for iteration in range(1, args.num_iterations + 1):
        learner.start_iteration(iteration)
        for step in range(0, args.num_steps):
            action = learner.act(step)
            next_obs, reward, terminations, truncations, infos = envs.step(action.cpu().numpy())
            learner.observe(step, next_obs, reward, np.logical_or(terminations, truncations))
            global_step = learner.global_step
            if "final_info" in infos:
                for info in infos["final_info"]:
                    if info and "episode" in info:
                        print(f"global_step={global_step}, episodic_return={info['episode']['r']}")
                        writer.add_scalar("charts/episodic_return", info["episode"]["r"], global_step)
                        writer.add_scalar("charts/episodic_length", info["episode"]["l"], global_step)
        learner.finish_rollout()
        m = learner.update()

        global_step = learner.global_step
        writer.add_scalar("losses/td_loss", m["td_loss"], global_step)
        writer.add_scalar("losses/q_values", m["q_values"], global_step)
        print("SPS:", int(global_step / (time.time() - start_time)))
        writer.add_scalar("charts/SPS", int(global_step / (time.time() - start_time)), global_step)

    envs.close()
    writer.close()
    return learner


if __name__ == "__main__":
    main()
