"""Drop-in for ``cleanrl/pqn_atari_envpool_lstm.py``: recurrent PQN on EnvPool Atari (LayerNorm NatureCNN on one frame -> LSTM).

    python cleanrl_amd/pqn_atari_envpool_lstm.py --env-id Breakout-v5 --num-envs 8 --seed 1 [--no-cuda]

Same flags, defaults, stdout lines and scalar tags as the reference.  ``AtariLSTMQNetwork`` (cleanrl_amd/agents.py) is the
reference's network; its trunk and the gx GEMM stay torch on every backend.  With ``MI355PPO_PQN=fused`` (the default on a GPU) the
recurrent tail runs in the library: a rollout step's LSTM cell + ``q_func`` + e-greedy in one launch, the update's recurrence as
one scan each way (csrc/lstm.hip), ``q_func`` + TD loss forward and backward (csrc/pqn_lstm.hip), Q(lambda) and clip + RAdam on
flat buffers (csrc/pqn.hip).  ``MI355PPO_LSTM`` is not read.  Without envpool the synthetic (N, 1, 84, 84) uint8 Atari stand-in
(gym API, ``lives`` in ``info``) is used.
"""
from __future__ import annotations

import os
import sys
import time
from collections import deque
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import AtariLSTMQNetwork  # noqa: E402
from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner  # noqa: E402
from cleanrl_amd.ppo_atari_envpool import RecordEpisodeStatistics  # noqa: E402


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
    env_id: str = "Breakout-v5"
    """the id of the environment"""
    total_timesteps: int = 10000000
    """total timesteps of the experiments"""
    learning_rate: float = 2.5e-4
    """the learning rate of the optimizer"""
    num_envs: int = 8
    """the number of parallel game environments"""
    num_steps: int = 128
    """the number of steps to run in each environment per policy rollout"""
    anneal_lr: bool = True
    """Toggle learning rate annealing for policy and value networks"""
    gamma: float = 0.99
    """the discount factor gamma"""
    num_minibatches: int = 4
    """the number of mini-batches"""
    update_epochs: int = 4
    """the K epochs to update the policy"""
    max_grad_norm: float = 0.5
    """the maximum norm for the gradient clipping"""
    start_e: float = 1
    """the starting epsilon for exploration"""
    end_e: float = 0.01
    """the ending epsilon for exploration"""
    exploration_fraction: float = 0.10
    """the fraction of `total_timesteps` it takes from start_e to end_e"""
    q_lambda: float = 0.65
    """the lambda for the Q-Learning algorithm"""

    # to be filled in runtime
    batch_size: int = 0
    """the batch size (computed in runtime)"""
    minibatch_size: int = 0
    """the mini-batch size (computed in runtime)"""
    num_iterations: int = 0
    """the number of iterations (computed in runtime)"""


def make_envs(args):
    if E.have_envpool():
        import envpool

        envs = envpool.make(args.env_id, env_type="gym", num_envs=args.num_envs, episodic_life=True, reward_clip=True, seed=args.seed,
                            stack_num=1)
        envs.num_envs = args.num_envs
        envs.single_action_space = envs.action_space
        envs.single_observation_space = envs.observation_space
        return RecordEpisodeStatistics(envs)
    print("[cleanrl_amd] envpool not installed: using the synthetic (N,1,84,84) uint8 Atari stand-in (gym API)", file=sys.stderr)
    return E.SyntheticAtariVecEnv(args.num_envs, seed=args.seed, n_actions=4, api="gym", frames=1)


def main(argv=None):
    args = cli.parse(Args, argv)
    args.batch_size = int(args.num_envs * args.num_steps)
    args.minibatch_size = int(args.batch_size // args.num_minibatches)
    args.num_iterations = args.total_timesteps // args.batch_size
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args)
    q_network = AtariLSTMQNetwork(envs).to(device)
    learner = LSTMPQNLearner(q_network, args, envs.single_observation_space.shape, envs.single_action_space.n, args.num_envs, device,
                             obs_space=envs.single_observation_space)

    avg_returns = deque(maxlen=20)
    start_time = time.time()
    learner.reset(envs.reset())
    for iteration in range(1, args.num_iterations + 1):
        learner.start_iteration(iteration)
        for step in range(0, args.num_steps):
            action = learner.act(step)
            next_obs, reward, next_done, info = envs.step(action.cpu().numpy())
            learner.observe(step, next_obs, reward, next_done)
            global_step = learner.global_step
            for idx, d in enumerate(next_done):
                if d and info["lives"][idx] == 0:
                    print(f"global_step={global_step}, episodic_return={info['r'][idx]}")
                    avg_returns.append(info["r"][idx])
                    writer.add_scalar("charts/avg_episodic_return", np.average(avg_returns), global_step)
                    writer.add_scalar("charts/episodic_return", info["r"][idx], global_step)
                    writer.add_scalar("charts/episodic_length", info["l"][idx], global_step)
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
