"""Drop-in for ``cleanrl/rainbow_atari.py``: Rainbow (noisy dueling distributional double-Q learning with prioritized n-step replay).

    python cleanrl_amd/rainbow_atari.py --env-id BreakoutNoFrameskip-v4 --seed 1 [--no-cuda]

Same flags, defaults, stdout lines and scalar tags as the reference.  ``NoisyDuelingDistributionalNetwork`` (cleanrl_amd/agents.py) is the
reference's network; ``RainbowLearner`` (cleanrl_amd/learner_rainbow.py) holds the prioritized replay buffer and runs the action logic, the
training step and the target update.  There is no epsilon-greedy here: the action is the argmax of the noisy online network, which stays
in training mode.  ``MI355PPO_OFFPOLICY=fused`` keeps the two frame rings and the sum tree in device memory and runs the trunk on this
library's kernels and the noise composition, head, loss, projection and priority update on csrc/rainbow.hip;
``torch`` runs the reference's ops.  With gymnasium the reference's wrapper stack (cleanrl_amd/atari_wrappers.py) is used, without it the
built-in stand-in.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork  # noqa: E402
from cleanrl_amd.learner_rainbow import RainbowLearner  # noqa: E402


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
    save_model: bool = False
    """whether to save model into the `runs/{run_name}` folder"""
    upload_model: bool = False
    """whether to upload the saved model to huggingface"""
    hf_entity: str = ""
    """the user or org name of the model repository from the Hugging Face Hub"""

    env_id: str = "BreakoutNoFrameskip-v4"
    """the id of the environment"""
    total_timesteps: int = 10000000
    """total timesteps of the experiments"""
    learning_rate: float = 0.0000625
    """the learning rate of the optimizer"""
    num_envs: int = 1
    """the number of parallel game environments"""
    buffer_size: int = 1000000
    """the replay memory buffer size"""
    gamma: float = 0.99
    """the discount factor gamma"""
    tau: float = 1.0
    """the target network update rate"""
    target_network_frequency: int = 8000
    """the timesteps it takes to update the target network"""
    batch_size: int = 32
    """the batch size of sample from the reply memory"""
    start_e: float = 1
    """the starting epsilon for exploration"""
    end_e: float = 0.01
    """the ending epsilon for exploration"""
    exploration_fraction: float = 0.10
    """the fraction of `total-timesteps` it takes from start-e to go end-e"""
    learning_starts: int = 80000
    """timestep to start learning"""
    train_frequency: int = 4
    """the frequency of training"""
    n_step: int = 3
    """the number of steps to look ahead for n-step Q learning"""
    prioritized_replay_alpha: float = 0.5
    """alpha parameter for prioritized replay buffer"""
    prioritized_replay_beta: float = 0.4
    """beta parameter for prioritized replay buffer"""
    prioritized_replay_eps: float = 1e-6
    """epsilon parameter for prioritized replay buffer"""
    n_atoms: int = 51
    """the number of atoms"""
    v_min: float = -10
    """the return lower bound"""
    v_max: float = 10
    """the return upper bound"""


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
    assert args.num_envs == 1, "vectorized envs are not supported at the moment"
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args, run_name, [args.seed + i for i in range(args.num_envs)])
    q_network = NoisyDuelingDistributionalNetwork(envs, args.n_atoms, args.v_min, args.v_max).to(device)
    target_network = NoisyDuelingDistributionalNetwork(envs, args.n_atoms, args.v_min, args.v_max).to(device)
    target_network.load_state_dict(q_network.state_dict())
    learner = RainbowLearner(q_network, target_network, args, envs, device)
    start_time = time.time()

    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.total_timesteps):
        # anneal PER beta to 1
        learner.beta = min(
            1.0, args.prioritized_replay_beta + global_step * (1.0 - args.prioritized_replay_beta) / args.total_timesteps
        )
        actions = learner.act(obs)
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)

        if "final_info" in infos:
            for info in infos["final_info"]:
                if info and "episode" in info:
                    print(f"global_step={global_step}, episodic_return={info['episode']['r']}")
                    writer.add_scalar("charts/episodic_return", info["episode"]["r"], global_step)
                    writer.add_scalar("charts/episodic_length", info["episode"]["l"], global_step)

        real_next_obs = next_obs.copy()
        for idx, trunc in enumerate(truncations):
            if trunc:
                real_next_obs[idx] = infos["final_observation"][idx]
        learner.store(obs, actions, rewards, real_next_obs, terminations)
        obs = next_obs

        if global_step > args.learning_starts:
            if global_step % args.train_frequency == 0:
                learner.train_step()
                if global_step % 100 == 0:
                    m = learner.metrics()
                    writer.add_scalar("losses/td_loss", m["loss"], global_step)
                    writer.add_scalar("losses/q_values", m["q_values"], global_step)
                    sps = int(global_step / (time.time() - start_time))
                    print("SPS:", sps)
                    writer.add_scalar("charts/SPS", sps, global_step)
                    writer.add_scalar("charts/beta", learner.beta, global_step)
            if global_step % args.target_network_frequency == 0:
                learner.sync_target()

    if args.save_model:
        model_path = f"runs/{run_name}/{args.exp_name}.cleanrl_model"
        torch.save({"model_weights": q_network.state_dict(), "args": vars(args)}, model_path)
        print(f"model saved to {model_path}")
        if args.upload_model:
            raise SystemExit("--upload-model needs network access and cleanrl_utils.huggingface; not available here")
        print("[cleanrl_amd] the evaluation leg needs cleanrl_utils.evals; not available here", file=sys.stderr)

    envs.close()
    writer.close()
    return learner


if __name__ == "__main__":
    main()
