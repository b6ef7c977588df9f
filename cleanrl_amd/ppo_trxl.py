"""Drop-in for ``cleanrl/ppo_trxl/ppo_trxl.py``: PPO with a Transformer-XL policy over an episodic memory (memory tasks).

    python cleanrl_amd/ppo_trxl.py --env-id MortarMayhem-Grid-v0 --num-envs 32 --num-steps 512 --seed 1

The network, rollout, episodic-memory bookkeeping and update are the reference's (``TrXLAgent`` in cleanrl_amd/agents.py,
``TrXLLearner`` in cleanrl_amd/learner_trxl.py).  ``MI355PPO_TRXL=fused`` runs each layer's memory-window attention -- the
window gather, positional encoding, ``norm_kv``, keys, masked softmax and weighted sum -- as one HIP kernel that streams the
rows from the episode pool (csrc/trxl_attn.hip); the default ``torch`` runs the reference's ops.  GAE runs in the K1 kernel on
the GPU.  Without ``gymnasium`` / ``memory_gym`` the synthetic memory task of cleanrl_amd/envs.py stands in
(``SyntheticMemoryVecEnv``: vector or (84, 84, 3) image observations, Discrete or MultiDiscrete actions, by env id).

One deviation: before the first episode has ended the reference's print line raises ``KeyError`` (``episode_result["r_mean"]``);
here it prints ``nan`` for the return and length.
"""
from __future__ import annotations

import os
import sys
import time
from collections import deque
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import TrXLAgent  # noqa: E402
from cleanrl_amd.learner_trxl import TrXLLearner  # noqa: E402


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

    # Algorithm specific arguments
    env_id: str = "MortarMayhem-Grid-v0"
    """the id of the environment"""
    total_timesteps: int = 200000000
    """total timesteps of the experiments"""
    init_lr: float = 2.75e-4
    """the initial learning rate of the optimizer"""
    final_lr: float = 1.0e-5
    """the final learning rate of the optimizer after linearly annealing"""
    num_envs: int = 32
    """the number of parallel game environments"""
    num_steps: int = 512
    """the number of steps to run in each environment per policy rollout"""
    anneal_steps: int = 32 * 512 * 10000
    """the number of steps to linearly anneal the learning rate and entropy coefficient from initial to final"""
    gamma: float = 0.995
    """the discount factor gamma"""
    gae_lambda: float = 0.95
    """the lambda for the general advantage estimation"""
    num_minibatches: int = 8
    """the number of mini-batches"""
    update_epochs: int = 3
    """the K epochs to update the policy"""
    norm_adv: bool = False
    """Toggles advantages normalization"""
    clip_coef: float = 0.1
    """the surrogate clipping coefficient"""
    clip_vloss: bool = True
    """Toggles whether or not to use a clipped loss for the value function, as per the paper."""
    init_ent_coef: float = 0.0001
    """initial coefficient of the entropy bonus"""
    final_ent_coef: float = 0.000001
    """final coefficient of the entropy bonus after linearly annealing"""
    vf_coef: float = 0.5
    """coefficient of the value function"""
    max_grad_norm: float = 0.25
    """the maximum norm for the gradient clipping"""
    target_kl: float = None
    """the target KL divergence threshold"""

    # Transformer-XL specific arguments
    trxl_num_layers: int = 3
    """the number of transformer layers"""
    trxl_num_heads: int = 4
    """the number of heads used in multi-head attention"""
    trxl_dim: int = 384
    """the dimension of the transformer"""
    trxl_memory_length: int = 119
    """the length of TrXL's sliding memory window"""
    trxl_positional_encoding: str = "absolute"
    """the positional encoding type of the transformer, choices: "", "absolute", "learned" """
    reconstruction_coef: float = 0.0
    """the coefficient of the observation reconstruction loss, if set to 0.0 the reconstruction loss is not used"""

    # To be filled on runtime
    batch_size: int = 0
    """the batch size (computed in runtime)"""
    minibatch_size: int = 0
    """the mini-batch size (computed in runtime)"""
    num_iterations: int = 0
    """the number of iterations (computed in runtime)"""


def make_envs(args, run_name):
    """ppo_trxl.py's ``make_env`` stack when gymnasium and memory_gym are installed, else the synthetic memory task."""
    try:
        import gymnasium as gym
        import memory_gym  # noqa: F401
    except ImportError:
        print("[cleanrl_amd] gymnasium/memory_gym not installed: using the synthetic memory-task stand-in", file=sys.stderr)
        return E.SyntheticMemoryVecEnv(args.env_id, args.num_envs)

    def make_env(env_id, idx, capture_video, render_mode="debug_rgb_array"):
        if "MiniGrid" in env_id and render_mode == "debug_rgb_array":
            render_mode = "rgb_array"

        def thunk():
            if "MiniGrid" in env_id:
                from minigrid.wrappers import ImgObsWrapper, RGBImgPartialObsWrapper

                env = gym.make(env_id, agent_view_size=3, tile_size=28, render_mode=render_mode)
                env = ImgObsWrapper(RGBImgPartialObsWrapper(env, tile_size=28))
                env = gym.wrappers.TimeLimit(env, 96)
            else:
                env = gym.make(env_id, render_mode=render_mode)
            if capture_video and idx == 0:
                env = gym.wrappers.RecordVideo(env, f"videos/{run_name}")
            return gym.wrappers.RecordEpisodeStatistics(env)

        return thunk

    return gym.vector.SyncVectorEnv([make_env(args.env_id, i, args.capture_video) for i in range(args.num_envs)])


def action_space_shape_of(space):
    return (space.n,) if hasattr(space, "n") else tuple(int(n) for n in space.nvec)


def max_episode_steps_of(envs):
    """The reference's probe: the TimeLimit of ``envs.envs[0]``, else Memory Gym's attribute after a reset, else 1024."""
    max_episode_steps = envs.envs[0].spec.max_episode_steps
    if not max_episode_steps:
        envs.envs[0].reset()
        max_episode_steps = envs.envs[0].max_episode_steps
    if max_episode_steps <= 0:
        max_episode_steps = 1024
    return max_episode_steps


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
    observation_space = envs.single_observation_space
    action_space_shape = action_space_shape_of(envs.single_action_space)
    max_episode_steps = max_episode_steps_of(envs)
    args.trxl_memory_length = min(args.trxl_memory_length, max_episode_steps)

    agent = TrXLAgent(args, observation_space, action_space_shape, max_episode_steps).to(device)
    learner = TrXLLearner(agent, args, observation_space, action_space_shape, args.num_envs, max_episode_steps, device)

    start_time = time.time()
    episode_infos = deque(maxlen=100)
    next_obs, _ = envs.reset(seed=args.seed)
    learner.reset(next_obs)
    for iteration in range(1, args.num_iterations + 1):
        sampled_episode_infos = []
        learner.start_iteration()
        for step in range(args.num_steps):
            action = learner.act(step)
            next_obs, reward, terminations, truncations, infos = envs.step(action.cpu().numpy())
            learner.observe(step, next_obs, reward, terminations, truncations)
            if "final_info" in infos:
                for info in infos["final_info"]:
                    if info and "episode" in info:
                        sampled_episode_infos.append(info["episode"])
        learner.finish_rollout()
        m = learner.update()

        episode_infos.extend(sampled_episode_infos)
        episode_result = {}
        if len(episode_infos) > 0:
            for key in episode_infos[0].keys():
                episode_result[key + "_mean"] = np.mean([info[key] for info in episode_infos])
        global_step = learner.global_step
        sps = int(global_step / (time.time() - start_time))
        print("{:9} SPS={:4} return={:.2f} length={:.1f} pi_loss={:.3f} v_loss={:.3f} entropy={:.3f} r_loss={:.3f} value={:.3f} "
              "adv={:.3f}".format(iteration, sps, episode_result.get("r_mean", float("nan")), episode_result.get("l_mean", float("nan")),
                                  m["policy_loss"], m["value_loss"], m["entropy"], m["reconstruction_loss"], m["value_mean"],
                                  m["advantage_mean"]))
        if writer is not None:
            for key in episode_result:
                writer.add_scalar("episode/" + key, episode_result[key], global_step)
            writer.add_scalar("episode/value_mean", m["value_mean"], global_step)
            writer.add_scalar("episode/advantage_mean", m["advantage_mean"], global_step)
            writer.add_scalar("charts/learning_rate", m["learning_rate"], global_step)
            writer.add_scalar("charts/entropy_coefficient", m["entropy_coefficient"], global_step)
            for key in ("policy_loss", "value_loss", "loss", "entropy", "reconstruction_loss", "old_approx_kl", "approx_kl", "clipfrac",
                        "explained_variance"):
                writer.add_scalar("losses/" + key, m[key], global_step)
            writer.add_scalar("charts/SPS", sps, global_step)

    if args.save_model:
        model_path = f"runs/{run_name}/{args.exp_name}.cleanrl_model"
        os.makedirs(os.path.dirname(model_path), exist_ok=True)
        torch.save({"model_weights": agent.state_dict(), "args": vars(args)}, model_path)
        print(f"model saved to {model_path}")
    if writer is not None:
        writer.close()
    envs.close()
    return learner


if __name__ == "__main__":
    main()
