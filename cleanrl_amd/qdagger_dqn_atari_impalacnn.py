"""Drop-in for ``cleanrl/qdagger_dqn_atari_impalacnn.py``: QDagger (Agarwal et al. 2022) -- an IMPALA-CNN student reincarnated from a
``dqn_atari`` teacher on Atari frame stacks.

    python cleanrl_amd/qdagger_dqn_atari_impalacnn.py --env-id BreakoutNoFrameskip-v4 --seed 1 [--no-cuda]

Same flags, defaults, three phases (the teacher fills a replay buffer, the student trains offline on it, then online on its own),
stdout lines and scalar tags as the reference.  ``AtariImpalaQNetwork`` (cleanrl_amd/agents.py) is the reference's ``QNetwork``,
``AtariDQNNetwork`` its ``TeacherModel``; ``QDaggerLearner`` (cleanrl_amd/learner_qdagger.py) holds the replay buffers and runs the action
logic, the training steps and the target update.  ``MI355PPO_OFFPOLICY=fused`` keeps the frames as bytes in device memory and runs the
head, both losses and the head backward on csrc/qdagger.hip; with ``MI355PPO_IMPALA=fused`` the student's trunk runs on csrc/impala.hip
(DESIGN.md section 3.19); ``torch`` runs the reference's ops.

What the reference takes from packages that are not here:
  * ``rich.progress.track`` is a plain ``range``;
  * ``evaluate`` is written below after cleanrl_utils/evals/dqn_eval.py (its result feeds ``distill_coeff``: it is part of the algorithm);
    it runs on ``make_envs``' environment;
  * the teacher comes from ``MI355PPO_TEACHER_MODEL``, the path of a ``dqn_atari`` ``.cleanrl_model`` state dict (what
    ``cleanrl_amd/dqn_atari.py --save-model`` writes).  Without it the synthetic stand-in env gets a seeded randomly
    initialised teacher (a line on stderr says so; the hub is never consulted for the stand-in); a real env asks
    ``huggingface_hub`` when that is installed and otherwise stops with a ``SystemExit`` naming the variable.
"""
from __future__ import annotations

import os
import random
import sys
import time
from collections import deque
from dataclasses import dataclass

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cleanrl_amd import cli, envs as E, runner  # noqa: E402
from cleanrl_amd.agents import AtariDQNNetwork as TeacherModel  # noqa: E402
from cleanrl_amd.agents import AtariImpalaQNetwork as QNetwork  # noqa: E402
from cleanrl_amd.dqn_atari import linear_schedule, make_envs  # noqa: E402,F401
from cleanrl_amd.learner_qdagger import QDaggerLearner  # noqa: E402

TEACHER_ENV = "MI355PPO_TEACHER_MODEL"
STANDIN_TEACHER_SEED = 20220601


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

    # Algorithm specific arguments
    env_id: str = "BreakoutNoFrameskip-v4"
    """the id of the environment"""
    total_timesteps: int = 10000000
    """total timesteps of the experiments"""
    learning_rate: float = 1e-4
    """the learning rate of the optimizer"""
    num_envs: int = 1
    """the number of parallel game environments"""
    buffer_size: int = 1000000
    """the replay memory buffer size"""
    gamma: float = 0.99
    """the discount factor gamma"""
    tau: float = 1.0
    """the target network update rate"""
    target_network_frequency: int = 1000
    """the timesteps it takes to update the target network"""
    batch_size: int = 32
    """the batch size of sample from the reply memory"""
    start_e: float = 1.0
    """the starting epsilon for exploration"""
    end_e: float = 0.01
    """the ending epsilon for exploration"""
    exploration_fraction: float = 0.10
    """the fraction of `total-timesteps` it takes from start-e to go end-e"""
    learning_starts: int = 80000
    """timestep to start learning"""
    train_frequency: int = 4
    """the frequency of training"""

    # QDagger specific arguments
    teacher_policy_hf_repo: str = None
    """the huggingface repo of the teacher policy"""
    teacher_model_exp_name: str = "dqn_atari"
    """the experiment name of the teacher model"""
    teacher_eval_episodes: int = 10
    """the number of episodes to run the teacher policy evaluate"""
    teacher_steps: int = 500000
    """the number of steps to run the teacher policy to generate the replay buffer"""
    offline_steps: int = 500000
    """the number of steps to run the student policy with the teacher's replay buffer"""
    temperature: float = 1.0
    """the temperature parameter for qdagger"""


def load_teacher(args, envs, device):
    """The reference's ``hf_hub_download`` + ``TeacherModel(envs)`` + ``load_state_dict`` + ``eval()``."""
    path = os.environ.get(TEACHER_ENV)
    if not path and not E.have_gymnasium():
        # the stand-in env: no game a published teacher could have learnt, so the hub is never consulted
        print(f"[cleanrl_amd] {TEACHER_ENV} is not set: the stand-in env gets a randomly initialised teacher (seed {STANDIN_TEACHER_SEED})",
              file=sys.stderr)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(STANDIN_TEACHER_SEED)
            teacher_model = TeacherModel(envs)
        teacher_model = teacher_model.to(device)
        teacher_model.eval()
        return teacher_model
    if not path:
        try:
            from huggingface_hub import hf_hub_download
        except ImportError:
            raise SystemExit(f"the teacher policy needs {TEACHER_ENV}: the path of a dqn_atari .cleanrl_model state dict "
                             f"(python cleanrl_amd/dqn_atari.py --save-model writes one); huggingface_hub is not installed") from None
        path = hf_hub_download(repo_id=args.teacher_policy_hf_repo, filename=f"{args.teacher_model_exp_name}.cleanrl_model")
    teacher_model = TeacherModel(envs).to(device)
    teacher_model.load_state_dict(torch.load(path, map_location=device))
    teacher_model.eval()
    return teacher_model


def evaluate(model, args, run_name, eval_episodes: int, device, epsilon: float = 0.05):
    """cleanrl_utils/evals/dqn_eval.py's loop on ``model`` (the reference reloads the saved state dict into a fresh network, which
    holds the same weights): epsilon-greedy episodes on one fresh environment of seed 0 -> their returns."""
    envs = make_envs(args, run_name, [0])
    obs, _ = envs.reset()
    episodic_returns = []
    while len(episodic_returns) < eval_episodes:
        if random.random() < epsilon:
            actions = np.array([envs.single_action_space.sample() for _ in range(envs.num_envs)])
        else:
            with torch.no_grad():
                q_values = model(torch.Tensor(obs).to(device))
            actions = torch.argmax(q_values, dim=1).cpu().numpy()
        next_obs, _, _, _, infos = envs.step(actions)
        if "final_info" in infos:
            for info in infos["final_info"]:
                if not info or "episode" not in info:
                    continue
                print(f"eval_episode={len(episodic_returns)}, episodic_return={info['episode']['r']}")
                episodic_returns += [info["episode"]["r"]]
        obs = next_obs
    envs.close()
    return episodic_returns


def distill_coefficient(episodic_returns, teacher_episodic_returns):
    """qdagger_dqn_atari_impalacnn.py:399-402 over the 10-deep deque of the student's returns."""
    if len(episodic_returns) < 10:
        return 1.0
    return max(1 - np.mean(episodic_returns) / np.mean(teacher_episodic_returns), 0)


def real_next(next_obs, truncations, infos):
    real_next_obs = next_obs.copy()
    for idx, trunc in enumerate(truncations):
        if trunc:
            real_next_obs[idx] = infos["final_observation"][idx]
    return real_next_obs


def teacher_phase(args, envs, learner):
    """Fills the teacher's replay buffer (:274-288)."""
    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.teacher_steps):
        epsilon = linear_schedule(args.start_e, args.end_e, args.teacher_steps, global_step)
        actions = learner.act(obs, global_step, epsilon, teacher=True)
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)
        learner.store(obs, real_next(next_obs, truncations, infos), actions, rewards, terminations)
        obs = next_obs


def offline_phase(args, learner, writer, run_name, device, q_network):
    """Trains the student on the teacher's buffer with the QDagger loss (:291-339)."""
    for global_step in range(args.offline_steps):
        learner.train_step(1.0)
        if global_step % args.target_network_frequency == 0:
            learner.sync_target()
        if global_step % 100 == 0:
            m = learner.metrics()
            writer.add_scalar("charts/offline/loss", m["loss"], global_step)
            writer.add_scalar("charts/offline/q_loss", m["q_loss"], global_step)
            writer.add_scalar("charts/offline/distill_loss", m["distill_loss"], global_step)
        if global_step % 100000 == 0:
            model_path = f"runs/{run_name}/{args.exp_name}-offline-{global_step}.cleanrl_model"
            os.makedirs(os.path.dirname(model_path), exist_ok=True)
            torch.save(q_network.state_dict(), model_path)
            print(f"model saved to {model_path}")
            episodic_returns = evaluate(q_network, args, f"{run_name}-eval", 10, device, epsilon=args.end_e)
            print(episodic_returns)
            writer.add_scalar("charts/offline/avg_episodic_return", np.mean(episodic_returns), global_step)


def online_phase(args, envs, learner, writer, teacher_episodic_returns):
    """The student acts and trains on its own buffer; the distillation weight decays with its returns (:349-437)."""
    start_time = time.time()
    obs, _ = envs.reset(seed=args.seed)
    episodic_returns = deque(maxlen=10)
    for global_step in range(args.total_timesteps):
        global_step += args.offline_steps
        epsilon = linear_schedule(args.start_e, args.end_e, args.exploration_fraction * args.total_timesteps, global_step)
        actions = learner.act(obs, global_step, epsilon)
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)

        if "final_info" in infos:
            for info in infos["final_info"]:
                if not info or "episode" not in info:
                    continue
                print(f"global_step={global_step}, episodic_return={info['episode']['r']}")
                writer.add_scalar("charts/episodic_return", info["episode"]["r"], global_step)
                writer.add_scalar("charts/episodic_length", info["episode"]["l"], global_step)
                writer.add_scalar("charts/epsilon", epsilon, global_step)
                episodic_returns.append(info["episode"]["r"])
                break

        learner.store(obs, real_next(next_obs, truncations, infos), actions, rewards, terminations)
        obs = next_obs

        if global_step > args.learning_starts:
            if global_step % args.train_frequency == 0:
                distill_coeff = distill_coefficient(episodic_returns, teacher_episodic_returns)
                learner.train_step(distill_coeff)
                if global_step % 100 == 0:
                    m = learner.metrics()
                    writer.add_scalar("losses/loss", m["loss"], global_step)
                    writer.add_scalar("losses/td_loss", m["q_loss"], global_step)
                    writer.add_scalar("losses/distill_loss", m["distill_loss"], global_step)
                    writer.add_scalar("losses/q_values", m["q_values"], global_step)
                    writer.add_scalar("charts/distill_coeff", distill_coeff, global_step)
                    print("SPS:", int(global_step / (time.time() - start_time)))
                    print(distill_coeff)
                    writer.add_scalar("charts/SPS", int(global_step / (time.time() - start_time)), global_step)
            if global_step % args.target_network_frequency == 0:
                learner.sync_target()


def main(argv=None):
    args = cli.parse(Args, argv)
    assert args.num_envs == 1, "vectorized envs are not supported at the moment"
    if args.teacher_policy_hf_repo is None:
        args.teacher_policy_hf_repo = f"cleanrl/{args.env_id}-{args.teacher_model_exp_name}-seed1"
    run_name = f"{args.env_id}__{args.exp_name}__{args.seed}__{int(time.time())}"
    writer = runner.open_writer(args, run_name)
    runner.seed_everything(args)
    device = runner.select_device(args)

    envs = make_envs(args, run_name, [args.seed + i for i in range(args.num_envs)])
    q_network = QNetwork(envs).to(device)
    target_network = QNetwork(envs).to(device)
    target_network.load_state_dict(q_network.state_dict())

    # QDAGGER LOGIC:
    teacher_model = load_teacher(args, envs, device)
    teacher_episodic_returns = evaluate(teacher_model, args, f"{run_name}-teacher-eval", args.teacher_eval_episodes, device, epsilon=args.end_e)
    writer.add_scalar("charts/teacher/avg_episodic_return", np.mean(teacher_episodic_returns), 0)

    learner = QDaggerLearner(q_network, target_network, teacher_model, args, envs, device)
    teacher_phase(args, envs, learner)
    offline_phase(args, learner, writer, run_name, device, q_network)

    envs = make_envs(args, run_name, [args.seed + i for i in range(args.num_envs)])
    learner.start_online_phase(envs)
    online_phase(args, envs, learner, writer, teacher_episodic_returns)

    if args.save_model:
        model_path = f"runs/{run_name}/{args.exp_name}.cleanrl_model"
        os.makedirs(os.path.dirname(model_path), exist_ok=True)
        torch.save(q_network.state_dict(), model_path)
        print(f"model saved to {model_path}")
        episodic_returns = evaluate(q_network, args, f"{run_name}-eval", 10, device, epsilon=args.end_e)
        for idx, episodic_return in enumerate(episodic_returns):
            writer.add_scalar("eval/episodic_return", episodic_return, idx)
        if args.upload_model:
            raise SystemExit("--upload-model needs network access and cleanrl_utils.huggingface; not available here")

    envs.close()
    writer.close()
    return learner


if __name__ == "__main__":
    main()
