"""What tests/test_staging.py and tests/test_gpu_staging.py share: a small vector ``DQNLearner`` over several envs, one learner of each
frame-ring family, and the ``torch`` backend's host buffer in the device ring's layout."""
from types import SimpleNamespace

import torch

import dqn_atari_cases as A
import qdagger_cases as Q
import sac_atari_cases as S

O, N_ACTIONS, N_ENVS = 4, 2, 3                                    # the vector learner's sizes


def vector_learner(dev, backend, slots, M):
    from cleanrl_amd.agents import DQNNetwork
    from cleanrl_amd.envs import SamplingDiscrete
    from cleanrl_amd.learner_dqn import DQNLearner

    env = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(O,)), single_action_space=SamplingDiscrete(N_ACTIONS), num_envs=N_ENVS)
    args = SimpleNamespace(buffer_size=slots * N_ENVS, batch_size=M, learning_rate=2.5e-4, gamma=0.99, tau=1.0, n_atoms=1, v_min=-1, v_max=1)
    return DQNLearner(DQNNetwork(env).to(dev), DQNNetwork(env).to(dev), args, env, dev, c51=False, backend=backend)


def frame_learner(family, dev, backend, slots, M):
    if family == "dqn_atari":
        return A.make_learner(dev, False, backend, M=M, slots=slots)
    return {"sac_atari": S, "qdagger": Q}[family].make_learner(dev, backend, M=M, slots=slots)


def host_ring(rb):
    """The ``torch`` backend's buffer as the tensors of the ``fused`` ring: frames channels-last and the action column squeezed for the
    frame rings; obs | next_obs | float actions for the vector ring."""
    if rb.observations.ndim == 3:
        obs, actions = [torch.from_numpy(rb.observations), torch.from_numpy(rb.next_observations)], torch.from_numpy(rb.actions).float()
    else:
        hwc = lambda a: torch.from_numpy(a).permute(0, 1, 3, 4, 2)  # noqa: E731
        obs = [hwc(rb.observations)] + ([hwc(rb.next_observations)] if hasattr(rb, "next_observations") else [])
        actions = torch.from_numpy(rb.actions[:, :, 0])
    return obs + [actions, torch.from_numpy(rb.rewards), torch.from_numpy(rb.dones)]
