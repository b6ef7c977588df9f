"""``RainbowLearner`` (cleanrl_amd/learner_rainbow.py) on the CPU: the ``fused`` backend through the host twins beside the ``torch``
backend (the reference's ops), teacher-forced with one noise and one set of draws; the random streams both consume; refusals."""
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rainbow_replay import assert_lockstep, fill, lockstep_updates, make_learner

CPU = torch.device("cpu")


@pytest.mark.parametrize("n_atoms", [5, 51])
def test_fused_on_the_twins_keeps_step_with_the_torch_backend(n_atoms):
    T, F, out = lockstep_updates(CPU, n_atoms)
    assert_lockstep(out)
    (to, tt), (fo, ft) = T.flat_params(), F.flat_params()
    assert torch.allclose(fo, to, rtol=1e-3, atol=1e-5) and torch.allclose(ft, tt, rtol=1e-3, atol=1e-5)
    assert abs(F.rb.max_priority - float(T.rb.max_priority)) <= 1e-3 * float(T.rb.max_priority)
    assert T.step == F.step == 4


def test_both_backends_consume_the_same_random_streams():
    """A free-running update: two ``reset_noise`` (online, then target) and ``batch_size`` uniform draws leave torch's generator and
    ``np.random`` in the same state on both backends, and draw the same noise."""
    states = []
    for backend in ("torch", "fused"):
        L = make_learner(CPU, backend)
        obs = fill(L, 22)
        torch.manual_seed(5), np.random.seed(5), random.seed(5)
        a = L.act(obs)
        L.train_step()
        states.append((a, torch.get_rng_state(), np.random.get_state()[1].copy(), random.getstate(),
                       L.q_network.value_head[0].weight_epsilon.clone(), L.target_network.advantage_head[2].bias_epsilon.clone()))
    (a0, t0, n0, r0, e0, f0), (a1, t1, n1, r1, e1, f1) = states
    assert np.array_equal(a0, a1) and a0.dtype == a1.dtype == np.int64
    assert torch.equal(t0, t1) and np.array_equal(n0, n1) and r0 == r1 and torch.equal(e0, e1) and torch.equal(f0, f1)


def test_act_is_the_argmax_of_the_noisy_online_network_in_training_mode():
    for backend in ("torch", "fused"):
        L = make_learner(CPU, backend, n_atoms=51)
        obs = fill(L, 3)
        assert L.q_network.training
        with torch.no_grad():
            q = (L.q_network(torch.Tensor(obs)) * L.q_network.support).sum(2)
        assert np.array_equal(L.act(obs), q.argmax(1).numpy())


def test_out_of_limit_sizes_and_shapes_are_refused():
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        make_learner(CPU, "fused", n_atoms=102)
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        make_learner(CPU, "fused", n=19)
    make_learner(CPU, "torch", n_atoms=102)
    with pytest.raises(ValueError, match="backend"):
        make_learner(CPU, "eager")
