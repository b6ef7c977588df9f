"""``cleanrl_amd.staging.Staging`` on the CPU, and ``store`` through it for one learner of each ring family: the ``fused`` ring equals
the ``torch`` backend's host buffer (the reference's add rule) after the ring has wrapped twice."""
import numpy as np
import pytest
import torch

import dqn_atari_cases as A
import staging_cases as C
from cleanrl_amd.learner_dqn_atari import AtariDQNLearner
from cleanrl_amd.learner_qdagger import QDaggerLearner
from cleanrl_amd.learner_sac_atari import SACAtariLearner
from cleanrl_amd.staging import Staging

CPU = torch.device("cpu")
SLOTS, M = 7, 4
STEPS = 2 * SLOTS + 3


def test_cpu_group_is_one_plain_host_set():
    st = Staging(CPU, a=((3, 2), torch.float32), b=((4,), torch.int64))
    assert st.events == [] and st.mirror is None and len(st.sets) == 1
    ptrs = set()
    for k in range(3):
        h = st.begin()
        assert not any(t.is_pinned() for t in h.values())
        h["a"].fill_(k), h["b"].fill_(k)
        out = st.push()
        assert {n: t.data_ptr() for n, t in out.items()} == {n: t.data_ptr() for n, t in h.items()}
        assert (out["a"] == k).all() and (out["b"] == k).all() and out["a"].shape == (3, 2) and out["b"].dtype == torch.int64
        ptrs.add((out["a"].data_ptr(), out["b"].data_ptr()))
    assert len(ptrs) == 1                                        # successive writes land in the same two tensors


def vector_steps():
    rng = np.random.default_rng(3)
    shape = (C.N_ENVS, C.O)
    return [(rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32), rng.integers(0, C.N_ACTIONS, C.N_ENVS),
             rng.standard_normal(C.N_ENVS).astype(np.float32), rng.random(C.N_ENVS) < 0.3) for _ in range(STEPS)]


def frame_steps(n=6):
    steps = [[x.numpy() for x in s] for s in A.ring_steps(SLOTS, 1, STEPS)]
    for s in steps:
        s[2] = s[2] % n
    return steps


@pytest.mark.parametrize("family", ["dqn", "dqn_atari", "sac_atari", "qdagger"])
def test_store_fills_the_fused_ring_as_the_host_buffer(family):
    if family == "dqn":
        (T, F), steps = [C.vector_learner(CPU, b, SLOTS, M) for b in ("torch", "fused")], vector_steps()
    else:
        (T, F), steps = [C.frame_learner(family, CPU, b, SLOTS, M) for b in ("torch", "fused")], frame_steps()
    assert F.slots == T.slots == SLOTS
    for step in steps:
        T.store(*step), F.store(*step)
    assert (F.pos, F.full) == (T.pos, T.full) == (STEPS % SLOTS, True)
    want = C.host_ring(T.rb)
    assert len(want) == len(F.ring)
    for got, ref in zip(F.ring, want):
        assert got.dtype == ref.dtype and torch.equal(got, ref)


def test_the_frame_learners_share_one_staging():
    assert AtariDQNLearner.store is SACAtariLearner.store is QDaggerLearner.store
    assert AtariDQNLearner._stage_frames is SACAtariLearner._stage_frames is QDaggerLearner._stage_frames
    for name in ("store", "_staging_free", "_staging_used"):
        assert name not in vars(QDaggerLearner)
