"""``AtariDQNLearner`` (cleanrl_amd/learner_dqn_atari.py) on the CPU: the reference buffer's draws, the refusals, and one fused update
(host twins around torch's convolutions) against float64 autograd at DESIGN.md section 3.11's bar."""
import numpy as np
import pytest
import torch

import dqn_atari_cases as A

CPU = torch.device("cpu")


def test_sample_indices_reproduce_the_reference_draws():
    """Not full: ``randint(0, pos)``; full: ``(randint(1, slots) + pos) % slots``, never ``pos``; then ``env_indices``."""
    for backend in ("torch", "fused"):
        for steps in (3, 9):
            L, ref = A.make_learner(CPU, False, backend, M=8, slots=7), A.RefRing(7, 1)
            for s in A.ring_steps(7, 1, steps):
                step = [t.numpy() for t in s]
                step[2] = step[2] % 6
                L.store(*step), ref.add(*step)
            assert (L.pos, L.full) == (ref.pos, ref.full) and L.full == (steps >= 7)
            np.random.seed(5)
            bi, ei = L.sample_indices(64)
            np.random.seed(5)
            wb, we = ref.sample_indices(64)
            assert np.array_equal(bi, wb) and np.array_equal(ei, we) and (not L.full or L.pos not in bi)


def test_fused_store_keeps_the_reference_buffers_contents():
    L, T, ref = A.make_learner(CPU, False, "fused", M=8, slots=7), A.make_learner(CPU, False, "torch", M=8, slots=7), A.RefRing(7, 1)
    for s in A.ring_steps(7, 1, 10):
        step = [t.numpy() for t in s]
        L.store(*step), T.store(*step), ref.add(*step)
    assert torch.equal(L.ring[0], ref.frames_hwc()) and np.array_equal(T.rb.observations, ref.observations)
    assert torch.equal(L.ring[1], torch.from_numpy(ref.actions)) and np.array_equal(T.rb.actions[..., 0], ref.actions)


def test_sizes_outside_the_limits_and_a_ring_that_cannot_be_allocated_are_refused():
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        A.make_learner(CPU, True, "fused", n=18, n_atoms=57)
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        A.make_learner(CPU, False, "fused", M=1025)
    with pytest.raises(ValueError, match="at least 2 for c51"):
        A.make_learner(CPU, True, "fused", n_atoms=1)
    with pytest.raises(ValueError, match=r"--buffer-size.*MI355PPO_OFFPOLICY=torch"):
        A.make_learner(CPU, False, "fused", slots=10 ** 12)
    A.make_learner(CPU, True, "torch", n=18, n_atoms=57)                     # the torch backend has no such limits


@pytest.mark.parametrize("c51", [False, True])
def test_one_fused_update_on_the_cpu_against_float64(c51):
    """Gather, torch's convolutions, the head twins and ``h.backward(dh)``: the loss scalars and the whole flat gradient within twice
    the f32 torch reference's own error against float64 autograd, plus 2e-6."""
    L = A.make_learner(CPU, c51, "fused", M=8, slots=16, fill=True)
    bi, ei = np.arange(4, 12) % 16, np.zeros(8, np.int64)
    idx = L._stage_indices(bi, ei)
    L.update_kernels(idx[0], idx[1], adam=False)
    r64, r32 = A.reference_update(L, bi, ei, torch.float64), A.reference_update(L, bi, ei, torch.float32)
    for k, got in (("scalars", L._sc), ("grads", L.grads)):
        ok, err, own = A.within_bar(got, r64[k], r32[k])
        print(f"c51={c51} {k}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (k, err, own)


@pytest.mark.parametrize("c51", [False, True])
def test_both_backends_run_whole_steps_and_draw_the_same_streams(c51):
    """store / act / train_step / sync_target on both backends from one seed: the random-branch actions and the sampled indices are the
    same draws, the losses stay close (one trajectory up to rounding)."""
    import random

    out = {}
    for backend in ("torch", "fused"):
        random.seed(3), np.random.seed(3), torch.manual_seed(3)
        L = A.make_learner(CPU, c51, backend, M=4, slots=6)
        L.space.seed(3)
        acts, losses, seen = [], [], []
        real = L.sample_indices
        L.sample_indices = lambda m: (seen.append(real(m)), seen[-1])[1]
        for t, s in enumerate(A.ring_steps(6, 1, 9)):
            obs, nxt, _, rew, done = (x.numpy() for x in s)
            a = L.act(obs, t, 1.0 if t % 2 == 0 else 0.0)
            acts.append(a)
            L.store(obs, nxt, a, rew, done)
            if t >= 3:
                L.train_step()
                losses.append(L.metrics()["loss"])
                if t % 4 == 0:
                    L.sync_target()
        out[backend] = (acts, losses, seen)
    (ta, tl, ts), (fa, fl, fs) = out["torch"], out["fused"]
    assert all(np.array_equal(a, b) for a, b in zip(ta[::2], fa[::2]))       # the random branch: the action space's stream
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(ts, fs))
    assert np.allclose(tl, fl, rtol=1e-3, atol=1e-5) and np.isfinite(fl).all()
