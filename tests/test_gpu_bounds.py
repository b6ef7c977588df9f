"""The guard-band cases (tests/bounds_cases.py) on the device: every input, output, wrapper-owned buffer and workspace of an entry
point carved at its exact size out of one sentinel-filled allocation (tests/guard_arena.py) -- no word outside them may change,
and no result may depend on what the words that nobody wrote hold.  With the two entry points that had no test of their own."""
import numpy as np
import pytest
import torch

import bounds_cases as BC
import offpolicy_cases as C
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("case", BC.CASES, ids=[c.name for c in BC.CASES])
def test_entry_point_stays_inside_its_tensors_and_reads_only_what_was_written(case, monkeypatch):
    BC.check(case, ops, DEV, monkeypatch)


@pytest.mark.parametrize("rows", [1, 3, 257])          # one row; a ragged few; past one 256-thread block
@pytest.mark.parametrize("hw", [(2, 2), (84, 84)])     # one pixel quad; the workload's plane
def test_obs_shift_append_is_the_frame_stack_shift(rows, hw):
    """``out[r] = concat(prev[r][..., 1:4], newest[r][..., None])`` in the rows' (H, W, 4) layout: tests/test_pipeline.py's
    ``np.concatenate([prev[:, 1:], obs[:, 3:4]], axis=1)`` with the channel axis last."""
    g = torch.Generator().manual_seed(rows + hw[0])
    prev = torch.randint(0, 256, (rows, *hw, 4), dtype=torch.uint8, generator=g)
    newest = torch.randint(0, 256, (rows, *hw), dtype=torch.uint8, generator=g)
    out = torch.full((rows, *hw, 4), 0x5A, dtype=torch.uint8, device=DEV)
    ops.obs_shift_append_u8(prev.to(DEV), newest.to(DEV), out)
    assert torch.equal(out.cpu(), torch.cat([prev[..., 1:], newest[..., None]], -1))


def _synth_step64(state, reset, At, Bm, w, noise_k, steps, horizon, action):
    """One step of the formula of csrc/synth_env.hip's header comment in float64 numpy -> (state, reward, done, steps)."""
    state, reset, At, Bm, w, noise_k, steps, action = (t.numpy().astype(np.float64) for t in (state, reset, At, Bm, w, noise_k, steps, action))
    a = np.clip(action, -1, 1)
    nxt = noise_k + state @ At + a @ Bm
    reward = nxt @ w - 0.1 * (a * a).sum(1)
    t = steps + 1
    done = t >= horizon
    return np.where(done[:, None], reset, nxt), reward, done.astype(np.float32), np.where(done, 0, t).astype(np.float32)


def _synth_step32(state, reset, At, Bm, w, noise_k, steps, horizon, action):
    """The same step as f32 torch ops (what the env was before the kernel) -> (state, reward)."""
    a = action.clamp(-1, 1)
    nxt = noise_k + state @ At + a @ Bm
    reward = nxt @ w - 0.1 * (a * a).sum(1)
    done = steps + 1 >= horizon
    return torch.where(done[:, None], reset, nxt), reward


@pytest.mark.parametrize("alias", [True, False], ids=["obs_is_state", "separate_obs_row"])
@pytest.mark.parametrize("O,D", [(17, 6), (32, 8), (1, 1)])
@pytest.mark.parametrize("N", [1, 8, 9, 300])          # one env; a full block of 8 half-waves; one past it; 38 blocks, the last of 4 envs
def test_synth_continuous_step_against_float64(N, O, D, alias):
    """Twelve steps at horizon 5: the truncation and the reset are taken twice.  ``done`` and ``steps`` exactly; the states and
    rewards of the twelve steps within the project's bar (twice the deviation from float64 of the same formula as f32 torch ops,
    plus its floor).  Every step's references start from the kernel's own previous state: the bar is that of a step, the map's
    growth of an earlier rounding does not enter."""
    g = torch.Generator().manual_seed(N * 100 + O)
    state0, reset = torch.randn((N, O), generator=g), torch.randn((N, O), generator=g)
    At, Bm, w = torch.randn((O, O), generator=g) / max(O, 1) ** 0.5, torch.randn((D, O), generator=g), torch.randn(O, generator=g)
    noise = torch.randn((3, N, O), generator=g) * 0.1
    actions = [torch.randn((N, D), generator=g) * 1.5 for _ in range(12)]                      # a good share outside [-1, 1]
    assert any((a.abs() > 1).any() for a in actions)
    d = lambda t: t.to(DEV)  # noqa: E731
    state, steps = d(state0).clone(), torch.zeros(N, device=DEV)
    obs_row = state if alias else torch.full((N, O), float("nan"), device=DEV)
    reward, done = torch.full((N,), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    dAt, dBm, dw, dnoise, dreset = d(At), d(Bm), d(w), d(noise), d(reset)
    got, ref64, ref32, n_done = ([], []), ([], []), ([], []), 0
    for k, action in enumerate(actions):
        args = (state.cpu().clone(), reset, At, Bm, w, noise[k % 3], steps.cpu().clone(), 5.0, action)
        ops.synth_continuous_step(state, dreset, dAt, dBm, dw, dnoise, k, steps, 5.0, d(action), obs_row, reward, done)
        s64, r64, d64, t64 = _synth_step64(*args)
        s32, r32 = _synth_step32(*args)
        assert np.array_equal(done.cpu().numpy(), d64) and np.array_equal(steps.cpu().numpy(), t64), f"step {k}"
        assert torch.equal(obs_row, state)
        for i, (a, b, c) in enumerate(((state, s64, s32), (reward, r64, r32))):
            got[i].append(a.cpu().clone()), ref64[i].append(torch.from_numpy(b)), ref32[i].append(c)
        n_done += int(d64.sum())
    assert n_done == 2 * N
    for i, name in enumerate(("state", "reward")):
        ok, err, own = C.within_bar(torch.stack(got[i]), torch.stack(ref64[i]), torch.stack(ref32[i]))
        assert ok, f"{name}: err {err:.3e} against float64, the f32 formula's own {own:.3e}"
