"""The staging contract on a GPU (cleanrl_amd/staging.py): behind a queued delay, with no synchronisation in
between, 16 ``store``s of pairwise distinct transitions fill a 16-slot ring exactly as the ``torch`` backend's host buffer is filled.
Every frame is a pattern of its step number and the pixel index, so a frame torn or repeated by a host write that overtook a copy in
flight cannot pass.  The race itself is a matter of timing and is not hunted for: this pins what the guard promises."""
import numpy as np
import pytest
import torch

import staging_cases as C
from cleanrl_amd.rainbow_replay import DevicePrioritizedReplay, HostPrioritizedReplay
from cleanrl_amd.staging import Staging

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
SLOTS = 16
DELAY_N, DELAY_REPS = 8192, 4                                    # four 8192^3 float32 matmuls: measured 29.6 ms on an MI355X


@pytest.fixture(scope="module")
def delay():
    a = torch.randn((DELAY_N, DELAY_N), device=DEV)
    out = torch.empty_like(a)
    torch.mm(a, a, out=out)                                      # the first call's set-up stays out of the queued delay
    torch.cuda.synchronize()

    def queue():
        for _ in range(DELAY_REPS):
            torch.mm(a, a, out=out)

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(), queue(), t1.record()
    torch.cuda.synchronize()
    print(f"queued delay: {t0.elapsed_time(t1):.1f} ms")
    return queue


def frame(k):
    """(1, 4, 84, 84) u8: pixel i of pattern k is ``(i * (2k + 3) + 41k) mod 251``; the patterns differ pairwise in most pixels."""
    i = np.arange(4 * 84 * 84, dtype=np.int64)
    return ((i * (2 * k + 3) + 41 * k) % 251).astype(np.uint8).reshape(1, 4, 84, 84)


def frame_steps(n=6):
    """obs | next_obs | action | reward | done of step k: patterns 2k and 2k + 1, all pairwise distinct but the two dones."""
    return [(frame(2 * k), frame(2 * k + 1), np.array([k % n]), np.array([0.25 * k - 1.0], np.float32), np.array([k % 3 == 2])) for k in range(SLOTS)]


def vector_steps():
    N, n = C.N_ENVS, C.N_ACTIONS
    cell = np.arange(N * C.O, dtype=np.float32).reshape(N, C.O)
    return [(100.0 * k + cell, 100.0 * k + 50.0 + cell, (np.arange(N) + k) % n, 0.25 * k - np.arange(N, dtype=np.float32), (np.arange(N) + k) % 3 == 2)
            for k in range(SLOTS)]


@pytest.mark.parametrize("family", ["dqn", "dqn_atari", "sac_atari", "qdagger"])
def test_back_to_back_stores_behind_a_delay_fill_the_ring_as_the_host_buffer(family, delay):
    M = 8
    if family == "dqn":
        T, F, steps, N = C.vector_learner(CPU, "torch", SLOTS, M), C.vector_learner(DEV, "fused", SLOTS, M), vector_steps(), C.N_ENVS
    else:
        T, F, steps, N = C.frame_learner(family, CPU, "torch", SLOTS, M), C.frame_learner(family, DEV, "fused", SLOTS, M), frame_steps(), 1
    assert F.slots == SLOTS and F.device.type == "cuda"
    bi, ei = (np.arange(M) * 5 + 3) % SLOTS, np.arange(M) % N
    torch.cuda.synchronize()
    delay()
    for k, step in enumerate(steps):                             # nothing below synchronises until the ring is full
        F.store(*step)
        if k == 5:
            idx = F._stage_indices(bi, ei)
        if k == 9:
            rows = F._stage_obs(step[0]) if family == "dqn" else F._stage_frames(step[0])
            staged = step[0]
    torch.cuda.synchronize()
    for step in steps:
        T.store(*step)
    assert (F.pos, F.full) == (T.pos, T.full) == (0, True)
    want = C.host_ring(T.rb)
    assert len(want) == len(F.ring)
    for got, ref in zip(F.ring, want):
        assert got.dtype == ref.dtype and torch.equal(got.cpu(), ref)
    assert idx.is_cuda and torch.equal(idx.cpu(), torch.from_numpy(np.stack([bi, ei])))
    want_rows = torch.from_numpy(np.ascontiguousarray(staged))
    assert rows.is_cuda and torch.equal(rows.cpu(), want_rows if family == "dqn" else want_rows.permute(0, 2, 3, 1))


def test_back_to_back_adds_behind_a_delay_fill_the_prioritized_rings_as_the_host_buffer(delay):
    """``n_step=1``: the n-step window passes every transition through, so what is compared is what the add writes."""
    host = HostPrioritizedReplay(SLOTS, (4, 84, 84), 1, 0.99, 0.5, 0.4, 1e-6)
    dev = DevicePrioritizedReplay(SLOTS, DEV, 1, 0.99, 0.5, 0.4, 1e-6)
    steps = [(o, a, r, nxt, d) for o, nxt, a, r, d in frame_steps()]
    torch.cuda.synchronize()
    delay()
    for step in steps:
        assert dev.add(*step)
    torch.cuda.synchronize()
    for step in steps:
        assert host.add(*step)
    assert (dev.pos, dev.size) == (host.pos, host.size) == (0, SLOTS)
    hwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1)  # noqa: E731
    buf = [t.cpu() for t in dev.buf[:5]]
    assert torch.equal(buf[0], hwc(host.obs)) and torch.equal(buf[1], hwc(host.next_obs))
    assert torch.equal(buf[2], torch.from_numpy(host.actions))
    assert torch.equal(buf[3].view(torch.int32), torch.from_numpy(host.rewards).view(torch.int32))
    assert torch.equal(buf[4], torch.from_numpy(host.dones).float())


def test_a_set_is_rewritten_only_after_its_copy_has_left_it(delay):
    st = Staging(DEV, x=((1 << 20,), torch.int32))
    assert len(st.sets) == len(st.events) == 2 and all(t.is_pinned() for s in st.sets for t in s.values())
    torch.cuda.synchronize()
    delay()
    first = None
    for k in (1, 2, 3):
        h = st.begin()
        if k == 1:
            first = st.turn
        if k == 3:                                               # the first push's set has come round again
            assert st.turn == first and st.events[first].query()
            seen = st.mirror["x"].clone()                        # behind the second push's copy on the stream; the third is not issued yet
        h["x"].fill_(k)
        out = st.push()
        assert out["x"] is st.mirror["x"]
    torch.cuda.synchronize()
    assert (seen == 2).all()                                     # the second push whole: never the first, never a mix
    assert (st.mirror["x"] == 3).all()
