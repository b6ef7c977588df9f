"""Out-of-range replay indices on the host twins: ``op_clamp`` (csrc/offpolicy_rows.h) clamps ``batch_inds`` into ``[0, slots)`` and
``env_inds`` into ``[0, n_envs)``.  It is memory safety only: the clamped call returns the bits of the call with the
clamped indices written out, and reads nothing outside the ring."""
import torch

import offpolicy_cases as C
from cleanrl_amd import host_ops as H


def test_out_of_range_indices_are_clamped_into_the_ring():
    c = C.make_case(17, 6, 40, N=2, slots=9)
    want = C.run_entry_points(H, c, torch.device("cpu"))
    bi, ei = c.bi.clone(), c.ei.clone()
    tail = torch.arange(c.M) >= 11                               # the case builder gathers its rollout rows by the first 11 itself
    low_b, high_b, low_e, high_e = (m & tail for m in (bi == 0, bi == c.slots - 1, ei == 0, ei == c.N - 1))
    assert low_b.any() and high_b.any() and low_e.any() and high_e.any()
    bi[low_b], bi[high_b] = -3, c.slots + 1000
    ei[low_e], ei[high_e] = -1, c.N
    c.bi, c.ei = bi, ei
    got = C.run_entry_points(H, c, torch.device("cpu"))
    for k in ("y", "next_actions", "critic_grads", "critic_scalars", "actor_grads", "actor_loss", "dq_daction"):
        assert C.same(got[k], want[k]), k
