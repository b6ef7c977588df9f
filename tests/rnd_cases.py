"""Shared cases of the RND operators (csrc/rnd.hip): inputs, independent restatements of the reference's lines
(ppo_rnd_envpool.py:365-373, :390-400, :463-472, :512) in numpy / torch, and one runner that puts a case's tensors where the caller
says -- plain tensors of a device, or carves of a guard-band arena -- so that the twins, the device entry points and the
guard-band tests all run the same cases.  References are computed once per case and cached."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden
from cleanrl_amd.learner_rnd import RunningMeanStd

P = 84 * 84
NORMALIZE_M = (1, 3, 67)
MOMENT_B = (1, 2, 65, 257)              # one row, two, one more than a wave of rows, one more than a 256-row slab
MOMENT_B_SATURATED = 4099               # 16 slabs and 3 rows of all-255 frames: the largest sums a slab can hold
MOMENT_CASES = tuple((B, nhwc) for B in MOMENT_B for nhwc in (True, False)) + ((MOMENT_B_SATURATED, True),)
INTRINSIC_N = (1, 63, 65)               # one row, a ragged last workgroup of 4 rows, one row past 16 workgroups
FILTER_SHAPES = ((1, 1), (128, 3), (5, 130))
LOSS_M = (1, 2, 63, 257)                # ragged workgroups of 4 rows; 257: one row past the fold's 256 slots
LOSS_MASKS = (("none", 0.0), ("all", 1.0), ("quarter", 0.25))


def golden():
    return load_golden("rnd_iteration")["rnd_T8_N4"]


def to_nhwc(rows_nchw):
    return rows_nchw.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------- a. normalise
@functools.lru_cache(maxsize=None)
def normalize_case(M: int, gather: bool):
    """rows (B, 4, 84, 84) u8, float64 mean / var with variances small enough for both clips, pixels landing exactly on +-5, and
    (gather) an index that repeats rows and is out of order."""
    g = torch.Generator().manual_seed(100 + M + 7 * gather)
    B = 5 if gather else M
    rows = torch.randint(0, 256, (B, 4, 84, 84), generator=g, dtype=torch.uint8)
    mean = torch.rand(P, generator=g, dtype=torch.float64) * 255.0
    var = torch.rand(P, generator=g, dtype=torch.float64) * 400.0 + 1e-3
    var[::7] = 1e-2                                              # sd 0.1: both clips fire
    idx = torch.randint(0, B, (M,), generator=g) if gather else None
    if gather and M >= 3:
        idx[0], idx[1], idx[2] = 4, 0, 4
    first = int(idx[0]) if gather else 0
    x = rows[first, 3].reshape(-1).double()
    for k, (sd, z) in enumerate(((1.0, 5.0), (1.0, -5.0), (0.5, 5.0), (4.0, -5.0))):      # exactly representable: lands on the bound
        p = 11 + 13 * k
        var[p] = sd * sd
        mean[p] = x[p] - z * sd
    want64 = (rows[:, 3].reshape(B, 1, 84, 84) - mean.reshape(1, 1, 84, 84)) / torch.sqrt(var).reshape(1, 1, 84, 84)
    if gather:
        want64 = want64[idx]
    return dict(rows=rows, mean=mean, sd=torch.sqrt(var), idx=idx, preclip=want64, want=want64.clip(-5, 5).float())


def run_normalize(mod, c, nhwc, put, out_of):
    rows = put(to_nhwc(c["rows"]) if nhwc else c["rows"], "rows")
    idx = None if c["idx"] is None else put(c["idx"], "idx")
    M = c["want"].shape[0]
    return mod.rnd_normalize(rows, put(c["mean"], "mean"), put(c["sd"], "sd"), idx=idx, out=out_of((M, 1, 84, 84), torch.float32, "out"), nhwc=nhwc)


# ---------------------------------------------------------------------------------------------- b. moments
@functools.lru_cache(maxsize=None)
def moments_case(B: int):
    if B == MOMENT_B_SATURATED:
        return dict(rows=torch.full((B, 4, 84, 84), 255, dtype=torch.uint8), S1=np.full(P, 255 * B, np.uint64), S2=np.full(P, 65025 * B, np.uint64))
    g = torch.Generator().manual_seed(200 + B)
    rows = torch.randint(0, 256, (B, 4, 84, 84), generator=g, dtype=torch.uint8)
    x = rows[:, 3].reshape(B, P).numpy().astype(np.uint64)
    return dict(rows=rows, S1=x.sum(0), S2=(x * x).sum(0))


def run_moments(mod, c, nhwc, put, out_of):
    sums = out_of((2, P), torch.int64, "sums")
    sums.fill_(-0x0123456789ABCDEF)                              # garbage: the result must not depend on it
    return mod.rnd_obs_moments(put(to_nhwc(c["rows"]) if nhwc else c["rows"], "rows"), sums, nhwc=nhwc)


# ---------------------------------------------------------------------------------------------- c. intrinsic reward
@functools.lru_cache(maxsize=None)
def intrinsic_case(N: int):
    g = torch.Generator().manual_seed(300 + N)
    t, p = torch.randn(N, 512, generator=g), torch.randn(N, 512, generator=g) * 0.5
    return dict(target=t, predict=p, want64=(t.double() - p.double()).pow(2).sum(1) / 2)


def run_intrinsic(mod, c, put, out_of):
    return mod.rnd_intrinsic_reward(put(c["target"], "target"), put(c["predict"], "predict"), out_of((c["target"].shape[0],), torch.float32, "out"))


# ---------------------------------------------------------------------------------------------- d. reward filter
def reference_filter(raw, rewems, rms, gamma):
    """Lines :390-400 as written, on a (T, N) f32 numpy array: the Python loop over ``raw.T`` (so the filter runs along the env
    axis), float64 moments, ``update_from_moments`` with ``len()``.  -> (filtered (T, N), rewems (T,), scaled torch (T, N))."""
    per_env = []
    for rews in raw.T:
        rewems = rews if rewems is None else rewems * gamma + rews
        per_env.append(rewems)
    per_env = np.array(per_env)
    x = per_env.astype(np.float64)
    rms.update_from_moments(np.mean(x), np.var(x), len(per_env))
    scaled = torch.from_numpy(raw.copy())
    scaled /= np.sqrt(rms.var)
    return per_env.T.copy(), rewems, scaled


@functools.lru_cache(maxsize=None)
def filter_case(T: int, N: int, golden_raw: bool = False):
    """Two consecutive rollouts of raw intrinsic rewards with the reference's results after each."""
    g = torch.Generator().manual_seed(400 + 131 * T + N)
    raws = [(torch.rand(T, N, generator=g) * 3.0 + 0.01).numpy() for _ in range(2)]
    if golden_raw:
        raws[0] = golden()["raw_curiosity"].copy()
    rms, rewems, steps = RunningMeanStd(), None, []
    for raw in raws:
        filtered, rewems, scaled = reference_filter(raw, rewems, rms, 0.99)
        steps.append(dict(raw=raw, filtered=filtered, rewems=rewems.copy(), scaled=scaled, stats=(float(rms.mean), float(rms.var), float(rms.count))))
    return steps


def run_filter(mod, steps, put, out_of):
    """Both rollouts, the state carried on the device -> [(scaled, filtered, rewems, stats) clones]."""
    T, N = steps[0]["raw"].shape
    rewems = put(torch.zeros(T), "rewems")
    stats = put(torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64), "stats")
    outs = []
    for k, s in enumerate(steps):
        cur = put(torch.from_numpy(s["raw"].copy()), f"curiosity{k}")
        filtered = out_of((T, N), torch.float32, f"filtered{k}")
        mod.rnd_reward_filter_(cur, rewems, stats, 0.99, filtered)
        outs.append(tuple(t.clone() for t in (cur, filtered, rewems, stats)))
    return outs


# ---------------------------------------------------------------------------------------------- e. loss
def reference_loss(c, dtype):
    """:463-472 and :512 with autograd, in ``dtype``; the mask is drawn in f32 as the reference's ``torch.rand`` is."""
    p = c["predict"].to(dtype).requires_grad_(True)
    v = c["v_int"].to(dtype).requires_grad_(True)
    forward_loss = F.mse_loss(p, c["target"].to(dtype), reduction="none").mean(-1)
    mask = (c["u"] < c["proportion"]).to(dtype)
    forward_loss = (forward_loss * mask).sum() / torch.max(mask.sum(), torch.tensor([1], dtype=dtype))
    int_v_loss = 0.5 * ((v - c["int_returns"].to(dtype)[c["idx"]]) ** 2).mean()
    (int_v_loss * c["vf_coef"] + forward_loss.view(())).backward()
    return dict(scalars=torch.stack([int_v_loss.detach(), forward_loss.detach().view(())]), d_predict=p.grad, d_v_int=v.grad)


@functools.lru_cache(maxsize=None)
def loss_case(M: int, mask: str):
    g = torch.Generator().manual_seed(500 + M)
    B = 3 * M + 2
    c = dict(predict=torch.randn(M, 512, generator=g), target=torch.randn(M, 512, generator=g) * 0.7, u=torch.rand(M, generator=g),
             proportion=dict(LOSS_MASKS)[mask], v_int=torch.randn(M, generator=g), int_returns=torch.randn(B, generator=g) * 2.0,
             idx=torch.randperm(B, generator=g)[:M].contiguous(), vf_coef=0.5)
    c["ref64"], c["ref32"] = reference_loss(c, torch.float64), reference_loss(c, torch.float32)
    return c


def run_loss(mod, c, put, out_of):
    M = c["predict"].shape[0]
    sc, dp, dv = mod.rnd_loss_fwd_bwd(put(c["predict"], "predict"), put(c["target"], "target"), put(c["u"], "u"), c["proportion"],
                                      put(c["v_int"], "v_int"), put(c["int_returns"], "int_returns"), put(c["idx"], "idx"), c["vf_coef"],
                                      scalars=out_of((2,), torch.float32, "scalars"), d_predict=out_of((M, 512), torch.float32, "d_predict"),
                                      d_v_int=out_of((M,), torch.float32, "d_v_int"))
    return dict(scalars=sc, d_predict=dp, d_v_int=dv)


# ---------------------------------------------------------------------------------------------- placement
def plain(dev):
    """(put, out_of) for ordinary tensors of ``dev``."""
    return (lambda t, name: t.to(dev).contiguous()), (lambda shape, dtype, name: torch.empty(shape, dtype=dtype, device=dev))


def carved(arena):
    """(put, out_of) for carves of a guard-band arena (tests/guard_arena.py): inputs end at their last element, outputs too."""
    return (lambda t, name: arena.input(t.contiguous(), arena.stage + name)), (lambda shape, dtype, name: arena.carve(shape, dtype, arena.stage + name))


def every_entry_point(mod, put, out_of, stage=lambda name: None):
    """The small cases of all five operators through ``mod`` -> {name: tensor}: what the guard-band tests and the stream test
    compare between two runs."""
    out = {}
    for nhwc in (True, False):
        for gather in (False, True):
            stage(f"normalize nhwc={nhwc} gather={gather}")
            out[f"normalize {nhwc} {gather}"] = run_normalize(mod, normalize_case(3, gather), nhwc, put, out_of)
        stage(f"moments nhwc={nhwc}")
        out[f"moments {nhwc}"] = run_moments(mod, moments_case(257), nhwc, put, out_of)
    stage("intrinsic")
    out["intrinsic"] = run_intrinsic(mod, intrinsic_case(65), put, out_of)
    stage("filter")
    for k, o in enumerate(run_filter(mod, filter_case(5, 130), put, out_of)):
        for name, t in zip(("scaled", "filtered", "rewems", "stats"), o):
            out[f"filter {k} {name}"] = t
    for mask, _ in LOSS_MASKS:
        stage(f"loss {mask}")
        for k, v in run_loss(mod, loss_case(63, mask), put, out_of).items():
            out[f"loss {mask} {k}"] = v
    return out
