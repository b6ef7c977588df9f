"""The RND operators (csrc/rnd.hip), each defined once for the HIP entry point and its host twin, as the replay-ring
operators are (cleanrl_amd/replay_ops.py, whose ``Side`` this module takes): ``cleanrl_amd.ops`` and ``cleanrl_amd.host_ops`` bind
them to their side at import.  Nothing is coerced or copied; every check runs before the C call.
"""
from __future__ import annotations

import types

import numpy as np
import torch

from .replay_ops import _ptr

OPERATORS = ("rnd_normalize", "rnd_obs_moments", "rnd_intrinsic_reward", "rnd_reward_filter_", "rnd_loss_fwd_bwd",
             "leaky_relu_fwd", "leaky_relu_bwd")

RND_PIXELS, RND_FEATURES, RND_MAX_BATCH, RND_MAX_STEPS = 84 * 84, 512, 1 << 24, 1024
LEAKY_SLOPE = 0.01             # nn.LeakyReLU's default negative_slope (RNDModel's predictor / target)
_AMAX_WORDS = 256              # MI355PPO_AMAX_WORDS: uint32 words of an amax record (csrc/f16split.h)


def bind(side, namespace: dict) -> None:
    for name in OPERATORS:
        namespace[name] = types.MethodType(globals()[name], side)


def _frame(s, rows, nhwc: bool):
    """Observation rows of 4 stacked 84 x 84 frames, u8 -> (B, row_bytes, pixel_stride, byte_offset) of the newest frame."""
    B = rows.shape[0]
    s.chk(rows, torch.uint8, "rows", (B, 84, 84, 4) if nhwc else (B, 4, 84, 84))
    return B, 4 * RND_PIXELS, (4 if nhwc else 1), (3 if nhwc else 3 * RND_PIXELS)


def rnd_normalize(s, rows, mean, sd, idx=None, out=None, nhwc: bool = True):
    """``((x[:, 3] - mean) / sd).clip(-5, 5).float()`` in the reference's float64 with one rounding (ppo_rnd_envpool.py:365-370,
    :449-454) -> (M, 1, 84, 84) f32; ``idx`` (int64, optional) gathers rows; ``mean`` / ``sd``: float64, 7056 elements."""
    B, row_bytes, stride, off = _frame(s, rows, nhwc)
    mean = s.chk(mean.reshape(-1), torch.float64, "mean", (RND_PIXELS,))
    sd = s.chk(sd.reshape(-1), torch.float64, "sd", (RND_PIXELS,))
    M = B
    if idx is not None:
        (M,) = idx.shape
        s.chk(idx, torch.int64, "idx", (M,))
    if out is None:
        out = torch.empty((M, 1, 84, 84), dtype=torch.float32, device=rows.device)
    s.chk(out, torch.float32, "out", (M, 1, 84, 84))
    s.launch("mi355ppo_rnd_normalize_u8_f32", rows.device, _ptr(rows), B, row_bytes, stride, off, _ptr(idx), _ptr(mean), _ptr(sd), _ptr(out), M)
    return out


def rnd_obs_moments(s, rows, sums=None, nhwc: bool = True):
    """Exact per-pixel ``sum x`` and ``sum x^2`` of the newest frame over all rows -> sums (2, 7056) int64 (the C ABI's uint64:
    the values stay below 2^63), overwritten.  ``rnd_mean_var`` turns them into the batch mean and variance."""
    B, row_bytes, stride, off = _frame(s, rows, nhwc)
    if B >= RND_MAX_BATCH:
        raise ValueError(f"rnd_obs_moments: {B} rows: B * S2 - S1^2 is exact in 64 bits only for B < 2^24")
    if sums is None:
        sums = torch.empty((2, RND_PIXELS), dtype=torch.int64, device=rows.device)
    s.chk(sums, torch.int64, "sums", (2, RND_PIXELS))
    s.launch_ws("mi355ppo_rnd_obs_moments_u8", rows.device, "mi355ppo_rnd_obs_moments_workspace_bytes", (B,), _ptr(rows), B, row_bytes, stride,
                off, _ptr(sums))
    return sums


def rnd_mean_var(sums, B: int):
    """(mean, var) float64 arrays of 7056 from the exact sums of ``B`` rows: ``S1 / B`` and ``(B S2 - S1^2) / B^2`` with the
    numerator formed in 64-bit integers -- one rounding each.  ``S1 < 2^32`` and ``B^2 < 2^48`` are exact in float64; a numerator
    of 2^53 or more (possible from about 372,000 rows on) would round on its way to float64 before the division rounds again, so
    those elements are divided as Python integers, whose true division rounds once."""
    B = int(B)
    if not 0 < B < RND_MAX_BATCH:
        raise ValueError(f"rnd_mean_var: {B} rows: B * S2 - S1^2 is exact in 64 bits only for 0 < B < 2^24")
    S = sums.detach().cpu().numpy().astype(np.uint64)
    num = np.uint64(B) * S[1] - S[0] * S[0]
    var = num.astype(np.float64) / np.float64(B * B)
    for p in np.nonzero(num >= np.uint64(1 << 53))[0]:
        var[p] = int(num[p]) / (B * B)
    return S[0].astype(np.float64) / np.float64(B), var


def rnd_intrinsic_reward(s, target, predict, out=None):
    """``(target - predict).pow(2).sum(1) / 2`` (:373) over 512 features in one fixed order -> out (N,)."""
    N, F = target.shape
    s.chk(target, torch.float32, "target", (N, F))
    s.chk(predict, torch.float32, "predict", (N, F))
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=target.device)
    s.chk(out, torch.float32, "out", (N,))
    s.launch("mi355ppo_rnd_intrinsic_reward_f32", target.device, _ptr(target), _ptr(predict), _ptr(out), N, F)
    return out


def rnd_reward_filter_(s, curiosity, rewems, stats, gamma: float, filtered_out=None):
    """:390-400 in one call, in place: the reward filter along the env axis (state ``rewems`` (T,) f32), the running statistics
    ``stats`` = (mean, var, count) float64 updated from the filtered values' moments with count N, ``curiosity`` (T, N) divided by
    ``(float)sqrt(var)``.  ``filtered_out`` (T, N), optional: the filtered values."""
    T, N = curiosity.shape
    s.chk(curiosity, torch.float32, "curiosity", (T, N))
    s.chk(rewems, torch.float32, "rewems", (T,))
    s.chk(stats, torch.float64, "stats", (3,))
    if filtered_out is not None:
        s.chk(filtered_out, torch.float32, "filtered_out", (T, N))
    s.launch("mi355ppo_rnd_reward_filter_f32", curiosity.device, _ptr(curiosity), _ptr(rewems), _ptr(stats), _ptr(filtered_out), T, N,
             float(gamma))
    return curiosity


def rnd_loss_fwd_bwd(s, predict, target, u, update_proportion: float, v_int, int_returns, mb_inds, vf_coef: float, scalars=None,
                     d_predict=None, d_v_int=None):
    """The masked distillation loss and the intrinsic value loss of a minibatch (:463-472, :512) with their gradients ->
    (scalars (2,) = {int_v_loss, fwd_loss}, d_predict (M, 512), d_v_int (M,)): the gradients of
    ``vf_coef * int_v_loss + fwd_loss``; ``mask = u < update_proportion``."""
    M, F = predict.shape
    dev = predict.device
    s.chk(predict, torch.float32, "predict", (M, F))
    s.chk(target, torch.float32, "target", (M, F))
    s.chk(u, torch.float32, "u", (M,))
    s.chk(v_int, torch.float32, "v_int", (M,))
    B = int_returns.numel()
    s.chk(int_returns, torch.float32, "int_returns", (B,))
    s.chk(mb_inds, torch.int64, "mb_inds", (M,))
    if scalars is None:
        scalars = torch.empty(2, dtype=torch.float32, device=dev)
    if d_predict is None:
        d_predict = torch.empty((M, F), dtype=torch.float32, device=dev)
    if d_v_int is None:
        d_v_int = torch.empty(M, dtype=torch.float32, device=dev)
    s.chk(scalars, torch.float32, "scalars", (2,))
    s.chk(d_predict, torch.float32, "d_predict", (M, F))
    s.chk(d_v_int, torch.float32, "d_v_int", (M,))
    s.launch_ws("mi355ppo_rnd_loss_fwd_bwd_f32", dev, "mi355ppo_rnd_loss_workspace_bytes", (M,), _ptr(predict), _ptr(target), _ptr(u),
                float(update_proportion), _ptr(v_int), _ptr(int_returns), _ptr(mb_inds), B, float(vf_coef), _ptr(scalars), _ptr(d_predict),
                _ptr(d_v_int), M, F)
    return scalars, d_predict, d_v_int


# ------------------------------------------------------------------------------------------- LeakyReLU (csrc/leaky.hip)
def _leaky_tail(s, n, bits, amax):
    if bits is not None:
        s.chk(bits, torch.int32, "bits", ((n + 31) // 32,))
    if amax is not None:
        s.chk(amax, torch.int32, "amax record", (_AMAX_WORDS,))


def leaky_relu_fwd(s, z, out=None, bits=None, amax=None, slope: float = LEAKY_SLOPE):
    """``torch.nn.functional.leaky_relu(z, slope)`` in f32, bit for bit -> ``out`` (``z``'s shape; may be ``z`` itself).  ``bits``
    (optional, int32, ``(n + 31) // 32`` words): bit b of word w = ``z > 0`` of flat element 32 w + b.  ``amax`` (optional): ``out``'s
    amax record, zeroed by the caller; ``max |out|`` is folded into it."""
    n = z.numel()
    s.chk(z, torch.float32, "z")
    if n == 0:
        raise ValueError("leaky_relu_fwd: empty tensor")
    out = torch.empty_like(z) if out is None else out
    s.chk(out, torch.float32, "out", z.shape)
    _leaky_tail(s, n, bits, amax)
    s.launch("mi355ppo_leaky_relu_fwd_f32", z.device, _ptr(z), _ptr(out), _ptr(bits), _ptr(amax), n, float(slope))
    return out


def leaky_relu_bwd(s, da, bits, out=None, amax=None, slope: float = LEAKY_SLOPE):
    """``dz = bit ? da : da * (float)slope`` with the forward's ``bits`` -> ``out`` (``da``'s shape; may be ``da`` itself): the gradient
    of ``leaky_relu_fwd``, torch's bits.  ``amax`` (optional): ``out``'s amax record."""
    n = da.numel()
    s.chk(da, torch.float32, "da")
    if n == 0:
        raise ValueError("leaky_relu_bwd: empty tensor")
    if bits is None:
        raise TypeError("leaky_relu_bwd: the forward's mask bits are required")
    out = torch.empty_like(da) if out is None else out
    s.chk(out, torch.float32, "out", da.shape)
    _leaky_tail(s, n, bits, amax)
    s.launch("mi355ppo_leaky_relu_bwd_f32", da.device, _ptr(da), _ptr(bits), _ptr(out), _ptr(amax), n, float(slope))
    return out
