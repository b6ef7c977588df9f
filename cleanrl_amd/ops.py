"""Tensor-level operators over ``libmi355ppo.so`` -- the device side of the Python binding of the C ABI.

Written here: the wrappers that exist on the device only or whose host signature differs on purpose -- K1-K6 (GAE, the distributions,
the PPO losses with ``LossSlots``, Adam, the observation kernels), the fused MLP agents (``MlpNetPtrs``), the capturable optimizer steps
and the one-frame weight gradient -- each mirroring one seam of the reference's inline code (cited per function).  They take CUDA (=HIP)
``torch`` tensors only: torch is plumbing (device memory + the current stream), the computation is the HIP kernels, a CPU tensor raises.
Every wrapper ends in ``_launch(symbol, device, *args)``: the entry point on the device's current stream, a non-zero status raised as
``Mi355PpoError`` naming that symbol.

Every operator that has a host twin of the same signature is defined once, in cleanrl_amd/replay_ops.py, rnd_ops.py, ppg_ops.py and
twin_ops.py, and bound at the end of this file to the device side (``_chk``, ``_workspace``, ``_launch``); cleanrl_amd/host_ops.py binds
the same functions to the host side.  ``twins(where)`` picks between the two modules by device, and the autograd nodes written here
(``LSTMSeq`` / ``lstm_seq``, ``TrXLMemoryAttention`` / ``trxl_memory_attention``, ``ImpalaTrunk`` / ``impala_trunk``, ``Impala84Trunk`` /
``impala84_trunk``) go through it, so they take CPU tensors to the host twins on purpose: the agent's host path and the tests run the
same arithmetic as the device kernels.
"""
from __future__ import annotations

import ctypes
import sys

import torch

from . import _lib, ppg_ops, replay_ops, rnd_ops, twin_ops
from .replay_ops import _ptr
from .twin_ops import (AMAX_WORDS, IMPALA64, IMPALA84, IMPALA84_FRAME, IMPALA84_OUT, IMPALA_CHANNELS, IMPALA_FRAME, LN_MAX_D,  # noqa: F401
                       PQN_HIDDEN, PQN_MAX_ACTIONS, PQN_MAX_OBS, ImpalaFamily, impala_check, impala_family_param_shapes, pqn_param_count,
                       trxl_dims)

__all__ = [
    "gae", "categorical_sample", "categorical_logprob_entropy", "normal_sample", "normal_logprob_entropy",
    "ppo_loss_categorical", "ppo_loss_normal", "obs_u8_to_f32", "obs_nchw_to_nhwc_u8", "clip_adam_", "PPOLossCategorical", "PPOLossNormal",
    "CategoricalLogProbEntropy", "NormalLogProbEntropy", "LOSS_SCALAR_NAMES", "LSTMSeq", "lstm_seq", "lstm_seq_dw_hh",
    "ImpalaTrunk", "impala_trunk", "impala_param_shapes", "Impala84Trunk", "impala84_trunk", "impala84_param_shapes", "impala84_params",
    "TrXLMemoryAttention", "trxl_memory_attention", "TrXLLayer", "TrXLLayerPack", "trxl_layer", "trxl_layer_supported", "pqn_param_count", "radam_schedule", "clip_radam_sched_",
    "offpolicy_counts", "sac_actor_count", "dqn_counts", "dqn_limits_ok", "dqn_head_limits_ok", "qdagger_head_limits_ok",
    "rainbow_noisy_limits_ok", "rainbow_noisy_counts", "rainbow_new_buffer", "rainbow_head_limits_ok", "sacd_limits_ok", "rnd_mean_var",
    *replay_ops.OPERATORS, *rnd_ops.OPERATORS, *ppg_ops.OPERATORS, *twin_ops.OPERATORS,
]

LOSS_SCALAR_NAMES = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac")


def _stream(dev: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _NoSwitch:
    """Context manager that does nothing (the tensor's device is already the current one)."""

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NO_SWITCH = _NoSwitch()


def _on(dev: torch.device):
    """``with _on(dev):`` == ``with torch.cuda.device(dev):`` without the get/set-device round trips when ``dev`` is
    already current -- the normal case (one process per GPU); the wrappers sit on the rollout's per-step critical path,
    which is host-bound."""
    return _NO_SWITCH if dev.index is None or torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _launch(name: str, dev: torch.device, *args) -> None:
    """Enqueue the device entry point ``name`` on ``dev``'s current stream (every entry point that takes a stream takes it as its last
    argument) and raise ``Mi355PpoError`` naming it on a non-zero status."""
    with _on(dev):
        _lib.call(name, *args, _stream(dev))


def _chk(t: torch.Tensor, dtype, name: str, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/HIP tensor (libmi355ppo has no CPU path), got "
                        f"{type(t).__name__}{'' if not isinstance(t, torch.Tensor) else ' on ' + str(t.device)}")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def twins(where, *names):
    """The functions ``names`` for ``where`` (a tensor or a device): this module's HIP wrappers for CUDA, the ``*_cpu`` host twins
    of the same names (cleanrl_amd/host_ops.py) otherwise.  Without names: the module itself."""
    if (where.device if isinstance(where, torch.Tensor) else where).type == "cuda":
        mod = sys.modules[__name__]
    else:
        from . import host_ops as mod
    return tuple(getattr(mod, n) for n in names) if names else mod


_workspaces: dict = {}
_retired: list = []


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Per-(device, stream) scratch; calls ordered on one stream may share it (see mi355ppo.h)."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        if ws is not None:
            _retired.append(ws)      # a captured hipGraph may have baked this pointer in: an outgrown workspace is kept, never freed
        ws = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _workspaces[key] = ws
    return ws


# ------------------------------------------------------------------------------------------- K1
def gae(rewards, dones, values, next_done, next_value, gamma: float, gae_lambda: float, advantages=None, returns=None,
        variant: int = 0):
    """Fused GAE (reference: ppo_atari_multigpu.py:290-301).  Returns ``(advantages, returns)`` (T,N)."""
    T, N = rewards.shape
    _chk(rewards, torch.float32, "rewards", (T, N))
    _chk(dones, torch.float32, "dones", (T, N))
    _chk(values, torch.float32, "values", (T, N))
    next_done = _chk(next_done.reshape(-1), torch.float32, "next_done", (N,))
    next_value = _chk(next_value.reshape(-1), torch.float32, "next_value", (N,))
    if advantages is None:
        advantages = torch.empty_like(rewards)
    if returns is None:
        returns = torch.empty_like(rewards)
    _chk(advantages, torch.float32, "advantages", (T, N))
    _chk(returns, torch.float32, "returns", (T, N))
    _launch("mi355ppo_gae_f32_variant", rewards.device, _ptr(rewards), _ptr(dones), _ptr(values), _ptr(next_done), _ptr(next_value),
            _ptr(advantages), _ptr(returns), T, N, float(gamma), float(gae_lambda), int(variant))
    return advantages, returns


# ------------------------------------------------------------------------------------------- K2
def categorical_sample(logits, noise_exp1=None, seed: int = 0, offset: int = 0, action_f32_out=None,
                       logprob_out=None, want_entropy: bool = True, want_i64: bool = True, offset_base=None):
    """``Categorical(logits=logits)``: sample, log_prob, entropy (ppo_atari_multigpu.py:156-159).

    ``noise_exp1`` (B,A) Exponential(1) draws reproduces torch's multinomial draw for that noise
    (parity mode); otherwise a Philox stream keyed by ``(seed, offset)`` is used; ``offset_base`` (1-element int64 device
    tensor) is added to ``offset`` on the device, so a captured launch can be replayed at a new stream position.
    Returns ``(action_i64 | None, action_f32 | None, logprob, entropy | None)``.
    """
    B, A = logits.shape
    _chk(logits, torch.float32, "logits", (B, A))
    if noise_exp1 is not None:
        _chk(noise_exp1, torch.float32, "noise_exp1", (B, A))
    dev = logits.device
    a64 = torch.empty(B, dtype=torch.int64, device=dev) if want_i64 else None
    af = action_f32_out
    if af is not None:
        _chk(af, torch.float32, "action_f32_out", (B,))
    elif not want_i64:
        af = torch.empty(B, dtype=torch.float32, device=dev)
    lp = logprob_out if logprob_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    _chk(lp, torch.float32, "logprob_out", (B,))
    ent = torch.empty(B, dtype=torch.float32, device=dev) if want_entropy else None
    if offset_base is not None:
        _chk(offset_base, torch.int64, "offset_base", (1,))
    _launch("mi355ppo_categorical_sample_ctr_f32", dev, _ptr(logits), _ptr(noise_exp1), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
            _ptr(offset_base), _ptr(a64), _ptr(af), _ptr(lp), _ptr(ent), B, A)
    return a64, af, lp, ent


def categorical_logprob_entropy(logits, action):
    """log_prob / entropy of given actions (int64 or the reference's f32 storage)."""
    B, A = logits.shape
    _chk(logits, torch.float32, "logits", (B, A))
    dev = logits.device
    if action.dtype == torch.int64:
        a64, af = _chk(action, torch.int64, "action", (B,)), None
    else:
        a64, af = None, _chk(action, torch.float32, "action", (B,))
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    ent = torch.empty(B, dtype=torch.float32, device=dev)
    _launch("mi355ppo_categorical_logprob_entropy_f32", dev, _ptr(logits), _ptr(a64), _ptr(af), _ptr(lp), _ptr(ent), B, A)
    return lp, ent


def normal_sample(mean, logstd, noise=None, seed: int = 0, offset: int = 0, action_out=None, logprob_out=None):
    """``Normal(mean, exp(logstd))`` sample + summed log_prob/entropy (ppo_continuous_action.py:134-141)."""
    B, D = mean.shape
    _chk(mean, torch.float32, "mean", (B, D))
    logstd = _chk(logstd.reshape(-1), torch.float32, "logstd", (D,))
    if noise is not None:
        _chk(noise, torch.float32, "noise", (B, D))
    dev = mean.device
    act = action_out if action_out is not None else torch.empty_like(mean)
    _chk(act, torch.float32, "action_out", (B, D))
    lp = logprob_out if logprob_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    ent = torch.empty(B, dtype=torch.float32, device=dev)
    _launch("mi355ppo_normal_sample_f32", dev, _ptr(mean), _ptr(logstd), _ptr(noise), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
            _ptr(act), _ptr(lp), _ptr(ent), B, D)
    return act, lp, ent


def normal_logprob_entropy(mean, logstd, action):
    B, D = mean.shape
    _chk(mean, torch.float32, "mean", (B, D))
    logstd = _chk(logstd.reshape(-1), torch.float32, "logstd", (D,))
    _chk(action, torch.float32, "action", (B, D))
    dev = mean.device
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    ent = torch.empty(B, dtype=torch.float32, device=dev)
    _launch("mi355ppo_normal_logprob_entropy_f32", dev, _ptr(mean), _ptr(logstd), _ptr(action), _ptr(lp), _ptr(ent), B, D)
    return lp, ent


class CategoricalLogProbEntropy(torch.autograd.Function):
    """Differentiable ``(log_prob, entropy)`` of given actions: forward and backward are HIP kernels."""

    @staticmethod
    def forward(ctx, logits, action):
        logits_c = logits.detach().contiguous()
        action = action.contiguous()
        lp, ent = categorical_logprob_entropy(logits_c, action)
        ctx.save_for_backward(logits_c, action)
        return lp, ent

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        logits, action = ctx.saved_tensors
        B, A = logits.shape
        dlogits = torch.empty_like(logits)
        a64, af = (action, None) if action.dtype == torch.int64 else (None, action)
        g_lp = None if g_lp is None else _chk(g_lp.contiguous(), torch.float32, "g_logprob", (B,))
        g_ent = None if g_ent is None else _chk(g_ent.contiguous(), torch.float32, "g_entropy", (B,))
        _launch("mi355ppo_categorical_logprob_entropy_bwd_f32", logits.device, _ptr(logits), _ptr(a64), _ptr(af), _ptr(g_lp), _ptr(g_ent),
                _ptr(dlogits), B, A)
        return dlogits, None


class NormalLogProbEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, logstd, action):
        mean_c, action = mean.detach().contiguous(), action.contiguous()
        ls = logstd.detach().reshape(-1).contiguous()
        lp, ent = normal_logprob_entropy(mean_c, ls, action)
        ctx.save_for_backward(mean_c, ls, action)
        ctx.logstd_shape = logstd.shape
        return lp, ent

    @staticmethod
    def backward(ctx, g_lp, g_ent):
        mean, ls, action = ctx.saved_tensors
        B, D = mean.shape
        dmean, drows = torch.empty_like(mean), torch.empty_like(mean)
        g_lp = None if g_lp is None else _chk(g_lp.contiguous(), torch.float32, "g_logprob", (B,))
        g_ent = None if g_ent is None else _chk(g_ent.contiguous(), torch.float32, "g_entropy", (B,))
        _launch("mi355ppo_normal_logprob_entropy_bwd_f32", mean.device, _ptr(mean), _ptr(ls), _ptr(action), _ptr(g_lp), _ptr(g_ent),
                _ptr(dmean), _ptr(drows), B, D)
        return dmean, drows.sum(0).reshape(ctx.logstd_shape), None


# ------------------------------------------------------------------------------------------- K3
def _flat_batch(b_logprobs, b_advantages, b_returns, b_values):
    Bf = b_logprobs.numel()
    return (Bf, _chk(b_logprobs.reshape(-1), torch.float32, "b_logprobs"),
            _chk(b_advantages.reshape(-1), torch.float32, "b_advantages", (Bf,)),
            _chk(b_returns.reshape(-1), torch.float32, "b_returns", (Bf,)),
            _chk(b_values.reshape(-1), torch.float32, "b_values", (Bf,)))


class LossSlots:
    """Workspace slots for the deferred scalar fold of K3: minibatch k of an update runs ``ppo_loss_categorical(..., slot=(slots,
    k))`` (no fold launch) and ``slots.fold(n, out)`` turns the first n slots into rows of the (n, 7) scalar table in one
    launch."""

    def __init__(self, n: int, device: torch.device):
        lib = _lib.load()
        self.n, self.device = int(n), device
        self.stride = (lib.mi355ppo_loss_workspace_bytes(1, 0) + 255) // 256 * 256
        self.buf = torch.empty(self.n * self.stride, dtype=torch.uint8, device=device)

    def ptr(self, k: int):
        if not 0 <= k < self.n:
            raise IndexError(f"loss slot {k} out of range 0..{self.n - 1}")
        return ctypes.c_void_p(self.buf.data_ptr() + k * self.stride)

    def fold(self, n: int, out: torch.Tensor, first: int = 0) -> torch.Tensor:
        """rows first..first+n-1 of ``out`` (>= first+n, 7) <- slots first..first+n-1."""
        _chk(out, torch.float32, "out")
        if out.dim() != 2 or out.shape[1] != 7 or out.shape[0] < first + n or first + n > self.n:
            raise ValueError(f"fold: out {tuple(out.shape)} / slots {self.n} cannot hold rows {first}..{first + n - 1}")
        _launch("mi355ppo_loss_scalars_f32", self.device, self.ptr(first), self.stride, int(n),
                ctypes.c_void_p(out.data_ptr() + 28 * first))
        return out


def adv_stats(b_advantages, inds, minibatch_size: int, out=None):
    """``(mean, unbiased std + 1e-8)`` of ``b_advantages[inds[j*M:(j+1)*M]]`` for every minibatch j of one epoch's permutation,
    in one launch (ppo_atari_multigpu.py:337-338).  Returns a ``(ceil(len/M), 2)`` f32 tensor whose rows are the
    ``adv_mean_den`` argument of the loss entry points.  A minibatch of one row (``minibatch_size == 1`` or a ragged last one)
    gets ``(that advantage, NaN)``, as ``torch.std`` of one element is NaN; the loss calls refuse ``norm_adv`` on a one-row
    minibatch unless they are handed ``adv_mean_den``."""
    lib = _lib.load()
    flat = _chk(b_advantages.reshape(-1), torch.float32, "b_advantages")
    total = flat.numel() if inds is None else inds.numel()
    if inds is not None:
        _chk(inds, torch.int64, "inds", (total,))
    nseg = (total + minibatch_size - 1) // minibatch_size
    out = out if out is not None else torch.empty(nseg, 2, dtype=torch.float32, device=flat.device)
    _chk(out, torch.float32, "out", (nseg, 2))
    ws = _workspace(flat.device, lib.mi355ppo_adv_stats_workspace_bytes(total, int(minibatch_size)))
    _launch("mi355ppo_adv_stats_f32", flat.device, _ptr(flat), _ptr(inds), total, int(minibatch_size), _ptr(out), _ptr(ws), ws.numel())
    return out


PACK_FLOATS = 8       # floats per packed behaviour row: {action, old log-prob, advantage, return, old value, 0, 0, 0}


def batch_pack(b_actions, b_logprobs, b_advantages, b_returns, b_values, out=None):
    """The five per-row behaviour arrays of the flat batch -> ``(B, 8)`` packed rows (one 32-byte gather per minibatch row in
    K3 instead of five 4-byte gathers; ppo_atari_multigpu.py:320-352).  Once per iteration, after GAE."""
    Bf, b_logprobs, b_advantages, b_returns, b_values = _flat_batch(b_logprobs, b_advantages, b_returns, b_values)
    b_actions = _chk(b_actions.reshape(-1), torch.float32, "b_actions (f32 storage, as the reference)", (Bf,))
    dev = b_logprobs.device
    out = out if out is not None else torch.empty((Bf, PACK_FLOATS), dtype=torch.float32, device=dev)
    _chk(out, torch.float32, "pack", (Bf, PACK_FLOATS))
    _launch("mi355ppo_batch_pack_f32", dev, _ptr(b_actions), _ptr(b_logprobs), _ptr(b_advantages), _ptr(b_returns), _ptr(b_values),
            _ptr(out), Bf)
    return out


def adv_stats_packed(pack, inds, minibatch_size: int, out=None):
    """:func:`adv_stats` reading the advantages out of the packed rows of :func:`batch_pack`."""
    lib = _lib.load()
    _chk(pack, torch.float32, "pack")
    if pack.dim() != 2 or pack.shape[1] != PACK_FLOATS:
        raise ValueError(f"pack: expected (B, {PACK_FLOATS}), got {tuple(pack.shape)}")
    total = pack.shape[0] if inds is None else inds.numel()
    if inds is not None:
        _chk(inds, torch.int64, "inds", (total,))
    nseg = (total + minibatch_size - 1) // minibatch_size
    out = out if out is not None else torch.empty(nseg, 2, dtype=torch.float32, device=pack.device)
    _chk(out, torch.float32, "out", (nseg, 2))
    ws = _workspace(pack.device, lib.mi355ppo_adv_stats_workspace_bytes(total, int(minibatch_size)))
    _launch("mi355ppo_adv_stats_packed_f32", pack.device, _ptr(pack), _ptr(inds), total, int(minibatch_size), _ptr(out), _ptr(ws),
            ws.numel())
    return out


def ppo_loss_categorical_packed(new_logits, new_value, mb_inds, pack, clip_coef: float, ent_coef: float, vf_coef: float,
                                norm_adv: bool = True, clip_vloss: bool = True, scalars_out=None, dlogits_out=None,
                                dvalue_out=None, adv_mean_den=None, slot=None):
    """:func:`ppo_loss_categorical` on the packed rows of :func:`batch_pack` (bit-identical results).  ``adv_mean_den`` (a row
    of :func:`adv_stats_packed`) is required when ``norm_adv`` is set."""
    lib = _lib.load()
    M, A = new_logits.shape
    _chk(new_logits, torch.float32, "new_logits", (M, A))
    new_value = _chk(new_value.reshape(-1), torch.float32, "new_value", (M,))
    dev = new_logits.device
    if mb_inds is not None:
        _chk(mb_inds, torch.int64, "mb_inds", (M,))
    _chk(pack, torch.float32, "pack")
    if pack.dim() != 2 or pack.shape[1] != PACK_FLOATS:
        raise ValueError(f"pack: expected (B, {PACK_FLOATS}), got {tuple(pack.shape)}")
    if norm_adv and adv_mean_den is None and M > 1:          # (M == 1 has no unbiased std: the library refuses the call below)
        adv_mean_den = adv_stats_packed(pack, mb_inds, M)[0] if mb_inds is not None else adv_stats_packed(pack[:M], None, M)[0]
    if adv_mean_den is not None:
        _chk(adv_mean_den, torch.float32, "adv_mean_den", (2,))
    dlogits = dlogits_out if dlogits_out is not None else torch.empty_like(new_logits)
    dvalue = dvalue_out if dvalue_out is not None else torch.empty(M, dtype=torch.float32, device=dev)
    if slot is not None:
        slots, k = slot
        ws_ptr, ws_bytes, scalars = slots.ptr(k), slots.stride, None
    else:
        scalars = scalars_out if scalars_out is not None else torch.empty(7, dtype=torch.float32, device=dev)
        ws = _workspace(dev, lib.mi355ppo_loss_workspace_bytes(M, 0))
        ws_ptr, ws_bytes = _ptr(ws), ws.numel()
    _launch("mi355ppo_loss_categorical_packed_fwd_bwd_f32", dev, _ptr(new_logits), _ptr(new_value), _ptr(mb_inds), _ptr(pack), M, A,
            float(clip_coef), float(ent_coef), float(vf_coef), int(bool(norm_adv)), int(bool(clip_vloss)), _ptr(adv_mean_den),
            _ptr(scalars), _ptr(dlogits), _ptr(dvalue), ws_ptr, ws_bytes)
    return scalars, dlogits, dvalue


def ppo_loss_categorical(new_logits, new_value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                         clip_coef: float, ent_coef: float, vf_coef: float, norm_adv: bool = True,
                         clip_vloss: bool = True, scalars_out=None, dlogits_out=None, dvalue_out=None, adv_mean_den=None,
                         slot=None):
    """Fused minibatch loss fwd+bwd (ppo_atari_multigpu.py:320-355 + autograd backward).

    Returns ``(scalars7, dlogits, dvalue)``; ``scalars7`` = LOSS_SCALAR_NAMES order, on device.  ``adv_mean_den``: the
    minibatch's row of :func:`adv_stats` (skips the statistics launch).  ``slot=(LossSlots, k)``: defer the scalar fold
    (``scalars7`` is then None; ``LossSlots.fold`` produces it later).
    """
    lib = _lib.load()
    M, A = new_logits.shape
    _chk(new_logits, torch.float32, "new_logits", (M, A))
    new_value = _chk(new_value.reshape(-1), torch.float32, "new_value", (M,))
    dev = new_logits.device
    if mb_inds is not None:
        _chk(mb_inds, torch.int64, "mb_inds", (M,))
    Bf, b_logprobs, b_advantages, b_returns, b_values = _flat_batch(b_logprobs, b_advantages, b_returns, b_values)
    b_actions = _chk(b_actions.reshape(-1), torch.float32, "b_actions (f32 storage, as the reference)", (Bf,))
    if adv_mean_den is not None:
        _chk(adv_mean_den, torch.float32, "adv_mean_den", (2,))
    dlogits = dlogits_out if dlogits_out is not None else torch.empty_like(new_logits)
    dvalue = dvalue_out if dvalue_out is not None else torch.empty(M, dtype=torch.float32, device=dev)
    if slot is not None:
        slots, k = slot
        ws_ptr, ws_bytes, scalars = slots.ptr(k), slots.stride, None
    else:
        scalars = scalars_out if scalars_out is not None else torch.empty(7, dtype=torch.float32, device=dev)
        ws = _workspace(dev, lib.mi355ppo_loss_workspace_bytes(M, 0))
        ws_ptr, ws_bytes = _ptr(ws), ws.numel()
    _launch("mi355ppo_loss_categorical_fwd_bwd_f32", dev, _ptr(new_logits), _ptr(new_value), _ptr(mb_inds), _ptr(b_actions),
            _ptr(b_logprobs), _ptr(b_advantages), _ptr(b_returns), _ptr(b_values), M, A, float(clip_coef), float(ent_coef), float(vf_coef),
            int(bool(norm_adv)), int(bool(clip_vloss)), _ptr(adv_mean_den), _ptr(scalars), _ptr(dlogits), _ptr(dvalue), ws_ptr, ws_bytes)
    return scalars, dlogits, dvalue


def ppo_loss_normal(new_mean, logstd, new_value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                    clip_coef: float, ent_coef: float, vf_coef: float, norm_adv: bool = True, clip_vloss: bool = True,
                    scalars_out=None, adv_mean_den=None):
    """Continuous-action loss fwd+bwd (ppo_continuous_action.py:265-300).
    Returns ``(scalars7, dmean, dlogstd, dvalue)``."""
    lib = _lib.load()
    M, D = new_mean.shape
    _chk(new_mean, torch.float32, "new_mean", (M, D))
    logstd_flat = _chk(logstd.reshape(-1), torch.float32, "logstd", (D,))
    new_value = _chk(new_value.reshape(-1), torch.float32, "new_value", (M,))
    dev = new_mean.device
    if mb_inds is not None:
        _chk(mb_inds, torch.int64, "mb_inds", (M,))
    Bf, b_logprobs, b_advantages, b_returns, b_values = _flat_batch(b_logprobs, b_advantages, b_returns, b_values)
    b_actions = _chk(b_actions.reshape(Bf, D), torch.float32, "b_actions", (Bf, D))
    if adv_mean_den is not None:
        _chk(adv_mean_den, torch.float32, "adv_mean_den", (2,))
    scalars = scalars_out if scalars_out is not None else torch.empty(7, dtype=torch.float32, device=dev)
    dmean = torch.empty_like(new_mean)
    dlogstd = torch.empty(D, dtype=torch.float32, device=dev)
    dvalue = torch.empty(M, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_loss_workspace_bytes(M, D))
    _launch("mi355ppo_loss_normal_fwd_bwd_f32", dev, _ptr(new_mean), _ptr(logstd_flat), _ptr(new_value), _ptr(mb_inds), _ptr(b_actions),
            _ptr(b_logprobs), _ptr(b_advantages), _ptr(b_returns), _ptr(b_values), M, D, float(clip_coef), float(ent_coef), float(vf_coef),
            int(bool(norm_adv)), int(bool(clip_vloss)), _ptr(adv_mean_den), _ptr(scalars), _ptr(dmean), _ptr(dlogstd), _ptr(dvalue),
            _ptr(ws), ws.numel())
    return scalars, dmean, dlogstd, dvalue


class PPOLossCategorical(torch.autograd.Function):
    """``loss = PPOLossCategorical.apply(logits, value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns,
    b_values, clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss)`` -> (loss, scalars7).  ``loss.backward()``
    feeds the precomputed dlogits / dvalue into the network's autograd graph."""

    @staticmethod
    def forward(ctx, logits, value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, clip_coef,
                ent_coef, vf_coef, norm_adv, clip_vloss):
        scalars, dlogits, dvalue = ppo_loss_categorical(
            logits.detach().contiguous(), value.detach().contiguous(), mb_inds, b_actions, b_logprobs, b_advantages,
            b_returns, b_values, clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss)
        ctx.save_for_backward(dlogits, dvalue)
        ctx.value_shape = value.shape
        ctx.mark_non_differentiable(scalars)
        return scalars[0].clone(), scalars

    @staticmethod
    def backward(ctx, grad_loss, _grad_scalars):
        dlogits, dvalue = ctx.saved_tensors
        return (grad_loss * dlogits, (grad_loss * dvalue).reshape(ctx.value_shape)) + (None,) * 11


class PPOLossNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, logstd, value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, clip_coef,
                ent_coef, vf_coef, norm_adv, clip_vloss):
        scalars, dmean, dlogstd, dvalue = ppo_loss_normal(
            mean.detach().contiguous(), logstd.detach().contiguous(), value.detach().contiguous(), mb_inds, b_actions,
            b_logprobs, b_advantages, b_returns, b_values, clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss)
        ctx.save_for_backward(dmean, dlogstd, dvalue)
        ctx.value_shape, ctx.logstd_shape = value.shape, logstd.shape
        ctx.mark_non_differentiable(scalars)
        return scalars[0].clone(), scalars

    @staticmethod
    def backward(ctx, grad_loss, _grad_scalars):
        dmean, dlogstd, dvalue = ctx.saved_tensors
        return (grad_loss * dmean, (grad_loss * dlogstd).reshape(ctx.logstd_shape),
                (grad_loss * dvalue).reshape(ctx.value_shape)) + (None,) * 11


# ------------------------------------------------------------------------------------------- K5
def obs_u8_to_f32(src_u8, inds=None, out=None, scale_255: bool = True):
    """Gather rows of a uint8 observation buffer and convert to f32 (``b_obs[mb_inds]`` then ``x / 255.0``,
    ppo_atari_multigpu.py:320,154).  ``src_u8``: (R, ...) uint8; ``inds``: (rows,) int64 or None."""
    _chk(src_u8, torch.uint8, "src_u8")
    dev = src_u8.device
    row_shape = tuple(src_u8.shape[1:])
    row_bytes = 1
    for s in row_shape:
        row_bytes *= s
    if inds is not None:
        _chk(inds, torch.int64, "inds")
        rows = inds.numel()
    else:
        rows = src_u8.shape[0]
    if out is None:
        out = torch.empty((rows,) + row_shape, dtype=torch.float32, device=dev)
    _chk(out, torch.float32, "out", (rows,) + row_shape)
    _launch("mi355ppo_obs_u8_to_f32", dev, _ptr(src_u8), _ptr(inds), _ptr(out), rows, row_bytes, int(bool(scale_255)))
    return out


def obs_nchw_to_nhwc_u8(src, out=None):
    """(rows, C, H, W) uint8 -> (rows, H, W, C) uint8, the rollout buffer's pixel-interleaved layout."""
    _chk(src, torch.uint8, "src")
    rows, C, H, W = src.shape
    if out is None:
        out = torch.empty((rows, H, W, C), dtype=torch.uint8, device=src.device)
    _chk(out, torch.uint8, "out", (rows, H, W, C))
    _launch("mi355ppo_obs_nchw_to_nhwc_u8", src.device, _ptr(src), _ptr(out), rows, C, H * W)
    return out


def obs_shift_append_u8(prev_rows, newest, out):
    """FrameStack(4) delta store: ``out[r] = concat(prev_rows[r][..., 1:4], newest[r][..., None])`` on (rows, H, W, 4) uint8
    rows and (rows, H, W) uint8 planes -- the next observation of envs that were not reset."""
    rows, H, W, C = prev_rows.shape
    assert C == 4, "the delta store is defined for 4-frame stacks"
    _chk(prev_rows, torch.uint8, "prev_rows", (rows, H, W, 4))
    _chk(newest, torch.uint8, "newest", (rows, H, W))
    _chk(out, torch.uint8, "out", (rows, H, W, 4))
    _launch("mi355ppo_obs_shift_append_u8_c4", out.device, _ptr(prev_rows), _ptr(newest), _ptr(out), rows, H * W)
    return out


# ---------------------------------------------------------------------------------------- a8/a9
def clip_adam_(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, max_grad_norm: float, grad_scale: float = 1.0,
               beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-5, total_norm_out=None):
    """In-place fused ``grads*grad_scale -> clip_grad_norm_ -> Adam.step`` on flat f32 buffers
    (ppo_atari_multigpu.py:368-377).  Zeroes ``grads`` for the next backward.  ``step`` is 1-based."""
    lib = _lib.load()
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nm, (n,))
    dev = params.device
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_clip_adam_workspace_bytes(n))
    _launch("mi355ppo_clip_adam_f32", dev, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(grad_scale),
            float(max_grad_norm), float(lr), float(beta1), float(beta2), float(eps), int(step), _ptr(total_norm_out), _ptr(ws), ws.numel())
    return total_norm_out


def adam_schedule(lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999):
    """The two schedule-dependent constants of Adam step ``step`` (1-based) as the kernels consume them (host floats):
    ``(-(lr / (1 - beta1^step)), sqrt(1 - beta2^step))`` -- computed by the library, so that eager and captured steps agree bit
    for bit."""
    out = (ctypes.c_float * 2)()
    _lib.call("mi355ppo_adam_schedule_f32", float(lr), float(beta1), float(beta2), int(step), out)
    return float(out[0]), float(out[1])


def clip_adam_sched_(params, grads, exp_avg, exp_avg_sq, sched2, max_grad_norm: float, grad_scale: float = 1.0, beta1: float = 0.9,
                     beta2: float = 0.999, eps: float = 1e-5, total_norm_out=None):
    """``clip_adam_`` with the step's (step_size, bias_correction2_sqrt) read from the 2-float DEVICE tensor ``sched2``
    (``adam_schedule`` values copied there by the caller): capturable, replayable with the next step's schedule."""
    lib = _lib.load()
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nm, (n,))
    _chk(sched2, torch.float32, "sched2", (2,))
    dev = params.device
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_clip_adam_workspace_bytes(n))
    _launch("mi355ppo_clip_adam_sched_f32", dev, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(grad_scale),
            float(max_grad_norm), float(beta1), float(beta2), float(eps), _ptr(sched2), _ptr(total_norm_out), _ptr(ws), ws.numel())
    return total_norm_out


# ------------------------------------------------------------------------------------------- K7: the fused MLP agents
MLP_MAX_OBS, MLP_MAX_OUT, MLP_HIDDEN = 512, 20, 64      # (round 6: the WIDE kernels of csrc/mlp.hip -- Humanoid's 376 / 17; up to 32 / 8: the narrow ones)


class MlpNetPtrs:
    """The six parameter tensors of one 64-64 tanh MLP (``nn.Sequential(Linear, Tanh, Linear, Tanh, Linear)``, ppo.py:100-117)
    as the C ABI wants them: a host array of six device pointers (weights in torch's (out, in) layout), and the same for their
    ``.grad`` views.  Built once per network: parameters and gradients of a flat-buffer agent never move."""

    def __init__(self, seq):
        lin = [m for m in seq if isinstance(m, torch.nn.Linear)]
        assert len(lin) == 3 and lin[0].out_features == MLP_HIDDEN and lin[1].in_features == MLP_HIDDEN and \
            lin[1].out_features == MLP_HIDDEN and lin[2].in_features == MLP_HIDDEN, "the fused MLP kernels are the reference's 64-64 networks"
        self.obs_dim, self.n_out = lin[0].in_features, lin[2].out_features
        self.tensors = [t for m in lin for t in (m.weight, m.bias)]
        for t in self.tensors:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        self.params = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in self.tensors])
        self._grad_ptrs = None

    def grads(self):
        g = [t.grad for t in self.tensors]
        assert all(x is not None and x.is_contiguous() for x in g), "fused MLP backward needs allocated .grad tensors (flat buffers)"
        key = tuple(x.data_ptr() for x in g)
        if self._grad_ptrs is None or self._grad_ptrs[0] != key:
            self._grad_ptrs = (key, (ctypes.c_void_p * 6)(*key))
        return self._grad_ptrs[1]

    def refresh(self):
        """Re-read the parameter pointers (after ``module.to(...)`` / a flat-buffer rebind)."""
        self.params = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in self.tensors])


def mlp_supported(obs_dim: int, n_out: int) -> bool:
    return 0 < obs_dim <= MLP_MAX_OBS and 0 < n_out <= MLP_MAX_OUT


def mlp_forward(obs, actor: MlpNetPtrs, critic: MlpNetPtrs, actor_out=None, value_out=None):
    """Both networks' forward in one launch -> ``(actor_out (B, n_out), value (B))``."""
    B, O = obs.shape
    _chk(obs, torch.float32, "obs", (B, actor.obs_dim))
    dev = obs.device
    out = actor_out if actor_out is not None else torch.empty((B, actor.n_out), dtype=torch.float32, device=dev)
    val = value_out if value_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    _chk(out, torch.float32, "actor_out", (B, actor.n_out))
    _chk(val, torch.float32, "value_out", (B,))
    _launch("mi355ppo_mlp_fwd_f32", dev, _ptr(obs), B, O, actor.params, critic.params, actor.n_out, _ptr(out), _ptr(val))
    return out, val


def mlp_act_categorical(obs, actor: MlpNetPtrs, critic: MlpNetPtrs, noise_exp1=None, seed: int = 0, offset: int = 0, offset_base=None,
                        action_f32_out=None, logprob_out=None, value_out=None, want_i64: bool = True, want_entropy: bool = False,
                        want_logits: bool = False):
    """One rollout step of the Categorical MLP agent (ppo.py:205-210): both forwards + sample + log_prob (+ entropy) in one launch.
    -> ``(action_i64 | None, action_f32 | None, logprob, entropy | None, value, logits | None)``."""
    B, O = obs.shape
    _chk(obs, torch.float32, "obs", (B, actor.obs_dim))
    dev, A = obs.device, actor.n_out
    if noise_exp1 is not None:
        _chk(noise_exp1, torch.float32, "noise_exp1", (B, A))
    a64 = torch.empty(B, dtype=torch.int64, device=dev) if want_i64 else None
    af = action_f32_out if action_f32_out is not None else (None if want_i64 else torch.empty(B, dtype=torch.float32, device=dev))
    lp = logprob_out if logprob_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    val = value_out if value_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    for t, nm in ((af, "action_f32_out"), (lp, "logprob_out"), (val, "value_out")):
        if t is not None:
            _chk(t, torch.float32, nm, (B,))
    ent = torch.empty(B, dtype=torch.float32, device=dev) if want_entropy else None
    logits = torch.empty((B, A), dtype=torch.float32, device=dev) if want_logits else None
    if offset_base is not None:
        _chk(offset_base, torch.int64, "offset_base", (1,))
    _launch("mi355ppo_mlp_act_categorical_f32", dev, _ptr(obs), B, O, actor.params, critic.params, A, _ptr(noise_exp1),
            int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _ptr(offset_base), _ptr(a64), _ptr(af), _ptr(lp), _ptr(ent), _ptr(val),
            _ptr(logits))
    return a64, af, lp, ent, val, logits


def mlp_act_normal(obs, actor: MlpNetPtrs, critic: MlpNetPtrs, logstd, noise=None, seed: int = 0, offset: int = 0, offset_base=None,
                   action_out=None, logprob_out=None, value_out=None, want_entropy: bool = False, want_mean: bool = False):
    """One rollout step of the continuous-action agent (ppo_continuous_action.py:221-226) in one launch.
    -> ``(action (B, D), logprob, entropy | None, value, mean | None)``."""
    B, O = obs.shape
    _chk(obs, torch.float32, "obs", (B, actor.obs_dim))
    dev, D = obs.device, actor.n_out
    logstd = _chk(logstd.reshape(-1), torch.float32, "logstd", (D,))
    if noise is not None:
        _chk(noise, torch.float32, "noise", (B, D))
    act = action_out if action_out is not None else torch.empty((B, D), dtype=torch.float32, device=dev)
    _chk(act, torch.float32, "action_out", (B, D))
    lp = logprob_out if logprob_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    val = value_out if value_out is not None else torch.empty(B, dtype=torch.float32, device=dev)
    _chk(lp, torch.float32, "logprob_out", (B,))
    _chk(val, torch.float32, "value_out", (B,))
    ent = torch.empty(B, dtype=torch.float32, device=dev) if want_entropy else None
    mean = torch.empty((B, D), dtype=torch.float32, device=dev) if want_mean else None
    if offset_base is not None:
        _chk(offset_base, torch.int64, "offset_base", (1,))
    _launch("mi355ppo_mlp_act_normal_f32", dev, _ptr(obs), B, O, actor.params, critic.params, _ptr(logstd), D, _ptr(noise),
            int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _ptr(offset_base), _ptr(act), _ptr(lp), _ptr(ent), _ptr(val), _ptr(mean))
    return act, lp, ent, val, mean


def mlp_ppo_fwd_bwd(b_obs, mb_inds, actor: MlpNetPtrs, critic: MlpNetPtrs, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                    clip_coef, ent_coef, vf_coef, norm_adv=True, clip_vloss=True, adv_mean_den=None, scalars_out=None, logstd=None,
                    logstd_grad=None, mean_shift=None, rows_per_block: int = 0):
    """One minibatch of the update of an MLP agent in two launches (ppo.py:250-287 / ppo_continuous_action.py:265-302 up to and
    including ``loss.backward()``): gather, both forwards, distribution, PPO loss, both backward passes.  Gradients are ADDED to
    the networks' ``.grad`` tensors (and ``logstd_grad``); -> the seven scalars of K3.  ``logstd`` given = Normal head."""
    lib = _lib.load()
    Bf, O = b_obs.shape
    _chk(b_obs, torch.float32, "b_obs", (Bf, actor.obs_dim))
    dev, nout = b_obs.device, actor.n_out
    if mb_inds is not None:
        _chk(mb_inds, torch.int64, "mb_inds")
        M = mb_inds.numel()
    else:
        M = Bf
    _, lpv, advv, retv, valv = _flat_batch(b_logprobs, b_advantages, b_returns, b_values)
    normal = logstd is not None
    _chk(b_actions, torch.float32, "b_actions", (Bf, nout) if normal else (Bf,))
    if norm_adv:
        if adv_mean_den is None:
            adv_mean_den = adv_stats(advv, mb_inds, M)[0]
        _chk(adv_mean_den, torch.float32, "adv_mean_den", (2,))
    sc = scalars_out if scalars_out is not None else torch.empty(7, dtype=torch.float32, device=dev)
    _chk(sc, torch.float32, "scalars_out", (7,))
    nbytes = lib.mi355ppo_mlp_ppo_workspace_bytes(M, O, nout, int(rows_per_block))
    if nbytes == 0:
        raise ValueError(f"mlp_ppo_fwd_bwd: unsupported shape (obs_dim={O} <= {MLP_MAX_OBS}, n_out={nout} <= {MLP_MAX_OUT})")
    ws = _workspace(dev, nbytes)
    if normal:
        ls = _chk(logstd.reshape(-1), torch.float32, "logstd", (nout,))
        lg = _chk(logstd_grad.reshape(-1), torch.float32, "logstd_grad", (nout,))
        if mean_shift is not None:
            _chk(mean_shift, torch.float32, "mean_shift", (M, nout))
        _launch("mi355ppo_mlp_ppo_normal_fwd_bwd_f32", dev, _ptr(b_obs), _ptr(mb_inds), M, O, actor.params, critic.params, _ptr(ls), nout,
                _ptr(mean_shift), _ptr(b_actions), _ptr(lpv), _ptr(advv), _ptr(retv), _ptr(valv), float(clip_coef), float(ent_coef),
                float(vf_coef), int(bool(norm_adv)), int(bool(clip_vloss)), _ptr(adv_mean_den), actor.grads(), critic.grads(), _ptr(lg),
                _ptr(sc), int(rows_per_block), _ptr(ws), ws.numel())
    else:
        _launch("mi355ppo_mlp_ppo_categorical_fwd_bwd_f32", dev, _ptr(b_obs), _ptr(mb_inds), M, O, actor.params, critic.params, nout,
                _ptr(b_actions), _ptr(lpv), _ptr(advv), _ptr(retv), _ptr(valv), float(clip_coef), float(ent_coef), float(vf_coef),
                int(bool(norm_adv)), int(bool(clip_vloss)), _ptr(adv_mean_den), actor.grads(), critic.grads(), _ptr(sc),
                int(rows_per_block), _ptr(ws), ws.numel())
    return sc


# ------------------------------------------------------------------------------------------- K8: the 256-wide tanh MLP agents
MLP256_MAX_OBS, MLP256_MAX_OUT, MLP256_HIDDEN, MLP256_TILE = 256, 32, 256, 64


def mlp256_supported(obs_dim: int, n_out: int) -> bool:
    return 1 <= obs_dim <= MLP256_MAX_OBS and 1 <= n_out <= MLP256_MAX_OUT


class Mlp256Nets:
    """Actor-mean and critic ``nn.Sequential(Linear(O, 256), Tanh, Linear(256, 256), Tanh, Linear(256, n_out))`` for the K8 kernels
    (csrc/mlp256.hip): the parameter / gradient pointer blocks, the weight pack and the workspace.  The pack is a derived weight in the
    sense of ``cnn.TrunkBuffers._derived``: valid for ``(weights_version, the tensors' version counters, their addresses)`` and re-derived
    INTO the same buffer when that tag moved -- whoever rewrites the parameters through raw pointers bumps ``weights_version``.  (The rule is
    stated here again, not shared: ``_derived`` tags ONE tensor per entry and lives on the NatureCNN trunk's buffer object with its all-packs
    launch; this pack is one buffer derived from twelve tensors of an agent that has no trunk.)  The
    workspace is this object's own (the loss kernel between forward and backward uses the shared per-stream one); an outgrown
    one is kept, never freed: a captured graph may have baked its address in."""

    def __init__(self, actor, critic):
        self.nets = [[m for m in seq if isinstance(m, torch.nn.Linear)] for seq in (actor, critic)]
        a, c = self.nets
        assert len(a) == 3 and len(c) == 3, "three Linear layers per network"
        self.obs_dim, self.n_out = a[0].in_features, a[2].out_features
        for lin, no in ((a, self.n_out), (c, 1)):
            assert (lin[0].in_features, lin[0].out_features) == (self.obs_dim, MLP256_HIDDEN) and lin[2].out_features == no and \
                (lin[1].in_features, lin[1].out_features, lin[2].in_features) == (MLP256_HIDDEN,) * 3, "the K8 kernels are O-256-256-n_out networks"
        assert mlp256_supported(self.obs_dim, self.n_out), "outside the K8 kernels' shapes"
        self.tensors = [[t for m in lin for t in (m.weight, m.bias)] for lin in self.nets]
        for t in self.tensors[0] + self.tensors[1]:
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        self.device = self.tensors[0][0].device
        self.weights_version = 0
        self._pack = None            # (tag, uint8 tensor)
        self._ws, self._old_ws = None, []

    def _ptrs(self, tensors):
        return (ctypes.c_void_p * 6)(*[t.data_ptr() for t in tensors])

    def pack(self):
        ts = self.tensors[0] + self.tensors[1]
        tag = (self.weights_version, tuple(t._version for t in ts), tuple(t.data_ptr() for t in ts))
        if self._pack is None or self._pack[0] != tag:
            nbytes = _lib.load().mi355ppo_mlp256_pack_bytes(self.obs_dim, self.n_out)
            buf = self._pack[1] if self._pack is not None else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _launch("mi355ppo_mlp256_pack_f32", self.device, self._ptrs(self.tensors[0]), self._ptrs(self.tensors[1]), self.obs_dim, self.n_out,
                    _ptr(buf), buf.numel())
            self._pack = (tag, buf)
        return self._pack[1]

    def workspace(self, M: int):
        nbytes = _lib.load().mi355ppo_mlp256_workspace_bytes(int(M), self.obs_dim, self.n_out)
        if self._ws is None or self._ws.numel() < nbytes:
            if self._ws is not None:
                self._old_ws.append(self._ws)
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def saved(self, M: int):
        """Views of the workspace after a saving forward / the data gradient: ``(h1, h2, dz2, dz1)``, each (2 networks, M, 256)."""
        f = self.workspace(M).view(torch.float32)
        n = 2 * M * MLP256_HIDDEN
        return tuple(f[i * n:(i + 1) * n].view(2, M, MLP256_HIDDEN) for i in range(4))

    def grads(self):
        out = []
        for ts in self.tensors:
            g = [t.grad for t in ts]
            assert all(x is not None and x.is_contiguous() for x in g), "the K8 backward needs allocated .grad tensors (flat buffers)"
            out.append(self._ptrs(g))
        return out


def mlp256_forward(obs, nets: Mlp256Nets, inds=None, save: bool = False, mean_out=None, value_out=None):
    """Both networks' forward chain on ``obs[inds]`` (``inds`` None: ``obs``) in one launch -> ``(mean (M, n_out), value (M))``.
    ``save``: h1 / h2 of both networks stay in ``nets``' workspace for ``mlp256_backward``."""
    Bf, O = obs.shape
    _chk(obs, torch.float32, "obs", (Bf, nets.obs_dim))
    dev = obs.device
    M = Bf
    if inds is not None:
        _chk(inds, torch.int64, "inds")
        M = inds.numel()
    mean = mean_out if mean_out is not None else torch.empty((M, nets.n_out), dtype=torch.float32, device=dev)
    value = value_out if value_out is not None else torch.empty(M, dtype=torch.float32, device=dev)
    _chk(mean, torch.float32, "mean_out", (M, nets.n_out))
    _chk(value, torch.float32, "value_out", (M,))
    ws = nets.workspace(M) if save else None
    _launch("mi355ppo_mlp256_fwd_f32", dev, _ptr(obs), _ptr(inds), M, O, nets.n_out, _ptr(nets.pack()), _ptr(mean), _ptr(value), _ptr(ws),
            ws.numel() if save else 0)
    return mean, value


def mlp256_backward(obs, nets: Mlp256Nets, dmean, dvalue, inds=None, slabs: int = 0):
    """The backward of ``mlp256_forward(..., save=True)``: the data-gradient chain (one launch), then the six weight and six bias
    gradients over row slabs and their fold in slab order (two launches).  The gradients are ADDED to the parameters' ``.grad``."""
    M = dmean.shape[0]
    _chk(obs, torch.float32, "obs", (obs.shape[0], nets.obs_dim))
    _chk(dmean, torch.float32, "dmean", (M, nets.n_out))
    dvalue = _chk(dvalue.reshape(-1), torch.float32, "dvalue", (M,))
    if inds is not None:
        _chk(inds, torch.int64, "inds", (M,))
    dev, ws = obs.device, nets.workspace(M)
    _launch("mi355ppo_mlp256_dgrad_f32", dev, _ptr(dmean), _ptr(dvalue), M, nets.obs_dim, nets.n_out, _ptr(nets.pack()), _ptr(ws), ws.numel())
    ga, gc = nets.grads()
    _launch("mi355ppo_mlp256_wgrad_f32", dev, _ptr(obs), _ptr(inds), _ptr(dmean), _ptr(dvalue), M, nets.obs_dim, nets.n_out, ga, gc, int(slabs),
            _ptr(ws), ws.numel())


# ------------------------------------------------------------------------------------------- LSTM
def lstm_seq_dw_hh(dgx, record):
    """d W_hh = sum_t dgx[t]^T hk_t (hk: the record's plane 5), as the reference's per-step graphs accumulate it: one product of
    B rows per step (one batched GEMM), then the sum over T -- not one GEMM over T*B rows, whose single accumulation chain is
    several times less accurate at update sizes (T*B = 8,192: 1.5e-6 against float64 on the device, the loop's 2.5e-7)."""
    T, B, G = dgx.shape
    H = G // 4
    hk = record[5 * T * B * H:6 * T * B * H].view(T, B, H)
    return torch.bmm(dgx.transpose(1, 2), hk).sum(0)


_LSTM = ("lstm_seq_forward", "lstm_seq_backward")


class LSTMSeq(torch.autograd.Function):
    """Differentiable ``(gx, w_hh, h0, c0, done) -> (h, hT, cT)``: the scan forward records its activations, the backward scan
    returns d gx and d (h0, c0), and d w_hh is one GEMM over the record's hk plane.  The HIP kernels run for CUDA tensors, the
    host twins for CPU ones (same arithmetic), so the plumbing is testable without a GPU.  ``lstm_seq`` picks the record-free
    forward when no gradient is wanted."""

    @staticmethod
    def forward(ctx, gx, w_hh, h0, c0, done):
        fwd, _ = twins(gx, *_LSTM)
        w = w_hh.detach().contiguous()
        d = done.detach().to(torch.float32).contiguous()
        h, hT, cT, rec = fwd(gx.detach().contiguous(), w, h0.detach().contiguous(), c0.detach().contiguous(), d, record=True)
        ctx.save_for_backward(rec, w, d)
        return h, hT, cT

    @staticmethod
    def backward(ctx, dh, dhT, dcT):
        rec, w, d = ctx.saved_tensors
        _, bwd = twins(w, *_LSTM)
        T, B = d.shape
        H = w.shape[1]
        dh = torch.zeros((T, B, H), device=w.device) if dh is None else dh.contiguous()
        dhT = None if dhT is None else dhT.contiguous()
        dcT = None if dcT is None else dcT.contiguous()
        dgx, dh0, dc0 = bwd(dh, dhT, dcT, rec, w, d, want_dh0=ctx.needs_input_grad[2], want_dc0=ctx.needs_input_grad[3])
        dw = lstm_seq_dw_hh(dgx, rec) if ctx.needs_input_grad[1] else None
        return dgx, dw, dh0, dc0, None


def lstm_seq(gx, w_hh, h0, c0, done):
    """``LSTMSeq.apply`` when a gradient is wanted, else the inference scan without a record (the rollout step, the bootstrap)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (gx, w_hh, h0, c0)):
        return LSTMSeq.apply(gx, w_hh, h0, c0, done)
    fwd, _ = twins(gx, *_LSTM)
    h, hT, cT, _ = fwd(gx.contiguous(), w_hh.detach().contiguous(), h0.contiguous(), c0.contiguous(),
                       done.to(torch.float32).contiguous())
    return h, hT, cT


# ------------------------------------------------------------------------------------------- TrXL
_TRXL = ("trxl_attn_forward", "trxl_attn_backward")


def _trxl_inputs(memory, ep, rows, pos, mask, pe):
    """The non-differentiable inputs in the kernels' dtypes: int64 indices, uint8 mask (any nonzero keeps a row)."""
    pe = None if pe is None else pe.detach().to(torch.float32).contiguous()
    pos = None if pe is None else pos.to(torch.int64).contiguous()
    return (memory.detach().contiguous(), ep.to(torch.int64).contiguous(), rows.to(torch.int64).contiguous(), pos,
            (mask != 0).to(torch.uint8).contiguous(), pe)


class TrXLMemoryAttention(torch.autograd.Function):
    """Differentiable ``(q~, gamma, beta; memory, layer, ep, rows, pos, mask, pe) -> u`` (B,H,d): the window gather, positional
    encoding, norm_kv, scores, masked softmax and weighted sum of one TrXL layer in one streaming pass (csrc/trxl_attn.hip).
    The memory, indices, mask and pe get no gradient.  The HIP kernels run for CUDA tensors, the host twins for CPU ones."""

    @staticmethod
    def forward(ctx, q, gamma, beta, memory, layer, ep, rows, pos, mask, pe):
        fwd, _ = twins(q, *_TRXL)
        memory, ep, rows, pos, mask, pe = _trxl_inputs(memory, ep, rows, pos, mask, pe)
        q, gamma, beta = q.detach().contiguous(), gamma.detach().contiguous(), beta.detach().contiguous()
        u, stats = fwd(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q)
        ctx.layer = layer
        ctx.save_for_backward(q, gamma, beta, memory, ep, rows, pos, mask, pe, u, stats)
        return u

    @staticmethod
    def backward(ctx, du):
        q, gamma, beta, memory, ep, rows, pos, mask, pe, u, stats = ctx.saved_tensors
        _, bwd = twins(q, *_TRXL)
        dq, dgamma, dbeta = bwd(memory, ctx.layer, ep, rows, pos, mask, pe, gamma, beta, q, u, stats, du.contiguous())
        return dq, dgamma, dbeta, None, None, None, None, None, None, None


def trxl_memory_attention(q, gamma, beta, memory, layer: int, ep, rows, pos, mask, pe):
    """``TrXLMemoryAttention.apply`` when a gradient is wanted, else the forward alone (the rollout step, the bootstrap)."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, gamma, beta)):
        return TrXLMemoryAttention.apply(q, gamma, beta, memory, layer, ep, rows, pos, mask, pe)
    fwd, _ = twins(q, *_TRXL)
    memory, ep, rows, pos, mask, pe = _trxl_inputs(memory, ep, rows, pos, mask, pe)
    u, _ = fwd(memory, layer, ep, rows, pos, mask, pe, gamma.detach().contiguous(), beta.detach().contiguous(), q.detach().contiguous())
    return u


# ------------------------------------------------------------------------------------------- TrXL: a whole layer (csrc/trxl_layer.hip)
# the 13 parameters of agents.TrXLTransformerLayer in module order; norm_kv's two belong to the attention kernel
TRXL_LAYER_PARAMS = ("attention.values.weight", "attention.keys.weight", "attention.queries.weight", "attention.fc_out.weight",
                     "attention.fc_out.bias", "layer_norm_q.weight", "layer_norm_q.bias", "norm_kv.weight", "norm_kv.bias",
                     "layer_norm_attn.weight", "layer_norm_attn.bias", "fc_projection.0.weight", "fc_projection.0.bias")
_TRXL_NORM_KV = (7, 8)
TRXL_LAYER_SAVED = ("x1", "f", "n1", "n2", "df", "dx1")


def trxl_layer_supported(D: int, H: int) -> bool:
    return _lib.load().mi355ppo_trxl_layer_pack_bytes(int(D), int(H)) > 0


class TrXLLayerPack:
    """The derived weights of one TransformerLayer for the ``layer`` kernels: A = blockdiag(Wq^T Wk), Wvo = blockdiag(Wv^T) Wo^T and Wp as
    split f16 fragments, with the biases and LayerNorm vectors.  Valid for ``(the 13 tensors' version counters, their addresses)`` and
    re-derived INTO the same buffer when that tag moved (``Mlp256Nets.pack``'s rule): an optimizer's in-place step advances the counters.
    ``slabs``: the weight gradient's slab count (0: the library's default)."""

    def __init__(self, D: int, H: int, device, slabs: int = 0):
        if not trxl_layer_supported(D, H):
            raise ValueError(f"TrXL layer kernels: D={D} H={H} (need D % 64 == 0, D <= 512, H dividing 64)")
        self.D, self.H, self.device, self.slabs = int(D), int(H), torch.device(device), int(slabs)
        self._pack = None            # (tag, uint8 tensor)

    def _check(self, params):
        D, d = self.D, self.D // self.H
        shapes = [(d, d)] * 3 + [(D, D)] + [(D,)] * 7 + [(D, D), (D,)]
        assert len(params) == len(shapes), "a TransformerLayer has 13 parameters"
        return [_chk(p, torch.float32, n, s) for p, n, s in zip(params, TRXL_LAYER_PARAMS, shapes)]

    def pack(self, params, out=None):
        params = self._check([p.detach() for p in params])
        tag = (tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
        if out is not None or self._pack is None or self._pack[0] != tag:
            nbytes = _lib.load().mi355ppo_trxl_layer_pack_bytes(self.D, self.H)
            buf = out if out is not None else self._pack[1] if self._pack is not None else torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _launch("mi355ppo_trxl_layer_pack_f32", self.device, twin_ops._ptr_array(params), self.D, self.H, _ptr(buf), buf.numel())
            self._pack = (tag, buf)
        return self._pack[1]

    def workspace(self, B: int):
        """A fresh workspace for one forward / backward pair of ``B`` rows (the autograd node keeps it until its backward ran)."""
        return torch.empty(_lib.load().mi355ppo_trxl_layer_workspace_bytes(int(B), self.D, self.H), dtype=torch.uint8, device=self.device)

    def saved(self, ws, B: int):
        """Views of a workspace's (B, D) planes by name (``TRXL_LAYER_SAVED``)."""
        f, n = ws.view(torch.float32), B * self.D
        return {k: f[i * n:(i + 1) * n].view(B, self.D) for i, k in enumerate(TRXL_LAYER_SAVED)}


def _trxl_layer_call(name, pk: TrXLLayerPack, pack, ws, out, *ins):
    B = ins[0].shape[0]
    for i, t in enumerate(ins):
        _chk(t, torch.float32, f"{name} input {i}", (B, pk.D))
    out = torch.empty((B, pk.D), dtype=torch.float32, device=pk.device) if out is None else _chk(out, torch.float32, "out", (B, pk.D))
    _launch(name, pk.device, *[_ptr(t) for t in ins], B, pk.D, pk.H, _ptr(pack), _ptr(out), _ptr(ws), 0 if ws is None else ws.numel())
    return out


def trxl_layer_pre_forward(x, pk, pack, ws=None, out=None):
    """q~ = LN_q(x) A (B, D); with ``ws`` the backward's LN_q(x) and statistics are saved."""
    return _trxl_layer_call("mi355ppo_trxl_layer_pre_fwd_f32", pk, pack, ws, out, x)


def trxl_layer_post_forward(x, u, pk, pack, ws=None, out=None):
    """y = relu(LN_attn(x1) Wp^T + b_p) + x1, x1 = (u Wvo + b_o) + x; with ``ws`` x1, the ReLU output and LN_attn(x1) are saved."""
    return _trxl_layer_call("mi355ppo_trxl_layer_post_fwd_f32", pk, pack, ws, out, x, u)


def trxl_layer_post_backward(dy, pk, pack, ws, out=None):
    """du of the attention's output from dy; df and dx1 stay in ``ws``."""
    return _trxl_layer_call("mi355ppo_trxl_layer_post_bwd_f32", pk, pack, ws, out, dy)


def trxl_layer_pre_backward(dqt, x, pk, pack, ws, out=None):
    """dx from the attention backward's dq~ and the skip's dx1 in ``ws``."""
    return _trxl_layer_call("mi355ppo_trxl_layer_pre_bwd_f32", pk, pack, ws, out, dqt, x)


def trxl_layer_wgrad(u, dqt, params, grads, pk, ws, slabs: int = 0):
    """The eleven parameter gradients of the dense half, ADDED into ``grads`` (13 tensors in ``TRXL_LAYER_PARAMS`` order; norm_kv's are
    left alone)."""
    B = u.shape[0]
    _chk(u, torch.float32, "u", (B, pk.D))
    _chk(dqt, torch.float32, "dqt", (B, pk.D))
    params = pk._check([p.detach() for p in params])
    for g, p in zip(grads, params):
        _chk(g, torch.float32, "grad", p.shape)
    _launch("mi355ppo_trxl_layer_wgrad_f32", pk.device, _ptr(u), _ptr(dqt), twin_ops._ptr_array(params), twin_ops._ptr_array(list(grads)), B, pk.D, pk.H,
            int(slabs), _ptr(ws), ws.numel())


def _trxl_layer_forward(x, params, pk, memory, layer, ep, rows, pos, mask, pe, ws):
    B, D, H = x.shape[0], pk.D, pk.H
    pack = pk.pack(params)
    qt = trxl_layer_pre_forward(x, pk, pack, ws)
    u, stats = trxl_attn_forward(memory, layer, ep, rows, pos, mask, pe, params[7].detach().contiguous(), params[8].detach().contiguous(),  # noqa: F821
                                 qt.view(B, H, D // H))
    return pack, qt, u, stats, trxl_layer_post_forward(x, u.view(B, D), pk, pack, ws)


class TrXLLayer(torch.autograd.Function):
    """Differentiable ``(x, the layer's 13 parameters; memory, layer, ep, rows, pos, mask, pe, pack holder) -> y``: one whole
    TransformerLayer of ppo_trxl.py -- pre (LN_q, q~) -> ``TrXLMemoryAttention``'s kernels -> post (values / fc_out, skip, LN_attn,
    fc_projection, skip) -- and the same in reverse, on csrc/trxl_layer.hip and csrc/trxl_attn.hip.  CUDA tensors only."""

    @staticmethod
    def forward(ctx, x, *rest):
        params, (memory, layer, ep, rows, pos, mask, pe, pk) = rest[:13], rest[13:]
        memory, ep, rows, pos, mask, pe = _trxl_inputs(memory, ep, rows, pos, mask, pe)
        x = x.detach().contiguous()
        ws = pk.workspace(x.shape[0])
        pack, qt, u, stats, y = _trxl_layer_forward(x, params, pk, memory, layer, ep, rows, pos, mask, pe, ws)
        ctx.layer, ctx.pk, ctx.pack, ctx.has_pe = layer, pk, pack, pe is not None
        ctx.save_for_backward(x, qt, u, stats, ws, memory, ep, rows, mask, *(() if pe is None else (pos, pe)), *params)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, qt, u, stats, ws, memory, ep, rows, mask, *tail = ctx.saved_tensors
        (pos, pe), params = (tail[:2], tail[2:]) if ctx.has_pe else ((None, None), tail)
        pk, pack = ctx.pk, ctx.pack
        B, D, H = x.shape[0], pk.D, pk.H
        du = trxl_layer_post_backward(dy.contiguous(), pk, pack, ws)
        gkv, bkv = params[7].detach().contiguous(), params[8].detach().contiguous()
        dqt, dgkv, dbkv = trxl_attn_backward(memory, ctx.layer, ep, rows, pos, mask, pe, gkv, bkv, qt.view(B, H, D // H), u, stats,  # noqa: F821
                                             du.view(B, H, D // H))
        dqt = dqt.view(B, D)
        dx = trxl_layer_pre_backward(dqt, x, pk, pack, ws)
        grads = [dgkv if i == 7 else dbkv if i == 8 else torch.zeros_like(p) for i, p in enumerate(params)]
        trxl_layer_wgrad(u.view(B, D), dqt, params, grads, pk, ws, pk.slabs)
        return (dx, *grads, None, None, None, None, None, None, None, None)


def trxl_layer(x, params, pk: TrXLLayerPack, memory, layer: int, ep, rows, pos, mask, pe):
    """``TrXLLayer.apply`` when a gradient is wanted, else the two forward launches around the attention forward with nothing saved (the
    rollout step, the bootstrap value)."""
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return TrXLLayer.apply(x, *params, memory, layer, ep, rows, pos, mask, pe, pk)
    memory, ep, rows, pos, mask, pe = _trxl_inputs(memory, ep, rows, pos, mask, pe)
    return _trxl_layer_forward(x.detach().contiguous(), params, pk, memory, layer, ep, rows, pos, mask, pe, None)[4]


# ------------------------------------------------------------------------------------------- IMPALA-CNN trunks
def _impala_trunk(f: ImpalaFamily, name: str, what: str):
    """The autograd node and the grad-or-not dispatcher of one trunk family (twin_ops.IMPALA64 / IMPALA84)."""
    names = (name + "_forward", name + "_backward")
    H, W, C = f.frame

    def forward(ctx, x, *params):
        ctx.flagged = bool(params) and isinstance(params[-1], bool)              # ``(x, *params, pooled)``: the 64 family's trailing flag
        if ctx.flagged:
            *params, pooled = params
        kw = {"pooled": True} if ctx.flagged and pooled else {}
        fwd, _ = twins(x, *names)
        xs = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in params]
        impala_check(f, xs, ps)
        y, saved, arg = fwd(xs, ps, **kw)
        ctx.save_for_backward(xs, saved, arg, *ps)
        ctx.kw = kw
        return y

    def backward(ctx, dy):
        xs, saved, arg, *ps = ctx.saved_tensors
        _, bwd = twins(xs, *names)
        return (None, *bwd(xs, ps, saved, arg, dy.contiguous(), **ctx.kw), *((None,) if ctx.flagged else ()))

    doc = (f"Differentiable ``(x, *params) -> y``: the three ConvSequences of {what} on channels-last {f.frames} x (B,{H},{W},{C}) "
           f"{f.suffix}, y (B,{','.join(map(str, f.out))}) channels-last.  The backward returns the 30 parameter gradients and None "
           f"for the frames (no input gradient is computed).  The HIP kernels run for CUDA tensors, the host twins for CPU ones "
           f"(same arithmetic).  The 64x64x3 family also takes ``(x, *params, pooled)``: a trailing bool that picks the kernels with "
           f"the max pools fused into the conv launches (same bits; one more None from the backward).")
    # created under its own name: autograd names the backward node (``ImpalaTrunkBackward``) when the class is made
    Trunk = type(name.capitalize() + "Trunk", (torch.autograd.Function,),
                 {"__doc__": doc, "__module__": __name__, "forward": staticmethod(forward), "backward": staticmethod(backward)})

    def trunk(x, params, pooled: bool = False):
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return Trunk.apply(x, *params, True) if pooled else Trunk.apply(x, *params)
        fwd, _ = twins(x, *names)
        ps = [p.detach().contiguous() for p in params]
        impala_check(f, x, ps)
        return fwd(x.contiguous(), ps, **({"pooled": True} if pooled else {}))[0]

    trunk.__doc__ = (f"``{name.capitalize()}Trunk.apply`` when a gradient is wanted, else the forward alone (acting, an old-policy or target pass).  "
                     f"``pooled`` (the 64x64x3 family): the kernels with the max pools fused into the conv launches, same bits.")
    trunk.__name__ = trunk.__qualname__ = name + "_trunk"
    return Trunk, trunk


ImpalaTrunk, impala_trunk = _impala_trunk(IMPALA64, "impala", "the IMPALA-CNN (ppo_procgen.py / ppg_procgen.py)")
Impala84Trunk, impala84_trunk = _impala_trunk(IMPALA84, "impala84", "the Atari IMPALA-CNN (qdagger_dqn_atari_impalacnn.py)")


def impala_param_shapes():
    """The 30 trunk parameters' shapes in state_dict order (per sequence: conv, res_block0.conv0 / conv1, res_block1.conv0 / conv1;
    weight then bias)."""
    return impala_family_param_shapes(IMPALA64)


def impala84_param_shapes():
    """The 30 trunk parameters' shapes of the Atari IMPALA-CNN (qdagger_dqn_atari_impalacnn.py:164-181) in state_dict order."""
    return impala_family_param_shapes(IMPALA84)


def impala84_params(net):
    """The trunk's 30 parameters of a module whose ``network[0..2]`` are the three ConvSequences."""
    return [p for i in range(3) for p in net.network[i].parameters()]


def synth_continuous_step(state, reset_state, At, Bm, w, noise, k: int, steps, horizon: float, action, obs_out, reward, done, k_base=None):
    """One step of the device-resident continuous-control stand-in env (test / bench support, not the reference path)."""
    N, O = state.shape
    D = action.shape[1]
    bank = noise.shape[0]
    for t, nm, shp in ((state, "state", (N, O)), (reset_state, "reset_state", (N, O)), (At, "At", (O, O)), (Bm, "Bm", (D, O)), (w, "w", (O,)),
                       (noise, "noise", (bank, N, O)), (steps, "steps", (N,)), (action, "action", (N, D)), (obs_out, "obs_out", (N, O)),
                       (reward, "reward", (N,)), (done, "done", (N,))):
        _chk(t, torch.float32, nm, shp)
    if k_base is not None:
        _chk(k_base, torch.int64, "k_base", (1,))
    dev = state.device
    _launch("mi355ppo_synth_continuous_step_f32", dev, _ptr(state), _ptr(reset_state), _ptr(At), _ptr(Bm), _ptr(w), _ptr(noise), bank,
            int(k) & (2**64 - 1), _ptr(k_base), _ptr(steps), float(horizon), _ptr(action), _ptr(obs_out), _ptr(reward), _ptr(done), N, O, D)


# ------------------------------------------------------------------------------------------- PQN: what has no host twin
def conv1q1_fwd_amax(obs_u8, pack, bias, inds, out, bits, dst_amax):
    """``twin_ops.conv1q1_fwd`` into the caller's ``out`` with the amax record ``dst_amax``, as cleanrl_amd/cnn.py's one-frame trunk
    calls it; both are required."""
    if out is None or dst_amax is None:
        raise TypeError(f"conv1q1_fwd_amax: expected CUDA/HIP tensors for out and dst_amax, got {type(out).__name__} / {type(dst_amax).__name__}")
    return twin_ops.conv1q1_fwd(_SIDE, obs_u8, pack, bias, inds, out, bits, dst_amax)


def conv1q1_fwd_bits(obs_u8, pack, bias, inds, out, bits):
    """The same without the amax record; ``bits`` is required."""
    if bits is None:
        raise ValueError("conv1q1_fwd_bits: the mask words are required")
    if out is None:
        raise TypeError("conv1q1_fwd_bits: expected a CUDA/HIP tensor for out, got NoneType")
    return twin_ops.conv1q1_fwd(_SIDE, obs_u8, pack, bias, inds, out, bits)


def conv1p1_wgrad(obs_u8, dz, dz_amax, inds=None, out=None):
    """``(dW (32, 1, 8, 8), db (32,))`` of ``Conv2d(1, 32, 8, stride=4)`` from the uint8 frames (rows, 84, 84) through ``inds`` and the
    pre-activation gradient ``dz`` (M, 20, 20, 32) with its amax record (kernel P1: dz in two f16 terms, exact frame operand, fixed-order
    fold -- the same input gives the same bits)."""
    frames = twin_ops.frames_u8(_SIDE, obs_u8, "conv1p1_wgrad")
    images = dz.shape[0]
    _chk(dz, torch.float32, "dz", (images, 20, 20, 32))
    if inds is not None:
        _chk(inds, torch.int64, "inds", (images,))
    elif frames.shape[0] != images:
        raise ValueError(f"conv1p1_wgrad: {frames.shape[0]} frames for {images} rows of dz")
    _chk(dz_amax, torch.int32, "dz_amax", (AMAX_WORDS,))
    dev = dz.device
    if out is not None:
        dW, db = _chk(out[0], torch.float32, "dW", (32, 1, 8, 8)), _chk(out[1], torch.float32, "db", (32,))
    else:
        dW, db = torch.empty((32, 1, 8, 8), dtype=torch.float32, device=dev), torch.empty(32, dtype=torch.float32, device=dev)
    ws = _workspace(dev, _lib.load().mi355ppo_cnn_conv1p1_wgrad_workspace_bytes(images))
    _launch("mi355ppo_cnn_conv1p1_wgrad_f16x2", dev, _ptr(frames), _ptr(inds), _ptr(dz), _ptr(dW), _ptr(db), images, _ptr(ws), ws.numel(),
            _ptr(dz_amax))
    return dW, db


def radam_schedule(lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999):
    """The 8-float schedule slot of RAdam step ``step`` (1-based), as the library forms it (host floats)."""
    out = (ctypes.c_float * 8)()
    _lib.call("mi355ppo_radam_schedule_f32", float(lr), float(beta1), float(beta2), int(step), out)
    return [float(x) for x in out]


def clip_radam_sched_(params, grads, exp_avg, exp_avg_sq, sched8, max_grad_norm: float, beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8, total_norm_out=None):
    """``clip_radam_`` (cleanrl_amd/twin_ops.py) with the step's slot (``radam_schedule`` values) read from the 8-float DEVICE tensor
    ``sched8``: capturable.  Its host twin is ``clip_radam_``'s."""
    lib = _lib.load()
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nm, (n,))
    _chk(sched8, torch.float32, "sched8", (8,))
    dev = params.device
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_clip_radam_workspace_bytes(n))
    _launch("mi355ppo_clip_radam_sched_f32", dev, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(max_grad_norm),
            float(beta1), float(beta2), float(eps), _ptr(sched8), _ptr(total_norm_out), _ptr(ws), ws.numel())
    return total_norm_out


# ------------------------------------------------------------------------------------------- the operators defined once for both sides
# The device side of cleanrl_amd/replay_ops.py, rnd_ops.py (§3.22), ppg_ops.py (§3.23) and twin_ops.py: ``_chk``, the
# workspace of the entry point's ``*_workspace_bytes``, the current stream.
from .replay_ops import (ATARI_FRAME, DQN_HEAD_HIDDEN, DQN_HEAD_MAX_OUT, DQN_HEAD_MAX_ROWS, DQN_HIDDEN, DQN_MAX_ACT, DQN_MAX_ATOMS,  # noqa: E402,F401
                         DQN_MAX_OBS, DQN_MAX_OUT, OFFPOLICY_HIDDEN, OFFPOLICY_MAX_ACT, OFFPOLICY_MAX_OBS, QDAGGER_HIDDEN, QDAGGER_MAX_ROWS,
                         RAINBOW_HEAD_IN, RAINBOW_MAX_BATCH, dqn_counts, dqn_head_limits_ok, dqn_limits_ok, offpolicy_counts,
                         qdagger_head_limits_ok, rainbow_head_limits_ok, rainbow_new_buffer, rainbow_noisy_counts, rainbow_noisy_limits_ok,
                         sac_actor_count, sacd_limits_ok)


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)          # this module's ``torch``: the guard-band tests carve allocations by patching it


def _device_launch(name: str, dev: torch.device, *args) -> None:
    _launch(name, dev, *args)                                   # looked up at call time: the tests count launches on ``ops._launch``


def _device_launch_ws(name: str, dev: torch.device, ws_bytes: str, dims, *args) -> None:
    ws = _workspace(dev, getattr(_lib.load(), ws_bytes)(*dims))
    _launch(name, dev, *args, _ptr(ws), ws.numel())


from .ppg_ops import PPG_HIDDEN, PPG_MAX_ACT, PPG_MAX_ROWS, PPG_MIN_ACT  # noqa: E402,F401
from .rnd_ops import RND_FEATURES, RND_MAX_BATCH, RND_MAX_STEPS, RND_PIXELS, rnd_mean_var  # noqa: E402,F401

_SIDE = replay_ops.Side(False, _chk, _device_launch, _device_launch_ws, _empty)
for _module in (replay_ops, rnd_ops, ppg_ops, twin_ops):
    replay_ops.bind(_module, _SIDE, globals())
