"""Tensor-level operators over ``libmi355ppo.so`` -- the Python host side of the C ABI.

Each function mirrors one seam of the reference's inline PPO code (cited per function) and takes
CUDA (=HIP) ``torch`` tensors only: torch is plumbing here (device memory + the current stream), the
computation is the HIP kernels.  Every wrapper ends in ``_launch(symbol, device, *args)``: the entry point on the device's current
stream, a non-zero status raised as ``Mi355PpoError`` naming that symbol.  Passing a CPU tensor raises; there is no CPU fallback in
this module.  The one exception is ``twins``: the autograd nodes ``LSTMSeq`` / ``lstm_seq``, ``TrXLMemoryAttention`` /
``trxl_memory_attention`` and ``ImpalaTrunk`` / ``impala_trunk`` (and the TrXL / PQN learners, for their whole device) take CPU tensors
to the host twins (cleanrl_amd/host_ops.py) on purpose: the agent's host path and the tests run the same arithmetic as the device
kernels.  The operators of the replay-ring families (``replay_add`` .. ``sacd_actor_fwd_bwd``) are defined in
cleanrl_amd/replay_ops.py, once for this module and host_ops, and bound at the end of this file to the device side.
"""
from __future__ import annotations

import ctypes
import sys

import torch

from . import _lib, ppg_ops, replay_ops, rnd_ops
from .replay_ops import _ptr

__all__ = [
    "gae", "categorical_sample", "categorical_logprob_entropy", "normal_sample", "normal_logprob_entropy",
    "ppo_loss_categorical", "ppo_loss_normal", "obs_u8_to_f32", "obs_nchw_to_nhwc_u8", "clip_adam_", "PPOLossCategorical", "PPOLossNormal",
    "CategoricalLogProbEntropy", "NormalLogProbEntropy", "LOSS_SCALAR_NAMES", "lstm_seq_forward", "lstm_seq_backward", "LSTMSeq",
    "lstm_seq", "lstm_seq_dw_hh", "impala_forward", "impala_backward", "impala_maxpool_forward", "impala_maxpool_backward",
    "ImpalaTrunk", "impala_trunk", "impala_param_shapes", "impala84_forward", "impala84_backward", "Impala84Trunk", "impala84_trunk",
    "impala84_param_shapes", "impala84_params", "qdagger_head_limits_ok", "qdagger_head_act", "qdagger_head_fwd_bwd", "trxl_attn_forward", "trxl_attn_backward", "TrXLMemoryAttention", "trxl_memory_attention",
    "pqn_param_count", "pqn_egreedy", "pqn_qlambda", "pqn_td_loss", "pqn_mlp_forward", "pqn_mlp_act", "pqn_mlp_td_fwd_bwd", "radam_schedule",
    "clip_radam_", "clip_radam_sched_", "pqn_lstm_act", "pqn_lstm_td_fwd_bwd", "offpolicy_counts", "replay_add", "ddpg_act", "td3_target",
    "td3_critic_fwd_bwd", "td3_actor_fwd_bwd", "polyak_", "sac_actor_count", "sac_policy", "sac_target", "sac_actor_fwd_bwd", "sac_alpha_",
    "dqn_counts", "dqn_limits_ok", "dqn_act", "dqn_td_fwd_bwd", "c51_fwd_bwd",
    "dqn_head_limits_ok", "replay_add_u8", "replay_gather_u8", "dqn_head_act", "dqn_head_td_fwd_bwd", "c51_head_fwd_bwd",
    "rainbow_noisy_limits_ok", "rainbow_noisy_counts", "rainbow_new_buffer", "rainbow_per_add_u8", "rainbow_per_sample", "rainbow_per_gather_u8",
    "rainbow_per_update", "rainbow_noisy_compose", "rainbow_noisy_grad", "rainbow_head_limits_ok", "rainbow_head_act", "rainbow_head_fwd_bwd",
    "sacd_limits_ok", "replay_add2_u8", "replay_gather2_u8", "sacd_head_act", "sacd_critic_fwd_bwd", "sacd_actor_fwd_bwd",
    "rnd_normalize", "rnd_obs_moments", "rnd_mean_var", "rnd_intrinsic_reward", "rnd_reward_filter_", "rnd_loss_fwd_bwd",
    "ppg_aux_gather", "ppg_old_logits_", "ppg_aux_fwd_bwd", "clip_adam_split_",
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


def _ptr_array(ts):
    """A host array of the tensors' data pointers (a network's parameters / gradients as the C ABI takes them)."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


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


# ------------------------------------------------------------------------------------------- LSTM
def _lstm_dims(gx, done):
    if gx.dim() != 3 or gx.shape[2] % 4:
        raise ValueError(f"gx: expected (T, B, 4H), got {tuple(gx.shape)}")
    T, B, G = gx.shape
    if tuple(done.shape) != (T, B):
        raise ValueError(f"done: expected (T, B) = {(T, B)}, got {tuple(done.shape)}")
    return T, B, G // 4


def lstm_seq_forward(gx, w_hh, h0, c0, done, record: bool = False):
    """The done-masked LSTM scan of ppo_atari_lstm.py:140-158 (``get_states``) in one launch: ``gx`` (T,B,4H) = x W_ih^T + b_ih +
    b_hh, ``w_hh`` (4H,H), ``h0`` / ``c0`` (B,H), ``done`` (T,B); H = 128.  Returns ``(h (T,B,H), hT, cT, record | None)``; the
    record (7 T B H floats, layout in include/mi355ppo.h) feeds ``lstm_seq_backward``."""
    T, B, H = _lstm_dims(gx, done)
    _chk(gx, torch.float32, "gx", (T, B, 4 * H))
    _chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    _chk(h0, torch.float32, "h0", (B, H))
    _chk(c0, torch.float32, "c0", (B, H))
    _chk(done, torch.float32, "done", (T, B))
    dev = gx.device
    h = torch.empty((T, B, H), device=dev)
    hT, cT = torch.empty((B, H), device=dev), torch.empty((B, H), device=dev)
    rec = torch.empty(7 * T * B * H, device=dev) if record else None
    _launch("mi355ppo_lstm_seq_fwd_f32", dev, _ptr(gx), _ptr(w_hh), _ptr(h0), _ptr(c0), _ptr(done), _ptr(h), _ptr(hT), _ptr(cT), _ptr(rec),
            T, B, H)
    return h, hT, cT, rec


def lstm_seq_backward(dh, dhT, dcT, record, w_hh, done, want_dh0: bool = True, want_dc0: bool = True):
    """Backward of ``lstm_seq_forward`` (BPTT with the state gradient masked by keep_t): ``dh`` (T,B,H) from the heads, ``dhT`` /
    ``dcT`` (B,H) or None.  Returns ``(dgx (T,B,4H), dh0 | None, dc0 | None)``; dW_hh = dgx^T hk is the caller's GEMM."""
    T, B, H = dh.shape
    _chk(dh, torch.float32, "dh", (T, B, H))
    if dhT is not None:
        _chk(dhT, torch.float32, "dhT", (B, H))
    if dcT is not None:
        _chk(dcT, torch.float32, "dcT", (B, H))
    _chk(record, torch.float32, "record", (7 * T * B * H,))
    _chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    _chk(done, torch.float32, "done", (T, B))
    dev = dh.device
    dgx = torch.empty((T, B, 4 * H), device=dev)
    dh0 = torch.empty((B, H), device=dev) if want_dh0 else None
    dc0 = torch.empty((B, H), device=dev) if want_dc0 else None
    _launch("mi355ppo_lstm_seq_bwd_f32", dev, _ptr(dh), _ptr(dhT), _ptr(dcT), _ptr(record), _ptr(w_hh), _ptr(done), _ptr(dgx), _ptr(dh0),
            _ptr(dc0), T, B, H)
    return dgx, dh0, dc0


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
def trxl_dims(memory, rows, q):
    """(E, T_ep, layers, D, B, L, H) of one attention call; shapes as in include/mi355ppo.h (TRXL)."""
    if memory.dim() != 4:
        raise ValueError(f"memory: expected (E, T_ep, layers, D), got {tuple(memory.shape)}")
    if rows.dim() != 2 or q.dim() != 3:
        raise ValueError(f"rows: expected (B, L), q: expected (B, H, d); got {tuple(rows.shape)}, {tuple(q.shape)}")
    E, T, layers, D = memory.shape
    B, L = rows.shape
    H = q.shape[1]
    if tuple(q.shape) != (B, H, D // max(H, 1)) or H * q.shape[2] != D:
        raise ValueError(f"q: expected (B={B}, H, D/H) with D={D}, got {tuple(q.shape)}")
    return E, T, layers, D, B, L, H


def _trxl_checked(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q):
    E, T, layers, D, B, L, H = trxl_dims(memory, rows, q)
    _chk(memory, torch.float32, "memory")
    _chk(ep, torch.int64, "ep", (B,))
    _chk(rows, torch.int64, "rows", (B, L))
    _chk(mask, torch.uint8, "mask", (B, L))
    if pe is not None:
        _chk(pe, torch.float32, "pe")
        _chk(pos, torch.int64, "pos", (B, L))
    _chk(gamma, torch.float32, "gamma", (D,))
    _chk(beta, torch.float32, "beta", (D,))
    _chk(q, torch.float32, "q", (B, H, D // H))
    return E, T, layers, D, B, L, H


def _trxl_launch(name: str, dev, err, *args) -> None:
    """``_launch`` with the call's error word between ``args`` and the four sizes: a caller-owned ``err`` is zeroed and left unread;
    with None one is allocated and read back (one sync) unless the stream is being captured into a graph."""
    own = err is None
    err = torch.zeros(1, dtype=torch.int32, device=dev) if own else err.zero_()
    _launch(name, dev, *args[:-4], _ptr(err), *args[-4:])
    if own and not torch.cuda.is_current_stream_capturing() and int(err.item()) != 0:
        raise IndexError(f"{name}: an episode, row or position index was outside the memory / pe table (clamped on the device)")


def trxl_attn_forward(memory, layer: int, ep, rows, pos, mask, pe, gamma, beta, q, err=None):
    """The episodic-memory attention of one TrXL layer (ppo_trxl.py: MultiHeadAttention.forward over norm_kv of the window
    rows): ``u`` (B,H,d) = sum_j softmax(s)_j LN(mem[ep, rows_j, layer] + pe[pos_j])_h and ``stats`` (B,H,2) (max, sum) for the
    backward.  ``q`` is q~ = W_k^T q (``q @ keys.weight``); ``pe`` may be None.  ``err`` (int32, 1 element): a caller-owned
    error word (zeroed here, left unread); with None one is allocated and checked after the launch."""
    E, T, layers, D, B, L, H = _trxl_checked(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q)
    dev = q.device
    u = torch.empty((B, H, D // H), device=dev)
    stats = torch.empty((B, H, 2), device=dev)
    P = 0 if pe is None else pe.shape[0]
    _trxl_launch("mi355ppo_trxl_attn_fwd_f32", dev, err, _ptr(memory), E, T, layers, int(layer), _ptr(ep), _ptr(rows), _ptr(pos),
                 _ptr(mask), _ptr(pe), P, _ptr(gamma), _ptr(beta), _ptr(q), _ptr(u), _ptr(stats), B, L, D, H)
    return u, stats


def trxl_attn_backward(memory, layer: int, ep, rows, pos, mask, pe, gamma, beta, q, u, stats, du, err=None):
    """Backward of ``trxl_attn_forward`` -> (dq (B,H,d), dgamma (D), dbeta (D)); no gradient reaches the memory."""
    E, T, layers, D, B, L, H = _trxl_checked(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q)
    _chk(u, torch.float32, "u", (B, H, D // H))
    _chk(stats, torch.float32, "stats", (B, H, 2))
    _chk(du, torch.float32, "du", (B, H, D // H))
    dev = q.device
    dq = torch.empty((B, H, D // H), device=dev)
    rows_ws = torch.empty((2, B, D), device=dev)
    dgamma, dbeta = torch.empty(D, device=dev), torch.empty(D, device=dev)
    P = 0 if pe is None else pe.shape[0]
    _trxl_launch("mi355ppo_trxl_attn_bwd_f32", dev, err, _ptr(memory), E, T, layers, int(layer), _ptr(ep), _ptr(rows), _ptr(pos),
                 _ptr(mask), _ptr(pe), P, _ptr(gamma), _ptr(beta), _ptr(q), _ptr(u), _ptr(stats), _ptr(du), _ptr(dq), _ptr(rows_ws),
                 _ptr(dgamma), _ptr(dbeta), B, L, D, H)
    return dq, dgamma, dbeta


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


# ------------------------------------------------------------------------------------------- IMPALA-CNN trunk
IMPALA_CHANNELS = (16, 32, 32)
IMPALA_FRAME = (64, 64, 3)


def impala_param_shapes():
    """The 30 trunk parameters' shapes in state_dict order (per sequence: conv, res_block0.conv0 / conv1, res_block1.conv0 / conv1;
    weight then bias)."""
    shapes, cin = [], IMPALA_FRAME[2]
    for c in IMPALA_CHANNELS:
        for i in range(5):
            ci = cin if i == 0 else c
            shapes += [(c, ci, 3, 3), (c,)]
        cin = c
    return shapes


def _impala_check(x, params):
    if x.dim() != 4 or tuple(x.shape[1:]) != IMPALA_FRAME or x.shape[0] < 1:
        raise ValueError(f"x: expected channels-last frames (B, 64, 64, 3), got {tuple(x.shape)}")
    if len(params) != 30:
        raise ValueError(f"params: expected the trunk's 30 weights and biases, got {len(params)}")
    for i, (p, shp) in enumerate(zip(params, impala_param_shapes())):
        if tuple(p.shape) != shp:
            raise ValueError(f"params[{i}]: expected shape {shp}, got {tuple(p.shape)} (channels must be {list(IMPALA_CHANNELS)})")


def impala_forward(x, params):
    """The IMPALA-CNN trunk (ppo_procgen.py:86-124 / ppg_procgen.py:123-165, three ConvSequences) on the HIP kernels of
    csrc/impala.hip: x (B,64,64,3) f32 channels-last frames, params the 30 conv weights / biases in state_dict order.
    Returns ``(y (B,8,8,32) channels-last, saved, argmax)``; the last two feed ``impala_backward``."""
    lib = _lib.load()
    _impala_check(x, params)
    _chk(x, torch.float32, "x")
    for i, p in enumerate(params):
        _chk(p, torch.float32, f"params[{i}]")
    B, dev = x.shape[0], x.device
    y = torch.empty((B, 8, 8, 32), device=dev)
    saved = torch.empty(int(lib.mi355ppo_impala_saved_floats(B)), device=dev)
    arg = torch.empty(int(lib.mi355ppo_impala_argmax_bytes(B)), dtype=torch.uint8, device=dev)
    nws = int(lib.mi355ppo_impala_workspace_bytes(B, 0))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _launch("mi355ppo_impala_fwd_f32", dev, _ptr(x), _ptr_array(params), _ptr(y), _ptr(saved), _ptr(arg), B, *IMPALA_FRAME,
            *IMPALA_CHANNELS, _ptr(ws), nws)
    return y, saved, arg


def impala_backward(x, params, saved, arg, dy):
    """Backward of ``impala_forward``: dy (B,8,8,32) channels-last -> the 30 parameter gradients (one flat buffer's views, written
    by deterministic fixed-order folds); no input gradient."""
    lib = _lib.load()
    _impala_check(x, params)
    B, dev = x.shape[0], x.device
    _chk(dy, torch.float32, "dy", (B, 8, 8, 32))
    _chk(saved, torch.float32, "saved", (int(lib.mi355ppo_impala_saved_floats(B)),))
    _chk(arg, torch.uint8, "argmax", (int(lib.mi355ppo_impala_argmax_bytes(B)),))
    flat = torch.empty(sum(p.numel() for p in params), device=dev)
    grads, o = [], 0
    for p in params:
        grads.append(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()
    nws = int(lib.mi355ppo_impala_workspace_bytes(B, 1))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _launch("mi355ppo_impala_bwd_f32", dev, _ptr(x), _ptr_array(params), _ptr(saved), _ptr(arg), _ptr(dy), _ptr_array(grads), B,
            *IMPALA_FRAME, *IMPALA_CHANNELS, _ptr(ws), nws)
    return grads


def impala_maxpool_forward(x):
    """The trunks' max pool (3, stride 2, pad 1) alone on channels-last x (B,H,W,C) -> (y, argmax bytes (B,(H+1)/2,(W+1)/2,C))."""
    _chk(x, torch.float32, "x")
    B, H, W, C = x.shape
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), device=x.device)
    arg = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.uint8, device=x.device)
    _launch("mi355ppo_impala_maxpool_fwd_f32", x.device, _ptr(x), _ptr(y), _ptr(arg), B, H, W, C)
    return y, arg


def impala_maxpool_backward(dy, arg, size=None):
    """Backward of ``impala_maxpool_forward``: dx (B,H,H,C), H = ``size`` (default 2 Ho; the 21 -> 11 pool needs it said)."""
    _chk(dy, torch.float32, "dy")
    B, Ho, Wo, C = dy.shape
    _chk(arg, torch.uint8, "argmax", tuple(dy.shape))
    H = 2 * Ho if size is None else int(size)
    dx = torch.empty((B, H, H, C), device=dy.device)
    _launch("mi355ppo_impala_maxpool_bwd_f32", dy.device, _ptr(dy), _ptr(arg), _ptr(dx), B, H, H, C)
    return dx


_IMPALA = ("impala_forward", "impala_backward")


class ImpalaTrunk(torch.autograd.Function):
    """Differentiable ``(x, *params) -> y``: the three ConvSequences of the IMPALA-CNN on channels-last frames x (B,64,64,3),
    y (B,8,8,32) channels-last.  The backward returns the 30 parameter gradients and None for the frames (no input gradient
    is computed).  The HIP kernels run for CUDA tensors, the host twins for CPU ones (same arithmetic)."""

    @staticmethod
    def forward(ctx, x, *params):
        fwd, _ = twins(x, *_IMPALA)
        xs = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in params]
        _impala_check(xs, ps)
        y, saved, arg = fwd(xs, ps)
        ctx.save_for_backward(xs, saved, arg, *ps)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, saved, arg, *ps = ctx.saved_tensors
        _, bwd = twins(xs, *_IMPALA)
        grads = bwd(xs, ps, saved, arg, dy.contiguous())
        return (None, *grads)


def impala_trunk(x, params):
    """``ImpalaTrunk.apply`` when a gradient is wanted, else the forward alone (the rollout step, the old-policy pass)."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return ImpalaTrunk.apply(x, *params)
    fwd, _ = twins(x, *_IMPALA)
    ps = [p.detach().contiguous() for p in params]
    _impala_check(x, ps)
    return fwd(x.contiguous(), ps)[0]


# ----------------------------------------------------------------- IMPALA-CNN trunk on Atari stacks (the 84 family)
IMPALA84_FRAME = (84, 84, 4)
IMPALA84_OUT = (11, 11, 32)


def impala84_param_shapes():
    """The 30 trunk parameters' shapes of the Atari IMPALA-CNN (qdagger_dqn_atari_impalacnn.py:164-181) in state_dict order."""
    shapes, cin = [], IMPALA84_FRAME[2]
    for c in IMPALA_CHANNELS:
        for i in range(5):
            shapes += [(c, cin if i == 0 else c, 3, 3), (c,)]
        cin = c
    return shapes


def impala84_params(net):
    """The trunk's 30 parameters of a module whose ``network[0..2]`` are the three ConvSequences."""
    return [p for i in range(3) for p in net.network[i].parameters()]


def _impala84_check(x, params):
    if x.dim() != 4 or tuple(x.shape[1:]) != IMPALA84_FRAME or x.shape[0] < 1:
        raise ValueError(f"x: expected channels-last frame stacks (B, 84, 84, 4), got {tuple(x.shape)}")
    if x.dtype != torch.uint8:
        raise TypeError(f"x: expected the ring's uint8 rows, got {x.dtype} (the trunk reads bytes; no f32 copy of the frames is made)")
    if len(params) != 30:
        raise ValueError(f"params: expected the trunk's 30 weights and biases, got {len(params)}")
    for i, (p, shp) in enumerate(zip(params, impala84_param_shapes())):
        if tuple(p.shape) != shp:
            raise ValueError(f"params[{i}]: expected shape {shp}, got {tuple(p.shape)} (channels must be {list(IMPALA_CHANNELS)})")


def impala84_forward(x, params):
    """The IMPALA-CNN trunk of the QDagger student on the HIP kernels of csrc/impala.hip: x (B,84,84,4) u8 channels-last rows
    (what ``replay_gather_u8`` writes), read as byte / 255; params the 30 conv weights / biases in state_dict order.  Returns
    ``(y (B,11,11,32) channels-last, saved, argmax)``; the last two feed ``impala84_backward``."""
    lib = _lib.load()
    _impala84_check(x, params)
    _chk(x, torch.uint8, "x")
    for i, p in enumerate(params):
        _chk(p, torch.float32, f"params[{i}]")
    B, dev = x.shape[0], x.device
    y = torch.empty((B, *IMPALA84_OUT), device=dev)
    saved = torch.empty(int(lib.mi355ppo_impala84_saved_floats(B)), device=dev)
    arg = torch.empty(int(lib.mi355ppo_impala84_argmax_bytes(B)), dtype=torch.uint8, device=dev)
    nws = int(lib.mi355ppo_impala84_workspace_bytes(B, 0))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _launch("mi355ppo_impala84_fwd_u8", dev, _ptr(x), _ptr_array(params), _ptr(y), _ptr(saved), _ptr(arg), B, *IMPALA84_FRAME,
            *IMPALA_CHANNELS, _ptr(ws), nws)
    return y, saved, arg


def impala84_backward(x, params, saved, arg, dy):
    """Backward of ``impala84_forward``: dy (B,11,11,32) channels-last -> the 30 parameter gradients (one flat buffer's views,
    written by deterministic fixed-order folds); no gradient for the frames."""
    lib = _lib.load()
    _impala84_check(x, params)
    B, dev = x.shape[0], x.device
    _chk(x, torch.uint8, "x")
    _chk(dy, torch.float32, "dy", (B, *IMPALA84_OUT))
    _chk(saved, torch.float32, "saved", (int(lib.mi355ppo_impala84_saved_floats(B)),))
    _chk(arg, torch.uint8, "argmax", (int(lib.mi355ppo_impala84_argmax_bytes(B)),))
    for i, p in enumerate(params):
        _chk(p, torch.float32, f"params[{i}]")
    flat = torch.empty(sum(p.numel() for p in params), device=dev)
    grads, o = [], 0
    for p in params:
        grads.append(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()
    nws = int(lib.mi355ppo_impala84_workspace_bytes(B, 1))
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    _launch("mi355ppo_impala84_bwd_u8", dev, _ptr(x), _ptr_array(params), _ptr(saved), _ptr(arg), _ptr(dy), _ptr_array(grads), B,
            *IMPALA84_FRAME, *IMPALA_CHANNELS, _ptr(ws), nws)
    return grads


_IMPALA84 = ("impala84_forward", "impala84_backward")


class Impala84Trunk(torch.autograd.Function):
    """Differentiable ``(x, *params) -> y``: the three ConvSequences of the Atari IMPALA-CNN on u8 channels-last stacks x
    (B,84,84,4), y (B,11,11,32) channels-last.  The backward returns the 30 parameter gradients and None for the frames.  The
    HIP kernels run for CUDA tensors, the host twins for CPU ones (same arithmetic)."""

    @staticmethod
    def forward(ctx, x, *params):
        fwd, _ = twins(x, *_IMPALA84)
        xs = x.detach().contiguous()
        ps = [p.detach().contiguous() for p in params]
        _impala84_check(xs, ps)
        y, saved, arg = fwd(xs, ps)
        ctx.save_for_backward(xs, saved, arg, *ps)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, saved, arg, *ps = ctx.saved_tensors
        _, bwd = twins(xs, *_IMPALA84)
        grads = bwd(xs, ps, saved, arg, dy.contiguous())
        return (None, *grads)


def impala84_trunk(x, params):
    """``Impala84Trunk.apply`` when a gradient is wanted, else the forward alone (acting, the target network)."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return Impala84Trunk.apply(x, *params)
    fwd, _ = twins(x, *_IMPALA84)
    ps = [p.detach().contiguous() for p in params]
    _impala84_check(x, ps)
    return fwd(x.contiguous(), ps)[0]


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


# ------------------------------------------------------------------------------------------- PQN (csrc/pqn.hip)
PQN_MAX_OBS, PQN_MAX_ACTIONS, PQN_HIDDEN = 64, 18, (120, 84)


def pqn_param_count(obs_dim: int, n_actions: int) -> int:
    """Parameters of pqn.py's QNetwork (Linear -> LayerNorm(120) -> ReLU -> Linear -> LayerNorm(84) -> ReLU -> Linear)."""
    return 120 * obs_dim + 360 + 84 * 120 + 252 + 85 * n_actions


def pqn_egreedy(q, random_actions, u, epsilon: float, actions_out, values_out, action_i64_out=None):
    """pqn.py's action logic on a computed ``q`` (N, A): argmax (torch's tie / NaN rule), ``values[step]`` = q at the greedy index,
    ``rand < epsilon`` and ``where``.  ``actions_out`` / ``values_out`` are the step's storage rows (N,) f32."""
    N, A = q.shape
    _chk(q, torch.float32, "q")
    _chk(random_actions, torch.int64, "random_actions", (N,))
    _chk(u, torch.float32, "u", (N,))
    _chk(actions_out, torch.float32, "actions_out", (N,))
    _chk(values_out, torch.float32, "values_out", (N,))
    if action_i64_out is not None:
        _chk(action_i64_out, torch.int64, "action_i64_out", (N,))
    _launch("mi355ppo_pqn_egreedy_f32", q.device, _ptr(q), _ptr(random_actions), _ptr(u), float(epsilon), _ptr(actions_out),
            _ptr(values_out), _ptr(action_i64_out), N, A)
    return actions_out, values_out


def pqn_qlambda(rewards, dones, values, next_done, next_q, gamma: float, q_lambda: float, returns=None):
    """The ``# Compute Q(lambda) targets`` block (bootstrap ``torch.max(next_q, dim=-1)`` included) -> returns (T, N)."""
    T, N = rewards.shape
    A = next_q.shape[-1]
    for t, nm in ((rewards, "rewards"), (dones, "dones"), (values, "values")):
        _chk(t, torch.float32, nm, (T, N))
    next_done = _chk(next_done.reshape(-1), torch.float32, "next_done", (N,))
    _chk(next_q, torch.float32, "next_q", (N, A))
    if returns is None:
        returns = torch.empty_like(rewards)
    _chk(returns, torch.float32, "returns", (T, N))
    _launch("mi355ppo_pqn_qlambda_f32", rewards.device, _ptr(rewards), _ptr(dones), _ptr(values), _ptr(next_done), _ptr(next_q),
            _ptr(returns), T, N, A, float(gamma), float(q_lambda))
    return returns


def pqn_td_loss(q, mb_inds, b_actions, b_returns, dq=None, scalars=None):
    """``q.gather(1, b_actions[mb_inds].long())`` + ``F.mse_loss(b_returns[mb_inds], old_val)`` and its gradient -> (dq (M, A),
    scalars (2,) = {td_loss, mean(old_val)})."""
    M, A = q.shape
    _chk(q, torch.float32, "q")
    _chk(mb_inds, torch.int64, "mb_inds", (M,))
    B = b_actions.numel()
    b_actions = _chk(b_actions.reshape(-1), torch.float32, "b_actions", (B,))
    b_returns = _chk(b_returns.reshape(-1), torch.float32, "b_returns", (B,))
    dq = torch.empty_like(q) if dq is None else _chk(dq, torch.float32, "dq", (M, A))
    scalars = torch.empty(2, dtype=torch.float32, device=q.device) if scalars is None else _chk(scalars, torch.float32, "scalars", (2,))
    _launch("mi355ppo_pqn_td_loss_fwd_bwd_f32", q.device, _ptr(q), _ptr(mb_inds), _ptr(b_actions), _ptr(b_returns), _ptr(dq), _ptr(scalars),
            M, A, B)
    return dq, scalars


# ---- the LayerNorm NatureCNN of pqn_atari_envpool.py (csrc/layernorm.hip; the pre-activation forwards: cleanrl_amd/ln_cnn.py)
AMAX_WORDS = 256      # MI355PPO_AMAX_WORDS: uint32 words of an amax record (csrc/f16split.h)
LN_MAX_D = 16384


def _ln_dims(z, C: int, HW: int):
    rows, D = z.shape[0], int(C) * int(HW)
    if rows <= 0 or C <= 0 or HW <= 0 or C % 4 or D > LN_MAX_D or z.numel() != rows * D:
        raise ValueError(f"layernorm: rows of C * HW = {C} * {HW} floats (C a multiple of 4, at most {LN_MAX_D}), got {tuple(z.shape)}")
    return rows, D


def layernorm_relu_fwd(z, gamma, beta, C: int, HW: int, eps: float = 1e-5, out=None, mean=None, rstd=None, bits=None, amax=None):
    """``relu(layer_norm(z))`` over rows ``z`` (rows, ..) of C * HW floats in (H, W, C) order, ``gamma`` / ``beta`` in torch's (C, H, W)
    order -> ``(a, mean (rows,), rstd (rows,))``.  ``bits`` (int32, ``z.numel() // 32`` words) receives ``a > 0`` in the layout of the
    ``*_bits`` forwards, ``amax`` (one zeroed row of ``cnn.new_amax``) a's amax record."""
    rows, D = _ln_dims(z, C, HW)
    _chk(z, torch.float32, "z")
    _chk(gamma, torch.float32, "gamma")
    _chk(beta, torch.float32, "beta")
    if gamma.numel() != D or beta.numel() != D:
        raise ValueError(f"layernorm: gamma / beta must hold {D} floats, got {gamma.numel()} / {beta.numel()}")
    dev = z.device
    out = torch.empty_like(z) if out is None else _chk(out, torch.float32, "out", z.shape)
    mean = torch.empty(rows, dtype=torch.float32, device=dev) if mean is None else _chk(mean, torch.float32, "mean", (rows,))
    rstd = torch.empty(rows, dtype=torch.float32, device=dev) if rstd is None else _chk(rstd, torch.float32, "rstd", (rows,))
    if bits is not None:
        if D % 32:
            raise ValueError(f"layernorm: mask bits need C * HW % 32 == 0, got {D}")
        _chk(bits, torch.int32, "bits", (rows * D // 32,))
    if amax is not None:
        _chk(amax, torch.int32, "amax", (AMAX_WORDS,))
    _launch("mi355ppo_layernorm_relu_fwd_f32", dev, _ptr(z), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(mean), _ptr(rstd), _ptr(bits), _ptr(amax),
            rows, int(C), int(HW), float(eps))
    return out, mean, rstd


def layernorm_relu_bwd(dy, z, mean, rstd, gamma, C: int, HW: int, act=None, dz=None, dgamma=None, dbeta=None, amax=None):
    """Backward of ``layernorm_relu_fwd``: ``dy`` is the gradient at ``a`` already under the mask ``a > 0`` -- or, with ``act`` given, is
    masked here by ``act > 0`` -> ``(dz, dgamma, dbeta)`` (the parameter gradients in torch's (C, H, W) order, overwritten; ``amax``
    receives dz's amax record).  The same input gives the same bits on every call."""
    rows, D = _ln_dims(z, C, HW)
    _chk(z, torch.float32, "z")
    _chk(dy, torch.float32, "dy", z.shape)
    if act is not None:
        _chk(act, torch.float32, "act", z.shape)
    _chk(mean, torch.float32, "mean", (rows,))
    _chk(rstd, torch.float32, "rstd", (rows,))
    _chk(gamma, torch.float32, "gamma")
    if gamma.numel() != D:
        raise ValueError(f"layernorm: gamma must hold {D} floats, got {gamma.numel()}")
    dev = z.device
    dz = torch.empty_like(z) if dz is None else _chk(dz, torch.float32, "dz", z.shape)
    dgamma = torch.empty_like(gamma) if dgamma is None else _chk(dgamma, torch.float32, "dgamma", gamma.shape)
    dbeta = torch.empty_like(gamma) if dbeta is None else _chk(dbeta, torch.float32, "dbeta", gamma.shape)
    if amax is not None:
        _chk(amax, torch.int32, "amax", (AMAX_WORDS,))
    ws = _workspace(dev, _lib.load().mi355ppo_layernorm_bwd_workspace_bytes(rows, int(C), int(HW)))
    _launch("mi355ppo_layernorm_relu_bwd_f32", dev, _ptr(dy), _ptr(act), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dz), _ptr(dgamma),
            _ptr(dbeta), _ptr(amax), rows, int(C), int(HW), _ptr(ws), ws.numel())
    return dz, dgamma, dbeta


def conv1q_pre_fwd(obs_u8, pack, bias, inds=None, out=None):
    """``conv1(obs_u8[inds] / 255) + bias`` WITHOUT the ReLU on kernel Q -- the input of the network's first LayerNorm; ``pack`` = kernel Q's
    pack of the weight (``cnn.repack_weights(W, 1, cnn.MODE_FWD_Q)``).  ``relu`` of the result is the ReLU forward's, bit for bit."""
    _chk(obs_u8, torch.uint8, "src")
    if tuple(obs_u8.shape[1:]) != (84, 84, 4):
        raise ValueError(f"conv1q_pre_fwd: source rows must be (84, 84, 4) uint8, got {tuple(obs_u8.shape)}")
    images = obs_u8.shape[0] if inds is None else inds.numel()
    if inds is not None:
        _chk(inds, torch.int64, "inds")
    _chk(pack, torch.float32, "Bt", (_lib.load().mi355ppo_cnn_conv1q_pack_bytes() // 4,))
    _chk(bias, torch.float32, "bias", (32,))
    out = torch.empty((images, 20, 20, 32), dtype=torch.float32, device=obs_u8.device) if out is None else _chk(out, torch.float32, "out",
                                                                                                               (images, 20, 20, 32))
    _launch("mi355ppo_cnn_conv1q_pre_fwd", obs_u8.device, _ptr(obs_u8), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), images)
    return out


def _frames_u8(obs_u8, what):
    """(rows, 84, 84) uint8 frames: ``(N, 1, 84, 84)`` and ``(N, 84, 84, 1)`` are the same bytes -> the (rows, 84, 84) view."""
    _chk(obs_u8, torch.uint8, "src")
    if tuple(obs_u8.shape[1:]) not in ((84, 84), (1, 84, 84), (84, 84, 1)):
        raise ValueError(f"{what}: source rows must be (84, 84) uint8 frames, got {tuple(obs_u8.shape)}")
    return obs_u8.view(-1, 84, 84)


def conv1q1_pack(W, out=None):
    """Kernel Q1's pack of a ``Conv2d(1, 32, 8, stride=4)`` weight (32, 1, 8, 8), as f32 storage (kernel Q's digits in the one-channel layout)."""
    _chk(W, torch.float32, "W", (32, 1, 8, 8))
    n = _lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4
    out = torch.empty(n, dtype=torch.float32, device=W.device) if out is None else _chk(out, torch.float32, "pack", (n,))
    _launch("mi355ppo_cnn_conv1q1_pack", W.device, _ptr(W), _ptr(out))
    return out


def conv1q1_pre_fwd(obs_u8, pack, bias, inds=None, out=None):
    """``conv1(obs_u8[inds] / 255) + bias`` WITHOUT the ReLU for ONE-channel frames (rows, 84, 84) uint8 on kernel Q1 -- the input of the first
    LayerNorm of pqn_atari_envpool_lstm.py's network; ``pack = conv1q1_pack(W)``.  (M, 20, 20, 32) f32, kernel Q's arithmetic: exact."""
    frames = _frames_u8(obs_u8, "conv1q1_pre_fwd")
    images = frames.shape[0] if inds is None else inds.numel()
    if inds is not None:
        _chk(inds, torch.int64, "inds")
    _chk(pack, torch.float32, "pack", (_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,))
    _chk(bias, torch.float32, "bias", (32,))
    out = torch.empty((images, 20, 20, 32), dtype=torch.float32, device=frames.device) if out is None else _chk(out, torch.float32, "out",
                                                                                                               (images, 20, 20, 32))
    _launch("mi355ppo_cnn_conv1q1_pre_fwd", frames.device, _ptr(frames), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), images)
    return out


def _conv1q1_relu_args(obs_u8, pack, bias, inds, out, bits, what):
    frames = _frames_u8(obs_u8, what)
    images = frames.shape[0] if inds is None else inds.numel()
    if inds is not None:
        _chk(inds, torch.int64, "inds")
    _chk(pack, torch.float32, "pack", (_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,))
    _chk(bias, torch.float32, "bias", (32,))
    _chk(out, torch.float32, "out", (images, 20, 20, 32))
    if bits is not None:
        _chk(bits, torch.int32, "bits", (images * 400,))
    return frames, images


def conv1q1_fwd_amax(obs_u8, pack, bias, inds, out, bits, dst_amax):
    """``relu(conv1(obs_u8[inds] / 255) + bias)`` for ONE-channel frames (rows, 84, 84) uint8 on kernel Q1 -- conv1 of ppo_atari_lstm.py's
    network; ``pack = conv1q1_pack(W)``.  Folds ``max(out)`` into the amax record ``dst_amax`` and, when ``bits`` is given, writes
    ``out > 0`` as bits (int32, ``out.numel() // 32`` words: word w, bit b <-> flat element 32 w + b)."""
    frames, images = _conv1q1_relu_args(obs_u8, pack, bias, inds, out, bits, "conv1q1_fwd_amax")
    _chk(dst_amax, torch.int32, "dst_amax", (AMAX_WORDS,))
    _launch("mi355ppo_cnn_conv1q1_fwd_amax", frames.device, _ptr(frames), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), _ptr(bits), images,
            _ptr(dst_amax))
    return out


def conv1q1_fwd_bits(obs_u8, pack, bias, inds, out, bits):
    """The same without the amax record; ``bits`` is required."""
    if bits is None:
        raise ValueError("conv1q1_fwd_bits: the mask words are required")
    frames, images = _conv1q1_relu_args(obs_u8, pack, bias, inds, out, bits, "conv1q1_fwd_bits")
    _launch("mi355ppo_cnn_conv1q1_fwd_bits", frames.device, _ptr(frames), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), _ptr(bits), images)
    return out


def conv1p1_wgrad(obs_u8, dz, dz_amax, inds=None, out=None):
    """``(dW (32, 1, 8, 8), db (32,))`` of ``Conv2d(1, 32, 8, stride=4)`` from the uint8 frames (rows, 84, 84) through ``inds`` and the
    pre-activation gradient ``dz`` (M, 20, 20, 32) with its amax record (kernel P1: dz in two f16 terms, exact frame operand, fixed-order
    fold -- the same input gives the same bits)."""
    frames = _frames_u8(obs_u8, "conv1p1_wgrad")
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


def _pqn_net(obs, params, n_actions):
    N, O = obs.shape
    _chk(obs, torch.float32, "obs")
    _chk(params, torch.float32, "params", (pqn_param_count(O, n_actions),))
    return N, O


def pqn_mlp_forward(obs, params, n_actions: int, q_out=None):
    """``QNetwork.forward`` of pqn.py on the flat parameters (``agent.parameters()`` order) -> q (N, A)."""
    N, O = _pqn_net(obs, params, n_actions)
    q_out = torch.empty((N, n_actions), dtype=torch.float32, device=obs.device) if q_out is None else _chk(q_out, torch.float32, "q_out",
                                                                                                            (N, n_actions))
    _launch("mi355ppo_pqn_mlp_fwd_f32", obs.device, _ptr(obs), _ptr(params), _ptr(q_out), N, O, int(n_actions))
    return q_out


def pqn_mlp_act(obs, params, n_actions: int, random_actions, u, epsilon: float, actions_out, values_out, action_i64_out=None,
                obs_row_out=None, done_in=None, done_row_out=None):
    """One rollout step of pqn.py in one launch: forward, e-greedy, the ``actions`` / ``values`` (and optionally ``obs`` /
    ``dones``) storage rows."""
    N, O = _pqn_net(obs, params, n_actions)
    _chk(random_actions, torch.int64, "random_actions", (N,))
    _chk(u, torch.float32, "u", (N,))
    _chk(actions_out, torch.float32, "actions_out", (N,))
    _chk(values_out, torch.float32, "values_out", (N,))
    if action_i64_out is not None:
        _chk(action_i64_out, torch.int64, "action_i64_out", (N,))
    if obs_row_out is not None:
        _chk(obs_row_out, torch.float32, "obs_row_out", (N, O))
    if done_row_out is not None:
        _chk(done_in, torch.float32, "done_in", (N,))
        _chk(done_row_out, torch.float32, "done_row_out", (N,))
    _launch("mi355ppo_pqn_mlp_act_f32", obs.device, _ptr(obs), _ptr(params), _ptr(random_actions), _ptr(u), float(epsilon),
            _ptr(actions_out), _ptr(values_out), _ptr(action_i64_out), _ptr(obs_row_out), _ptr(done_in), _ptr(done_row_out), N, O,
            int(n_actions))
    return actions_out, values_out


def pqn_mlp_td_fwd_bwd(b_obs, mb_inds, params, b_actions, b_returns, grads, n_actions: int, scalars=None):
    """One minibatch of pqn.py: gather, forward, TD loss, backward.  OVERWRITES ``grads`` (flat) with d loss / d params and returns
    scalars (2,) = {td_loss, mean(old_val)}."""
    B, O = _pqn_net(b_obs, params, n_actions)
    (M,) = mb_inds.shape
    _chk(mb_inds, torch.int64, "mb_inds", (M,))
    b_actions = _chk(b_actions.reshape(-1), torch.float32, "b_actions", (B,))
    b_returns = _chk(b_returns.reshape(-1), torch.float32, "b_returns", (B,))
    _chk(grads, torch.float32, "grads", params.shape)
    dev = b_obs.device
    scalars = torch.empty(2, dtype=torch.float32, device=dev) if scalars is None else _chk(scalars, torch.float32, "scalars", (2,))
    lib = _lib.load()
    ws = _workspace(dev, lib.mi355ppo_pqn_mlp_td_workspace_bytes(M, O, int(n_actions)))
    _launch("mi355ppo_pqn_mlp_td_fwd_bwd_f32", dev, _ptr(b_obs), B, _ptr(mb_inds), _ptr(params), _ptr(b_actions), _ptr(b_returns),
            _ptr(grads), _ptr(scalars), M, O, int(n_actions), _ptr(ws), ws.numel())
    return scalars


def radam_schedule(lr: float, step: int, beta1: float = 0.9, beta2: float = 0.999):
    """The 8-float schedule slot of RAdam step ``step`` (1-based), as the library forms it (host floats)."""
    out = (ctypes.c_float * 8)()
    _lib.call("mi355ppo_radam_schedule_f32", float(lr), float(beta1), float(beta2), int(step), out)
    return [float(x) for x in out]


def _flat4(params, grads, exp_avg, exp_avg_sq):
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _chk(t, torch.float32, nm, (n,))
    return n


def clip_radam_(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, max_grad_norm: float, beta1: float = 0.9, beta2: float = 0.999,
                eps: float = 1e-8, total_norm_out=None):
    """In-place ``clip_grad_norm_`` + ``optim.RAdam`` step ``step`` (1-based) on flat f32 buffers; zeroes ``grads``."""
    lib = _lib.load()
    n = _flat4(params, grads, exp_avg, exp_avg_sq)
    dev = params.device
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_clip_radam_workspace_bytes(n))
    _launch("mi355ppo_clip_radam_f32", dev, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(max_grad_norm), float(lr),
            float(beta1), float(beta2), float(eps), int(step), _ptr(total_norm_out), _ptr(ws), ws.numel())
    return total_norm_out


def clip_radam_sched_(params, grads, exp_avg, exp_avg_sq, sched8, max_grad_norm: float, beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8, total_norm_out=None):
    """``clip_radam_`` with the step's slot (``radam_schedule`` values) read from the 8-float DEVICE tensor ``sched8``: capturable."""
    lib = _lib.load()
    n = _flat4(params, grads, exp_avg, exp_avg_sq)
    _chk(sched8, torch.float32, "sched8", (8,))
    dev = params.device
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_clip_radam_workspace_bytes(n))
    _launch("mi355ppo_clip_radam_sched_f32", dev, _ptr(params), _ptr(grads), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(max_grad_norm),
            float(beta1), float(beta2), float(eps), _ptr(sched8), _ptr(total_norm_out), _ptr(ws), ws.numel())
    return total_norm_out


# ------------------------------------------------------------------------------------------- recurrent PQN (csrc/pqn_lstm.hip)
def pqn_lstm_act(gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions=None, u=None, epsilon: float = 0.0, h_out=None, c_out=None,
                 q_out=None, actions_out=None, values_out=None, action_i64_out=None, done_row_out=None):
    """The recurrent tail of one rollout step of pqn_atari_envpool_lstm.py in one launch: the done reset, ONE LSTM cell on ``gx``
    (N, 4H) = x W_ih^T + b_ih + b_hh (bit-equal to ``lstm_seq_forward`` at T = 1), ``q_func`` and e-greedy into the step's storage
    rows.  ``h_out`` / ``c_out`` (N, H) may be ``h_in`` / ``c_in``.  Every output is optional: with only ``q_out`` it is the
    bootstrap's ``q_network(next_obs, ...)``.  Returns ``q_out``."""
    N, G = gx.shape
    H = G // 4
    A = wq.shape[0]
    _chk(gx, torch.float32, "gx", (N, 4 * H))
    _chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    _chk(h_in, torch.float32, "h_in", (N, H))
    _chk(c_in, torch.float32, "c_in", (N, H))
    _chk(done_in, torch.float32, "done_in", (N,))
    _chk(wq, torch.float32, "wq", (A, H))
    _chk(bq, torch.float32, "bq", (A,))
    for t, dt, nm, shape in ((random_actions, torch.int64, "random_actions", (N,)), (u, torch.float32, "u", (N,)),
                             (h_out, torch.float32, "h_out", (N, H)), (c_out, torch.float32, "c_out", (N, H)),
                             (q_out, torch.float32, "q_out", (N, A)), (actions_out, torch.float32, "actions_out", (N,)),
                             (values_out, torch.float32, "values_out", (N,)), (action_i64_out, torch.int64, "action_i64_out", (N,)),
                             (done_row_out, torch.float32, "done_row_out", (N,))):
        if t is not None:
            _chk(t, dt, nm, shape)
    _launch("mi355ppo_pqn_lstm_act_f32", gx.device, _ptr(gx), _ptr(w_hh), _ptr(h_in), _ptr(c_in), _ptr(done_in), _ptr(wq), _ptr(bq),
            _ptr(random_actions), _ptr(u), float(epsilon), _ptr(h_out), _ptr(c_out), _ptr(q_out), _ptr(actions_out), _ptr(values_out),
            _ptr(action_i64_out), _ptr(done_row_out), N, H, A)
    return q_out


def pqn_lstm_td_fwd_bwd(h, mb_inds, b_actions, b_returns, wq, bq, dwq, dbq, dh=None, scalars=None):
    """``q_func(h).gather(1, b_actions[mb_inds].long())`` + ``F.mse_loss(b_returns[mb_inds], old_val)`` of one minibatch, forward and
    backward: ``h`` (M, H) are the scan's rows in minibatch order.  OVERWRITES ``dwq`` (A, H) / ``dbq`` (A) (views of the flat
    gradient) and returns ``(dh (M, H), scalars (2,) = {td_loss, mean(old_val)})``."""
    M, H = h.shape
    A = wq.shape[0]
    _chk(h, torch.float32, "h")
    _chk(mb_inds, torch.int64, "mb_inds", (M,))
    B = b_actions.numel()
    b_actions = _chk(b_actions.reshape(-1), torch.float32, "b_actions", (B,))
    b_returns = _chk(b_returns.reshape(-1), torch.float32, "b_returns", (B,))
    _chk(wq, torch.float32, "wq", (A, H))
    _chk(bq, torch.float32, "bq", (A,))
    _chk(dwq, torch.float32, "dwq", (A, H))
    _chk(dbq, torch.float32, "dbq", (A,))
    dev = h.device
    dh = torch.empty_like(h) if dh is None else _chk(dh, torch.float32, "dh", (M, H))
    scalars = torch.empty(2, dtype=torch.float32, device=dev) if scalars is None else _chk(scalars, torch.float32, "scalars", (2,))
    ws = _workspace(dev, _lib.load().mi355ppo_pqn_lstm_td_workspace_bytes(M, A))
    _launch("mi355ppo_pqn_lstm_td_fwd_bwd_f32", dev, _ptr(h), _ptr(mb_inds), _ptr(b_actions), _ptr(b_returns), _ptr(wq), _ptr(bq), _ptr(dh),
            _ptr(dwq), _ptr(dbq), _ptr(scalars), M, H, A, B, _ptr(ws), ws.numel())
    return dh, scalars


# ------------------------------------------------------------------------------------------- the replay-ring families
# The device side of cleanrl_amd/replay_ops.py: ``_chk``, the workspace of the entry point's ``*_workspace_bytes``, the current stream.
from .replay_ops import (ATARI_FRAME, DQN_HEAD_HIDDEN, DQN_HEAD_MAX_OUT, DQN_HEAD_MAX_ROWS, DQN_HIDDEN, DQN_MAX_ACT, DQN_MAX_ATOMS,  # noqa: E402,F401
                         DQN_MAX_OBS, DQN_MAX_OUT, OFFPOLICY_HIDDEN, OFFPOLICY_MAX_ACT, OFFPOLICY_MAX_OBS, QDAGGER_HIDDEN, QDAGGER_MAX_ROWS,
                         RAINBOW_HEAD_IN, RAINBOW_MAX_BATCH, dqn_counts, dqn_head_limits_ok, dqn_limits_ok, offpolicy_counts,
                         qdagger_head_limits_ok, rainbow_head_limits_ok, rainbow_new_buffer, rainbow_noisy_counts, rainbow_noisy_limits_ok,
                         sac_actor_count, sacd_limits_ok)


def _device_launch(name: str, dev: torch.device, *args) -> None:
    _launch(name, dev, *args)                                   # looked up at call time: the tests count launches on ``ops._launch``


def _device_launch_ws(name: str, dev: torch.device, ws_bytes: str, dims, *args) -> None:
    ws = _workspace(dev, getattr(_lib.load(), ws_bytes)(*dims))
    _launch(name, dev, *args, _ptr(ws), ws.numel())


_SIDE = replay_ops.Side(False, _chk, _device_launch, _device_launch_ws)
replay_ops.bind(_SIDE, globals())

# ------------------------------------------------------------------------------------------- RND (csrc/rnd.hip)
from .rnd_ops import RND_FEATURES, RND_MAX_BATCH, RND_MAX_STEPS, RND_PIXELS, rnd_mean_var  # noqa: E402,F401

rnd_ops.bind(_SIDE, globals())

# ------------------------------------------------------------------------------------------- PPG's auxiliary phase (csrc/ppg.hip)
from .ppg_ops import PPG_HIDDEN, PPG_MAX_ACT, PPG_MAX_ROWS, PPG_MIN_ACT  # noqa: E402,F401

ppg_ops.bind(_SIDE, globals())
