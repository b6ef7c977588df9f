"""Host (CPU) path: the ``*_cpu`` host-pointer twins of ``libmi355ppo.so`` behind the same seams as the GPU path.

Selected ONLY when the user asks for a CPU device (``--no-cuda``: BASELINE config A "CartPole on CPU,
plumbing", and the world_size-2 ``gloo`` tests of the data-parallel logic).  It is not a fallback: a
CUDA device always runs the HIP kernels and raises if ``libmi355ppo.so`` is missing, and these functions
refuse CUDA tensors.  The twins (csrc/host_twins.hip, declared in include/mi355ppo.h) are the device
kernels' own row / element functions compiled for the host, so the CPU loop crosses the SAME C ABI seams
as the GPU loop.

Written here: the twins whose signature differs from the device wrapper's on purpose (they allocate their outputs and take what the
CPU learners hold, converted through ``_f32``) -- GAE (ppo.py:218-231), the fused loss forward + backward as autograd nodes
(ppo.py:250-285; the learners whose loss has extra terms cross the same twin on their logits / value and add their terms outside) and,
for tests, sampling, clip + Adam, the observation conversion, kernel Q's pack and the library's exp / log.  Every other twin -- the
replay-ring families, RND, PPG's auxiliary phase, the LSTM scan, the TrXL memory attention, the IMPALA trunks, PQN and its LayerNorm
trunk pieces -- is the operator of cleanrl_amd/replay_ops.py, rnd_ops.py, ppg_ops.py or twin_ops.py, defined once and bound at the end
of this file to the host side, which checks like ``ops`` (nothing coerced or copied) and calls ``name + "_cpu"``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ppg_ops, replay_ops, rnd_ops, twin_ops
from .ops import pqn_param_count, radam_schedule  # noqa: F401
from .ppg_ops import PPG_HIDDEN, PPG_MAX_ACT, PPG_MAX_ROWS, PPG_MIN_ACT  # noqa: F401
from .rnd_ops import RND_FEATURES, RND_MAX_BATCH, RND_MAX_STEPS, RND_PIXELS, rnd_mean_var  # noqa: F401
from .replay_ops import (ATARI_FRAME, DQN_HEAD_HIDDEN, DQN_HEAD_MAX_OUT, DQN_HEAD_MAX_ROWS, DQN_HIDDEN, DQN_MAX_ACT, DQN_MAX_ATOMS,  # noqa: F401
                         DQN_MAX_OBS, DQN_MAX_OUT, OFFPOLICY_HIDDEN, OFFPOLICY_MAX_ACT, OFFPOLICY_MAX_OBS, QDAGGER_HIDDEN, QDAGGER_MAX_ROWS,
                         RAINBOW_HEAD_IN, RAINBOW_MAX_BATCH, dqn_counts, dqn_head_limits_ok, dqn_limits_ok, offpolicy_counts,
                         qdagger_head_limits_ok, rainbow_head_limits_ok, rainbow_new_buffer, rainbow_noisy_counts, rainbow_noisy_limits_ok,
                         sac_actor_count, sacd_limits_ok)

LOSS_SCALARS = 7


def _p(t):
    if t is None:
        return None
    if t.device.type != "cpu":
        raise TypeError("cleanrl_amd.host_ops works on CPU tensors only (CUDA tensors run the HIP kernels: cleanrl_amd.ops)")
    if not t.is_contiguous():
        raise ValueError("host twins take contiguous tensors")
    return ctypes.c_void_p(t.data_ptr())


def _out(t, dtype, numel, name):
    """Pointer of a caller-owned tensor that a twin WRITES ``numel`` elements of ``dtype`` through: unlike an input it cannot be
    coerced into a copy, so a wrong dtype or a short tensor is refused here instead of overrunning host memory."""
    ptr = _p(t)
    if t is not None and t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if t is not None and t.numel() < numel:
        raise ValueError(f"{name}: expected {numel} elements, got {t.numel()}")
    return ptr


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def gae(rewards, dones, values, next_done, next_value, gamma, gae_lambda):
    """ppo.py:218-231 through ``mi355ppo_gae_f32_cpu`` -> (advantages, returns); bit-equal to the reference's loop."""
    T, N = rewards.shape
    r, d, v = _f32(rewards), _f32(dones), _f32(values)
    nd, nv = _f32(next_done).reshape(-1), _f32(next_value).reshape(-1)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    _lib.call("mi355ppo_gae_f32_cpu", _p(r), _p(d), _p(v), _p(nd), _p(nv), _p(adv), _p(ret), T, N, float(gamma), float(gae_lambda))
    return adv, ret


class _CategoricalLossTwin(torch.autograd.Function):
    """K3 on the host: ``mi355ppo_loss_categorical_fwd_bwd_f32_cpu`` computes the loss scalars AND d loss / d (logits, value)
    in one pass (ppo.py:250-285 + its autograd down to the network outputs); backward hands the stored gradients on."""

    @staticmethod
    def forward(ctx, logits, value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, hp):
        M, A = logits.shape
        lg, vl = _f32(logits), _f32(value).reshape(-1)
        inds = mb_inds.to(torch.int64).contiguous()
        scalars = torch.empty(LOSS_SCALARS)
        dlogits, dvalue = torch.empty_like(lg), torch.empty_like(vl)
        _lib.call("mi355ppo_loss_categorical_fwd_bwd_f32_cpu", _p(lg), _p(vl), _p(inds), _p(_f32(b_actions)), _p(_f32(b_logprobs)),
                  _p(_f32(b_advantages)), _p(_f32(b_returns)), _p(_f32(b_values)), M, A, hp["clip_coef"], hp["ent_coef"], hp["vf_coef"],
                  int(hp["norm_adv"]), int(hp["clip_vloss"]), None, _p(scalars), _p(dlogits), _p(dvalue))
        ctx.save_for_backward(dlogits, dvalue.reshape(value.shape))
        ctx.mark_non_differentiable(scalars)
        return scalars[0].clone(), scalars

    @staticmethod
    def backward(ctx, g_loss, _g_scalars):
        dlogits, dvalue = ctx.saved_tensors
        return dlogits * g_loss, dvalue * g_loss, None, None, None, None, None, None, None


class _NormalLossTwin(torch.autograd.Function):
    """K3' on the host (``mi355ppo_loss_normal_fwd_bwd_f32_cpu``, ppo_continuous_action.py:265-300 + autograd)."""

    @staticmethod
    def forward(ctx, mean, logstd, value, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, hp):
        M, D = mean.shape
        mu, ls, vl = _f32(mean), _f32(logstd).reshape(-1), _f32(value).reshape(-1)
        inds = mb_inds.to(torch.int64).contiguous()
        scalars = torch.empty(LOSS_SCALARS)
        dmean, dlogstd, dvalue = torch.empty_like(mu), torch.empty_like(ls), torch.empty_like(vl)
        _lib.call("mi355ppo_loss_normal_fwd_bwd_f32_cpu", _p(mu), _p(ls), _p(vl), _p(inds), _p(_f32(b_actions)), _p(_f32(b_logprobs)),
                  _p(_f32(b_advantages)), _p(_f32(b_returns)), _p(_f32(b_values)), M, D, hp["clip_coef"], hp["ent_coef"], hp["vf_coef"],
                  int(hp["norm_adv"]), int(hp["clip_vloss"]), None, _p(scalars), _p(dmean), _p(dlogstd), _p(dvalue))
        ctx.save_for_backward(dmean, dlogstd.reshape(logstd.shape), dvalue.reshape(value.shape))
        ctx.mark_non_differentiable(scalars)
        return scalars[0].clone(), scalars

    @staticmethod
    def backward(ctx, g_loss, _g_scalars):
        dmean, dlogstd, dvalue = ctx.saved_tensors
        return dmean * g_loss, dlogstd * g_loss, dvalue * g_loss, None, None, None, None, None, None, None


def _hp(clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss):
    return dict(clip_coef=float(clip_coef), ent_coef=float(ent_coef), vf_coef=float(vf_coef), norm_adv=bool(norm_adv),
                clip_vloss=bool(clip_vloss))


def ppo_loss_categorical(logits, newvalue, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, clip_coef,
                         ent_coef, vf_coef, norm_adv, clip_vloss):
    """(loss, scalars7 in ops.LOSS_SCALAR_NAMES order) of one minibatch from the network outputs and the FLAT batch arrays
    (the twin gathers rows ``mb_inds`` itself, as the device kernel does); ``loss.backward()`` reaches logits and value."""
    return _CategoricalLossTwin.apply(logits, newvalue, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                                      _hp(clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss))


def ppo_loss_normal(mean, logstd, newvalue, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values, clip_coef,
                    ent_coef, vf_coef, norm_adv, clip_vloss):
    """The continuous-action twin: mean (M, D), logstd (D) or (1, D); ``loss.backward()`` reaches mean, logstd and value."""
    return _NormalLossTwin.apply(mean, logstd, newvalue, mb_inds, b_actions, b_logprobs, b_advantages, b_returns, b_values,
                                 _hp(clip_coef, ent_coef, vf_coef, norm_adv, clip_vloss))


def categorical_sample(logits, noise_exp1=None, seed=0, offset=0):
    """``mi355ppo_categorical_sample_f32_cpu`` -> (action int64, logprob, entropy).  With ``noise_exp1`` None the draws come from
    the device kernel's Philox stream (same words for the same (seed, offset, row))."""
    lg = _f32(logits)
    B, A = lg.shape
    act, lp, ent = torch.empty(B, dtype=torch.int64), torch.empty(B), torch.empty(B)
    nz = _f32(noise_exp1) if noise_exp1 is not None else None
    _lib.call("mi355ppo_categorical_sample_f32_cpu", _p(lg), _p(nz), int(seed), int(offset), _p(act), None, _p(lp), _p(ent), B, A)
    return act, lp, ent


def categorical_logprob_entropy(logits, action):
    lg = _f32(logits)
    B, A = lg.shape
    act = action.to(torch.int64).contiguous()
    lp, ent = torch.empty(B), torch.empty(B)
    _lib.call("mi355ppo_categorical_logprob_entropy_f32_cpu", _p(lg), _p(act), None, _p(lp), _p(ent), B, A)
    return lp, ent


def categorical_logprob_entropy_bwd(logits, action, g_logprob, g_entropy):
    lg = _f32(logits)
    B, A = lg.shape
    act = action.to(torch.int64).contiguous()
    out = torch.empty_like(lg)
    _lib.call("mi355ppo_categorical_logprob_entropy_bwd_f32_cpu", _p(lg), _p(act), None,
              _p(_f32(g_logprob)) if g_logprob is not None else None, _p(_f32(g_entropy)) if g_entropy is not None else None, _p(out), B, A)
    return out


def normal_sample(mean, logstd, noise=None, seed=0, offset=0):
    mu, ls = _f32(mean), _f32(logstd).reshape(-1)
    B, D = mu.shape
    act, lp, ent = torch.empty_like(mu), torch.empty(B), torch.empty(B)
    nz = _f32(noise) if noise is not None else None
    _lib.call("mi355ppo_normal_sample_f32_cpu", _p(mu), _p(ls), _p(nz), int(seed), int(offset), _p(act), _p(lp), _p(ent), B, D)
    return act, lp, ent


def normal_logprob_entropy(mean, logstd, action):
    mu, ls, ac = _f32(mean), _f32(logstd).reshape(-1), _f32(action)
    B, D = mu.shape
    lp, ent = torch.empty(B), torch.empty(B)
    _lib.call("mi355ppo_normal_logprob_entropy_f32_cpu", _p(mu), _p(ls), _p(ac), _p(lp), _p(ent), B, D)
    return lp, ent


def normal_logprob_entropy_bwd(mean, logstd, action, g_logprob, g_entropy):
    mu, ls, ac = _f32(mean), _f32(logstd).reshape(-1), _f32(action)
    B, D = mu.shape
    dmean, dls = torch.empty_like(mu), torch.empty_like(mu)
    _lib.call("mi355ppo_normal_logprob_entropy_bwd_f32_cpu", _p(mu), _p(ls), _p(ac), _p(_f32(g_logprob)) if g_logprob is not None else None,
              _p(_f32(g_entropy)) if g_entropy is not None else None, _p(dmean), _p(dls), B, D)
    return dmean, dls


def _flat4(params, grads, exp_avg, exp_avg_sq):
    n = params.numel()
    return [_out(t, torch.float32, n, nm) for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"))]


def clip_adam_(params, grads, exp_avg, exp_avg_sq, step, lr, max_grad_norm, grad_scale=1.0, beta1=0.9, beta2=0.999, eps=1e-5):
    """In place on flat f32 CPU buffers (``mi355ppo_clip_adam_f32_cpu``): grads * grad_scale -> global-norm clip -> Adam; the
    gradient buffer is zeroed.  Returns the pre-clip norm."""
    norm = torch.empty(1)
    _lib.call("mi355ppo_clip_adam_f32_cpu", *_flat4(params, grads, exp_avg, exp_avg_sq), params.numel(), float(grad_scale),
              float(max_grad_norm), float(lr), beta1, beta2, eps, int(step), _p(norm))
    return norm


def obs_u8_to_f32(src_u8, inds=None, scale_255=True):
    src = src_u8.contiguous()
    rows_total = src.shape[0]
    row_bytes = src.numel() // max(rows_total, 1)
    idx = inds.to(torch.int64).contiguous() if inds is not None else None
    rows = idx.numel() if idx is not None else rows_total
    out = torch.empty((rows,) + tuple(src.shape[1:]), dtype=torch.float32)
    _lib.call("mi355ppo_obs_u8_to_f32_cpu", _p(src), _p(idx), _p(out), rows, row_bytes, int(bool(scale_255)))
    return out


def conv1q_pack(W):
    """``mi355ppo_cnn_conv1q_pack_cpu``: kernel Q's pack of a (32, 4, 8, 8) weight, as f32 storage."""
    pack = torch.empty(_lib.load().mi355ppo_cnn_conv1q_pack_bytes() // 4, dtype=torch.float32)
    _lib.call("mi355ppo_cnn_conv1q_pack_cpu", _p(_f32(W)), _p(pack))
    return pack


def sac_exp_log(x):
    """The library's own exp and log (csrc/sac_rows.h) on a float32 CPU tensor -> (exp, log)."""
    x = _f32(x).reshape(-1)
    e, l = torch.empty_like(x), torch.empty_like(x)
    _lib.call("mi355ppo_sac_exp_log_f32_cpu", _p(x), _p(e), _p(l), x.numel())
    return e, l


# ------------------------------------------------------------------------------------------- the operators defined once for both sides
# The host side of cleanrl_amd/replay_ops.py, rnd_ops.py (§3.22), ppg_ops.py (§3.23) and twin_ops.py: ``ops._chk`` for
# CPU tensors, and the ``*_cpu`` twin, which takes neither workspace nor stream.
def _chk(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a CPU tensor, got {type(t).__name__}")
    if t.device.type != "cpu":
        raise TypeError("cleanrl_amd.host_ops works on CPU tensors only (CUDA tensors run the HIP kernels: cleanrl_amd.ops)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _empty(shape, dtype, dev):
    return torch.empty(shape, dtype=dtype, device=dev)          # this module's ``torch``: the guard-band tests carve allocations by patching it


def _twin(name, dev, *args):
    _lib.call(name + "_cpu", *args)


def _twin_ws(name, dev, ws_bytes, dims, *args):
    _lib.call(name + "_cpu", *args)


_SIDE = replay_ops.Side(True, _chk, _twin, _twin_ws, _empty)
for _module in (replay_ops, rnd_ops, ppg_ops, twin_ops):
    replay_ops.bind(_module, _SIDE, globals())
