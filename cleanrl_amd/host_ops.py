"""Host (CPU) path: the ``*_cpu`` host-pointer twins of ``libmi355ppo.so`` behind the same seams as the GPU path.

Selected ONLY when the user asks for a CPU device (``--no-cuda``: BASELINE config A "CartPole on CPU,
plumbing", and the world_size-2 ``gloo`` tests of the data-parallel logic).  It is not a fallback: a
CUDA device always runs the HIP kernels and raises if ``libmi355ppo.so`` is missing, and these functions
refuse CUDA tensors.  The twins (csrc/host_twins.hip, declared in include/mi355ppo.h) are the device
kernels' own row / element functions compiled for the host, so the CPU loop crosses the SAME C ABI seams
as the GPU loop: GAE (ppo.py:218-231), the fused loss forward + backward (ppo.py:250-285 and its autograd),
the LSTM sequence scans of ppo_atari_lstm.py (opt-in: ``MI355PPO_LSTM=fused``), the TrXL memory attention of ppo_trxl.py
(opt-in: ``MI355PPO_TRXL=fused``) and, for tests, sampling and clip + Adam.  The learners whose loss has extra terms (LSTM state, RND's second value
head and distillation loss) cross the same twin on their logits / value and add their terms outside.  The twins of the replay-ring
families (``replay_add`` .. ``sacd_actor_fwd_bwd``) are not written here: cleanrl_amd/replay_ops.py defines each operator
once, and the end of this file binds them to the host side, which checks like ``ops`` (nothing coerced) and calls ``name + "_cpu"``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from . import ppg_ops, replay_ops, rnd_ops
from .ops import IMPALA84_OUT, IMPALA_CHANNELS, _lstm_dims, _ptr_array, pqn_param_count, radam_schedule, trxl_dims  # noqa: F401
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


def _i64(t):
    return t.detach().to(torch.int64).contiguous()


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


def lstm_seq_forward(gx, w_hh, h0, c0, done, record: bool = False):
    """The done-masked LSTM scan (ppo_atari_lstm.py:140-158) through ``mi355ppo_lstm_seq_fwd_f32_cpu`` -> (h, hT, cT, record | None);
    gx (T,B,4H), w_hh (4H,H), h0 / c0 (B,H), done (T,B).  Same arithmetic as the device scan (csrc/lstm_rows.h)."""
    T, B, H = _lstm_dims(gx, done)
    g, w, h0, c0, d = _f32(gx), _f32(w_hh), _f32(h0), _f32(c0), _f32(done)
    h, hT, cT = torch.empty((T, B, H)), torch.empty((B, H)), torch.empty((B, H))
    rec = torch.empty(7 * T * B * H) if record else None
    _lib.call("mi355ppo_lstm_seq_fwd_f32_cpu", _p(g), _p(w), _p(h0), _p(c0), _p(d), _p(h), _p(hT), _p(cT), _p(rec), T, B, H)
    return h, hT, cT, rec


def lstm_seq_backward(dh, dhT, dcT, record, w_hh, done, want_dh0: bool = True, want_dc0: bool = True):
    """Backward of ``lstm_seq_forward`` through ``mi355ppo_lstm_seq_bwd_f32_cpu`` -> (dgx (T,B,4H), dh0 | None, dc0 | None);
    dhT / dcT may be None (= zeros)."""
    T, B, H = dh.shape
    d, w, g = _f32(done), _f32(w_hh), _f32(dh)
    dhT = None if dhT is None else _f32(dhT)
    dcT = None if dcT is None else _f32(dcT)
    dgx = torch.empty((T, B, 4 * H))
    dh0 = torch.empty((B, H)) if want_dh0 else None
    dc0 = torch.empty((B, H)) if want_dc0 else None
    _lib.call("mi355ppo_lstm_seq_bwd_f32_cpu", _p(g), _p(dhT), _p(dcT), _p(record), _p(w), _p(d), _p(dgx), _p(dh0), _p(dc0), T, B, H)
    return dgx, dh0, dc0


def _trxl_args(memory, ep, rows, pos, mask, pe, gamma, beta, q):
    E, T, layers, D, B, L, H = trxl_dims(memory, rows, q)
    m, g, b, qq = _f32(memory), _f32(gamma), _f32(beta), _f32(q)
    e, r = ep.to(torch.int64).contiguous(), rows.to(torch.int64).contiguous()
    k = (mask != 0).to(torch.uint8).contiguous()
    p = None if pe is None else _f32(pe)
    ps = None if pe is None else pos.to(torch.int64).contiguous()
    return (E, T, layers, D, B, L, H), (m, e, r, ps, k, p, g, b, qq)


def trxl_attn_forward(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q):
    """The TrXL memory attention of one layer through ``mi355ppo_trxl_attn_fwd_f32_cpu`` -> (u (B,H,d), stats (B,H,2)); same
    arithmetic as the device kernel (csrc/trxl_rows.h).  An out-of-range index raises."""
    (E, T, layers, D, B, L, H), (m, e, r, ps, k, p, g, b, qq) = _trxl_args(memory, ep, rows, pos, mask, pe, gamma, beta, q)
    u, stats = torch.empty((B, H, D // H)), torch.empty((B, H, 2))
    _lib.call("mi355ppo_trxl_attn_fwd_f32_cpu", _p(m), E, T, layers, int(layer), _p(e), _p(r), _p(ps), _p(k), _p(p),
              0 if p is None else p.shape[0], _p(g), _p(b), _p(qq), _p(u), _p(stats), B, L, D, H)
    return u, stats


def trxl_attn_backward(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q, u, stats, du):
    """Backward of ``trxl_attn_forward`` through ``mi355ppo_trxl_attn_bwd_f32_cpu`` -> (dq (B,H,d), dgamma (D), dbeta (D))."""
    (E, T, layers, D, B, L, H), (m, e, r, ps, k, p, g, b, qq) = _trxl_args(memory, ep, rows, pos, mask, pe, gamma, beta, q)
    dq, rows_ws = torch.empty((B, H, D // H)), torch.empty((2, B, D))
    dgamma, dbeta = torch.empty(D), torch.empty(D)
    _lib.call("mi355ppo_trxl_attn_bwd_f32_cpu", _p(m), E, T, layers, int(layer), _p(e), _p(r), _p(ps), _p(k), _p(p),
              0 if p is None else p.shape[0], _p(g), _p(b), _p(qq), _p(_f32(u)), _p(_f32(stats)), _p(_f32(du)), _p(dq), _p(rows_ws),
              _p(dgamma), _p(dbeta), B, L, D, H)
    return dq, dgamma, dbeta


def impala_forward(x, params):
    """The IMPALA-CNN trunk through ``mi355ppo_impala_fwd_f32_cpu``: x (B,64,64,3) channels-last frames, params the 30 conv
    weights / biases in state_dict order -> (y (B,8,8,32) channels-last, saved, argmax).  Same arithmetic as the device kernels
    (csrc/impala_rows.h)."""
    lib = _lib.load()
    B, H, W, C = x.shape
    xs, ps = _f32(x), [_f32(p) for p in params]
    y = torch.empty((B, 8, 8, 32))
    saved = torch.empty(max(int(lib.mi355ppo_impala_saved_floats(B)), 1))
    arg = torch.empty(max(int(lib.mi355ppo_impala_argmax_bytes(B)), 1), dtype=torch.uint8)
    _lib.call("mi355ppo_impala_fwd_f32_cpu", _p(xs), _ptr_array([_p_t(p) for p in ps]), _p(y), _p(saved), _p(arg), B, H, W, C, *IMPALA_CHANNELS)
    return y, saved, arg


def impala_backward(x, params, saved, arg, dy):
    """Backward of ``impala_forward`` through ``mi355ppo_impala_bwd_f32_cpu`` -> the 30 parameter gradients (no input gradient)."""
    B, H, W, C = x.shape
    xs, ps, g = _f32(x), [_f32(p) for p in params], _f32(dy)
    grads = [torch.empty(p.shape) for p in ps]
    _lib.call("mi355ppo_impala_bwd_f32_cpu", _p(xs), _ptr_array([_p_t(p) for p in ps]), _p(saved), _p(arg), _p(g),
              _ptr_array([_p_t(t) for t in grads]), B, H, W, C, *IMPALA_CHANNELS)
    return grads


def impala84_forward(x, params):
    """The Atari IMPALA-CNN trunk through ``mi355ppo_impala84_fwd_u8_cpu``: x (B,84,84,4) u8 channels-last stacks -> (y (B,11,11,32)
    channels-last, saved, argmax).  Same arithmetic as the device kernels (csrc/impala_rows.h)."""
    lib = _lib.load()
    if x.dtype != torch.uint8:
        raise TypeError(f"x: expected uint8 frame stacks, got {x.dtype}")
    B, H, W, C = x.shape
    xs, ps = x.contiguous(), [_f32(p) for p in params]
    y = torch.empty((B, *IMPALA84_OUT))
    saved = torch.empty(max(int(lib.mi355ppo_impala84_saved_floats(B)), 1))
    arg = torch.empty(max(int(lib.mi355ppo_impala84_argmax_bytes(B)), 1), dtype=torch.uint8)
    _lib.call("mi355ppo_impala84_fwd_u8_cpu", _p(xs), _ptr_array([_p_t(p) for p in ps]), _p(y), _p(saved), _p(arg), B, H, W, C, *IMPALA_CHANNELS)
    return y, saved, arg


def impala84_backward(x, params, saved, arg, dy):
    """Backward of ``impala84_forward`` through ``mi355ppo_impala84_bwd_u8_cpu`` -> the 30 parameter gradients (none for the frames)."""
    if x.dtype != torch.uint8:
        raise TypeError(f"x: expected uint8 frame stacks, got {x.dtype}")
    B, H, W, C = x.shape
    xs, ps, g = x.contiguous(), [_f32(p) for p in params], _f32(dy)
    grads = [torch.empty(p.shape) for p in ps]
    _lib.call("mi355ppo_impala84_bwd_u8_cpu", _p(xs), _ptr_array([_p_t(p) for p in ps]), _p(saved), _p(arg), _p(g),
              _ptr_array([_p_t(t) for t in grads]), B, H, W, C, *IMPALA_CHANNELS)
    return grads


def impala_maxpool_forward(x):
    """The trunks' max pool (3, stride 2, pad 1) on channels-last x (B,H,W,C) -> (y (B,(H+1)/2,(W+1)/2,C), argmax bytes)."""
    B, H, W, C = x.shape
    xs = _f32(x)
    y = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C))
    arg = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.uint8)
    _lib.call("mi355ppo_impala_maxpool_fwd_f32_cpu", _p(xs), _p(y), _p(arg), B, H, W, C)
    return y, arg


def impala_maxpool_backward(dy, arg, size=None):
    """Backward of ``impala_maxpool_forward``: dx (B,H,H,C) from dy and the argmax, H = ``size`` (default 2 Ho)."""
    B, Ho, Wo, C = dy.shape
    g = _f32(dy)
    H = 2 * Ho if size is None else int(size)
    dx = torch.empty((B, H, H, C))
    _lib.call("mi355ppo_impala_maxpool_bwd_f32_cpu", _p(g), _p(arg.contiguous()), _p(dx), B, H, H, C)
    return dx


def _p_t(t):
    _p(t)                       # the CPU / contiguity checks
    return t


# ------------------------------------------------------------------------------------------- PQN twins (csrc/pqn.hip)
def _pqn_params(params, obs_dim, n_actions):
    p = _f32(params)
    if p.numel() != pqn_param_count(obs_dim, n_actions):
        raise ValueError(f"params: expected the {pqn_param_count(obs_dim, n_actions)} flat parameters of a ({obs_dim}, {n_actions}) QNetwork, "
                         f"got {p.numel()}")
    return p


def pqn_egreedy(q, random_actions, u, epsilon, actions_out, values_out, action_i64_out=None):
    """``mi355ppo_pqn_egreedy_f32_cpu``: the e-greedy row of pqn.py's rollout (see ops.pqn_egreedy); writes the storage rows in place."""
    N, A = q.shape
    q, rnd, uu = _f32(q), _i64(random_actions), _f32(u)
    _lib.call("mi355ppo_pqn_egreedy_f32_cpu", _p(q), _p(rnd), _p(uu), float(epsilon), _out(actions_out, torch.float32, N, "actions_out"),
              _out(values_out, torch.float32, N, "values_out"), _out(action_i64_out, torch.int64, N, "action_i64_out"), N, A)
    return actions_out, values_out


def pqn_qlambda(rewards, dones, values, next_done, next_q, gamma, q_lambda, returns=None):
    T, N = rewards.shape
    A = next_q.shape[-1]
    r, d, v, nd, nq = _f32(rewards), _f32(dones), _f32(values), _f32(next_done).reshape(-1), _f32(next_q)
    returns = torch.empty_like(r) if returns is None else returns
    _lib.call("mi355ppo_pqn_qlambda_f32_cpu", _p(r), _p(d), _p(v), _p(nd), _p(nq), _out(returns, torch.float32, T * N, "returns"), T, N, A,
              float(gamma), float(q_lambda))
    return returns


def pqn_td_loss(q, mb_inds, b_actions, b_returns, dq=None, scalars=None):
    M, A = q.shape
    qq, inds, ba, br = _f32(q), _i64(mb_inds), _f32(b_actions).reshape(-1), _f32(b_returns).reshape(-1)
    dq = torch.empty_like(qq) if dq is None else dq
    scalars = torch.empty(2) if scalars is None else scalars
    _lib.call("mi355ppo_pqn_td_loss_fwd_bwd_f32_cpu", _p(qq), _p(inds), _p(ba), _p(br), _out(dq, torch.float32, M * A, "dq"),
              _out(scalars, torch.float32, 2, "scalars"), M, A, ba.numel())
    return dq, scalars


def layernorm_relu_fwd(z, gamma, beta, C, HW, eps=1e-5, out=None, mean=None, rstd=None, bits=None, amax=None):
    """``mi355ppo_layernorm_relu_fwd_f32_cpu`` (see ops.layernorm_relu_fwd): the device's bits; an amax record's value lands in its word 0."""
    rows, D = z.shape[0], int(C) * int(HW)
    zz, g, b = _f32(z), _f32(gamma), _f32(beta)
    if zz.numel() != rows * D or g.numel() != D or b.numel() != D:
        raise ValueError(f"layernorm: rows of {D} floats with {D} gamma / beta, got {tuple(z.shape)}, {g.numel()}, {b.numel()}")
    out = torch.empty_like(zz) if out is None else out
    mean = torch.empty(rows) if mean is None else mean
    rstd = torch.empty(rows) if rstd is None else rstd
    _lib.call("mi355ppo_layernorm_relu_fwd_f32_cpu", _p(zz), _p(g), _p(b), _out(out, torch.float32, rows * D, "out"),
              _out(mean, torch.float32, rows, "mean"), _out(rstd, torch.float32, rows, "rstd"),
              _out(bits, torch.int32, rows * D // 32 if D % 32 == 0 else rows * D, "bits"), _out(amax, torch.int32, 256, "amax"), rows, int(C), int(HW),
              float(eps))
    return out, mean, rstd


def layernorm_relu_bwd(dy, z, mean, rstd, gamma, C, HW, act=None, dz=None, dgamma=None, dbeta=None, amax=None):
    """``mi355ppo_layernorm_relu_bwd_f32_cpu`` (see ops.layernorm_relu_bwd)."""
    rows, D = z.shape[0], int(C) * int(HW)
    zz, dd, g, m, r = _f32(z), _f32(dy), _f32(gamma), _f32(mean), _f32(rstd)
    aa = None if act is None else _f32(act)
    if zz.numel() != rows * D or dd.numel() != rows * D or g.numel() != D or m.numel() != rows or r.numel() != rows or (aa is not None and aa.numel() != rows * D):
        raise ValueError(f"layernorm: rows of {D} floats, got z {tuple(z.shape)}, dy {tuple(dy.shape)}, gamma {g.numel()}")
    dz = torch.empty_like(zz) if dz is None else dz
    dgamma = torch.empty_like(g) if dgamma is None else dgamma
    dbeta = torch.empty_like(g) if dbeta is None else dbeta
    _lib.call("mi355ppo_layernorm_relu_bwd_f32_cpu", _p(dd), _p(aa), _p(zz), _p(m), _p(r), _p(g), _out(dz, torch.float32, rows * D, "dz"),
              _out(dgamma, torch.float32, D, "dgamma"), _out(dbeta, torch.float32, D, "dbeta"), _out(amax, torch.int32, 256, "amax"), rows, int(C),
              int(HW))
    return dz, dgamma, dbeta


def conv1q_pack(W):
    """``mi355ppo_cnn_conv1q_pack_cpu``: kernel Q's pack of a (32, 4, 8, 8) weight, as f32 storage."""
    pack = torch.empty(_lib.load().mi355ppo_cnn_conv1q_pack_bytes() // 4, dtype=torch.float32)
    _lib.call("mi355ppo_cnn_conv1q_pack_cpu", _p(_f32(W)), _p(pack))
    return pack


def conv1q_pre_fwd(obs_u8, pack, bias, inds=None, out=None):
    """``mi355ppo_cnn_conv1q_pre_fwd_cpu`` (see ops.conv1q_pre_fwd)."""
    if obs_u8.dtype != torch.uint8 or tuple(obs_u8.shape[1:]) != (84, 84, 4):
        raise ValueError(f"conv1q_pre_fwd: source rows must be (84, 84, 4) uint8, got {tuple(obs_u8.shape)} {obs_u8.dtype}")
    ii = None if inds is None else _i64(inds)
    if ii is not None and ii.numel() and (int(ii.min()) < 0 or int(ii.max()) >= obs_u8.shape[0]):
        raise ValueError("conv1q_pre_fwd: inds out of range")
    images = obs_u8.shape[0] if ii is None else ii.numel()
    out = torch.empty((images, 20, 20, 32)) if out is None else out
    _lib.call("mi355ppo_cnn_conv1q_pre_fwd_cpu", _p(obs_u8.contiguous()), _p(ii), _p(pack), _p(_f32(bias)),
              _out(out, torch.float32, images * 12800, "out"), images)
    return out


def conv1q1_pack(W, out=None):
    """``mi355ppo_cnn_conv1q1_pack_cpu``: kernel Q1's pack of a (32, 1, 8, 8) weight, as f32 storage."""
    n = _lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4
    if tuple(W.shape) != (32, 1, 8, 8):
        raise ValueError(f"conv1q1_pack: the weight must be (32, 1, 8, 8), got {tuple(W.shape)}")
    out = torch.empty(n, dtype=torch.float32) if out is None else out
    _lib.call("mi355ppo_cnn_conv1q1_pack_cpu", _p(_f32(W)), _out(out, torch.float32, n, "pack"))
    return out


def conv1q1_pre_fwd(obs_u8, pack, bias, inds=None, out=None):
    """``mi355ppo_cnn_conv1q1_pre_fwd_cpu`` (see ops.conv1q1_pre_fwd)."""
    if obs_u8.dtype != torch.uint8 or tuple(obs_u8.shape[1:]) not in ((84, 84), (1, 84, 84), (84, 84, 1)):
        raise ValueError(f"conv1q1_pre_fwd: source rows must be (84, 84) uint8 frames, got {tuple(obs_u8.shape)} {obs_u8.dtype}")
    frames = obs_u8.contiguous().view(-1, 84, 84)
    ii = None if inds is None else _i64(inds)
    if ii is not None and ii.numel() and (int(ii.min()) < 0 or int(ii.max()) >= frames.shape[0]):
        raise ValueError("conv1q1_pre_fwd: inds out of range")
    images = frames.shape[0] if ii is None else ii.numel()
    out = torch.empty((images, 20, 20, 32)) if out is None else out
    _lib.call("mi355ppo_cnn_conv1q1_pre_fwd_cpu", _p(frames), _p(ii), _p(pack), _p(_f32(bias)), _out(out, torch.float32, images * 12800, "out"),
              images)
    return out


def conv1q1_fwd(obs_u8, pack, bias, inds=None, out=None, bits=None, amax=None):
    """``mi355ppo_cnn_conv1q1_fwd_cpu`` (see ops.conv1q1_fwd_amax / ops.conv1q1_fwd_bits): the ReLU forward, the device's bits; ``bits``
    (int32, 400 words per image) and ``amax`` (a record: its value lands in word 0) are optional."""
    if obs_u8.dtype != torch.uint8 or tuple(obs_u8.shape[1:]) not in ((84, 84), (1, 84, 84), (84, 84, 1)):
        raise ValueError(f"conv1q1_fwd: source rows must be (84, 84) uint8 frames, got {tuple(obs_u8.shape)} {obs_u8.dtype}")
    frames = obs_u8.contiguous().view(-1, 84, 84)
    ii = None if inds is None else _i64(inds)
    if ii is not None and ii.numel() and (int(ii.min()) < 0 or int(ii.max()) >= frames.shape[0]):
        raise ValueError("conv1q1_fwd: inds out of range")
    images = frames.shape[0] if ii is None else ii.numel()
    out = torch.empty((images, 20, 20, 32)) if out is None else out
    _lib.call("mi355ppo_cnn_conv1q1_fwd_cpu", _p(frames), _p(ii), _p(pack), _p(_f32(bias)), _out(out, torch.float32, images * 12800, "out"),
              _out(bits, torch.int32, images * 400, "bits"), _out(amax, torch.int32, 256, "amax"), images)
    return out


def pqn_mlp_forward(obs, params, n_actions, q_out=None):
    N, O = obs.shape
    x, p = _f32(obs), _pqn_params(params, O, n_actions)
    q_out = torch.empty((N, n_actions)) if q_out is None else q_out
    _lib.call("mi355ppo_pqn_mlp_fwd_f32_cpu", _p(x), _p(p), _out(q_out, torch.float32, N * n_actions, "q_out"), N, O, int(n_actions))
    return q_out


def pqn_mlp_act(obs, params, n_actions, random_actions, u, epsilon, actions_out, values_out, action_i64_out=None, obs_row_out=None,
                done_in=None, done_row_out=None):
    N, O = obs.shape
    x, p, rnd, uu = _f32(obs), _pqn_params(params, O, n_actions), _i64(random_actions), _f32(u)
    din = None if done_in is None else _f32(done_in)
    _lib.call("mi355ppo_pqn_mlp_act_f32_cpu", _p(x), _p(p), _p(rnd), _p(uu), float(epsilon), _out(actions_out, torch.float32, N, "actions_out"),
              _out(values_out, torch.float32, N, "values_out"), _out(action_i64_out, torch.int64, N, "action_i64_out"),
              _out(obs_row_out, torch.float32, N * O, "obs_row_out"), _p(din), _out(done_row_out, torch.float32, N, "done_row_out"), N, O,
              int(n_actions))
    return actions_out, values_out


def pqn_mlp_td_fwd_bwd(b_obs, mb_inds, params, b_actions, b_returns, grads, n_actions, scalars=None):
    B, O = b_obs.shape
    x, p, inds = _f32(b_obs), _pqn_params(params, O, n_actions), _i64(mb_inds)
    ba, br = _f32(b_actions).reshape(-1), _f32(b_returns).reshape(-1)
    scalars = torch.empty(2) if scalars is None else scalars
    _lib.call("mi355ppo_pqn_mlp_td_fwd_bwd_f32_cpu", _p(x), B, _p(inds), _p(p), _p(ba), _p(br), _out(grads, torch.float32, p.numel(), "grads"),
              _out(scalars, torch.float32, 2, "scalars"), inds.numel(), O, int(n_actions))
    return scalars


def clip_radam_(params, grads, exp_avg, exp_avg_sq, step, lr, max_grad_norm, beta1=0.9, beta2=0.999, eps=1e-8, total_norm_out=None):
    """``mi355ppo_clip_radam_f32_cpu``: clip_grad_norm_ + RAdam step ``step`` on flat CPU buffers (in place; zeroes grads)."""
    total = torch.empty(1) if total_norm_out is None else total_norm_out
    _lib.call("mi355ppo_clip_radam_f32_cpu", *_flat4(params, grads, exp_avg, exp_avg_sq), params.numel(), float(max_grad_norm), float(lr),
              float(beta1), float(beta2), float(eps), int(step), _out(total, torch.float32, 1, "total_norm_out"))
    return total


# ------------------------------------------------------------------------------------------- recurrent PQN twins (csrc/pqn_lstm.hip)
def pqn_lstm_act(gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions=None, u=None, epsilon=0.0, h_out=None, c_out=None, q_out=None,
                 actions_out=None, values_out=None, action_i64_out=None, done_row_out=None):
    """``mi355ppo_pqn_lstm_act_f32_cpu`` (see ops.pqn_lstm_act): writes the given outputs in place; ``h_out`` / ``c_out`` may be
    ``h_in`` / ``c_in``."""
    N, G = gx.shape
    H, A = G // 4, wq.shape[0]
    for t, nm in ((h_in, "h_in"), (c_in, "c_in")):          # possibly aliased by an output: taken as they are, never copied
        if t.dtype != torch.float32 or tuple(t.shape) != (N, H):
            raise ValueError(f"{nm}: expected f32 {(N, H)}, got {t.dtype} {tuple(t.shape)}")
    g, w, d, q_w, q_b = _f32(gx), _f32(w_hh), _f32(done_in).reshape(-1), _f32(wq), _f32(bq)
    if w.shape != (4 * H, H) or d.numel() != N or q_w.shape != (A, H) or q_b.numel() != A:
        raise ValueError("pqn_lstm_act: w_hh (4H, H), done_in (N,), wq (A, H), bq (A,) expected")
    rnd = None if random_actions is None else _i64(random_actions)
    uu = None if u is None else _f32(u)
    _lib.call("mi355ppo_pqn_lstm_act_f32_cpu", _p(g), _p(w), _p(h_in), _p(c_in), _p(d), _p(q_w), _p(q_b), _p(rnd), _p(uu), float(epsilon),
              _out(h_out, torch.float32, N * H, "h_out"), _out(c_out, torch.float32, N * H, "c_out"),
              _out(q_out, torch.float32, N * A, "q_out"), _out(actions_out, torch.float32, N, "actions_out"),
              _out(values_out, torch.float32, N, "values_out"), _out(action_i64_out, torch.int64, N, "action_i64_out"),
              _out(done_row_out, torch.float32, N, "done_row_out"), N, H, A)
    return q_out


def pqn_lstm_td_fwd_bwd(h, mb_inds, b_actions, b_returns, wq, bq, dwq, dbq, dh=None, scalars=None):
    """``mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu`` (see ops.pqn_lstm_td_fwd_bwd): the device's bits."""
    M, H = h.shape
    A = wq.shape[0]
    hh, inds, ba, br, q_w, q_b = _f32(h), _i64(mb_inds), _f32(b_actions).reshape(-1), _f32(b_returns).reshape(-1), _f32(wq), _f32(bq)
    if inds.numel() != M or q_w.shape != (A, H) or q_b.numel() != A or br.numel() != ba.numel():
        raise ValueError("pqn_lstm_td_fwd_bwd: mb_inds (M,), wq (A, H), bq (A,), b_actions / b_returns of one length expected")
    dh = torch.empty((M, H)) if dh is None else dh
    scalars = torch.empty(2) if scalars is None else scalars
    _lib.call("mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu", _p(hh), _p(inds), _p(ba), _p(br), _p(q_w), _p(q_b), _out(dh, torch.float32, M * H, "dh"),
              _out(dwq, torch.float32, A * H, "dwq"), _out(dbq, torch.float32, A, "dbq"), _out(scalars, torch.float32, 2, "scalars"), M, H, A,
              ba.numel())
    return dh, scalars


def sac_exp_log(x):
    """The library's own exp and log (csrc/sac_rows.h) on a float32 CPU tensor -> (exp, log)."""
    x = _f32(x).reshape(-1)
    e, l = torch.empty_like(x), torch.empty_like(x)
    _lib.call("mi355ppo_sac_exp_log_f32_cpu", _p(x), _p(e), _p(l), x.numel())
    return e, l


# ------------------------------------------------------------------------------------------- the replay-ring families
# The host side of cleanrl_amd/replay_ops.py: ``ops._chk`` for CPU tensors, and the ``*_cpu`` twin, which takes neither workspace nor stream.
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


def _twin(name, dev, *args):
    _lib.call(name + "_cpu", *args)


def _twin_ws(name, dev, ws_bytes, dims, *args):
    _lib.call(name + "_cpu", *args)


_SIDE = replay_ops.Side(True, _chk, _twin, _twin_ws)
replay_ops.bind(_SIDE, globals())

# ------------------------------------------------------------------------------------------- RND (csrc/rnd.hip)
from .rnd_ops import RND_FEATURES, RND_MAX_BATCH, RND_MAX_STEPS, RND_PIXELS, rnd_mean_var  # noqa: E402,F401

rnd_ops.bind(_SIDE, globals())

# ------------------------------------------------------------------------------------------- PPG's auxiliary phase (csrc/ppg.hip)
from .ppg_ops import PPG_HIDDEN, PPG_MAX_ACT, PPG_MAX_ROWS, PPG_MIN_ACT  # noqa: E402,F401

ppg_ops.bind(_SIDE, globals())
