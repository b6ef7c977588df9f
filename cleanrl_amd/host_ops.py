"""Host (CPU) path: the ``*_cpu`` host-pointer twins of ``libmi355ppo.so`` behind the same seams as the GPU path.

Selected ONLY when the user asks for a CPU device (``--no-cuda``: BASELINE config A "CartPole on CPU,
plumbing", and the world_size-2 ``gloo`` tests of the data-parallel logic).  It is not a fallback: a
CUDA device always runs the HIP kernels and raises if ``libmi355ppo.so`` is missing, and these functions
refuse CUDA tensors.  The twins (csrc/host_twins.hip, declared in include/mi355ppo.h) are the device
kernels' own row / element functions compiled for the host, so the CPU loop crosses the SAME C ABI seams
as the GPU loop: GAE (ppo.py:218-231), the fused loss forward + backward (ppo.py:250-285 and its autograd),
the LSTM sequence scans of ppo_atari_lstm.py (opt-in: ``MI355PPO_LSTM=fused``), the TrXL memory attention of ppo_trxl.py
(opt-in: ``MI355PPO_TRXL=fused``) and, for tests, sampling and clip + Adam.  The learners whose loss has extra terms (LSTM state, RND's second value
head and distillation loss) cross the same twin on their logits / value and add their terms outside.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from .ops import ATARI_FRAME, IMPALA84_OUT, IMPALA_CHANNELS, _lstm_dims, _ptr_array, dqn_counts, dqn_head_limits_ok, dqn_limits_ok, offpolicy_counts, pqn_param_count, radam_schedule, rainbow_head_limits_ok, rainbow_new_buffer, rainbow_noisy_counts, rainbow_noisy_limits_ok, _rainbow_head, _rainbow_head_update_args, sac_actor_count, sacd_limits_ok, _frame_ring2, _sacd_heads, trxl_dims  # noqa: F401  (one definition for both modules)

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


# ------------------------------------------------------------------------------------------- DDPG / TD3 twins (csrc/offpolicy.hip)
def _in(t, dtype, shape, name):
    """An input the twin reads ``prod(shape)`` elements of: taken as it is (the ring is never copied)."""
    _p(t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected {dtype} {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return ctypes.c_void_p(t.data_ptr())


def _ring_dims(ring):
    obs, nxt, act, rew, done = ring
    slots, N, O = obs.shape
    A = act.shape[-1]
    ptrs = [_in(t, torch.float32, shape, nm) for t, nm, shape in (
        (obs, "ring obs", (slots, N, O)), (nxt, "ring next_obs", (slots, N, O)), (act, "ring actions", (slots, N, A)),
        (rew, "ring rewards", (slots, N)), (done, "ring dones", (slots, N)))]
    return slots, N, O, A, ptrs


def replay_add(ring, pos, obs, next_obs, actions, rewards, dones):
    slots, N, O, A, rp = _ring_dims(ring)
    _lib.call("mi355ppo_replay_add_f32_cpu", _in(obs, torch.float32, (N, O), "obs"), _in(next_obs, torch.float32, (N, O), "next_obs"),
              _in(actions, torch.float32, (N, A), "actions"), _in(rewards, torch.float32, (N,), "rewards"),
              _in(dones, torch.float32, (N,), "dones"), *rp, int(pos), slots, N, O, A)


def ddpg_act(obs, actor_params, action_scale, action_bias, noise_row, low, high, actions_out):
    N, O = obs.shape
    (A,) = action_scale.shape
    nz = None if noise_row is None else _in(noise_row, torch.float32, (A,), "noise_row")
    _lib.call("mi355ppo_ddpg_act_f32_cpu", _in(obs, torch.float32, (N, O), "obs"),
              _in(actor_params, torch.float32, (offpolicy_counts(O, A)[0],), "actor_params"), _in(action_scale, torch.float32, (A,), "action_scale"),
              _in(action_bias, torch.float32, (A,), "action_bias"), nz, _in(low, torch.float32, (A,), "low"), _in(high, torch.float32, (A,), "high"),
              _out(actions_out, torch.float32, N * A, "actions_out"), N, O, A)
    return actions_out


def td3_target(ring, batch_inds, env_inds, target_actor, target_critics, n_critics, action_scale, action_bias, noise, policy_noise,
               noise_clip, low0, high0, gamma, next_q_value, next_actions_out=None):
    slots, N, O, A, rp = _ring_dims(ring)
    (M,) = batch_inds.shape
    pa, pq = offpolicy_counts(O, A)
    nz = None if noise is None else _in(noise, torch.float32, (M, A), "noise")
    _lib.call("mi355ppo_td3_target_f32_cpu", rp[1], rp[3], rp[4], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(target_actor, torch.float32, (pa,), "target_actor"),
              _in(target_critics, torch.float32, (int(n_critics) * pq,), "target_critics"), int(n_critics),
              _in(action_scale, torch.float32, (A,), "action_scale"), _in(action_bias, torch.float32, (A,), "action_bias"), nz,
              float(policy_noise), float(noise_clip), float(low0), float(high0), float(gamma),
              _out(next_q_value, torch.float32, M, "next_q_value"), _out(next_actions_out, torch.float32, M * A, "next_actions_out"), M, O, A)
    return next_q_value


def td3_critic_fwd_bwd(ring, batch_inds, env_inds, critics, n_critics, next_q_value, grads, scalars):
    slots, N, O, A, rp = _ring_dims(ring)
    (M,) = batch_inds.shape
    P = int(n_critics) * offpolicy_counts(O, A)[1]
    _lib.call("mi355ppo_td3_critic_fwd_bwd_f32_cpu", rp[0], rp[2], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(critics, torch.float32, (P,), "critics"), int(n_critics),
              _in(next_q_value, torch.float32, (M,), "next_q_value"), _out(grads, torch.float32, P, "grads"),
              _out(scalars, torch.float32, 2 * int(n_critics), "scalars"), M, O, A)
    return scalars


def td3_actor_fwd_bwd(ring, batch_inds, env_inds, actor, qf1, action_scale, action_bias, grads, actor_loss, dq_daction_out=None):
    slots, N, O, A, rp = _ring_dims(ring)
    (M,) = batch_inds.shape
    pa, pq = offpolicy_counts(O, A)
    _lib.call("mi355ppo_td3_actor_fwd_bwd_f32_cpu", rp[0], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(actor, torch.float32, (pa,), "actor"),
              _in(qf1, torch.float32, (pq,), "qf1"), _in(action_scale, torch.float32, (A,), "action_scale"),
              _in(action_bias, torch.float32, (A,), "action_bias"), _out(grads, torch.float32, pa, "grads"),
              _out(actor_loss, torch.float32, 1, "actor_loss"), _out(dq_daction_out, torch.float32, M * A, "dq_daction_out"), M, O, A)
    return actor_loss


def polyak_(params, target_params, tau):
    n = params.numel()
    _lib.call("mi355ppo_polyak_f32_cpu", _in(params, torch.float32, (n,), "params"), _out(target_params, torch.float32, n, "target_params"),
              n, float(tau))
    return target_params


# ------------------------------------------------------------------------------------------- SAC twins (csrc/sac.hip)
def sac_exp_log(x):
    """The library's own exp and log (csrc/sac_rows.h) on a float32 CPU tensor -> (exp, log)."""
    x = _f32(x).reshape(-1)
    e, l = torch.empty_like(x), torch.empty_like(x)
    _lib.call("mi355ppo_sac_exp_log_f32_cpu", _p(x), _p(e), _p(l), x.numel())
    return e, l


def sac_policy(obs, actor, action_scale, action_bias, eps, actions_out=None, log_pi_out=None, batch_inds=None, env_inds=None):
    rows, A = eps.shape
    if batch_inds is None:
        slots, N, O = 0, 0, obs.shape[-1]
        op, bi, ei = _in(obs, torch.float32, (rows, O), "obs"), None, None
    else:
        slots, N, O = obs.shape
        op = _in(obs, torch.float32, (slots, N, O), "obs")
        bi, ei = _in(batch_inds, torch.int64, (rows,), "batch_inds"), _in(env_inds, torch.int64, (rows,), "env_inds")
    _lib.call("mi355ppo_sac_policy_f32_cpu", op, bi, ei, slots, N, _in(actor, torch.float32, (sac_actor_count(O, A),), "actor"),
              _in(action_scale, torch.float32, (A,), "action_scale"), _in(action_bias, torch.float32, (A,), "action_bias"),
              _in(eps, torch.float32, (rows, A), "eps"), _out(actions_out, torch.float32, rows * A, "actions_out"),
              _out(log_pi_out, torch.float32, rows, "log_pi_out"), rows, O, A)
    return actions_out, log_pi_out


def sac_target(ring, batch_inds, env_inds, actor, target_critics, action_scale, action_bias, eps, alpha, gamma, next_q_value,
               next_actions_out=None, log_pi_out=None):
    slots, N, O, A, rp = _ring_dims(ring)
    (M,) = batch_inds.shape
    _lib.call("mi355ppo_sac_target_f32_cpu", rp[1], rp[3], rp[4], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(actor, torch.float32, (sac_actor_count(O, A),), "actor"),
              _in(target_critics, torch.float32, (2 * offpolicy_counts(O, A)[1],), "target_critics"),
              _in(action_scale, torch.float32, (A,), "action_scale"), _in(action_bias, torch.float32, (A,), "action_bias"),
              _in(eps, torch.float32, (M, A), "eps"), _in(alpha, torch.float32, (1,), "alpha"), float(gamma),
              _out(next_q_value, torch.float32, M, "next_q_value"), _out(next_actions_out, torch.float32, M * A, "next_actions_out"),
              _out(log_pi_out, torch.float32, M, "log_pi_out"), M, O, A)
    return next_q_value


def sac_actor_fwd_bwd(ring, batch_inds, env_inds, actor, critics, action_scale, action_bias, eps, alpha, grads, actor_loss,
                      log_pi_out=None, dmean_out=None, du_out=None):
    slots, N, O, A, rp = _ring_dims(ring)
    (M,) = batch_inds.shape
    pa = sac_actor_count(O, A)
    _lib.call("mi355ppo_sac_actor_fwd_bwd_f32_cpu", rp[0], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(actor, torch.float32, (pa,), "actor"),
              _in(critics, torch.float32, (2 * offpolicy_counts(O, A)[1],), "critics"), _in(action_scale, torch.float32, (A,), "action_scale"),
              _in(action_bias, torch.float32, (A,), "action_bias"), _in(eps, torch.float32, (M, A), "eps"),
              _in(alpha, torch.float32, (1,), "alpha"), _out(grads, torch.float32, pa, "grads"), _out(actor_loss, torch.float32, 1, "actor_loss"),
              _out(log_pi_out, torch.float32, M, "log_pi_out"), _out(dmean_out, torch.float32, M * A, "dmean_out"),
              _out(du_out, torch.float32, M * A, "du_out"), M, O, A)
    return actor_loss


def sac_alpha_(log_pi, target_entropy, log_alpha, exp_avg, exp_avg_sq, step, lr, alpha_out, alpha_loss_out, sched2=None, beta1=0.9,
               beta2=0.999, eps=1e-8):
    """The twin takes the Adam step count by value; ``sched2`` (the device path's schedule in device memory) is refused."""
    if sched2 is not None:
        raise ValueError("sac_alpha_: the host twin takes `step` and `lr`; a schedule tensor is the device path's (cleanrl_amd.ops)")
    (M,) = log_pi.shape
    _lib.call("mi355ppo_sac_alpha_f32_cpu", _in(log_pi, torch.float32, (M,), "log_pi"), M, float(target_entropy),
              _out(log_alpha, torch.float32, 1, "log_alpha"), _out(exp_avg, torch.float32, 1, "exp_avg"),
              _out(exp_avg_sq, torch.float32, 1, "exp_avg_sq"), float(lr), float(beta1), float(beta2), float(eps), int(step),
              _out(alpha_out, torch.float32, 1, "alpha_out"), _out(alpha_loss_out, torch.float32, 1, "alpha_loss_out"))
    return alpha_out


# ------------------------------------------------------------------------------------------- DQN / C51 twins (csrc/dqn.hip)
def _opt_out(t, numel, name):
    return None if t is None else _out(t, torch.float32, numel, name)


def dqn_act(obs, params, n_actions, actions_out, atoms=None, q_out=None):
    N, O = obs.shape
    na = 1 if atoms is None else atoms.numel()
    _lib.call("mi355ppo_dqn_act_f32_cpu", _in(obs, torch.float32, (N, O), "obs"),
              _in(params, torch.float32, (dqn_counts(O, n_actions, na),), "params"),
              None if atoms is None else _in(atoms, torch.float32, (na,), "atoms"), _out(actions_out, torch.int64, N, "actions_out"),
              _opt_out(q_out, N * n_actions, "q_out"), N, O, int(n_actions), na)
    return actions_out


def _dqn_ring(ring):
    slots, N, O, A, rp = _ring_dims(ring)
    if A != 1:
        raise ValueError(f"ring actions: the DQN / C51 ring stores one action index per env, got width {A}")
    return slots, N, O, rp


def dqn_td_fwd_bwd(ring, batch_inds, env_inds, online, target, n_actions, gamma, grads, scalars, target_q_out=None, td_target_out=None):
    slots, N, O, rp = _dqn_ring(ring)
    (M,) = batch_inds.shape
    P = dqn_counts(O, n_actions)
    _lib.call("mi355ppo_dqn_td_fwd_bwd_f32_cpu", *rp, _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(online, torch.float32, (P,), "online"),
              _in(target, torch.float32, (P,), "target"), float(gamma), _out(grads, torch.float32, P, "grads"),
              _out(scalars, torch.float32, 2, "scalars"), _opt_out(target_q_out, M * n_actions, "target_q_out"),
              _opt_out(td_target_out, M, "td_target_out"), M, O, int(n_actions))
    return scalars


def c51_fwd_bwd(ring, batch_inds, env_inds, online, target, atoms, n_actions, gamma, v_min, v_max, grads, scalars, next_pmfs_out=None,
                target_pmfs_out=None):
    slots, N, O, rp = _dqn_ring(ring)
    (M,) = batch_inds.shape
    na = atoms.numel()
    P = dqn_counts(O, n_actions, na)
    _lib.call("mi355ppo_c51_fwd_bwd_f32_cpu", *rp, _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _in(online, torch.float32, (P,), "online"),
              _in(target, torch.float32, (P,), "target"), _in(atoms, torch.float32, (na,), "atoms"), float(gamma), float(v_min), float(v_max),
              _out(grads, torch.float32, P, "grads"), _out(scalars, torch.float32, 2, "scalars"),
              _opt_out(next_pmfs_out, M * na, "next_pmfs_out"), _opt_out(target_pmfs_out, M * na, "target_pmfs_out"), M, O, int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- Atari DQN / C51 twins (csrc/dqn_atari.hip)
def _frame_ring(ring):
    frames, act, rew, done = ring
    slots, N = frames.shape[:2]
    specs = ((frames, torch.uint8, (slots, N) + ATARI_FRAME, "ring frames"), (act, torch.int64, (slots, N), "ring actions"),
             (rew, torch.float32, (slots, N), "ring rewards"), (done, torch.float32, (slots, N), "ring dones"))
    return slots, N, [_in(t, dt, shape, nm) for t, dt, shape, nm in specs]


def replay_add_u8(ring, pos, obs, next_obs, actions, rewards, dones):
    slots, N, rp = _frame_ring(ring)
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_replay_add_u8_cpu", _in(obs, torch.uint8, (N, C, H, W), "obs"), _in(next_obs, torch.uint8, (N, C, H, W), "next_obs"),
              _in(actions, torch.int64, (N,), "actions"), _in(rewards, torch.float32, (N,), "rewards"), _in(dones, torch.float32, (N,), "dones"),
              *rp, int(pos), slots, N)


def replay_gather_u8(ring, batch_inds, env_inds, frames_out, actions_out, rewards_out, dones_out):
    slots, N, rp = _frame_ring(ring)
    (M,) = batch_inds.shape
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_replay_gather_u8_cpu", *rp, _in(batch_inds, torch.int64, (M,), "batch_inds"), _in(env_inds, torch.int64, (M,), "env_inds"),
              slots, N, _out(frames_out, torch.uint8, 2 * M * H * W * C, "frames_out"), _out(actions_out, torch.int64, M, "actions_out"),
              _out(rewards_out, torch.float32, M, "rewards_out"), _out(dones_out, torch.float32, M, "dones_out"), M)
    return frames_out


def dqn_head_act(h, w, b, n_actions, actions_out, atoms=None, q_out=None):
    N, hidden = h.shape
    na = 1 if atoms is None else atoms.numel()
    J = int(n_actions) * na
    _lib.call("mi355ppo_dqn_head_act_f32_cpu", _in(h, torch.float32, (N, hidden), "h"), _in(w, torch.float32, (J, hidden), "w"),
              _in(b, torch.float32, (J,), "b"), None if atoms is None else _in(atoms, torch.float32, (na,), "atoms"),
              _out(actions_out, torch.int64, N, "actions_out"), _opt_out(q_out, N * n_actions, "q_out"), N, hidden, int(n_actions), na)
    return actions_out


def _head_update_ptrs(h, h_next, w, b, w_target, b_target, actions, rewards, dones, J):
    M, hidden = h.shape
    return M, hidden, [_in(h, torch.float32, (M, hidden), "h"), _in(h_next, torch.float32, (M, hidden), "h_next"),
                       _in(w, torch.float32, (J, hidden), "w"), _in(b, torch.float32, (J,), "b"),
                       _in(w_target, torch.float32, (J, hidden), "w_target"), _in(b_target, torch.float32, (J,), "b_target")], [
                       _in(actions, torch.int64, (M,), "actions"), _in(rewards, torch.float32, (M,), "rewards"),
                       _in(dones, torch.float32, (M,), "dones")]


def _head_grads(dh, dw, db, scalars, M, hidden, J):
    return [_out(dh, torch.float32, M * hidden, "dh"), _out(dw, torch.float32, J * hidden, "dw"), _out(db, torch.float32, J, "db"),
            _out(scalars, torch.float32, 2, "scalars")]


def dqn_head_td_fwd_bwd(h, h_next, w, b, w_target, b_target, actions, rewards, dones, n_actions, gamma, dh, dw, db, scalars,
                        target_q_out=None, td_target_out=None):
    J = int(n_actions)
    M, hidden, nets, batch = _head_update_ptrs(h, h_next, w, b, w_target, b_target, actions, rewards, dones, J)
    _lib.call("mi355ppo_dqn_head_td_fwd_bwd_f32_cpu", *nets, *batch, float(gamma), *_head_grads(dh, dw, db, scalars, M, hidden, J),
              _opt_out(target_q_out, M * J, "target_q_out"), _opt_out(td_target_out, M, "td_target_out"), M, hidden, J)
    return scalars


def c51_head_fwd_bwd(h, h_next, w, b, w_target, b_target, atoms, actions, rewards, dones, n_actions, gamma, v_min, v_max, dh, dw, db, scalars,
                     next_pmfs_out=None, target_pmfs_out=None):
    na = atoms.numel()
    J = int(n_actions) * na
    M, hidden, nets, batch = _head_update_ptrs(h, h_next, w, b, w_target, b_target, actions, rewards, dones, J)
    _lib.call("mi355ppo_c51_head_fwd_bwd_f32_cpu", *nets, _in(atoms, torch.float32, (na,), "atoms"), *batch, float(gamma), float(v_min),
              float(v_max), *_head_grads(dh, dw, db, scalars, M, hidden, J), _opt_out(next_pmfs_out, M * na, "next_pmfs_out"),
              _opt_out(target_pmfs_out, M * na, "target_pmfs_out"), M, hidden, int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- QDagger head twins (csrc/qdagger.hip)
def qdagger_head_act(h, w, b, actions_out, q_out=None):
    N, hidden = h.shape
    n = b.numel()
    _lib.call("mi355ppo_qdagger_head_act_f32_cpu", _in(h, torch.float32, (N, hidden), "h"), _in(w, torch.float32, (n, hidden), "w"),
              _in(b, torch.float32, (n,), "b"), _out(actions_out, torch.int64, N, "actions_out"), _opt_out(q_out, N * n, "q_out"), N, hidden, n)
    return actions_out


def qdagger_head_fwd_bwd(h, h_next, w, b, w_target, b_target, teacher_q, actions, rewards, dones, gamma, temperature, distill_coeff, dh, dw, db,
                         scalars, target_q_out=None, td_target_out=None):
    n = b.numel()
    M, hidden, nets, batch = _head_update_ptrs(h, h_next, w, b, w_target, b_target, actions, rewards, dones, n)
    _lib.call("mi355ppo_qdagger_head_fwd_bwd_f32_cpu", *nets, _in(teacher_q, torch.float32, (M, n), "teacher_q"), *batch, float(gamma),
              float(temperature), float(distill_coeff), _out(dh, torch.float32, M * hidden, "dh"), _out(dw, torch.float32, n * hidden, "dw"),
              _out(db, torch.float32, n, "db"), _out(scalars, torch.float32, 4, "scalars"), _opt_out(target_q_out, M * n, "target_q_out"),
              _opt_out(td_target_out, M, "td_target_out"), M, hidden, n)
    return scalars


# ------------------------------------------------------------------------------------------- Rainbow twins (csrc/rainbow_twins.hip)
def _per_buffer(buf):
    ring_obs, ring_next, act, rew, done, tree, state, size = buf
    slots = ring_obs.shape[0]
    specs = ((ring_obs, torch.uint8, (slots,) + ATARI_FRAME, "ring obs"), (ring_next, torch.uint8, (slots,) + ATARI_FRAME, "ring next_obs"),
             (act, torch.int64, (slots,), "ring actions"), (rew, torch.float32, (slots,), "ring rewards"),
             (done, torch.float32, (slots,), "ring dones"), (tree, torch.float32, (2 * slots - 1,), "tree"), (state, torch.float32, (2,), "state"),
             (size, torch.int64, (1,), "size"))
    return slots, [_in(t, dt, shape, nm) for t, dt, shape, nm in specs]


def rainbow_per_add_u8(buf, pos, obs, next_obs, action, reward, done, alpha):
    slots, bp = _per_buffer(buf)
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_rainbow_per_add_u8_cpu", _in(obs, torch.uint8, (1, C, H, W), "obs"), _in(next_obs, torch.uint8, (1, C, H, W), "next_obs"),
              _in(action, torch.int64, (1,), "action"), _in(reward, torch.float32, (1,), "reward"), _in(done, torch.float32, (1,), "done"),
              *bp, int(pos), slots, float(alpha))


def rainbow_per_sample(buf, u, indices_out, weights_out):
    slots, bp = _per_buffer(buf)
    (B,) = u.shape
    _lib.call("mi355ppo_rainbow_per_sample_cpu", _in(u, torch.float64, (B,), "u"), bp[5], bp[6], bp[7], slots,
              _out(indices_out, torch.int64, B, "indices_out"), _out(weights_out, torch.float32, B, "weights_out"), B)
    return indices_out, weights_out


def rainbow_per_gather_u8(buf, indices, frames_out, actions_out, rewards_out, dones_out):
    slots, bp = _per_buffer(buf)
    (M,) = indices.shape
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_rainbow_per_gather_u8_cpu", *bp[:5], _in(indices, torch.int64, (M,), "indices"), slots,
              _out(frames_out, torch.uint8, 2 * M * H * W * C, "frames_out"), _out(actions_out, torch.int64, M, "actions_out"),
              _out(rewards_out, torch.float32, M, "rewards_out"), _out(dones_out, torch.float32, M, "dones_out"), M)
    return frames_out


def rainbow_per_update(buf, indices, loss_per_sample, alpha, eps):
    slots, bp = _per_buffer(buf)
    (B,) = indices.shape
    _lib.call("mi355ppo_rainbow_per_update_cpu", _in(indices, torch.int64, (B,), "indices"),
              _in(loss_per_sample, torch.float32, (B,), "loss_per_sample"), bp[5], bp[6], slots, float(alpha), float(eps), B)


def rainbow_noisy_compose(params, eps, effective, n_actions, n_atoms):
    E, P = rainbow_noisy_counts(n_actions, n_atoms)
    _lib.call("mi355ppo_rainbow_noisy_compose_f32_cpu", _in(params, torch.float32, (P,), "params"), _in(eps, torch.float32, (E,), "eps"),
              _out(effective, torch.float32, E, "effective"), int(n_actions), int(n_atoms))
    return effective


def rainbow_noisy_grad(effective_grad, eps, grads, n_actions, n_atoms):
    E, P = rainbow_noisy_counts(n_actions, n_atoms)
    _lib.call("mi355ppo_rainbow_noisy_grad_f32_cpu", _in(effective_grad, torch.float32, (E,), "effective_grad"),
              _in(eps, torch.float32, (E,), "eps"), _out(grads, torch.float32, P, "grads"), int(n_actions), int(n_atoms))
    return grads


def _host_chk(t, dtype, name, shape):
    return _in(t, dtype, shape, name)


def rainbow_head_act(h, w_out, b_out, support, n_actions, actions_out, q_out=None):
    N, na, J = _rainbow_head(h, w_out, b_out, support, n_actions, _host_chk)
    _lib.call("mi355ppo_rainbow_head_act_f32_cpu", _p(h), _p(w_out), _p(b_out), _p(support), _out(actions_out, torch.int64, N, "actions_out"),
              _opt_out(q_out, N * n_actions, "q_out"), N, int(n_actions), na)
    return actions_out


def rainbow_head_fwd_bwd(h, h_next, h_next_target, w_out, b_out, w_out_target, b_out_target, support, actions, rewards, dones, weights,
                         n_actions, gamma_n, v_min, v_max, dh, dw_out, db_out, scalars, loss_per_sample, best_actions_out=None,
                         next_pmfs_out=None, target_pmfs_out=None):
    M, na = _rainbow_head_update_args(h, h_next, h_next_target, w_out, b_out, w_out_target, b_out_target, support, actions, rewards, dones, weights,
                                      n_actions, dh, dw_out, db_out, scalars, loss_per_sample, best_actions_out, next_pmfs_out, target_pmfs_out,
                                      _host_chk)
    _lib.call("mi355ppo_rainbow_head_fwd_bwd_f32_cpu", _p(h), _p(h_next), _p(h_next_target), _p(w_out), _p(b_out), _p(w_out_target), _p(b_out_target),
              _p(support), _p(actions), _p(rewards), _p(dones), _p(weights), float(gamma_n), float(v_min), float(v_max), _p(dh), _p(dw_out),
              _p(db_out), _p(scalars), _p(loss_per_sample), _p(best_actions_out), _p(next_pmfs_out), _p(target_pmfs_out), M, int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- discrete SAC on Atari twins (csrc/sac_atari_twins.hip)
def replay_add2_u8(ring, pos, obs, next_obs, actions, rewards, dones):
    slots, N = _frame_ring2(ring, _host_chk)
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_replay_add2_u8_cpu", _in(obs, torch.uint8, (N, C, H, W), "obs"), _in(next_obs, torch.uint8, (N, C, H, W), "next_obs"),
              _in(actions, torch.int64, (N,), "actions"), _in(rewards, torch.float32, (N,), "rewards"), _in(dones, torch.float32, (N,), "dones"),
              *[_p(t) for t in ring], int(pos), slots, N)


def replay_gather2_u8(ring, batch_inds, env_inds, frames_out, actions_out, rewards_out, dones_out):
    slots, N = _frame_ring2(ring, _host_chk)
    (M,) = batch_inds.shape
    H, W, C = ATARI_FRAME
    _lib.call("mi355ppo_replay_gather2_u8_cpu", *[_p(t) for t in ring], _in(batch_inds, torch.int64, (M,), "batch_inds"),
              _in(env_inds, torch.int64, (M,), "env_inds"), slots, N, _out(frames_out, torch.uint8, 2 * M * H * W * C, "frames_out"),
              _out(actions_out, torch.int64, M, "actions_out"), _out(rewards_out, torch.float32, M, "rewards_out"),
              _out(dones_out, torch.float32, M, "dones_out"), M)
    return frames_out


def sacd_head_act(h, w, b, noise_exp1, actions_out, probs_out=None):
    N, hidden, n = _sacd_heads((h,), ((w, b),), _host_chk)
    _lib.call("mi355ppo_sacd_head_act_f32_cpu", _p(h), _p(w), _p(b), _in(noise_exp1, torch.float32, (N, n), "noise_exp1"),
              _out(actions_out, torch.int64, N, "actions_out"), _opt_out(probs_out, N * n, "probs_out"), N, hidden, n)
    return actions_out


def sacd_critic_fwd_bwd(hs, heads, actions, rewards, dones, alpha, gamma, dhs, grads, scalars, v_out=None, y_out=None):
    M, hidden, n = _sacd_heads(hs, heads, _host_chk)
    if len(hs) != 5:
        raise ValueError(f"the critic update takes five heads, got {len(hs)}")
    outs = [_out(dhs[0], torch.float32, M * hidden, "dh1"), _out(dhs[1], torch.float32, M * hidden, "dh2")]
    for i in range(2):
        outs += [_out(grads[i][0], torch.float32, n * hidden, f"dw{i + 1}"), _out(grads[i][1], torch.float32, n, f"db{i + 1}")]
    _lib.call("mi355ppo_sacd_critic_fwd_bwd_f32_cpu", *[_p(h) for h in hs], *[_p(t) for wb in heads for t in wb],
              _in(actions, torch.int64, (M,), "actions"), _in(rewards, torch.float32, (M,), "rewards"), _in(dones, torch.float32, (M,), "dones"),
              _in(alpha, torch.float32, (1,), "alpha"), float(gamma), *outs, _out(scalars, torch.float32, 4, "scalars"),
              _opt_out(v_out, M, "v_out"), _opt_out(y_out, M, "y_out"), M, hidden, n)
    return scalars


def sacd_actor_fwd_bwd(hs, heads, alpha, target_entropy, dh, dw, db, entropy_rows, actor_loss):
    M, hidden, n = _sacd_heads(hs, heads, _host_chk)
    if len(hs) != 3:
        raise ValueError(f"the actor update takes three heads, got {len(hs)}")
    _lib.call("mi355ppo_sacd_actor_fwd_bwd_f32_cpu", *[_p(h) for h in hs], *[_p(t) for wb in heads for t in wb],
              _in(alpha, torch.float32, (1,), "alpha"), float(target_entropy), _out(dh, torch.float32, M * hidden, "dh"),
              _out(dw, torch.float32, n * hidden, "dw"), _out(db, torch.float32, n, "db"), _out(entropy_rows, torch.float32, M, "entropy_rows"),
              _out(actor_loss, torch.float32, 1, "actor_loss"), M, hidden, n)
    return actor_loss
