"""The PPG auxiliary-phase operators (csrc/ppg.hip), each defined once for the HIP entry point and its host twin, as the
RND operators are (cleanrl_amd/rnd_ops.py): ``cleanrl_amd.ops`` and ``cleanrl_amd.host_ops`` bind them to their side at import.
Nothing is coerced or copied; every check runs before the C call.

A minibatch is ``cols`` (n,) int64, distinct stored rollouts; flat row ``t * n + i`` is ``(t, cols[i])`` -- ``flatten01`` over (T, n).
The host side also checks ``0 <= cols < R``; the device side cannot without a device->host copy, and the kernels clamp.
"""
from __future__ import annotations

import types

import torch

from .replay_ops import _ptr

OPERATORS = ("ppg_aux_gather", "ppg_old_logits_", "ppg_aux_fwd_bwd", "clip_adam_split_")

PPG_HIDDEN, PPG_MIN_ACT, PPG_MAX_ACT, PPG_MAX_ROWS = 256, 2, 30, 1 << 16


def bind(side, namespace: dict) -> None:
    for name in OPERATORS:
        namespace[name] = types.MethodType(globals()[name], side)


def _cols(s, cols, R: int, fn: str) -> int:
    (n,) = cols.shape
    s.chk(cols, torch.int64, "cols", (n,))
    if not 0 < n <= R:
        raise ValueError(f"{fn}: {n} cols of {R} stored rollouts: 1 <= n <= R")
    if s.host and (int(cols.min()) < 0 or int(cols.max()) >= R):
        raise ValueError(f"{fn}: cols must lie in [0, {R})")
    return n


def _head_dims(fn: str, A: int, H: int) -> None:
    if H != PPG_HIDDEN:
        raise ValueError(f"{fn}: hidden width {H}: the kernels are written for {PPG_HIDDEN}")
    if not PPG_MIN_ACT <= A <= PPG_MAX_ACT:
        raise ValueError(f"{fn}: {A} actions: {PPG_MIN_ACT} <= A <= {PPG_MAX_ACT} (A + 2 outputs fit one 32-output tile)")


def _rows(fn: str, T: int, n: int) -> int:
    if T * n > PPG_MAX_ROWS:
        raise ValueError(f"{fn}: {T * n} rows exceed {PPG_MAX_ROWS}")
    return T * n


def ppg_aux_gather(s, aux_obs, cols, out=None):
    """``obs_u8_to_f32(flatten01(aux_obs.index_select(1, cols)))`` in one launch (ppg_procgen.py:436-438): aux_obs (T, R, ...) u8 ->
    out (T * n, ...) f32 = byte / 255."""
    s.chk(aux_obs, torch.uint8, "aux_obs")
    if aux_obs.dim() < 3:
        raise ValueError(f"ppg_aux_gather: aux_obs must be (T, R, ...), got {tuple(aux_obs.shape)}")
    T, R = aux_obs.shape[:2]
    row_shape = tuple(aux_obs.shape[2:])
    row_bytes = 1
    for d in row_shape:
        row_bytes *= d
    if T < 1 or R < 1 or row_bytes < 4 or row_bytes % 4:
        raise ValueError(f"ppg_aux_gather: aux_obs {tuple(aux_obs.shape)}: T, R >= 1 and rows of a positive multiple of 4 bytes")
    n = _cols(s, cols, R, "ppg_aux_gather")
    if T * n >= 1 << 31:
        raise ValueError(f"ppg_aux_gather: {T * n} rows exceed 2^31 - 1")
    if out is None:
        out = torch.empty((T * n,) + row_shape, dtype=torch.float32, device=aux_obs.device)
    s.chk(out, torch.float32, "out", (T * n,) + row_shape)
    s.launch("mi355ppo_ppg_aux_gather_u8_f32", aux_obs.device, _ptr(aux_obs), _ptr(cols), _ptr(out), T, n, R, row_bytes)
    return out


def ppg_old_logits_(s, h, weight, bias, cols, aux_pi):
    """The old policy of a minibatch (:424-433): ``Categorical(logits=h @ weight.T + bias).logits`` written into
    ``aux_pi[:, cols]`` (aux_pi (T, R, A)); h (T * n, 256)."""
    s.chk(aux_pi, torch.float32, "aux_pi")
    if aux_pi.dim() != 3:
        raise ValueError(f"ppg_old_logits_: aux_pi must be (T, R, A), got {tuple(aux_pi.shape)}")
    T, R, A = aux_pi.shape
    n = _cols(s, cols, R, "ppg_old_logits_")
    M, H = h.shape
    _head_dims("ppg_old_logits_", A, H)
    s.chk(h, torch.float32, "h", (_rows("ppg_old_logits_", T, n), H))
    s.chk(weight, torch.float32, "weight", (A, H))
    s.chk(bias, torch.float32, "bias", (A,))
    s.launch("mi355ppo_ppg_old_logits_f32", h.device, _ptr(h), _ptr(weight), _ptr(bias), _ptr(cols), _ptr(aux_pi), T, n, R, A, H)
    return aux_pi


def ppg_aux_fwd_bwd(s, h, heads, aux_pi, aux_returns, cols, beta_clone: float, inv_accum: float, head_grads, accumulate: bool,
                    scalars=None, dh=None):
    """The three heads, the joint loss of an auxiliary minibatch and its backward (:449-462) -> (scalars (3,) = {kl_loss,
    aux_value_loss, real_value_loss}, dh (M, 256)).  ``heads`` = (actor.weight, actor.bias, critic.weight, critic.bias,
    aux_critic.weight, aux_critic.bias); ``head_grads``: their six gradients, overwritten (``accumulate`` False) or added to.  dh and
    the gradients are those of ``(aux_value_loss + beta_clone * kl_loss + real_value_loss) * inv_accum``."""
    fn = "ppg_aux_fwd_bwd"
    s.chk(aux_pi, torch.float32, "aux_pi")
    if aux_pi.dim() != 3:
        raise ValueError(f"{fn}: aux_pi must be (T, R, A), got {tuple(aux_pi.shape)}")
    T, R, A = aux_pi.shape
    n = _cols(s, cols, R, fn)
    M, H = h.shape
    _head_dims(fn, A, H)
    s.chk(h, torch.float32, "h", (_rows(fn, T, n), H))
    s.chk(aux_returns, torch.float32, "aux_returns", (T, R))
    if len(heads) != 6 or len(head_grads) != 6:
        raise ValueError(f"{fn}: six head tensors and six gradients")
    names = ("actor.weight", "actor.bias", "critic.weight", "critic.bias", "aux_critic.weight", "aux_critic.bias")
    shapes = ((A, H), (A,), (1, H), (1,), (1, H), (1,))
    for t, g, nm, shape in zip(heads, head_grads, names, shapes):
        s.chk(t, torch.float32, nm, shape)
        s.chk(g, torch.float32, nm + " gradient", shape)
    dev = h.device
    if scalars is None:
        scalars = torch.empty(3, dtype=torch.float32, device=dev)
    if dh is None:
        dh = torch.empty((M, H), dtype=torch.float32, device=dev)
    s.chk(scalars, torch.float32, "scalars", (3,))
    s.chk(dh, torch.float32, "dh", (M, H))
    s.launch_ws("mi355ppo_ppg_aux_fwd_bwd_f32", dev, "mi355ppo_ppg_aux_workspace_bytes", (M, A), _ptr(h), *[_ptr(t) for t in heads], _ptr(aux_pi),
                _ptr(aux_returns), _ptr(cols), T, n, R, A, H, float(beta_clone), float(inv_accum), _ptr(scalars), _ptr(dh),
                *[_ptr(g) for g in head_grads], int(bool(accumulate)))
    return scalars, dh


def clip_adam_split_(s, params, grads, exp_avg, exp_avg_sq, n_split: int, step_head: int, step_tail: int, lr: float, max_grad_norm: float,
                     grad_scale: float = 1.0, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-5, total_norm_out=None):
    """``clip_adam_`` with two Adam step counts (:466-468): one global-norm clip over all ``n`` gradients times ``grad_scale``, then
    ``step_head``'s bias corrections on ``[0, n_split)`` and ``step_tail``'s on ``[n_split, n)``.  Zeroes ``grads``.  -> the norm (1,)."""
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        s.chk(t, torch.float32, nm, (n,))
    if not (n > 0 and 0 <= int(n_split) <= n and int(step_head) >= 1 and int(step_tail) >= 1):
        raise ValueError(f"clip_adam_split_: n={n} n_split={n_split} step_head={step_head} step_tail={step_tail}: 0 <= n_split <= n, steps >= 1")
    if total_norm_out is None:
        total_norm_out = torch.empty(1, dtype=torch.float32, device=params.device)
    s.chk(total_norm_out, torch.float32, "total_norm_out", (1,))
    s.launch_ws("mi355ppo_clip_adam_split_f32", params.device, "mi355ppo_clip_adam_workspace_bytes", (n,), _ptr(params), _ptr(grads), _ptr(exp_avg),
                _ptr(exp_avg_sq), n, int(n_split), float(grad_scale), float(max_grad_norm), float(lr), float(beta1), float(beta2), float(eps),
                int(step_head), int(step_tail), _ptr(total_norm_out))
    return total_norm_out
