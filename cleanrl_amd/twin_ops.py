"""The operators of the LSTM scan, the TrXL memory attention, the IMPALA-CNN trunks, PQN and its LayerNorm NatureCNN pieces, each
defined once for the HIP entry point and its host twin, the way cleanrl_amd/replay_ops.py defines the replay-ring operators: the first
parameter ``s`` is a ``replay_ops.Side``, every argument is validated through ``s.chk`` (exact dtype, contiguous, exact shape; nothing
is coerced or copied, and every check precedes the C call), the buffers an operator allocates itself come from ``s.empty`` on its
inputs' device, and there is one call, through ``s.launch`` or ``s.launch_ws``.  ``cleanrl_amd.ops`` and ``cleanrl_amd.host_ops`` bind
``OPERATORS`` to their side with ``replay_ops.bind``.

Where a twin's argument list is not its entry point's minus the tail, the call says so in one ``if s.host:``: the TrXL entry points
take an error word, the IMPALA entry points a workspace of the call's own, and the one-frame ReLU forward is one twin for two entry
points.  The checks that need the indices' values (``inds out of range``) would cost the device a synchronisation and stay host-only.
What the kernels do not take (sizes, limits) is the library's to refuse, by its status; only the LayerNorm operators also refuse their
limits here, on the device side, as they always did.  This module imports neither ``ops`` nor ``host_ops``.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

from . import _lib
from .replay_ops import _ptr

OPERATORS = (
    "lstm_seq_forward", "lstm_seq_backward", "trxl_attn_forward", "trxl_attn_backward",
    "impala_forward", "impala_backward", "impala84_forward", "impala84_backward", "impala_maxpool_forward", "impala_maxpool_backward",
    "pqn_egreedy", "pqn_qlambda", "pqn_td_loss", "pqn_mlp_forward", "pqn_mlp_act", "pqn_mlp_td_fwd_bwd", "clip_radam_",
    "pqn_lstm_act", "pqn_lstm_td_fwd_bwd",
    "layernorm_relu_fwd", "layernorm_relu_bwd", "conv1q_pre_fwd", "conv1q1_pack", "conv1q1_pre_fwd", "conv1q1_fwd",
)


def _ptr_array(ts):
    """A host array of the tensors' data pointers (a network's parameters / gradients as the C ABI takes them)."""
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


# ------------------------------------------------------------------------------------------- LSTM (csrc/lstm_seq.hip)
def _lstm_dims(gx, done):
    if gx.dim() != 3 or gx.shape[2] % 4:
        raise ValueError(f"gx: expected (T, B, 4H), got {tuple(gx.shape)}")
    T, B, G = gx.shape
    if tuple(done.shape) != (T, B):
        raise ValueError(f"done: expected (T, B) = {(T, B)}, got {tuple(done.shape)}")
    return T, B, G // 4


def lstm_seq_forward(s, gx, w_hh, h0, c0, done, record: bool = False):
    """The done-masked LSTM scan of ppo_atari_lstm.py:140-158 (``get_states``) in one launch: ``gx`` (T,B,4H) = x W_ih^T + b_ih +
    b_hh, ``w_hh`` (4H,H), ``h0`` / ``c0`` (B,H), ``done`` (T,B); H = 128.  Returns ``(h (T,B,H), hT, cT, record | None)``; the
    record (7 T B H floats, layout in include/mi355ppo.h) feeds ``lstm_seq_backward``."""
    chk = s.chk
    T, B, H = _lstm_dims(gx, done)
    chk(gx, torch.float32, "gx", (T, B, 4 * H))
    chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    chk(h0, torch.float32, "h0", (B, H))
    chk(c0, torch.float32, "c0", (B, H))
    chk(done, torch.float32, "done", (T, B))
    dev = gx.device
    h, hT, cT = s.empty((T, B, H), torch.float32, dev), s.empty((B, H), torch.float32, dev), s.empty((B, H), torch.float32, dev)
    rec = s.empty(7 * T * B * H, torch.float32, dev) if record else None
    s.launch("mi355ppo_lstm_seq_fwd_f32", dev, _ptr(gx), _ptr(w_hh), _ptr(h0), _ptr(c0), _ptr(done), _ptr(h), _ptr(hT), _ptr(cT),
             _ptr(rec), T, B, H)
    return h, hT, cT, rec


def lstm_seq_backward(s, dh, dhT, dcT, record, w_hh, done, want_dh0: bool = True, want_dc0: bool = True):
    """Backward of ``lstm_seq_forward`` (BPTT with the state gradient masked by keep_t): ``dh`` (T,B,H) from the heads, ``dhT`` /
    ``dcT`` (B,H) or None (= zeros).  Returns ``(dgx (T,B,4H), dh0 | None, dc0 | None)``; dW_hh = dgx^T hk is the caller's GEMM."""
    T, B, H = dh.shape
    s.chk(dh, torch.float32, "dh", (T, B, H))
    if dhT is not None:
        s.chk(dhT, torch.float32, "dhT", (B, H))
    if dcT is not None:
        s.chk(dcT, torch.float32, "dcT", (B, H))
    s.chk(record, torch.float32, "record", (7 * T * B * H,))
    s.chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    s.chk(done, torch.float32, "done", (T, B))
    dgx = s.empty((T, B, 4 * H), torch.float32, dh.device)
    dh0 = s.empty((B, H), torch.float32, dh.device) if want_dh0 else None
    dc0 = s.empty((B, H), torch.float32, dh.device) if want_dc0 else None
    s.launch("mi355ppo_lstm_seq_bwd_f32", dh.device, _ptr(dh), _ptr(dhT), _ptr(dcT), _ptr(record), _ptr(w_hh), _ptr(done), _ptr(dgx),
             _ptr(dh0), _ptr(dc0), T, B, H)
    return dgx, dh0, dc0


# ------------------------------------------------------------------------------------------- TrXL (csrc/trxl_attn.hip)
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


def _trxl_checked(s, memory, ep, rows, pos, mask, pe, gamma, beta, q):
    E, T, layers, D, B, L, H = trxl_dims(memory, rows, q)
    s.chk(memory, torch.float32, "memory")
    s.chk(ep, torch.int64, "ep", (B,))
    s.chk(rows, torch.int64, "rows", (B, L))
    if getattr(mask, "dtype", None) is torch.bool:                               # a bool row is the kernel's byte (0 / 1): the same memory, nothing copied
        mask = mask.view(torch.uint8)
    s.chk(mask, torch.uint8, "mask", (B, L))
    if pe is not None:
        s.chk(pe, torch.float32, "pe")
        s.chk(pos, torch.int64, "pos", (B, L))
    s.chk(gamma, torch.float32, "gamma", (D,))
    s.chk(beta, torch.float32, "beta", (D,))
    s.chk(q, torch.float32, "q", (B, H, D // H))
    return E, T, layers, D, B, L, H, mask


def _trxl_launch(s, name: str, dev, err, sizes, *args) -> None:
    """An index outside the memory / pe table: the twin refuses the call by its status; the device entry point takes an error word
    between ``args`` and the four ``sizes`` (the kernel clamps the index and sets the word).  A caller-owned ``err`` is zeroed and left
    unread; with None one is allocated and read back (one sync) unless the stream is being captured into a graph."""
    if s.host:
        if err is not None:
            raise ValueError(f"{name}: the host twin has no error word; `err` is the device path's (cleanrl_amd.ops)")
        return s.launch(name, dev, *args, *sizes)
    own = err is None
    err = (s.empty(1, torch.int32, dev) if own else err).zero_()
    s.launch(name, dev, *args, _ptr(err), *sizes)
    if own and not torch.cuda.is_current_stream_capturing() and int(err.item()) != 0:
        raise IndexError(f"{name}: an episode, row or position index was outside the memory / pe table (clamped on the device)")


def trxl_attn_forward(s, memory, layer: int, ep, rows, pos, mask, pe, gamma, beta, q, err=None):
    """The episodic-memory attention of one TrXL layer (ppo_trxl.py: MultiHeadAttention.forward over norm_kv of the window
    rows): ``u`` (B,H,d) = sum_j softmax(s)_j LN(mem[ep, rows_j, layer] + pe[pos_j])_h and ``stats`` (B,H,2) (max, sum) for the
    backward.  ``q`` is q~ = W_k^T q (``q @ keys.weight``); ``pe`` may be None.  ``mask`` is uint8 or bool (any nonzero keeps a row).  ``err``
    (int32, 1 element, device side only): a caller-owned error word (zeroed here, left unread); with None an out-of-range index raises."""
    E, T, layers, D, B, L, H, mask = _trxl_checked(s, memory, ep, rows, pos, mask, pe, gamma, beta, q)
    u, stats = s.empty((B, H, D // H), torch.float32, q.device), s.empty((B, H, 2), torch.float32, q.device)
    _trxl_launch(s, "mi355ppo_trxl_attn_fwd_f32", q.device, err, (B, L, D, H), _ptr(memory), E, T, layers, int(layer), _ptr(ep), _ptr(rows),
                 _ptr(pos), _ptr(mask), _ptr(pe), 0 if pe is None else pe.shape[0], _ptr(gamma), _ptr(beta), _ptr(q), _ptr(u), _ptr(stats))
    return u, stats


def trxl_attn_backward(s, memory, layer: int, ep, rows, pos, mask, pe, gamma, beta, q, u, stats, du, err=None):
    """Backward of ``trxl_attn_forward`` -> (dq (B,H,d), dgamma (D), dbeta (D)); no gradient reaches the memory."""
    E, T, layers, D, B, L, H, mask = _trxl_checked(s, memory, ep, rows, pos, mask, pe, gamma, beta, q)
    s.chk(u, torch.float32, "u", (B, H, D // H))
    s.chk(stats, torch.float32, "stats", (B, H, 2))
    s.chk(du, torch.float32, "du", (B, H, D // H))
    dq, rows_ws = s.empty((B, H, D // H), torch.float32, q.device), s.empty((2, B, D), torch.float32, q.device)
    dgamma, dbeta = s.empty(D, torch.float32, q.device), s.empty(D, torch.float32, q.device)
    _trxl_launch(s, "mi355ppo_trxl_attn_bwd_f32", q.device, err, (B, L, D, H), _ptr(memory), E, T, layers, int(layer), _ptr(ep), _ptr(rows),
                 _ptr(pos), _ptr(mask), _ptr(pe), 0 if pe is None else pe.shape[0], _ptr(gamma), _ptr(beta), _ptr(q), _ptr(u), _ptr(stats),
                 _ptr(du), _ptr(dq), _ptr(rows_ws), _ptr(dgamma), _ptr(dbeta))
    return dq, dgamma, dbeta


# ------------------------------------------------------------------------------------------- IMPALA-CNN trunks (csrc/impala.hip)
IMPALA_CHANNELS = (16, 32, 32)

# One trunk family: the frames it reads (shape, dtype, what the error text calls them), its output rows, and its entry points' symbol stem
# and dtype suffix; from those, once: the 30 parameters' shapes and the symbols ``{stem}_fwd_{suffix}`` / ``{stem}_bwd_{suffix}`` /
# ``{stem}_saved_floats`` / ``{stem}_argmax_bytes`` / ``{stem}_workspace_bytes``.
ImpalaFamily = namedtuple("ImpalaFamily", "frame dtype frames out stem suffix shapes fwd bwd saved_floats argmax_bytes workspace_bytes")


def _impala_family(frame, dtype, frames, out, stem, suffix):
    shapes, cin = [], frame[2]
    for c in IMPALA_CHANNELS:
        for i in range(5):
            shapes += [(c, cin if i == 0 else c, 3, 3), (c,)]
        cin = c
    return ImpalaFamily(frame, dtype, frames, out, stem, suffix, tuple(shapes), f"{stem}_fwd_{suffix}", f"{stem}_bwd_{suffix}",
                        stem + "_saved_floats", stem + "_argmax_bytes", stem + "_workspace_bytes")


IMPALA64 = _impala_family((64, 64, 3), torch.float32, "frames", (8, 8, 32), "mi355ppo_impala", "f32")           # ppo_procgen / ppg_procgen
IMPALA84 = _impala_family((84, 84, 4), torch.uint8, "frame stacks", (11, 11, 32), "mi355ppo_impala84", "u8")     # the QDagger student
IMPALA_FRAME, IMPALA84_FRAME, IMPALA84_OUT = IMPALA64.frame, IMPALA84.frame, IMPALA84.out


def impala_family_param_shapes(f: ImpalaFamily):
    """The 30 trunk parameters' shapes in state_dict order (per sequence: conv, res_block0.conv0 / conv1, res_block1.conv0 / conv1;
    weight then bias)."""
    return list(f.shapes)


def impala_check(f: ImpalaFamily, x, params):
    """The shapes of one trunk call (and, for byte frames, their dtype): what the autograd seam refuses before anything is copied."""
    if x.dim() != 4 or tuple(x.shape[1:]) != f.frame or x.shape[0] < 1:
        raise ValueError(f"x: expected channels-last {f.frames} (B, {', '.join(map(str, f.frame))}), got {tuple(x.shape)}")
    if f.dtype is torch.uint8 and x.dtype != torch.uint8:
        raise TypeError(f"x: expected the ring's uint8 rows, got {x.dtype} (the trunk reads bytes; no f32 copy of the frames is made)")
    if len(params) != 30:
        raise ValueError(f"params: expected the trunk's 30 weights and biases, got {len(params)}")
    for i, (p, shp) in enumerate(zip(params, f.shapes)):
        if tuple(p.shape) != shp:
            raise ValueError(f"params[{i}]: expected shape {shp}, got {tuple(p.shape)} (channels must be {list(IMPALA_CHANNELS)})")


def _impala_launch(s, f, backward: bool, pooled: bool, x, *args) -> None:
    """The device entry point also takes a workspace, this call's own allocation (not the stream's shared one); the twin takes none.
    ``pooled`` picks the device side's ``{stem}_fwd_pooled_{suffix}`` / ``_bwd_pooled_`` (the 64x64x3 family's only; same arguments, same
    bits); the host side ignores it: the plain pair's twins are theirs too."""
    name, B = f.bwd if backward else f.fwd, x.shape[0]
    if s.host:
        return s.launch(name, x.device, *args, B, *f.frame, *IMPALA_CHANNELS)
    if pooled:
        name = name.replace("_fwd_", "_fwd_pooled_").replace("_bwd_", "_bwd_pooled_")
    ws = s.empty(int(getattr(_lib.load(), f.workspace_bytes)(B, int(backward))), torch.uint8, x.device)
    s.launch(name, x.device, *args, B, *f.frame, *IMPALA_CHANNELS, _ptr(ws), ws.numel())


def _impala_args(s, f, x, params):
    impala_check(f, x, params)
    s.chk(x, f.dtype, "x")
    for i, p in enumerate(params):
        s.chk(p, torch.float32, f"params[{i}]")
    lib = _lib.load()
    return int(getattr(lib, f.saved_floats)(x.shape[0])), int(getattr(lib, f.argmax_bytes)(x.shape[0]))


def impala_family_forward(s, f: ImpalaFamily, x, params, pooled: bool = False):
    B = x.shape[0]
    n_saved, n_arg = _impala_args(s, f, x, params)
    dev = x.device
    y, saved, arg = s.empty((B, *f.out), torch.float32, dev), s.empty(n_saved, torch.float32, dev), s.empty(n_arg, torch.uint8, dev)
    _impala_launch(s, f, False, pooled, x, _ptr(x), _ptr_array(params), _ptr(y), _ptr(saved), _ptr(arg))
    return y, saved, arg


def impala_family_backward(s, f: ImpalaFamily, x, params, saved, arg, dy, pooled: bool = False):
    B = x.shape[0]
    n_saved, n_arg = _impala_args(s, f, x, params)
    s.chk(dy, torch.float32, "dy", (B, *f.out))
    s.chk(saved, torch.float32, "saved", (n_saved,))
    s.chk(arg, torch.uint8, "argmax", (n_arg,))
    flat = s.empty(sum(p.numel() for p in params), torch.float32, x.device)
    grads, o = [], 0
    for p in params:
        grads.append(flat[o:o + p.numel()].view(p.shape))
        o += p.numel()
    _impala_launch(s, f, True, pooled, x, _ptr(x), _ptr_array(params), _ptr(saved), _ptr(arg), _ptr(dy), _ptr_array(grads))
    return grads


def impala_forward(s, x, params, pooled: bool = False):
    """The IMPALA-CNN trunk (ppo_procgen.py:86-124 / ppg_procgen.py:123-165, three ConvSequences; csrc/impala.hip, the twin the same
    arithmetic: csrc/impala_rows.h): x (B,64,64,3) f32 channels-last frames, params the 30 conv weights / biases in state_dict order.
    Returns ``(y (B,8,8,32) channels-last, saved, argmax)``; the last two feed ``impala_backward``.  ``pooled``: on the device, each
    sequence's conv + max pool as one kernel (the pre-pool plane stays in LDS); the same bits."""
    return impala_family_forward(s, IMPALA64, x, params, pooled)


def impala_backward(s, x, params, saved, arg, dy, pooled: bool = False):
    """Backward of ``impala_forward``: dy (B,8,8,32) channels-last -> the 30 parameter gradients (one flat buffer's views, written
    by deterministic fixed-order folds); no input gradient.  ``pooled``: on the device, the pools' backward inside the staging of the
    conv gradient kernels; the same bits, from either forward's ``saved`` / ``argmax``."""
    return impala_family_backward(s, IMPALA64, x, params, saved, arg, dy, pooled)


def impala84_forward(s, x, params):
    """The IMPALA-CNN trunk of the QDagger student (qdagger_dqn_atari_impalacnn.py:164-181): x (B,84,84,4) u8 channels-last rows
    (what ``replay_gather_u8`` writes), read as byte / 255; params the 30 conv weights / biases in state_dict order.  Returns
    ``(y (B,11,11,32) channels-last, saved, argmax)``; the last two feed ``impala84_backward``."""
    return impala_family_forward(s, IMPALA84, x, params)


def impala84_backward(s, x, params, saved, arg, dy):
    """Backward of ``impala84_forward``: dy (B,11,11,32) channels-last -> the 30 parameter gradients (one flat buffer's views,
    written by deterministic fixed-order folds); no gradient for the frames."""
    return impala_family_backward(s, IMPALA84, x, params, saved, arg, dy)


def impala_maxpool_forward(s, x):
    """The trunks' max pool (3, stride 2, pad 1) alone on channels-last x (B,H,W,C) -> (y, argmax bytes (B,(H+1)/2,(W+1)/2,C))."""
    s.chk(x, torch.float32, "x")
    B, H, W, C = x.shape
    out = (B, (H + 1) // 2, (W + 1) // 2, C)
    y, arg = s.empty(out, torch.float32, x.device), s.empty(out, torch.uint8, x.device)
    s.launch("mi355ppo_impala_maxpool_fwd_f32", x.device, _ptr(x), _ptr(y), _ptr(arg), B, H, W, C)
    return y, arg


def impala_maxpool_backward(s, dy, arg, size=None):
    """Backward of ``impala_maxpool_forward``: dx (B,H,H,C), H = ``size`` (default 2 Ho; the 21 -> 11 pool needs it said)."""
    s.chk(dy, torch.float32, "dy")
    B, Ho, Wo, C = dy.shape
    s.chk(arg, torch.uint8, "argmax", tuple(dy.shape))
    H = 2 * Ho if size is None else int(size)
    dx = s.empty((B, H, H, C), torch.float32, dy.device)
    s.launch("mi355ppo_impala_maxpool_bwd_f32", dy.device, _ptr(dy), _ptr(arg), _ptr(dx), B, H, H, C)
    return dx


# ------------------------------------------------------------------------------------------- PQN (csrc/pqn.hip)
PQN_MAX_OBS, PQN_MAX_ACTIONS, PQN_HIDDEN = 64, 18, (120, 84)


def pqn_param_count(obs_dim: int, n_actions: int) -> int:
    """Parameters of pqn.py's QNetwork (Linear -> LayerNorm(120) -> ReLU -> Linear -> LayerNorm(84) -> ReLU -> Linear)."""
    return 120 * obs_dim + 360 + 84 * 120 + 252 + 85 * n_actions


def _egreedy_rows(s, N, random_actions, u, actions_out, values_out, action_i64_out):
    chk = s.chk
    chk(random_actions, torch.int64, "random_actions", (N,))
    chk(u, torch.float32, "u", (N,))
    chk(actions_out, torch.float32, "actions_out", (N,))
    chk(values_out, torch.float32, "values_out", (N,))
    if action_i64_out is not None:
        chk(action_i64_out, torch.int64, "action_i64_out", (N,))


def pqn_egreedy(s, q, random_actions, u, epsilon: float, actions_out, values_out, action_i64_out=None):
    """pqn.py's action logic on a computed ``q`` (N, A): argmax (torch's tie / NaN rule), ``values[step]`` = q at the greedy index,
    ``rand < epsilon`` and ``where``.  ``actions_out`` / ``values_out`` are the step's storage rows (N,) f32, written in place."""
    N, A = q.shape
    s.chk(q, torch.float32, "q")
    _egreedy_rows(s, N, random_actions, u, actions_out, values_out, action_i64_out)
    s.launch("mi355ppo_pqn_egreedy_f32", q.device, _ptr(q), _ptr(random_actions), _ptr(u), float(epsilon), _ptr(actions_out),
             _ptr(values_out), _ptr(action_i64_out), N, A)
    return actions_out, values_out


def pqn_qlambda(s, rewards, dones, values, next_done, next_q, gamma: float, q_lambda: float, returns=None):
    """The ``# Compute Q(lambda) targets`` block (bootstrap ``torch.max(next_q, dim=-1)`` included) -> returns (T, N)."""
    T, N = rewards.shape
    A = next_q.shape[-1]
    for t, nm in ((rewards, "rewards"), (dones, "dones"), (values, "values")):
        s.chk(t, torch.float32, nm, (T, N))
    next_done = s.chk(next_done.reshape(-1), torch.float32, "next_done", (N,))
    s.chk(next_q, torch.float32, "next_q", (N, A))
    returns = s.empty((T, N), torch.float32, rewards.device) if returns is None else s.chk(returns, torch.float32, "returns", (T, N))
    s.launch("mi355ppo_pqn_qlambda_f32", rewards.device, _ptr(rewards), _ptr(dones), _ptr(values), _ptr(next_done), _ptr(next_q),
             _ptr(returns), T, N, A, float(gamma), float(q_lambda))
    return returns


def _batch_rows(s, b_actions, b_returns):
    """The flat batch's f32 action and return rows (any shape of B elements) -> (B, both as (B,))."""
    B = b_actions.numel()
    return B, s.chk(b_actions.reshape(-1), torch.float32, "b_actions", (B,)), s.chk(b_returns.reshape(-1), torch.float32, "b_returns", (B,))


def pqn_td_loss(s, q, mb_inds, b_actions, b_returns, dq=None, scalars=None):
    """``q.gather(1, b_actions[mb_inds].long())`` + ``F.mse_loss(b_returns[mb_inds], old_val)`` and its gradient -> (dq (M, A),
    scalars (2,) = {td_loss, mean(old_val)})."""
    M, A = q.shape
    s.chk(q, torch.float32, "q")
    s.chk(mb_inds, torch.int64, "mb_inds", (M,))
    B, b_actions, b_returns = _batch_rows(s, b_actions, b_returns)
    dq = s.empty((M, A), torch.float32, q.device) if dq is None else s.chk(dq, torch.float32, "dq", (M, A))
    scalars = s.empty((2,), torch.float32, q.device) if scalars is None else s.chk(scalars, torch.float32, "scalars", (2,))
    s.launch("mi355ppo_pqn_td_loss_fwd_bwd_f32", q.device, _ptr(q), _ptr(mb_inds), _ptr(b_actions), _ptr(b_returns), _ptr(dq), _ptr(scalars),
             M, A, B)
    return dq, scalars


def _pqn_net(s, obs, params, n_actions):
    N, O = obs.shape
    s.chk(obs, torch.float32, "obs")
    s.chk(params, torch.float32, "params", (pqn_param_count(O, n_actions),))
    return N, O


def pqn_mlp_forward(s, obs, params, n_actions: int, q_out=None):
    """``QNetwork.forward`` of pqn.py on the flat parameters (``agent.parameters()`` order) -> q (N, A)."""
    N, O = _pqn_net(s, obs, params, n_actions)
    q_out = s.empty((N, n_actions), torch.float32, obs.device) if q_out is None else s.chk(q_out, torch.float32, "q_out", (N, n_actions))
    s.launch("mi355ppo_pqn_mlp_fwd_f32", obs.device, _ptr(obs), _ptr(params), _ptr(q_out), N, O, int(n_actions))
    return q_out


def pqn_mlp_act(s, obs, params, n_actions: int, random_actions, u, epsilon: float, actions_out, values_out, action_i64_out=None,
                obs_row_out=None, done_in=None, done_row_out=None):
    """One rollout step of pqn.py in one launch: forward, e-greedy, the ``actions`` / ``values`` (and optionally ``obs`` /
    ``dones``) storage rows."""
    N, O = _pqn_net(s, obs, params, n_actions)
    _egreedy_rows(s, N, random_actions, u, actions_out, values_out, action_i64_out)
    if obs_row_out is not None:
        s.chk(obs_row_out, torch.float32, "obs_row_out", (N, O))
    if done_row_out is not None:
        s.chk(done_in, torch.float32, "done_in", (N,))
        s.chk(done_row_out, torch.float32, "done_row_out", (N,))
    s.launch("mi355ppo_pqn_mlp_act_f32", obs.device, _ptr(obs), _ptr(params), _ptr(random_actions), _ptr(u), float(epsilon),
             _ptr(actions_out), _ptr(values_out), _ptr(action_i64_out), _ptr(obs_row_out), _ptr(done_in), _ptr(done_row_out), N, O,
             int(n_actions))
    return actions_out, values_out


def pqn_mlp_td_fwd_bwd(s, b_obs, mb_inds, params, b_actions, b_returns, grads, n_actions: int, scalars=None):
    """One minibatch of pqn.py: gather, forward, TD loss, backward.  OVERWRITES ``grads`` (flat) with d loss / d params and returns
    scalars (2,) = {td_loss, mean(old_val)}."""
    B, O = _pqn_net(s, b_obs, params, n_actions)
    (M,) = mb_inds.shape
    s.chk(mb_inds, torch.int64, "mb_inds", (M,))
    b_actions = s.chk(b_actions.reshape(-1), torch.float32, "b_actions", (B,))
    b_returns = s.chk(b_returns.reshape(-1), torch.float32, "b_returns", (B,))
    s.chk(grads, torch.float32, "grads", params.shape)
    scalars = s.empty((2,), torch.float32, b_obs.device) if scalars is None else s.chk(scalars, torch.float32, "scalars", (2,))
    s.launch_ws("mi355ppo_pqn_mlp_td_fwd_bwd_f32", b_obs.device, "mi355ppo_pqn_mlp_td_workspace_bytes", (M, O, int(n_actions)), _ptr(b_obs), B,
                _ptr(mb_inds), _ptr(params), _ptr(b_actions), _ptr(b_returns), _ptr(grads), _ptr(scalars), M, O, int(n_actions))
    return scalars


def clip_radam_(s, params, grads, exp_avg, exp_avg_sq, step: int, lr: float, max_grad_norm: float, beta1: float = 0.9, beta2: float = 0.999,
                eps: float = 1e-8, total_norm_out=None):
    """In-place ``clip_grad_norm_`` + ``optim.RAdam`` step ``step`` (1-based) on flat f32 buffers; zeroes ``grads``.  Returns the
    pre-clip norm (1,).  (``ops.clip_radam_sched_``, the capturable step whose schedule is read from device memory, has this twin too.)"""
    n = params.numel()
    for t, nm in ((params, "params"), (grads, "grads"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        s.chk(t, torch.float32, nm, (n,))
    total_norm_out = s.empty((1,), torch.float32, params.device) if total_norm_out is None else s.chk(total_norm_out, torch.float32, "total_norm_out", (1,))
    s.launch_ws("mi355ppo_clip_radam_f32", params.device, "mi355ppo_clip_radam_workspace_bytes", (n,), _ptr(params), _ptr(grads), _ptr(exp_avg),
                _ptr(exp_avg_sq), n, float(max_grad_norm), float(lr), float(beta1), float(beta2), float(eps), int(step), _ptr(total_norm_out))
    return total_norm_out


# ------------------------------------------------------------------------------------------- recurrent PQN (csrc/pqn_lstm.hip)
def pqn_lstm_act(s, gx, w_hh, h_in, c_in, done_in, wq, bq, random_actions=None, u=None, epsilon: float = 0.0, h_out=None, c_out=None,
                 q_out=None, actions_out=None, values_out=None, action_i64_out=None, done_row_out=None):
    """The recurrent tail of one rollout step of pqn_atari_envpool_lstm.py in one launch: the done reset, ONE LSTM cell on ``gx``
    (N, 4H) = x W_ih^T + b_ih + b_hh (bit-equal to ``lstm_seq_forward`` at T = 1), ``q_func`` and e-greedy into the step's storage
    rows.  ``h_out`` / ``c_out`` (N, H) may be ``h_in`` / ``c_in``.  Every output is optional: with only ``q_out`` it is the
    bootstrap's ``q_network(next_obs, ...)``.  Returns ``q_out``."""
    chk = s.chk
    N, G = gx.shape
    H = G // 4
    A = wq.shape[0]
    chk(gx, torch.float32, "gx", (N, 4 * H))
    chk(w_hh, torch.float32, "w_hh", (4 * H, H))
    chk(h_in, torch.float32, "h_in", (N, H))
    chk(c_in, torch.float32, "c_in", (N, H))
    chk(done_in, torch.float32, "done_in", (N,))
    chk(wq, torch.float32, "wq", (A, H))
    chk(bq, torch.float32, "bq", (A,))
    for t, dt, nm, shape in ((random_actions, torch.int64, "random_actions", (N,)), (u, torch.float32, "u", (N,)),
                             (h_out, torch.float32, "h_out", (N, H)), (c_out, torch.float32, "c_out", (N, H)),
                             (q_out, torch.float32, "q_out", (N, A)), (actions_out, torch.float32, "actions_out", (N,)),
                             (values_out, torch.float32, "values_out", (N,)), (action_i64_out, torch.int64, "action_i64_out", (N,)),
                             (done_row_out, torch.float32, "done_row_out", (N,))):
        if t is not None:
            chk(t, dt, nm, shape)
    s.launch("mi355ppo_pqn_lstm_act_f32", gx.device, _ptr(gx), _ptr(w_hh), _ptr(h_in), _ptr(c_in), _ptr(done_in), _ptr(wq), _ptr(bq),
             _ptr(random_actions), _ptr(u), float(epsilon), _ptr(h_out), _ptr(c_out), _ptr(q_out), _ptr(actions_out), _ptr(values_out),
             _ptr(action_i64_out), _ptr(done_row_out), N, H, A)
    return q_out


def pqn_lstm_td_fwd_bwd(s, h, mb_inds, b_actions, b_returns, wq, bq, dwq, dbq, dh=None, scalars=None):
    """``q_func(h).gather(1, b_actions[mb_inds].long())`` + ``F.mse_loss(b_returns[mb_inds], old_val)`` of one minibatch, forward and
    backward: ``h`` (M, H) are the scan's rows in minibatch order.  OVERWRITES ``dwq`` (A, H) / ``dbq`` (A) (views of the flat
    gradient) and returns ``(dh (M, H), scalars (2,) = {td_loss, mean(old_val)})``."""
    M, H = h.shape
    A = wq.shape[0]
    s.chk(h, torch.float32, "h")
    s.chk(mb_inds, torch.int64, "mb_inds", (M,))
    B, b_actions, b_returns = _batch_rows(s, b_actions, b_returns)
    s.chk(wq, torch.float32, "wq", (A, H))
    s.chk(bq, torch.float32, "bq", (A,))
    s.chk(dwq, torch.float32, "dwq", (A, H))
    s.chk(dbq, torch.float32, "dbq", (A,))
    dh = s.empty((M, H), torch.float32, h.device) if dh is None else s.chk(dh, torch.float32, "dh", (M, H))
    scalars = s.empty((2,), torch.float32, h.device) if scalars is None else s.chk(scalars, torch.float32, "scalars", (2,))
    s.launch_ws("mi355ppo_pqn_lstm_td_fwd_bwd_f32", h.device, "mi355ppo_pqn_lstm_td_workspace_bytes", (M, A), _ptr(h), _ptr(mb_inds),
                _ptr(b_actions), _ptr(b_returns), _ptr(wq), _ptr(bq), _ptr(dh), _ptr(dwq), _ptr(dbq), _ptr(scalars), M, H, A, B)
    return dh, scalars


# ---- the LayerNorm NatureCNN of pqn_atari_envpool.py (csrc/layernorm.hip; the pre-activation forwards: cleanrl_amd/ln_cnn.py)
AMAX_WORDS = 256      # MI355PPO_AMAX_WORDS: uint32 words of an amax record (csrc/f16split.h)
LN_MAX_D = 16384


def _ln_dims(s, z, C: int, HW: int):
    """(rows, D).  The kernels' limits are refused here on the device side and by the twin itself (its status) on the host side."""
    rows, D = z.shape[0], int(C) * int(HW)
    if z.numel() != rows * D or not s.host and (rows <= 0 or C <= 0 or HW <= 0 or C % 4 or D > LN_MAX_D):
        raise ValueError(f"layernorm: rows of C * HW = {C} * {HW} floats (C a multiple of 4, at most {LN_MAX_D}), got {tuple(z.shape)}")
    return rows, D


def layernorm_relu_fwd(s, z, gamma, beta, C: int, HW: int, eps: float = 1e-5, out=None, mean=None, rstd=None, bits=None, amax=None):
    """``relu(layer_norm(z))`` over rows ``z`` (rows, ..) of C * HW floats in (H, W, C) order, ``gamma`` / ``beta`` in torch's (C, H, W)
    order -> ``(a, mean (rows,), rstd (rows,))``.  ``bits`` (int32, ``z.numel() // 32`` words) receives ``a > 0`` in the layout of the
    ``*_bits`` forwards, ``amax`` (one zeroed row of ``cnn.new_amax``) a's amax record (the twin's value lands in its word 0)."""
    s.chk(z, torch.float32, "z")
    rows, D = _ln_dims(s, z, C, HW)
    s.chk(gamma, torch.float32, "gamma")
    s.chk(beta, torch.float32, "beta")
    if gamma.numel() != D or beta.numel() != D:
        raise ValueError(f"layernorm: gamma / beta must hold {D} floats, got {gamma.numel()} / {beta.numel()}")
    out = s.empty(z.shape, torch.float32, z.device) if out is None else s.chk(out, torch.float32, "out", z.shape)
    mean = s.empty((rows,), torch.float32, z.device) if mean is None else s.chk(mean, torch.float32, "mean", (rows,))
    rstd = s.empty((rows,), torch.float32, z.device) if rstd is None else s.chk(rstd, torch.float32, "rstd", (rows,))
    if bits is not None:
        if D % 32 and not s.host:                               # (the twin refuses this itself, by its status)
            raise ValueError(f"layernorm: mask bits need C * HW % 32 == 0, got {D}")
        s.chk(bits, torch.int32, "bits", None if D % 32 else (rows * D // 32,))
    if amax is not None:
        s.chk(amax, torch.int32, "amax", (AMAX_WORDS,))
    s.launch("mi355ppo_layernorm_relu_fwd_f32", z.device, _ptr(z), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(mean), _ptr(rstd), _ptr(bits),
             _ptr(amax), rows, int(C), int(HW), float(eps))
    return out, mean, rstd


def layernorm_relu_bwd(s, dy, z, mean, rstd, gamma, C: int, HW: int, act=None, dz=None, dgamma=None, dbeta=None, amax=None):
    """Backward of ``layernorm_relu_fwd``: ``dy`` is the gradient at ``a`` already under the mask ``a > 0`` -- or, with ``act`` given, is
    masked here by ``act > 0`` -> ``(dz, dgamma, dbeta)`` (the parameter gradients in torch's (C, H, W) order, overwritten; ``amax``
    receives dz's amax record).  The same input gives the same bits on every call."""
    s.chk(z, torch.float32, "z")
    rows, D = _ln_dims(s, z, C, HW)
    s.chk(dy, torch.float32, "dy", z.shape)
    if act is not None:
        s.chk(act, torch.float32, "act", z.shape)
    s.chk(mean, torch.float32, "mean", (rows,))
    s.chk(rstd, torch.float32, "rstd", (rows,))
    s.chk(gamma, torch.float32, "gamma")
    if gamma.numel() != D:
        raise ValueError(f"layernorm: gamma must hold {D} floats, got {gamma.numel()}")
    dz = s.empty(z.shape, torch.float32, z.device) if dz is None else s.chk(dz, torch.float32, "dz", z.shape)
    dgamma = s.empty(gamma.shape, torch.float32, gamma.device) if dgamma is None else s.chk(dgamma, torch.float32, "dgamma", gamma.shape)
    dbeta = s.empty(gamma.shape, torch.float32, gamma.device) if dbeta is None else s.chk(dbeta, torch.float32, "dbeta", gamma.shape)
    if amax is not None:
        s.chk(amax, torch.int32, "amax", (AMAX_WORDS,))
    s.launch_ws("mi355ppo_layernorm_relu_bwd_f32", z.device, "mi355ppo_layernorm_bwd_workspace_bytes", (rows, int(C), int(HW)), _ptr(dy),
                _ptr(act), _ptr(z), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(dz), _ptr(dgamma), _ptr(dbeta), _ptr(amax), rows, int(C), int(HW))
    return dz, dgamma, dbeta


def _gathered(s, rows: int, inds, what: str) -> int:
    """The images a forward writes: all ``rows`` source rows, or those ``inds`` (int64) names.  An index outside the source is refused
    where reading it costs nothing, on the host side; the device kernels take the caller's word."""
    if inds is None:
        return rows
    s.chk(inds, torch.int64, "inds")
    if s.host and inds.numel() and (int(inds.min()) < 0 or int(inds.max()) >= rows):
        raise ValueError(f"{what}: inds out of range")
    return inds.numel()


def conv1q_pre_fwd(s, obs_u8, pack, bias, inds=None, out=None):
    """``conv1(obs_u8[inds] / 255) + bias`` WITHOUT the ReLU on kernel Q -- the input of the network's first LayerNorm; ``pack`` = kernel Q's
    pack of the weight (``cnn.repack_weights(W, 1, cnn.MODE_FWD_Q)``).  ``relu`` of the result is the ReLU forward's, bit for bit."""
    s.chk(obs_u8, torch.uint8, "src")
    if tuple(obs_u8.shape[1:]) != (84, 84, 4):
        raise ValueError(f"conv1q_pre_fwd: source rows must be (84, 84, 4) uint8, got {tuple(obs_u8.shape)}")
    images = _gathered(s, obs_u8.shape[0], inds, "conv1q_pre_fwd")
    s.chk(pack, torch.float32, "Bt", (_lib.load().mi355ppo_cnn_conv1q_pack_bytes() // 4,))
    s.chk(bias, torch.float32, "bias", (32,))
    out = s.empty((images, 20, 20, 32), torch.float32, obs_u8.device) if out is None else s.chk(out, torch.float32, "out", (images, 20, 20, 32))
    s.launch("mi355ppo_cnn_conv1q_pre_fwd", obs_u8.device, _ptr(obs_u8), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), images)
    return out


def frames_u8(s, obs_u8, what):
    """(rows, 84, 84) uint8 frames: ``(N, 1, 84, 84)`` and ``(N, 84, 84, 1)`` are the same bytes -> the (rows, 84, 84) view."""
    s.chk(obs_u8, torch.uint8, "src")
    if tuple(obs_u8.shape[1:]) not in ((84, 84), (1, 84, 84), (84, 84, 1)):
        raise ValueError(f"{what}: source rows must be (84, 84) uint8 frames, got {tuple(obs_u8.shape)}")
    return obs_u8.view(-1, 84, 84)


def conv1q1_pack(s, W, out=None):
    """Kernel Q1's pack of a ``Conv2d(1, 32, 8, stride=4)`` weight (32, 1, 8, 8), as f32 storage (kernel Q's digits in the one-channel layout)."""
    s.chk(W, torch.float32, "W", (32, 1, 8, 8))
    out = s.empty((_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,), torch.float32, W.device) if out is None else s.chk(out, torch.float32, "pack", (_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,))
    s.launch("mi355ppo_cnn_conv1q1_pack", W.device, _ptr(W), _ptr(out))
    return out


def _conv1q1_args(s, obs_u8, pack, bias, inds, out, what):
    frames = frames_u8(s, obs_u8, what)
    images = _gathered(s, frames.shape[0], inds, what)
    s.chk(pack, torch.float32, "pack", (_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,))
    s.chk(bias, torch.float32, "bias", (32,))
    out = s.empty((images, 20, 20, 32), torch.float32, frames.device) if out is None else s.chk(out, torch.float32, "out", (images, 20, 20, 32))
    return frames, images, out


def conv1q1_pre_fwd(s, obs_u8, pack, bias, inds=None, out=None):
    """``conv1(obs_u8[inds] / 255) + bias`` WITHOUT the ReLU for ONE-channel frames (rows, 84, 84) uint8 on kernel Q1 -- the input of the first
    LayerNorm of pqn_atari_envpool_lstm.py's network; ``pack = conv1q1_pack(W)``.  (M, 20, 20, 32) f32, kernel Q's arithmetic: exact."""
    frames, images, out = _conv1q1_args(s, obs_u8, pack, bias, inds, out, "conv1q1_pre_fwd")
    s.launch("mi355ppo_cnn_conv1q1_pre_fwd", frames.device, _ptr(frames), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), images)
    return out


def conv1q1_fwd(s, obs_u8, pack, bias, inds=None, out=None, bits=None, amax=None):
    """``relu(conv1(obs_u8[inds] / 255) + bias)`` for ONE-channel frames (rows, 84, 84) uint8 on kernel Q1 -- conv1 of ppo_atari_lstm.py's
    network; ``pack = conv1q1_pack(W)``.  With ``amax`` (an amax record) folds ``max(out)`` into it (the twin's value lands in its word 0);
    with ``bits`` (int32, ``out.numel() // 32`` words: word w, bit b <-> flat element 32 w + b) writes ``out > 0`` as bits.  The twin is
    one entry point and takes either, both or neither; on the device the call without a record is ``*_fwd_bits`` and needs ``bits``."""
    frames, images, out = _conv1q1_args(s, obs_u8, pack, bias, inds, out, "conv1q1_fwd")
    if bits is not None:
        s.chk(bits, torch.int32, "bits", (images * 400,))
    if amax is not None:
        s.chk(amax, torch.int32, "amax", (AMAX_WORDS,))
    args = (_ptr(frames), _ptr(inds), _ptr(pack), _ptr(bias), _ptr(out), _ptr(bits))
    if s.host:                                                  # one twin for the two entry points: the record before the count
        s.launch("mi355ppo_cnn_conv1q1_fwd", frames.device, *args, _ptr(amax), images)
    elif amax is not None:
        s.launch("mi355ppo_cnn_conv1q1_fwd_amax", frames.device, *args, images, _ptr(amax))
    elif bits is not None:
        s.launch("mi355ppo_cnn_conv1q1_fwd_bits", frames.device, *args, images)
    else:
        raise ValueError("conv1q1_fwd_bits: the mask words are required")
    return out
