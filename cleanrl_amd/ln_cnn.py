"""The LayerNorm NatureCNN of ``pqn_atari_envpool.py`` on the libmi355ppo kernels (``agents.AtariQNetwork.network[0:13]``: Conv ->
LayerNorm -> ReLU three times, Flatten, Linear(3136, 512) -> LayerNorm(512) -> ReLU) for uint8 channels-last rollout rows.

Every forward kernel of ``cnn.py`` fuses bias + ReLU into its epilogue; LayerNorm has to sit between the two.  So each layer is a
pre-activation forward (kernel Q's PRE instance, kernel Z's Z_BIAS epilogue: ``z = conv(src) + bias``) followed by the LayerNorm + ReLU
kernel (csrc/layernorm.hip), which also writes the ReLU mask bits and the amax record the next layer's f16 split needs.  Backward: with
``a = relu(LN(z))`` the data-gradient kernels' "gradient under the mask ``a > 0``" is the gradient at the LayerNorm's output, so the
chain is LN backward -> ``cnn.conv_wgrad`` / ``cnn.fc_wgrad`` -> ``cnn.conv_dgrad_packed`` / ``cnn.fc_dgrad_mask_packed``, the existing
kernels exactly as ``cnn.NatureTrunkFn.backward`` / ``cnn.LinearReLUHwcFn.backward`` use them.  The minibatch gather ``b_obs[mb_inds]``
and ``x / 255.0`` ride in kernel Q's loader.  The head ``Linear(512, A)`` stays torch.

The frame count comes from ``network[0].weight.shape[1]``: 4 (pqn_atari_envpool.py, rows (84, 84, 4)) or 1 (pqn_atari_envpool_lstm.py, rows
(84, 84) -- ``(N, 1, 84, 84)`` and ``(N, 84, 84, 1)`` are the same bytes).  With one channel conv1's forward, pack and weight gradient are
kernels Q1 / P1 (csrc/conv1q1.hip, csrc/conv1p1.hip); everything from the first LayerNorm on is the same code.

f16x2 split only: with ``MI355PPO_SPLIT=bf16x3``, ``MI355PPO_CONV=f`` or tensors beyond ``cnn.BUF_LIMIT`` the node raises
``NotImplementedError`` -- there is no fallback.
"""
from __future__ import annotations

import torch

from . import _lib, cnn
from .cnn import (BUF_LIMIT, MODE_DGRAD_S1, MODE_DGRAD_S2, MODE_FWD, MODE_FWD_Q, REC_A1, REC_A2, REC_A3, REC_DH, REC_DZ1, REC_DZ2, REC_DZ3,
                  _rec, _row_major)
from .ops import _chk, _launch, _ptr, _workspace, conv1p1_wgrad, conv1q1_pre_fwd, conv1q_pre_fwd, layernorm_relu_bwd, layernorm_relu_fwd

LN_EPS = 1e-5                 # nn.LayerNorm's default
# (C, HW) of the four LayerNorms: conv1 (20 x 20 x 32), conv2 (9 x 9 x 64), conv3 (7 x 7 x 64), Linear (512)
LN_DIMS = ((32, 400), (64, 81), (64, 49), (512, 1))


def conv_pre_packed(src: torch.Tensor, pack: torch.Tensor, bias: torch.Tensor, layer: int, src_rec: torch.Tensor,
                    out: torch.Tensor | None = None) -> torch.Tensor:
    """``conv(src) + bias`` of layer 2 / 3 WITHOUT the ReLU: kernel Z on the f16 split, whatever kernel the ReLU forward of this size
    runs on; ``pack = cnn.conv_zpack_f16x2(W, layer, MODE_FWD)``, ``src_rec`` = src's amax record.  ``relu`` of the result is
    ``cnn.conv_fwd_packed(..., amax=)``'s, bit for bit."""
    lib = _lib.load()
    cin, cout, k, _, hin, hout = cnn.LAYERS[layer]
    images = src.shape[0]
    _chk(src, torch.float32, "src", (images, hin, hin, cin))
    _chk(pack, torch.uint8, "pack", (lib.mi355ppo_fc_pack_f16x2_bytes(cout, cin * k * k),))
    _chk(bias, torch.float32, "bias", (cout,))
    if out is None:
        out = torch.empty((images, hout, hout, cout), dtype=torch.float32, device=src.device)
    _chk(out, torch.float32, "out", (images, hout, hout, cout))
    _launch("mi355ppo_cnn_conv_pre_packed_f16x2_f32", src.device, _ptr(src), _ptr(pack), _ptr(bias), _ptr(out), images, layer,
            _rec(src_rec, "src_amax"))
    return out


def fc_pre_packed(a: torch.Tensor, pack: torch.Tensor, bias: torch.Tensor, N: int, a_rec: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """``a @ B.T + bias`` WITHOUT the ReLU: kernel Z on the f16 split, K split over the grid below 8,192 rows exactly as
    ``cnn.fc_fwd_relu_packed(..., amax=)`` splits it; ``pack = cnn.fc_pack_f16x2(B)``, ``a_rec`` = a's amax record."""
    lib = _lib.load()
    M, K = a.shape
    lda = _row_major(a, "a")
    _chk(bias, torch.float32, "bias", (N,))
    _chk(pack, torch.uint8, "pack", (lib.mi355ppo_fc_pack_f16x2_bytes(N, K),))
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    _chk(out, torch.float32, "out", (M, N))
    nws = lib.mi355ppo_fc_fwd_workspace_bytes(M, N, K)
    ws = _workspace(a.device, nws) if nws else None
    _launch("mi355ppo_fc_pre_packed_f16x2_f32", a.device, _ptr(a), lda, _ptr(pack), _ptr(bias), _ptr(out), M, N, K, _ptr(ws),
            ws.numel() if nws else 0, _rec(a_rec, "a_amax"))
    return out


def fc_pre(a: torch.Tensor, W: torch.Tensor, b: torch.Tensor, bufs, a_rec: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """The FC layer's pre-activation for the trunk's (h, w, c)-ordered features: kernel Z from ``cnn.FCZ_MIN_ROWS`` rows on, below that
    ``torch.addmm`` on the (h, w, c)-ordered weight, as ``cnn.LinearReLUHwcFn`` does for rollout-sized calls."""
    if a.shape[0] >= cnn.FCZ_MIN_ROWS:
        return fc_pre_packed(a, bufs.fc_pack_fwd(W), b.detach().contiguous(), W.shape[0], a_rec, out)
    return torch.addmm(b.detach(), a, bufs.fc_weight(W).t(), out=out)


def _conv1(W1, bufs):
    """conv1 by its frame count -> ``(pack getter, pre-activation forward, weight gradient)``: kernels Q1 / P1 on one channel, kernel Q's PRE
    instance and kernel P on four (``cnn._conv1_family``'s idea for this node; dz1 in two f16 terms under its record, the uint8 frames are
    exact)."""
    if W1.shape[1] == 1:
        return bufs.q1_pack, conv1q1_pre_fwd, conv1p1_wgrad
    return (lambda W: bufs.weights(W, 1, MODE_FWD_Q), conv1q_pre_fwd,
            lambda obs, dz1, rec, inds: cnn.conv_wgrad(obs, dz1, 1, inds, amax=(None, rec)))


class LnNatureFn(torch.autograd.Function):
    """``h = relu(LN(fc(relu(LN(conv3(relu(LN(conv2(relu(LN(conv1(obs[inds] / 255))))))))))))`` as one autograd node; h is (M, 512)."""

    @staticmethod
    def forward(ctx, obs_u8, inds, trunk, want_grads, *params):
        W1, b1, g1, e1, W2, b2, g2, e2, W3, b3, g3, e3, Wf, bf, gf, ef = params
        bufs = trunk.bufs
        m = obs_u8.shape[0] if inds is None else inds.numel()
        dev = obs_u8.device
        if not bufs.f16(obs_u8) or m * 12800 * 4 >= BUF_LIMIT:
            raise NotImplementedError("MI355PPO_PQN_TRUNK=fused runs on the f16x2 split of kernel Z only: MI355PPO_SPLIT=bf16x3, MI355PPO_CONV=f "
                                      f"and batches of {BUF_LIMIT // 51200} images or more (32-bit buffer offsets) are not covered -- use "
                                      "MI355PPO_PQN_TRUNK=torch")
        a1, a2, a3 = bufs.get(m, dev, False)
        B = trunk.buffers(m, dev)
        z1, z2, z3, zf, h, stats = B["z1"], B["z2"], B["z3"], B["zf"], B["h"], B["stats"]
        rec = bufs.begin_pass(m, dev)         # one fill zeroes the records of this forward and of the backward that may follow
        grads = bool(want_grads)
        mb1, mb2, mb3 = bufs.get_bits(m, dev) if grads else (None, None, None)
        pack1, pre_fwd1, _ = _conv1(W1, bufs)
        pre_fwd1(obs_u8, pack1(W1), b1.detach(), inds, z1)
        layernorm_relu_fwd(z1, g1.detach(), e1.detach(), 32, 400, LN_EPS, a1, stats[0], stats[1], mb1, bufs.owns(REC_A1, a1))
        conv_pre_packed(a1, bufs.conv_zpack(W2, 2, MODE_FWD), b2.detach(), 2, rec[REC_A1], z2)
        layernorm_relu_fwd(z2, g2.detach(), e2.detach(), 64, 81, LN_EPS, a2, stats[2], stats[3], mb2, bufs.owns(REC_A2, a2))
        conv_pre_packed(a2, bufs.conv_zpack(W3, 3, MODE_FWD), b3.detach(), 3, rec[REC_A2], z3)
        layernorm_relu_fwd(z3, g3.detach(), e3.detach(), 64, 49, LN_EPS, a3, stats[4], stats[5], mb3, bufs.owns(REC_A3, a3))
        fc_pre(a3.view(m, 3136), Wf, bf, bufs, rec[REC_A3], zf)
        layernorm_relu_fwd(zf, gf.detach(), ef.detach(), 512, 1, LN_EPS, h, stats[6], stats[7])
        ctx.obs, ctx.inds, ctx.trunk, ctx.params, ctx.bits, ctx.m = obs_u8, inds, trunk, params, (mb1, mb2, mb3), m
        ctx.acts = (a1, a2, a3)
        return h

    @staticmethod
    def backward(ctx, dh):
        W1, b1, g1, e1, W2, b2, g2, e2, W3, b3, g3, e3, Wf, bf, gf, ef = ctx.params
        trunk, m = ctx.trunk, ctx.m
        bufs = trunk.bufs
        a1, a2, a3 = ctx.acts
        dev = a3.device
        mb1, mb2, mb3 = ctx.bits
        if mb1 is None:
            raise RuntimeError("LnNatureFn: the forward ran without gradients (no ReLU mask bits were written)")
        B = trunk.buffers(m, dev)
        z1, z2, z3, zf, h, stats = B["z1"], B["z2"], B["z3"], B["zf"], B["h"], B["stats"]
        G = trunk.grad_buffers(m, dev)
        dy1, dy2, dy3 = bufs.get(m, dev, True)
        dz1, dz2, dz3, dzf = G["dz1"], G["dz2"], G["dz3"], G["dzf"]
        a3f = a3.view(m, 3136)
        # FC: this layer's ReLU backward (dh comes from the torch head, unmasked) rides in the LayerNorm backward
        _, dgf, def_ = layernorm_relu_bwd(dh.contiguous(), zf, stats[6], stats[7], gf.detach(), 512, 1, act=h, dz=dzf, amax=bufs.owns(REC_DH, dzf))
        rf = bufs.rec_of(REC_DH, dzf)
        dbf = dzf.sum(0)
        dWf = cnn.fc_wgrad(dzf, a3f, 64, amax=(rf, bufs.rec_of(REC_A3, a3)))      # written in the (c, h, w) feature order of the weight itself
        cnn.fc_dgrad_mask_packed(dzf, bufs.fc_pack_dgrad(Wf), a3f, out=dy3.view(m, 3136), bits=mb3, amax=(rf, None))
        # layer 3
        _, dg3, de3 = layernorm_relu_bwd(dy3, z3, stats[4], stats[5], g3.detach(), 64, 49, dz=dz3, amax=bufs.owns(REC_DZ3, dz3))
        r3 = bufs.rec_of(REC_DZ3, dz3)
        dW3, db3 = cnn.conv_wgrad(a2, dz3, 3, amax=(bufs.rec_of(REC_A2, a2), r3))
        cnn.conv_dgrad_packed(dz3, bufs.conv_zpack(W3, 3, MODE_DGRAD_S1), a2, 3, dy2, bits=mb2, amax=(r3, None))
        # layer 2
        _, dg2, de2 = layernorm_relu_bwd(dy2, z2, stats[2], stats[3], g2.detach(), 64, 81, dz=dz2, amax=bufs.owns(REC_DZ2, dz2))
        r2 = bufs.rec_of(REC_DZ2, dz2)
        dW2, db2 = cnn.conv_wgrad(a1, dz2, 2, amax=(bufs.rec_of(REC_A1, a1), r2))
        cnn.conv_dgrad_packed(dz2, bufs.conv_zpack(W2, 2, MODE_DGRAD_S2), a1, 2, dy1, bits=mb1, amax=(r2, None))
        # layer 1
        _, dg1, de1 = layernorm_relu_bwd(dy1, z1, stats[0], stats[1], g1.detach(), 32, 400, dz=dz1, amax=bufs.owns(REC_DZ1, dz1))
        dW1, db1 = _conv1(W1, bufs)[2](ctx.obs, dz1, bufs.rec_of(REC_DZ1, dz1), ctx.inds)
        return (None, None, None, None, dW1, db1, dg1, de1, dW2, db2, dg2, de2, dW3, db3, dg3, de3, dWf, dbf, dgf, def_)


class LnNatureTrunk:
    """Callable owner of the node's buffers: ``trunk(obs_u8, inds, network) -> h (M, 512)`` for ``network`` =
    ``AtariQNetwork.network``.  Its ``bufs`` (a ``cnn._Buffers`` of its own) caches the weight packs: bump
    ``bufs.weights_version`` after every optimizer step that writes the parameters through raw pointers."""

    LAYERS = (0, 1, 3, 4, 6, 7, 10, 11)      # conv1, LN, conv2, LN, conv3, LN, Linear(3136, 512), LN(512) in network

    def __init__(self, network=None):
        self.bufs = cnn._Buffers()
        self._own = {}
        if network is not None:
            self.bufs.cache_weights = True
            self.bufs.pack_params = (network[0].weight, network[3].weight, network[6].weight, network[10].weight)

    def buffers(self, m: int, dev):
        """The pre-activations z1..z3, zf, the output h and the rows' (mean, rstd) of the four LayerNorms, one set per batch size."""
        shapes = {"z1": (m, 20, 20, 32), "z2": (m, 9, 9, 64), "z3": (m, 7, 7, 64), "zf": (m, 512), "h": (m, 512), "stats": (8, m)}
        return self._f32("fwd", m, dev, shapes)

    def grad_buffers(self, m: int, dev):
        return self._f32("bwd", m, dev, {"dz1": (m, 20, 20, 32), "dz2": (m, 9, 9, 64), "dz3": (m, 7, 7, 64), "dzf": (m, 512)})

    def _f32(self, kind, m, dev, shapes):
        return cnn._per_stream(self._own, dev, (kind, m, dev), lambda: {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()})

    def __call__(self, obs_u8, inds, network):
        params = []
        for i in self.LAYERS:
            params += [network[i].weight, network[i].bias]
        return LnNatureFn.apply(obs_u8, inds, self, torch.is_grad_enabled(), *params)
