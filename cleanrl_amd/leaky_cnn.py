"""The two LeakyReLU NatureCNNs of ``ppo_rnd_envpool.py``'s ``RNDModel`` on the libmi355ppo kernels, straight from the uint8 rollout rows:
``predictor[0:9]`` (Conv -> LeakyReLU three times, Flatten, Linear(3136, 512) -> ReLU; forward and backward) and the whole frozen ``target``
(the same stack ending in a plain Linear(3136, 512); forward only).  Their input is ONE frame, normalised and clipped:
``clip((u8 - mean[p]) / sd[p], -5, 5)`` -- an f32 value, so the integer conv1 kernels cannot read it.

conv1 is csrc/rnd_conv1.hip: the newest frame of each row is normalised once per pixel into LDS (the row function of ``ops.rnd_normalize``),
split into two f16 terms under the static scale 2^12, and multiplied from there; bias + LeakyReLU, the sign bits and the amax record ride in
the epilogue.  Layers 2 / 3 are the pre-activation forward of ``ln_cnn.conv_pre_packed`` (kernel Z's Z_BIAS epilogue) followed by
``ops.leaky_relu_fwd`` in place.  Backward: the data-gradient kernels fuse a ReLU mask, so they are called with an all-ones mask (filled once
per batch size) and ``ops.leaky_relu_bwd`` then applies the layer's own sign bits in place and writes the record the next weight- and
data-gradient kernels scale by; the weight gradients are ``cnn.conv_wgrad`` / ``cnn.fc_wgrad`` unchanged and conv1's is rnd_conv1.hip's.  A
leaky ``a3`` is never registered as ``bufs.last_a3_ptr``: ``cnn.LinearReLUHwcFn``'s fused conv3-ReLU mask must not fire on it.

f16x2 split only: with ``MI355PPO_SPLIT=bf16x3``, ``MI355PPO_CONV=f`` or tensors beyond ``cnn.BUF_LIMIT`` the node raises
``NotImplementedError`` -- there is no fallback.
"""
from __future__ import annotations

import torch

from . import _lib, cnn, ln_cnn, ops
from .cnn import BUF_LIMIT, MODE_DGRAD_S1, MODE_DGRAD_S2, MODE_FWD, REC_A1, REC_A2, REC_A3, REC_DH, REC_DZ1, REC_DZ2, REC_DZ3
from .ops import AMAX_WORDS, _chk, _launch, _ptr, _workspace
from .rnd_ops import LEAKY_SLOPE, RND_PIXELS

N1_PACK_SHAPE = (32, 64)      # conv1's weight as the (channels, kh * 8 + kw) matrix ``cnn.fc_pack_f16x2`` packs


def _frame(rows, nhwc: bool):
    """u8 observation rows of 4 stacked frames -> (B, row_bytes, pixel_stride, byte_offset) of the newest one (``rnd_ops._frame``)."""
    B = rows.shape[0]
    _chk(rows, torch.uint8, "rows", (B, 84, 84, 4) if nhwc else (B, 4, 84, 84))
    return B, 4 * RND_PIXELS, (4 if nhwc else 1), (3 if nhwc else 3 * RND_PIXELS)


def _stats(mean, sd):
    return _chk(mean.reshape(-1), torch.float64, "mean", (RND_PIXELS,)), _chk(sd.reshape(-1), torch.float64, "sd", (RND_PIXELS,))


def _rows_of(idx, B):
    """Images of a call: the index's length, or every row."""
    if idx is None:
        return B
    (M,) = idx.shape
    _chk(idx, torch.int64, "idx", (M,))
    return M


def rnd_conv1_fwd(rows, mean, sd, pack, bias, idx=None, out=None, bits=None, amax=None, nhwc: bool = True, slope: float = LEAKY_SLOPE):
    """``leaky_relu(conv1(x) + bias)`` -> (M, 20, 20, 32) f32 channels-last, ``x`` = ``ops.rnd_normalize(rows, mean, sd, idx)`` formed in
    LDS; ``pack = cnn.fc_pack_f16x2(W1.view(32, 64))``.  ``bits`` (optional, M * 400 int32 words): the pre-activation's sign ``z > 0`` in
    ``cnn.mask_words``' layout; ``amax`` (optional): the result's amax record, zeroed by the caller."""
    lib = _lib.load()
    B, row_bytes, stride, off = _frame(rows, nhwc)
    mean, sd = _stats(mean, sd)
    M = _rows_of(idx, B)
    _chk(pack, torch.uint8, "pack", (lib.mi355ppo_fc_pack_f16x2_bytes(*N1_PACK_SHAPE),))
    _chk(bias, torch.float32, "bias", (32,))
    if out is None:
        out = torch.empty((M, 20, 20, 32), dtype=torch.float32, device=rows.device)
    _chk(out, torch.float32, "out", (M, 20, 20, 32))
    if bits is not None:
        _chk(bits, torch.int32, "bits", (M * 400,))
    if amax is not None:
        _chk(amax, torch.int32, "amax record", (AMAX_WORDS,))
    _launch("mi355ppo_rnd_conv1_fwd_f16x2", rows.device, _ptr(rows), B, row_bytes, stride, off, _ptr(idx), _ptr(mean), _ptr(sd), _ptr(pack),
            _ptr(bias), _ptr(out), _ptr(bits), _ptr(amax), M, float(slope))
    return out


def rnd_conv1_wgrad(rows, mean, sd, dz, dz_amax, idx=None, out=None, nhwc: bool = True):
    """``(dW (32, 1, 8, 8), db (32,))`` of that convolution from the pre-activation gradient ``dz`` (M, 20, 20, 32) with its amax record and
    the same rows, index and statistics: dz in two f16 terms, x under its static scale, one partial per wave folded in a fixed order."""
    lib = _lib.load()
    B, row_bytes, stride, off = _frame(rows, nhwc)
    mean, sd = _stats(mean, sd)
    M = dz.shape[0]
    _chk(dz, torch.float32, "dz", (M, 20, 20, 32))
    if _rows_of(idx, B) != M:
        raise ValueError(f"rnd_conv1_wgrad: {M} rows of dz for {B if idx is None else idx.numel()} images")
    _chk(dz_amax, torch.int32, "dz_amax", (AMAX_WORDS,))
    dev = dz.device
    if out is not None:
        dW, db = _chk(out[0], torch.float32, "dW", (32, 1, 8, 8)), _chk(out[1], torch.float32, "db", (32,))
    else:
        dW, db = torch.empty((32, 1, 8, 8), dtype=torch.float32, device=dev), torch.empty(32, dtype=torch.float32, device=dev)
    ws = _workspace(dev, lib.mi355ppo_rnd_conv1_wgrad_workspace_bytes(M))
    _launch("mi355ppo_rnd_conv1_wgrad_f16x2", dev, _ptr(rows), B, row_bytes, stride, off, _ptr(idx), _ptr(mean), _ptr(sd), _ptr(dz), _ptr(dW),
            _ptr(db), M, _ptr(ws), ws.numel(), _ptr(dz_amax))
    return dW, db


def _trunk_fwd(trunk, rows, idx, mean, sd, nhwc, grads, W1, b1, W2, b2, W3, b3):
    """conv1 .. conv3 with their LeakyReLUs -> (a1, a2, a3, sign bits | Nones, the pass's records)."""
    bufs = trunk.bufs
    m = rows.shape[0] if idx is None else idx.numel()
    dev = rows.device
    if not bufs.f16(rows) or m * 12800 * 4 >= BUF_LIMIT:
        raise NotImplementedError("MI355PPO_RND_TRUNK=fused runs on the f16x2 split of kernel Z only: MI355PPO_SPLIT=bf16x3, MI355PPO_CONV=f "
                                  f"and batches of {BUF_LIMIT // 51200} images or more (32-bit buffer offsets) are not covered -- use "
                                  "MI355PPO_RND_TRUNK=torch")
    a1, a2, a3 = bufs.get(m, dev, False)
    rec = bufs.begin_pass(m, dev)             # one fill zeroes the records of this forward and of the backward that may follow
    mb1, mb2, mb3 = bufs.get_bits(m, dev) if grads else (None, None, None)
    rnd_conv1_fwd(rows, mean, sd, trunk.n1_pack(W1), b1.detach(), idx, a1, mb1, bufs.owns(REC_A1, a1), nhwc)
    ln_cnn.conv_pre_packed(a1, bufs.conv_zpack(W2, 2, MODE_FWD), b2.detach(), 2, rec[REC_A1], a2)
    ops.leaky_relu_fwd(a2, out=a2, bits=mb2, amax=bufs.owns(REC_A2, a2))
    ln_cnn.conv_pre_packed(a2, bufs.conv_zpack(W3, 3, MODE_FWD), b3.detach(), 3, rec[REC_A2], a3)
    ops.leaky_relu_fwd(a3, out=a3, bits=mb3, amax=bufs.owns(REC_A3, a3))
    return (a1, a2, a3), (mb1, mb2, mb3), rec


class LeakyNatureFn(torch.autograd.Function):
    """``h = relu(fc(leaky(conv3(leaky(conv2(leaky(conv1(x))))))))`` as one autograd node, x the normalised newest frame of ``rows[idx]``;
    h is (M, 512).  ``RNDModel.predictor[0:9]``."""

    @staticmethod
    def forward(ctx, rows, idx, mean, sd, trunk, want_grads, nhwc, *params):
        W1, b1, W2, b2, W3, b3, Wf, bf = params
        bufs = trunk.bufs
        grads = bool(want_grads)
        acts, bits, rec = _trunk_fwd(trunk, rows, idx, mean, sd, nhwc, grads, W1, b1, W2, b2, W3, b3)
        a3f = acts[2].view(acts[2].shape[0], 3136)
        h = cnn.fc_fwd_relu_packed(a3f, bufs.fc_pack_fwd(Wf), bf.detach().contiguous(), Wf.shape[0], amax=(rec[REC_A3], None))
        ctx.rows, ctx.idx, ctx.stats, ctx.trunk, ctx.params, ctx.nhwc = rows, idx, (mean, sd), trunk, params, nhwc
        ctx.acts, ctx.bits, ctx.h = acts, bits, h
        return h

    @staticmethod
    def backward(ctx, dh):
        W1, b1, W2, b2, W3, b3, Wf, bf = ctx.params
        trunk = ctx.trunk
        bufs = trunk.bufs
        a1, a2, a3 = ctx.acts
        mb1, mb2, mb3 = ctx.bits
        if mb1 is None:
            raise RuntimeError("LeakyNatureFn: the forward ran without gradients (no sign bits were written)")
        m, dev = a3.shape[0], a3.device
        one1, one2, one3 = trunk.ones(m, dev)
        dy1, dy2, dy3 = bufs.get(m, dev, True)
        a3f = a3.view(m, 3136)
        # FC: its own ReLU backward on the unmasked dh from the torch layers behind it; the record is measured (rec_of)
        dzf = torch.ops.aten.threshold_backward(dh.contiguous(), ctx.h, 0.0)
        rf = bufs.rec_of(REC_DH, dzf)
        dbf = dzf.sum(0)
        dWf = cnn.fc_wgrad(dzf, a3f, 64, amax=(rf, bufs.rec_of(REC_A3, a3)))      # written in the (c, h, w) feature order of the weight itself
        cnn.fc_dgrad_mask_packed(dzf, bufs.fc_pack_dgrad(Wf), a3f, out=dy3.view(m, 3136), bits=one3, amax=(rf, None))
        # layer 3
        dz3 = ops.leaky_relu_bwd(dy3, mb3, out=dy3, amax=bufs.owns(REC_DZ3, dy3))
        r3 = bufs.rec_of(REC_DZ3, dz3)
        dW3, db3 = cnn.conv_wgrad(a2, dz3, 3, amax=(bufs.rec_of(REC_A2, a2), r3))
        cnn.conv_dgrad_packed(dz3, bufs.conv_zpack(W3, 3, MODE_DGRAD_S1), a2, 3, dy2, bits=one2, amax=(r3, None))
        # layer 2
        dz2 = ops.leaky_relu_bwd(dy2, mb2, out=dy2, amax=bufs.owns(REC_DZ2, dy2))
        r2 = bufs.rec_of(REC_DZ2, dz2)
        dW2, db2 = cnn.conv_wgrad(a1, dz2, 2, amax=(bufs.rec_of(REC_A1, a1), r2))
        cnn.conv_dgrad_packed(dz2, bufs.conv_zpack(W2, 2, MODE_DGRAD_S2), a1, 2, dy1, bits=one1, amax=(r2, None))
        # layer 1
        dz1 = ops.leaky_relu_bwd(dy1, mb1, out=dy1, amax=bufs.owns(REC_DZ1, dy1))
        dW1, db1 = rnd_conv1_wgrad(ctx.rows, *ctx.stats, dz1, bufs.rec_of(REC_DZ1, dz1), ctx.idx, nhwc=ctx.nhwc)
        return (None,) * 7 + (dW1, db1, dW2, db2, dW3, db3, dWf, dbf)


class LeakyNatureTrunk:
    """Callable owner of a network's buffers and weight packs: ``trunk(rows, idx, mean, sd)`` -> (M, 512).  ``head=True``:
    ``RNDModel.predictor`` -- the autograd node over ``predictor[0:9]`` (``relu(fc(a3))``; ``predictor[9:]`` stays torch); bump
    ``bufs.weights_version`` after every optimizer step that writes the parameters through raw pointers.  ``head=False``: the frozen
    ``RNDModel.target``, forward only, its last layer through ``ln_cnn.fc_pre``; its packs are derived once."""

    LAYERS = (0, 2, 4, 7)         # conv1, conv2, conv3, Linear(3136, 512) in both Sequentials

    def __init__(self, network, head: bool):
        self.network, self.head = network, head
        self.bufs = cnn._Buffers()
        self.bufs.cache_weights = True
        self._ones = {}

    def n1_pack(self, W1):
        """``cnn.fc_pack_f16x2`` of conv1's (32, 64) matrix, cached like the other packs."""
        return self.bufs._derived("n1_pack", W1, lambda out: cnn.fc_pack_f16x2(W1.detach().view(*N1_PACK_SHAPE), None, out))

    def ones(self, m: int, dev):
        """All-ones mask words for the data gradients of a1, a2, a3 (their fused ReLU mask then passes everything); filled once per size."""
        return cnn._per_stream(self._ones, dev, ("ones", m, dev), lambda: [torch.full((cnn.mask_words(m * n),), -1, dtype=torch.int32, device=dev)
                                                                            for n in (20 * 20 * 32, 9 * 9 * 64, 7 * 7 * 64)])

    def params(self):
        out = []
        for i in self.LAYERS:
            out += [self.network[i].weight, self.network[i].bias]
        return out

    def __call__(self, rows, idx, mean, sd, nhwc: bool = True):
        params = self.params()
        if self.head:
            return LeakyNatureFn.apply(rows, idx, mean, sd, self, torch.is_grad_enabled(), nhwc, *params)
        with torch.no_grad():
            acts, _, rec = _trunk_fwd(self, rows, idx, mean, sd, nhwc, False, *params[:6])
            a3 = acts[2]
            return ln_cnn.fc_pre(a3.view(a3.shape[0], 3136), params[6], params[7], self.bufs, rec[REC_A3])
