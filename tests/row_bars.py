"""Per-row float64 bars for the matrix kernels on the two-term f16 split (csrc/f16split.h): kernels Z, G, R, RB, RS, RV (forwards and data
gradients) and V, U, W, Y, H (weight gradients).  Shared by tests/test_row_bars_model.py (CPU: the bar against a float64 model of the split
and against mutations of it) and tests/test_gpu_f16x2_rows.py (the kernels themselves).

The bar (``row_bar``): every ROW of the result -- a sample of the FC layer, an image of a convolution, an output channel of a weight gradient
-- is held to ``c`` times the error torch's own f32 result has against float64, RELATIVE TO THAT ROW'S OWN SCALE, plus a floor of two f32
roundings of the epilogue.  ``rho32``, the f32 yardstick, is torch on the CPU (f32 and f64) on a batch of at least 64 rows / 8 images of the
same recipe, so that a one-row case does not get a yardstick that is small by luck, and so that the yardstick depends neither on the
library under the device nor on another kernel of this project.

The recipes (``fc_case`` / ``conv_case`` / ``*_wgrad_case``) follow tests/test_gpu_f16x2.py and add a per-row (forward, data gradient) or
per-output-channel (weight gradient) factor over 2^-12 .. 2^-16, so that most rows lie far below the tensor's maximum: the split's scale is
per TENSOR, and a per-tensor bar says nothing about those rows.  Everything is generated on the CPU from one seeded generator and cached:
the references are computed once and shared by every route of a size."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

SPEC = {1: (4, 32, 8, 4, 84, 20), 2: (32, 64, 4, 2, 20, 9), 3: (64, 64, 3, 1, 9, 7)}      # cin, cout, k, stride, hin, hout

# The floor: the epilogue unscales by an exact power of two, adds the bias and stores -- two f32 roundings of a value no larger than the
# row's scale, 2^-23 of it; the floor is twice that.
FLOOR = 2.0 ** -22
RHO_MIN = 2.0 ** -24         # the yardstick is never taken below one f32 rounding
C_MAX = 16.0                 # no family's c may go above this; tests/test_row_bars_model.py rejects every mutation at this value too
# c per kernel family.  The project's rule is twice the f32 reference's own error; these kernels round their accumulator three times per
# 16-wide k-step (hi hi, hi lo, lo hi) where the reference rounds once: sqrt(3) for independent roundings, rounded up to another factor 2.
# A family whose arithmetic is faithful and still measures above 4 on the device gets its worst measured ratio times 1.5, rounded up, never
# above C_MAX (DESIGN.md 3.2 keeps the measured table).
C_CONV_FORWARD = 4.0         # kernels Z, R, RS: conv layers 2 / 3 forward (32 / 36 k-steps)
C_FC_FORWARD_SPLIT_K = 4.0   # kernel Z with K split over the grid (below 8,192 rows through the wrapper): chains of a few k-steps, folded in f32
# kernels Z (whole K) and G, FC forward: ONE accumulator over all 196 k-steps.  Measured 5.46 at worst (300 rows; 5.13 at 77): the device's
# v_mfma_f32_32x32x16_f16 rounds its accumulator after each 8-wide half of the k-step (``accumulate="f32-halves"`` below reproduces the
# device's error distribution and 30 % of its bits, the one-rounding model 5 %), six roundings per k-step, where torch's f32 GEMM on the
# CPU blocks K and fuses multiply-adds.  ceil(1.5 * 5.46) = 9.
C_FC_FORWARD = 9.0
C_DGRAD = 4.0                # kernels Z, G, R, RB, RV: FC and conv data gradients
C_WGRAD = 4.0                # kernels V, U, W, Y, H: weight gradients (rows = output channels)
C_BIAS_GRAD = 4.0            # the bias gradients that come out of the weight-gradient kernels (f32 sums, no split)

FC_ROWS_MIN, CONV_IMAGES_MIN = 64, 8      # the yardstick batch


# ------------------------------------------------------------------------------------------------------------------ the split, in float64
def scale_exp(amax: float) -> int:
    """csrc/f16split.h::f16_scale_exp (and tests/test_gpu_f16x2.py::_scale_exp): e with 2^e * amax in [2^14, 2^15), clamped to [-100, 60]."""
    bits = int(np.float32(amax).view(np.uint32))
    return max(-100, min(60, 141 - ((bits >> 23) & 0xFF)))


def split_terms(x):
    """f32 tensor -> (hi, lo, e) in float64: hi = f16(2^e x) to nearest, lo = f16(2^e x - hi), e from the tensor's maximum."""
    x = np.ascontiguousarray(torch.as_tensor(x).detach().cpu().numpy(), dtype=np.float32)
    e = scale_exp(float(np.abs(x).max())) if x.size else 60
    v = x.astype(np.float64) * 2.0 ** e                    # (a power of two times an f32: exact, as the kernel's v_mul_f32 is)
    hi = v.astype(np.float16).astype(np.float64)
    lo = (v - hi).astype(np.float16).astype(np.float64)    # (v - hi is exact in f32 and in f64)
    return hi, lo, e


def split_model(a, b, accumulate: str = "exact", drop_lo: str | None = None, drop_lohi_step: int | None = None, b_exact: bool = False):
    """``a @ b.T`` for f32 ``a`` (M, K), ``b`` (N, K) as the f16-split kernels form it, in float64: each operand in two f16 terms under
    its per-tensor power-of-two scale, the three products hi hi, hi lo, lo hi (lo lo is dropped), unscaled by the exact power of two.

    ``accumulate="exact"``: float64 sums -- what the split can represent.  ``"f32"``: one f32 accumulator, rounded after each of the three
    products of every 16-wide k-step (``v_mfma_f32_32x32x16_f16`` three times per step).  ``"f32-halves"``: rounded after each 8-wide half
    of each product, k 0..7 first -- what the instruction does on gfx950, judged by the bits of the FC forward.  ``b_exact``: ``b`` goes in as ONE exact term (the
    uint8 frames of the layer-1 weight gradient).  The mutations tests/test_row_bars_model.py must see rejected: ``drop_lo="a" | "b"``
    loses that operand's lo term everywhere, ``drop_lohi_step=s`` loses lo(a) hi(b) in k-step ``s`` alone."""
    ah, al, ea = split_terms(a)
    if b_exact:
        bh = np.ascontiguousarray(torch.as_tensor(b).detach().cpu().numpy(), dtype=np.float64)
        bl, eb = np.zeros_like(bh), 0
    else:
        bh, bl, eb = split_terms(b)
    if drop_lo == "a":
        al = np.zeros_like(al)
    elif drop_lo == "b":
        bl = np.zeros_like(bl)
    else:
        assert drop_lo is None
    K = ah.shape[1]
    assert bh.shape[1] == K
    if accumulate == "exact":
        acc = ah @ bh.T + ah @ bl.T + al @ bh.T
        if drop_lohi_step is not None:
            s = slice(16 * drop_lohi_step, 16 * drop_lohi_step + 16)
            acc -= al[:, s] @ bh[:, s].T
    else:
        assert accumulate in ("f32", "f32-halves")
        width = 16 if accumulate == "f32" else 8
        acc = np.zeros((ah.shape[0], bh.shape[0]), dtype=np.float32)
        for step in range((K + 15) // 16):
            for p, q, is_lohi in ((ah, bh, False), (ah, bl, False), (al, bh, True)):
                if is_lohi and step == drop_lohi_step:
                    continue
                for k0 in range(16 * step, min(16 * step + 16, K), width):
                    s = slice(k0, k0 + width)
                    acc = (acc.astype(np.float64) + p[:, s] @ q[:, s].T).astype(np.float32)      # exact 22-bit products, one rounding
        acc = acc.astype(np.float64)
    return torch.from_numpy(acc * 2.0 ** -(ea + eb))


# ----------------------------------------------------------------------------------------------------------------------------- the bar
def _rows(t, row_axis):
    t = torch.as_tensor(t).detach().double().cpu()
    t = t.movedim(row_axis, 0)
    return t.reshape(t.shape[0], -1)


def rho32_of(ref32_yard, ref64_yard, row_axis: int = 0) -> float:
    """The yardstick: the largest row-relative error of torch's f32 result against float64 over the rows of the yardstick batch, at least
    2^-24."""
    r32, r64 = _rows(ref32_yard, row_axis), _rows(ref64_yard, row_axis)
    assert r32.shape == r64.shape
    scale, err = r64.abs().amax(1), (r32 - r64).abs().amax(1)
    live = scale > 0
    assert bool(live.any()), "the yardstick batch is all zero"
    return max(float((err[live] / scale[live]).max()), RHO_MIN)


def row_bar(name, got, ref64, ref32_yard, ref64_yard, row_axis: int = 0, c: float = 4.0) -> float:
    """Assert ``max |got_r - ref64_r| <= (c * rho32 + 2^-22) * max |ref64_r|`` for every row r along ``row_axis`` (rows whose reference is
    all zero must be all zero), rho32 from the yardstick batch; -> the worst ``(err_r / scale_r) / rho32``."""
    assert 0 < c <= C_MAX, f"{name}: c = {c} (the bar never moves above {C_MAX})"
    rho = rho32_of(ref32_yard, ref64_yard, row_axis)
    g, r = _rows(got, row_axis), _rows(ref64, row_axis)
    assert g.shape == r.shape, f"{name}: shape {tuple(g.shape)} against the reference's {tuple(r.shape)}"
    assert bool(torch.isfinite(g).all()), f"{name}: non-finite values in the result"
    scale, err = r.abs().amax(1), (g - r).abs().amax(1)
    dead = scale == 0
    assert not bool((err[dead] != 0).any()), f"{name}: row {int(torch.nonzero(dead & (err != 0))[0])} must be all zero and is not"
    live = ~dead
    if not bool(live.any()):
        return 0.0
    rel = torch.where(live, err / scale.clamp_min(1e-300), torch.zeros_like(err))
    worst = int(rel.argmax())
    ratio = float(rel[worst]) / rho
    assert bool((err[live] <= (c * rho + FLOOR) * scale[live]).all()), (
        f"{name}: row {worst} of {g.shape[0]} (scale {float(scale[worst]):.3e}, {float(scale[worst] / scale.max()):.2e} of the tensor's) has "
        f"err / scale = {float(rel[worst]):.3e}; torch f32's own rho32 = {rho:.3e}; ratio {ratio:.2f} against c = {c:g} (+ floor {FLOOR:.2e})")
    return ratio


# ------------------------------------------------------------------------------------------------------------------------- the recipes
def packed_bits(mask: torch.Tensor) -> torch.Tensor:
    """bool tensor -> the int32 words of its bit mask (word w, bit b <-> flat element 32 w + b), as the ``*_bits`` forwards write them."""
    m = mask.reshape(-1, 32).to(torch.int64)
    w = (m << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def fc_case(M: int):
    """Linear(3136, 512), forward and data gradient, ``max(M, 64)`` rows: the kernel gets the first ``M``.  Forward rows over 2^-12, the
    gradient's over 2^-16 with 40 % zeros; the bias at 2^-8 of the largest rows' level, so that it neither swamps the small rows nor vanishes
    beside the large ones."""
    rows = max(M, FC_ROWS_MIN)
    g = torch.Generator().manual_seed(5000 + M)
    a = torch.relu(torch.randn(rows, 3136, generator=g)) * torch.exp(torch.randn(rows, 3136, generator=g)) * torch.exp2(-12 * torch.rand(rows, 1, generator=g))
    W = torch.randn(512, 3136, generator=g) / 56.0
    b = torch.randn(512, generator=g) * 0.1 * 2.0 ** -8
    dz = (torch.randn(rows, 512, generator=g) * torch.exp2(-16 * torch.rand(rows, 1, generator=g)) * 1e-4 * (torch.rand(rows, 512, generator=g) > 0.4))
    mask = a > 0
    return SimpleNamespace(
        M=M, a=a, W=W, b=b, dz=dz, mask=mask,
        h32=torch.relu(a @ W.t() + b), h64=torch.relu(a.double() @ W.double().t() + b.double()),
        da32=(dz @ W) * mask, da64=(dz.double() @ W.double()) * mask)


def conv_params(layer: int, seed: int):
    cin, cout, k, _, _, _ = SPEC[layer]
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) * 0.1 * 2.0 ** -8
    return W, b


@functools.lru_cache(maxsize=None)
def conv_case(layer: int, images: int):
    """Layer 2 / 3 forward and data gradient, ``max(images, 8)`` images (NHWC): per-image factors over 2^-12 on the forward's source and over
    2^-14 on dz, dz half zeros, the ReLU mask of the data gradient from an independent ``act`` (half set)."""
    cin, cout, k, st, hin, hout = SPEC[layer]
    n = max(images, CONV_IMAGES_MIN)
    W, b = conv_params(layer, 6000 + 10 * layer + images)
    g = torch.Generator().manual_seed(7000 + 10 * images + layer)
    x = (torch.relu(torch.randn(n, hin, hin, cin, generator=g)) * torch.exp(torch.randn(n, hin, hin, cin, generator=g))
         * torch.exp2(-12 * torch.rand(n, 1, 1, 1, generator=g)))
    act = torch.randn(n, hin, hin, cin, generator=g)
    dz = (torch.randn(n, hout, hout, cout, generator=g) * torch.exp2(-14 * torch.rand(n, 1, 1, 1, generator=g)) * 1e-3
          * (torch.rand(n, hout, hout, cout, generator=g) > 0.5))
    mask = act > 0
    size = (n, cin, hin, hin)
    return SimpleNamespace(
        layer=layer, images=images, x=x, W=W, b=b, act=act, dz=dz, mask=mask,
        y32=_nhwc(torch.relu(F.conv2d(_nchw(x), W, b, stride=st))), y64=_nhwc(torch.relu(F.conv2d(_nchw(x).double(), W.double(), b.double(), stride=st))),
        dx32=_nhwc(torch.nn.grad.conv2d_input(size, W, _nchw(dz), stride=st)) * mask,
        dx64=_nhwc(torch.nn.grad.conv2d_input(size, W.double(), _nchw(dz).double(), stride=st)) * mask)


def _wgrad_refs(src32, src64, dz, layer, images):
    """(dW32, dW64, db32, db64) of the first ``images`` images, torch on the CPU."""
    cin, cout, k, st, _, _ = SPEC[layer]
    z = _nchw(dz[:images])
    shape = (cout, cin, k, k)
    return (torch.nn.grad.conv2d_weight(_nchw(src32[:images]), shape, z, stride=st),
            torch.nn.grad.conv2d_weight(_nchw(src64[:images]), shape, z.double(), stride=st),
            dz[:images].sum((0, 1, 2)), dz[:images].double().sum((0, 1, 2)))


def _wgrad_case(layer, images, src, dz, src32, src64, **extra):
    n = dz.shape[0]
    yard = _wgrad_refs(src32, src64, dz, layer, n)
    own = yard if n == images else _wgrad_refs(src32, src64, dz, layer, images)
    return SimpleNamespace(layer=layer, images=images, src=src, dz=dz, dW32_yard=yard[0], dW64_yard=yard[1], db32_yard=yard[2], db64_yard=yard[3],
                           dW64=own[1], db64=own[3], **extra)


@functools.lru_cache(maxsize=None)
def conv_wgrad_case(layer: int, images: int):
    """Layer 2 / 3 weight gradient, ``max(images, 8)`` images: the recipe of tests/test_gpu_f16x2.py (per-image factors over 2^-10 on dz) with
    a per-output-channel factor over 2^-12 on top -- the small operand elements lie along the rows of dW."""
    cin, cout, k, st, hin, hout = SPEC[layer]
    n = max(images, CONV_IMAGES_MIN)
    g = torch.Generator().manual_seed(8000 + 10 * images + layer)
    src = torch.relu(torch.randn(n, hin, hin, cin, generator=g)) * torch.exp(torch.randn(n, hin, hin, cin, generator=g))
    dz = (torch.randn(n, hout, hout, cout, generator=g) * torch.exp2(-10 * torch.rand(n, 1, 1, 1, generator=g)) * 1e-3
          * torch.exp2(-12 * torch.rand(cout, generator=g)))
    return _wgrad_case(layer, images, src, dz, src, src.double())


@functools.lru_cache(maxsize=None)
def conv1_wgrad_case(images: int):
    """Layer-1 weight gradient through a row gather of uint8 frames (the reference divides by 255), dz half zeros, per-image and per-channel
    factors as in ``conv_wgrad_case``."""
    n = max(images, CONV_IMAGES_MIN)
    g = torch.Generator().manual_seed(9000 + images)
    obs = torch.randint(0, 256, (n + 5, 84, 84, 4), dtype=torch.uint8, generator=g)
    inds = torch.randperm(n + 5, generator=g)[:n]
    dz = (torch.randn(n, 20, 20, 32, generator=g) * torch.exp2(-10 * torch.rand(n, 1, 1, 1, generator=g)) * 1e-3
          * (torch.rand(n, 20, 20, 32, generator=g) > 0.5) * torch.exp2(-12 * torch.rand(32, generator=g)))
    return _wgrad_case(1, images, obs, dz, obs[inds].float() / 255.0, obs[inds].double() / 255.0, inds=inds)


@functools.lru_cache(maxsize=None)
def fc_wgrad_case(M: int):
    """Linear(3136, 512) weight gradient ``dz.T @ a``: per-sample factors over 2^-12 on dz as in tests/test_gpu_f16x2.py, a per-output-unit
    factor over 2^-12 on top (the rows of dW)."""
    rows = max(M, FC_ROWS_MIN)
    g = torch.Generator().manual_seed(9500 + M)
    a = torch.relu(torch.randn(rows, 3136, generator=g)) * torch.exp(torch.randn(rows, 3136, generator=g))
    dz = torch.randn(rows, 512, generator=g) * torch.exp2(-12 * torch.rand(rows, 1, generator=g)) * 1e-4 * torch.exp2(-12 * torch.rand(512, generator=g))
    dW64_yard = dz.double().t() @ a.double()
    return SimpleNamespace(M=M, a=a, dz=dz, dW32_yard=dz.t() @ a, dW64_yard=dW64_yard,
                           dW64=dW64_yard if rows == M else dz[:M].double().t() @ a[:M].double())


# ------------------------------------------------------------------------------------------- the recipes as GEMMs, for the float64 model
def gemm_forms():
    """Every recipe above as ``a @ b.T`` the way the kernels see it (im2col for the convolutions), at the yardstick batch's size, for
    tests/test_row_bars_model.py: -> a list of namespaces with the f32 operands ``a`` (M, K) and ``b`` (N, K), ``finish(product, f32)`` (the
    epilogue; -> the result with its rows along axis 0), ``ref32`` / ``ref64`` (torch's own results, rows along axis 0), ``c`` and, for the
    mutation that loses lo hi in ONE k-step, the step to lose it in."""
    forms = []

    def add(name, a, b, finish, ref32, ref64, c, b_exact=False):
        # the k-step a lost term shows in: where the operand `a` carries most of its magnitude.  (With a factor per k-index -- the weight
        # gradients sum over the images -- a step inside a small image moves no row at any bar.)
        K = a.shape[1]
        steps = F.pad(a.abs().double().sum(0), (0, (-K) % 16)).reshape(-1, 16).sum(1)
        forms.append(SimpleNamespace(name=name, a=a, b=b, finish=finish, ref32=ref32, ref64=ref64, c=c, b_exact=b_exact, step=int(steps.argmax())))

    def rnd(t, f32):      # the epilogue's stores (and its bias add) round to f32 in the f32 model, stay float64 in the exact one
        return t.float().double() if f32 else t

    fc = fc_case(FC_ROWS_MIN)
    add("fc forward", fc.a, fc.W, lambda p, f32: rnd(torch.relu(rnd(p, f32) + fc.b.double()), f32), fc.h32, fc.h64, C_FC_FORWARD)
    add("fc data gradient", fc.dz, fc.W.t().contiguous(), lambda p, f32: rnd(p, f32) * fc.mask, fc.da32, fc.da64, C_DGRAD)
    for layer in (2, 3):
        cin, cout, k, st, hin, hout = SPEC[layer]
        cv = conv_case(layer, CONV_IMAGES_MIN)
        n = cv.x.shape[0]
        cols = F.unfold(_nchw(cv.x), kernel_size=k, stride=st).permute(0, 2, 1).reshape(n * hout * hout, cin * k * k)
        add(f"conv{layer} forward", cols, cv.W.reshape(cout, -1),
            lambda p, f32, cv=cv, n=n: rnd(torch.relu(rnd(p, f32) + cv.b.double()), f32).reshape(n, -1), cv.y32.reshape(n, -1), cv.y64.reshape(n, -1), C_CONV_FORWARD)
        # data gradient: dz dilated by the stride and padded by k - 1, correlated with the flipped taps; K ordered (tap row, tap column,
        # output channel) as the kernels' packs are, so that a k-step lies inside one tap and the steps of the taps that hit only the
        # dilation's zeros add exact zeros
        z = torch.zeros(n, cout, (hout - 1) * st + 1, (hout - 1) * st + 1)
        z[:, :, ::st, ::st] = _nchw(cv.dz)
        zc = F.unfold(F.pad(z, (k - 1,) * 4), kernel_size=k).reshape(n, cout, k * k, hin * hin).permute(0, 3, 2, 1).reshape(n * hin * hin, k * k * cout)
        wf = cv.W.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, k * k * cout)
        add(f"conv{layer} data gradient", zc, wf, lambda p, f32, cv=cv, n=n: (rnd(p, f32).reshape(cv.mask.shape) * cv.mask).reshape(n, -1),
            cv.dx32.reshape(n, -1), cv.dx64.reshape(n, -1), C_DGRAD)
        wg = conv_wgrad_case(layer, CONV_IMAGES_MIN)
        wcols = F.unfold(_nchw(wg.src), kernel_size=k, stride=st).permute(1, 0, 2).reshape(cin * k * k, n * hout * hout)
        add(f"conv{layer} weight gradient", wg.dz.reshape(-1, cout).t().contiguous(), wcols, lambda p, f32: rnd(p, f32),
            wg.dW32_yard.reshape(cout, -1), wg.dW64_yard.reshape(cout, -1), C_WGRAD)
    w1 = conv1_wgrad_case(CONV_IMAGES_MIN)
    n = w1.dz.shape[0]
    frames = F.unfold(_nchw(w1.src[w1.inds].float()), kernel_size=8, stride=4).permute(1, 0, 2).reshape(256, n * 400)
    add("conv1 weight gradient", w1.dz.reshape(-1, 32).t().contiguous(), frames, lambda p, f32: rnd(rnd(p, f32) / 255.0, f32),
        w1.dW32_yard.reshape(32, -1), w1.dW64_yard.reshape(32, -1), C_WGRAD, b_exact=True)
    fw = fc_wgrad_case(200)
    add("fc weight gradient", fw.dz.t().contiguous(), fw.a.t().contiguous(), lambda p, f32: rnd(p, f32), fw.dW32_yard, fw.dW64_yard, C_WGRAD)
    return forms
