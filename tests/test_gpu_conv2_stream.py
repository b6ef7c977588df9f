"""Kernel RS (csrc/convrs.hip): the layer-2 forward with the source of a three-image group streamed through LDS by stride-parity class.

Forced with ``MI355PPO_CONV_RS=min:1`` at batch sizes whose last group holds one, two and three images, at a single group, and at 769 images --
257 groups, more than there are CUs, so that a workgroup walks two groups through the pipeline that crosses the group boundary.  Held against
kernel Z (``MI355PPO_CONV_R=0``): output, mask words and the output's amax record equal bit for bit -- the same products in the same order --; against
kernel R's resident instance (``MI355PPO_CONV_RS=0``): the same bits; against float64 ``relu(conv)`` with the bar of tests/test_gpu_f16x2.py
(|err| <= 2e-5 of the result's scale); a repeated call gives the same bits; and nothing is written behind the output or the mask words (the rows
of images a last group does not have are left to the buffer descriptor's range check)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from cleanrl_amd import cnn

DEV = torch.device("cuda:0")
IMAGES = [1, 2, 3, 4, 5, 7, 769]
GROUP = 3                                                  # images per group of kernel RS (RSGeom::G)
NAN_WORD, ONES_WORD = 0x7FC0DEAD, -1                       # guard patterns: a NaN behind the output, 0xFFFFFFFF behind the mask words


def _close(got, ref, what, tol=2e-5):
    got, ref = got.detach().double(), ref.detach().double()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert np.isfinite(err) and err <= tol * scale + 1e-30, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / max(scale, 1e-30):.2e})"


def _conv64(x_nhwc, W, b):
    B = x_nhwc.shape[0]
    cols = F.unfold(x_nhwc.permute(0, 3, 1, 2), kernel_size=4, stride=2)
    y = torch.einsum("nk,bkl->bln", W.reshape(64, -1), cols) + b
    return y.reshape(B, 9, 9, 64)


def _inputs(images):
    """a1 as the layer-1 forward leaves it: post-ReLU, per-image scales over about 2^-14 .. 1, one all-zero image (from two images on)."""
    g = torch.Generator(device=DEV).manual_seed(1000 + images)
    x = torch.relu(torch.randn(images, 20, 20, 32, device=DEV, generator=g)) * torch.exp(torch.randn(images, 20, 20, 32, device=DEV, generator=g))
    x = x * torch.exp2(-14 * torch.rand(images, 1, 1, 1, device=DEV, generator=g))
    if images >= 2:
        x[images // 2] = 0.0
    gc = torch.Generator().manual_seed(77 + images)
    W = (torch.randn(64, 32, 4, 4, generator=gc) / np.sqrt(32 * 16)).to(DEV)
    b = (torch.randn(64, generator=gc) * 0.1 * x.max().item()).to(DEV)
    return x.contiguous(), W, b


def _run(x, pack, b, rx, with_bits):
    """One guarded call: the output and the mask words carved out of buffers with a tail of one group's size; the tails must come back intact."""
    images = x.shape[0]
    n, nw = images * 81 * 64, images * 81 * 2
    ybuf = torch.full((n + GROUP * 81 * 64,), NAN_WORD, dtype=torch.int32, device=DEV)
    wbuf = torch.full((nw + GROUP * 81 * 2,), ONES_WORD, dtype=torch.int32, device=DEV)
    ry = cnn.new_amax(1, DEV)[0]
    y = cnn.conv_fwd_packed(x, pack, b, 2, out=ybuf[:n].view(torch.float32).view(images, 9, 9, 64), bits=wbuf[:nw] if with_bits else None, amax=(rx, ry))
    torch.cuda.synchronize()
    assert bool((ybuf[n:] == NAN_WORD).all()), "words behind the output were written"
    assert bool((wbuf[nw:] == ONES_WORD).all()) and (with_bits or bool((wbuf == ONES_WORD).all())), "words behind (or, without bits, in) the mask were written"
    return y.view(torch.int32).clone(), wbuf[:nw].clone(), cnn.amax_value(ry), y.max().item()


@pytest.mark.parametrize("images", IMAGES)
def test_kernel_rs_is_kernel_z_bit_for_bit_and_stays_inside_its_tensors(monkeypatch, images):
    lib = cnn._lib.load()
    x, W, b = _inputs(images)
    pack = cnn.conv_zpack_f16x2(W, 2, cnn.MODE_FWD)
    rx = cnn.new_amax(1, DEV)[0]
    cnn.absmax(x, rx)
    out = {}
    for route, env in (("Z", {"MI355PPO_CONV_R": "0", "MI355PPO_CONV_RS": "min:1"}), ("RS", {"MI355PPO_CONV_RS": "min:1"}), ("RS again", {"MI355PPO_CONV_RS": "min:1"}),
                       ("R", {"MI355PPO_CONV_R": "min:1", "MI355PPO_CONV_RS": "0"})):
        monkeypatch.delenv("MI355PPO_CONV_R", raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        assert chr(lib.mi355ppo_cnn_conv_packed_kernel_f16x2(images, 2, 0)) == ("Z" if route == "Z" else "R")
        out[route] = (_run(x, pack, b, rx, True), _run(x, pack, b, rx, False))
    (zy, zw, za, zm), (zy0, _, za0, _) = out["Z"]
    for route in ("RS", "RS again", "R"):
        (y, w, am, mx), (y0, _, am0, mx0) = out[route]
        assert torch.equal(y, zy) and torch.equal(w, zw) and am == za == mx == zm, f"{route} with mask bits against kernel Z, {images} images"
        assert torch.equal(y0, y) and am0 == am == mx0, f"{route} without mask bits, {images} images"
        if images >= 768:                                  # (below, kernel Z runs its 32-row tiles without the bits and 64-row tiles with them)
            assert torch.equal(y0, zy0) and am0 == za0
    y = out["RS"][0][0].view(torch.float32).view(images, 9, 9, 64)
    assert torch.equal(cnn.unpack_mask_bits(out["RS"][0][1], y.shape), y > 0)
    _close(y, torch.relu(_conv64(x.double(), W.double(), b.double())), f"kernel RS conv2 fwd, {images} images")
