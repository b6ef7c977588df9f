"""Kernel RV (csrc/convrv.hip): the layer-3 data gradient with seven images per group and the rows dealt to tiles by vertical border class.

Forced with ``MI355PPO_CONV_RV=min:1`` at batch sizes whose last group holds one, two, six and seven images (one and two groups), and at 1,800
images -- 258 groups, more than there are CUs, so that a workgroup carries its prefetched source and its ring slot across a group boundary (and
the ring's buffers change places: nine slots).  dz3 as the FC data gradient leaves it: masked, per-image scales spread over 2^-14 .. 1 (a read
into a neighbouring image would show), one all-zero image; one case with dz3 non-zero only in its rows 0 and 6 (the lines the skipped tap rows
would have read past).  Held against kernel Z (``MI355PPO_CONV_R=0``) and kernel R (``MI355PPO_CONV_RV=0``): gradient and amax record equal bit
for bit; a second call gives the same bits; against float64 autograd with the bar of tests/test_gpu_f16x2.py (|err| <= 2e-5 of the result's
scale); the words behind the gradient (one group's size) keep their NaN pattern; the route query keeps answering 'R'."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from cleanrl_amd import cnn

DEV = torch.device("cuda:0")
CASES = [(1, False), (2, False), (6, False), (7, False), (8, False), (13, False), (14, False), (15, False), (15, True), (1800, False)]
GROUP = 7                                                  # images per group of kernel RV (RVGeom::G)
NAN_WORD = 0x7FC0DEAD


def _close(got, ref, what, tol=2e-5):
    got, ref = got.detach().double(), ref.detach().double()
    scale = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert np.isfinite(err) and err <= tol * scale + 1e-30, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / max(scale, 1e-30):.2e})"


def _conv64(x_nhwc, W):
    B = x_nhwc.shape[0]
    cols = F.unfold(x_nhwc.permute(0, 3, 1, 2), kernel_size=3, stride=1)
    return torch.einsum("nk,bkl->bln", W.reshape(64, -1), cols).reshape(B, 7, 7, 64)


def _inputs(images, rows06):
    g = torch.Generator(device=DEV).manual_seed(4000 + images + (7 if rows06 else 0))
    act = torch.randn(images, 9, 9, 64, device=DEV, generator=g)
    dz = (torch.randn(images, 7, 7, 64, device=DEV, generator=g) * torch.exp2(-14 * torch.rand(images, 1, 1, 1, device=DEV, generator=g))
          * (torch.rand(images, 7, 7, 64, device=DEV, generator=g) > 0.5))
    if images >= 2:
        dz[images // 2] = 0.0
    if rows06:
        dz[:, 1:6] = 0.0
    m = (act > 0).reshape(-1, 32).to(torch.int64)          # word w, bit b <-> element 32 w + b of the flat activation
    w = (m << torch.arange(32, device=DEV)).sum(1)
    bits = ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)
    gc = torch.Generator().manual_seed(91 + images)
    W = (torch.randn(64, 64, 3, 3, generator=gc) / np.sqrt(64 * 9)).to(DEV)
    return act, dz.contiguous(), bits, W


def _run(dz, pack, bits, rz):
    """One guarded call: the gradient carved out of a buffer with a tail of one group's size; the tail must come back intact."""
    images = dz.shape[0]
    n = images * 81 * 64
    buf = torch.full((n + GROUP * 81 * 64,), NAN_WORD, dtype=torch.int32, device=DEV)
    rd = cnn.new_amax(1, DEV)[0]
    got = cnn.conv_dgrad_packed(dz, pack, None, 3, buf[:n].view(torch.float32).view(images, 9, 9, 64), bits=bits, amax=(rz, rd))
    torch.cuda.synchronize()
    assert bool((buf[n:] == NAN_WORD).all()), "words behind the gradient were written"
    return got.view(torch.int32).clone(), cnn.amax_value(rd), got.abs().max().item()


@pytest.mark.parametrize("images,rows06", CASES)
def test_kernel_rv_is_kernel_z_and_kernel_r_bit_for_bit_and_stays_inside_its_tensor(monkeypatch, images, rows06):
    lib = cnn._lib.load()
    act, dz, bits, W = _inputs(images, rows06)
    pack = cnn.conv_zpack_f16x2(W, 3, cnn.MODE_DGRAD_S1)
    rz = cnn.new_amax(1, DEV)[0]
    cnn.absmax(dz, rz)
    out = {}
    for route, env in (("Z", {"MI355PPO_CONV_R": "0", "MI355PPO_CONV_RV": "min:1"}), ("RV", {"MI355PPO_CONV_RV": "min:1"}), ("RV again", {"MI355PPO_CONV_RV": "min:1"}),
                       ("R", {"MI355PPO_CONV_R": "min:1", "MI355PPO_CONV_RV": "0"})):
        monkeypatch.delenv("MI355PPO_CONV_R", raising=False)
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        assert chr(lib.mi355ppo_cnn_conv_packed_kernel_f16x2(images, 3, 1)) == ("Z" if route == "Z" else "R")
        out[route] = _run(dz, pack, bits, rz)
    zy, za, zm = out["Z"]
    for route in ("RV", "RV again", "R"):
        y, am, mx = out[route]
        assert torch.equal(y, zy) and am == za == mx == zm, f"{route} against kernel Z, {images} images"
    x = act.double().requires_grad_(True)
    _conv64(x, W.double()).backward(dz.double())
    _close(out["RV"][0].view(torch.float32).view(images, 9, 9, 64), x.grad * (act > 0), f"kernel RV conv3 dgrad, {images} images")
