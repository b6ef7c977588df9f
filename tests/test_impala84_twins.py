"""The IMPALA-CNN trunk on Atari stacks (the 84 family of csrc/impala.hip) through its host twins: the 64x64x3 family held to
the digest minted before the kernels learned the second geometry, the 84 twin against float64 autograd of the reference's
modules, the max pool alone (84 / 42 / 21, the last one odd) against torch bit for bit, ``ops.Impala84Trunk`` on CPU tensors,
``agents.AtariImpalaQNetwork`` and the C ABI's refusals.  No GPU."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

import impala84_cases as C
from cleanrl_amd import _lib, agents, host_ops, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_64_family_twin_reproduces_the_digest_bit_for_bit():
    with open(os.path.join(GOLDEN, "impala64_twin_digest.json")) as f:
        want = json.load(f)
    assert C.digest64(host_ops) == want


def test_u8_staging_is_torchs_division():
    b = torch.arange(256, dtype=torch.uint8)
    x = b.view(1, 1, 64, 4).expand(1, 84, 64, 4)
    x = torch.cat([x, x[:, :, :20]], 2).contiguous()                # (1, 84, 84, 4): every byte value
    w = [torch.zeros(s) for s in ops.impala84_param_shapes()]
    w[0][:4, :, 1, 1] = torch.eye(4)                                 # layer 0 copies the centre pixel's channels 0..3
    _, saved, arg = host_ops.impala84_forward(x, w)
    P = saved[:42 * 42 * 16].view(42, 42, 16)                        # pooled layer-0 output: max over windows of copies
    want = F.max_pool2d((x.permute(0, 3, 1, 2) / 255.0), 3, 2, 1)[0].permute(1, 2, 0)
    assert torch.equal(P[..., :4], want)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("frames", C.FRAMES)
def test_twins_against_float64(B, frames):
    _, params = C.make_params(seed=B)
    x, dy = C.make_frames(frames, B, seed=B), C.upstream(B, seed=B + 7)
    y, saved, arg = host_ops.impala84_forward(x, params)
    grads = host_ops.impala84_backward(x, params, saved, arg, dy)
    assert y.shape == (B, 11, 11, 32) and saved.numel() == 227168 * B and arg.numel() == 46208 * B
    args = C.argmax_planes(arg, B)
    C.check_argmax(params, x, args)
    C.check_against_f64(("twin", frames, B), params, x, dy, y, grads, args)


@pytest.mark.parametrize("B,H,Cc", [(1, 84, 16), (2, 42, 32), (3, 21, 32)])
@pytest.mark.parametrize("kind", ["noise", "ties", "neg"])
def test_maxpool_twin_equals_torch_bit_for_bit(B, H, Cc, kind):
    g = torch.Generator().manual_seed(H + B)
    if kind == "noise":
        x = torch.randn((B, H, H, Cc), generator=g)
    elif kind == "ties":                                           # flat blocks and a quantised palette: exact ties everywhere
        x = torch.randint(0, 3, (B, H // 3, H // 3, Cc), generator=g).float().repeat_interleave(3, 1).repeat_interleave(3, 2)
        x = x + (torch.rand((B, H, H, Cc), generator=g) < 0.05).float()
    else:                                                          # all negative, ties at the borders and corners
        x = -torch.randint(1, 3, (B, H, H, Cc), generator=g).float()
    y, arg = host_ops.impala_maxpool_forward(x)
    ty, idx = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    Ho = (H + 1) // 2
    assert y.shape == (B, Ho, Ho, Cc) and torch.equal(y, ty.permute(0, 2, 3, 1))
    a = arg.permute(0, 3, 1, 2).long()
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Ho).view(1, 1, 1, Ho)
    assert torch.equal((2 * oy - 1 + a // 3) * H + (2 * ox - 1 + a % 3), idx)
    dy = torch.randn((B, Ho, Ho, Cc), generator=g)
    dx = host_ops.impala_maxpool_backward(dy, arg, size=H)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1))


def test_image_i_of_a_batch_is_image_i_alone():
    _, params = C.make_params(seed=4)
    x = C.make_frames("noise", 3, seed=4)
    y, _, a = host_ops.impala84_forward(x, params)
    y1, _, a1 = host_ops.impala84_forward(x[2:3].contiguous(), params)
    assert torch.equal(y[2], y1[0])
    assert all(torch.equal(p[2], q[0]) for p, q in zip(C.argmax_planes(a, 3), C.argmax_planes(a1, 1)))


def test_trunk_autograd_on_cpu_and_the_network(monkeypatch):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    torch.manual_seed(3)
    net = agents.AtariImpalaQNetwork(6)
    assert net.impala_backend == "fused"
    params = ops.impala84_params(net)
    x, dy = C.make_frames("noise", 2, seed=3), C.upstream(2, seed=4)
    y = ops.Impala84Trunk.apply(x, *params)
    assert y.shape == (2, 11, 11, 32)
    y.backward(dy)
    first = [p.grad.clone() for p in params]
    _, saved, arg = host_ops.impala84_forward(x, params)
    direct = host_ops.impala84_backward(x, params, saved, arg, dy)
    assert all(torch.equal(a, b) for a, b in zip(first, direct))
    ops.Impala84Trunk.apply(x, *params).backward(dy)                # autograd accumulates
    assert all(torch.equal(p.grad, a + a) for p, a in zip(params, first))
    with torch.no_grad():
        assert torch.equal(ops.impala84_trunk(x, params), y.detach())
    # the network: same keys / shapes as the reference's QNetwork, and the fused path agrees with the reference's lines
    keys = list(net.state_dict().keys())
    assert keys[:2] == ["network.0.conv.weight", "network.0.conv.bias"] and keys[-4:] == [
        "network.5.weight", "network.5.bias", "network.7.weight", "network.7.bias"]
    assert sum(p.numel() for p in net.parameters()) == 1090774
    nchw = x.permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        q_fused = net(nchw)
        net.impala_backend = "torch"
        q_ref = net(nchw)
    assert q_fused.shape == (2, 6) and (q_fused - q_ref).abs().max().item() <= 1e-5
    monkeypatch.setenv("MI355PPO_IMPALA", "hip")
    with pytest.raises(ValueError):
        agents.AtariImpalaQNetwork(6)


def test_refusals_leave_outputs_untouched():
    lib = _lib.load()
    B = 1
    x = torch.zeros((B, 84, 84, 4), dtype=torch.uint8)
    params = [torch.zeros(s) for s in ops.impala84_param_shapes()]
    P = (ctypes.c_void_p * 30)(*[p.data_ptr() for p in params])
    y = torch.full((B, 11, 11, 32), 7.0)
    saved = torch.full((int(lib.mi355ppo_impala84_saved_floats(B)),), 7.0)
    arg = torch.full((int(lib.mi355ppo_impala84_argmax_bytes(B)),), 9, dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for shape, ch in (((84, 84, 3), (16, 32, 32)), ((64, 64, 3), (16, 32, 32)), ((84, 42, 4), (16, 32, 32)), ((84, 84, 4), (16, 32, 64))):
        assert lib.mi355ppo_impala84_fwd_u8_cpu(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, *shape, *ch) == -1
        assert lib.mi355ppo_impala84_fwd_u8(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, *shape, *ch, ptr(saved), 1 << 40, None) == -1
    assert lib.mi355ppo_impala84_fwd_u8_cpu(ptr(x), P, ptr(y), ptr(saved), ptr(arg), 0, 84, 84, 4, 16, 32, 32) == -1
    assert lib.mi355ppo_impala84_fwd_u8(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, 84, 84, 4, 16, 32, 32, None, 0, None) == -4
    assert lib.mi355ppo_impala84_saved_floats(0) == 0 and lib.mi355ppo_impala84_workspace_bytes(-1, 1) == 0
    assert (y == 7.0).all() and (saved == 7.0).all() and (arg == 9).all()
    with pytest.raises(TypeError):                                 # the Python seam: bytes only
        ops.Impala84Trunk.apply(torch.rand((1, 84, 84, 4)), *params)
    with pytest.raises(ValueError):
        ops.Impala84Trunk.apply(torch.zeros((1, 64, 64, 4), dtype=torch.uint8), *params)
