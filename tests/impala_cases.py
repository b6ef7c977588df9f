"""Shared cases and the float64 yardstick of the IMPALA-CNN trunk kernels (csrc/impala.hip) and their host twins.

The yardstick is the reference's own modules (cleanrl_amd.agents: ConvSequence / ConvSequenceNormed, the lines of
cleanrl/ppo_procgen.py:86-124 and cleanrl/ppg_procgen.py:123-165) run functionally in float64 on the same f32 inputs.  Its max
pools take the window the kernel RECORDED (near a tie f32 and f64 may legitimately pick different maxima), so forward and
gradients are compared through the same windows; ``check_argmax`` verifies separately that every recorded argmax is a
valid maximum of its window (the first-maximum tie rule is held bit for bit against torch by the max-pool-alone tests).  Bar rule (as in lstm_cases.py / trxl_cases.py): the error
against float64 is at most twice the error of the reference's f32 torch lines plus a small floor."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from cleanrl_amd import envs as E
from cleanrl_amd.agents import PPGAgent, ProcgenAgent

# floors of the bar rule, set from the host-twin study before any GPU run (twin errors: forward 1e-7 .. 6e-7 of O(1) outputs,
# weight gradients 2e-7 .. 1e-6 norm-relative)
FWD_FLOOR = 2e-6          # max |y - y64| (outputs are O(1))
REL_FLOOR = 2e-6          # norm-relative error of each parameter gradient

INITS = ("procgen", "ppg")
FRAMES = ("noise", "flat")


def make_agent(init, seed=0):
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    torch.manual_seed(seed)
    return (ProcgenAgent if init == "procgen" else PPGAgent)(envs)


def trunk_params(agent):
    return [p for i in range(3) for p in agent.network[i].parameters()]


def make_frames(kind, B, seed=0):
    """(B, 64, 64, 3) f32 channels-last frames in [0, 1]: uniform noise, or u8 frames of flat 8x8 blocks (exact pool ties)."""
    g = torch.Generator().manual_seed(seed)
    if kind == "noise":
        return torch.rand((B, 64, 64, 3), generator=g)
    blocks = torch.randint(0, 6, (B, 8, 8, 3), generator=g).to(torch.float32) * 51.0
    x = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2)
    spots = torch.rand((B, 64, 64, 1), generator=g) < 0.02                    # a few isolated pixels break some flat regions
    x = torch.where(spots, torch.full_like(x, 255.0), x)
    return x / 255.0


def upstream(B, seed=1):
    return torch.randn((B, 8, 8, 32), generator=torch.Generator().manual_seed(seed))


def argmax_planes(arg, B):
    """The flat argmax record -> three (B, Ho, Wo, C) uint8 tensors."""
    out, o = [], 0
    for h, c in ((32, 16), (16, 32), (8, 32)):
        n = B * h * h * c
        out.append(arg[o:o + n].view(B, h, h, c))
        o += n
    return out


def _routed_pool(c, arg):
    """max_pool2d(3, 2, 1) of NCHW ``c`` through the recorded window-relative argmax (B, Ho, Wo, C)."""
    B, C, H, W = c.shape
    Ho = H // 2
    a = arg.permute(0, 3, 1, 2).long()
    oy = torch.arange(Ho).view(1, 1, Ho, 1)
    ox = torch.arange(Ho).view(1, 1, 1, Ho)
    iy, ix = 2 * oy - 1 + a // 3, 2 * ox - 1 + a % 3
    return c.flatten(2).gather(2, (iy * W + ix).flatten(2)).view(B, C, Ho, Ho)


def trunk_f64(x_nhwc, params, args=None):
    """The reference's three ConvSequences in float64 on NCHW; pools routed through ``args`` when given -> NCHW output."""
    x = x_nhwc.permute(0, 3, 1, 2).to(torch.float64)
    ps = [p.detach().to(torch.float64).requires_grad_(True) for p in params]
    for s in range(3):
        w = ps[10 * s:10 * s + 10]
        x = F.conv2d(x, w[0], w[1], padding=1)
        x = _routed_pool(x, args[s]) if args is not None else F.max_pool2d(x, 3, 2, 1)
        for b in range(2):
            h = F.conv2d(F.relu(x), w[2 + 4 * b], w[3 + 4 * b], padding=1)
            x = x + F.conv2d(F.relu(h), w[4 + 4 * b], w[5 + 4 * b], padding=1)
    return x, ps


def reference(agent, x_nhwc, dy_nhwc, args):
    """-> (y64 NHWC, grads64, y32 NHWC, grads32): float64 routed through ``args``, and the reference's f32 torch lines."""
    y64, ps = trunk_f64(x_nhwc, trunk_params(agent), args)
    y64.backward(dy_nhwc.permute(0, 3, 1, 2).to(torch.float64))
    g64 = [p.grad for p in ps]
    params = trunk_params(agent)
    for p in params:
        p.grad = None
    y32 = agent.network[:3](x_nhwc.permute(0, 3, 1, 2))
    g32 = torch.autograd.grad(y32, params, dy_nhwc.permute(0, 3, 1, 2))
    return y64.permute(0, 2, 3, 1).detach(), g64, y32.permute(0, 2, 3, 1).detach(), g32


def max_err(a, ref):
    return (a.double() - ref.double()).abs().max().item()


def rel_err(a, ref):
    return ((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


def assert_bar(name, err, ref_err, floor):
    assert err <= 2.0 * ref_err + floor, f"{name}: error {err:.3e} against float64 > 2 x the f32 reference lines' {ref_err:.3e} + {floor:.0e}"


def check_against_f64(agent, x, dy, y, grads, args):
    """y (B,8,8,32) and the 30 gradients of one kernel / twin run against the float64 yardstick, through the recorded argmax."""
    y64, g64, y32, g32 = reference(agent, x.cpu(), dy.cpu(), [a.cpu() for a in args])
    assert_bar("trunk output", max_err(y.cpu(), y64), max_err(y32, y64), FWD_FLOOR)
    names = [n for i in range(3) for n, _ in agent.network[i].named_parameters(prefix=f"network.{i}")]
    for n, g, r64, r32 in zip(names, grads, g64, g32):
        assert_bar(f"d {n}", rel_err(g.cpu(), r64), rel_err(r32, r64), REL_FLOOR)


def check_argmax(agent, x, args, tol=2e-5):
    """Each recorded argmax picks a maximum of its window: the float64 pre-pool value there is within ``tol`` (relative to the
    plane's scale) of the window's float64 maximum, and it is a valid position.  (The exact first-maximum rule on the kernel's
    own f32 values is held bit for bit by the max-pool-alone tests, whose inputs carry exact ties.)"""
    xs = x.cpu().permute(0, 3, 1, 2).to(torch.float64)
    ps = [p.detach().to(torch.float64) for p in trunk_params(agent)]
    for s in range(3):
        w = ps[10 * s:10 * s + 10]
        c = F.conv2d(xs, w[0], w[1], padding=1)
        a = args[s].cpu()
        B, Ho, Wo, C = a.shape
        ar = a.permute(0, 3, 1, 2).long()
        oy = torch.arange(Ho).view(1, 1, Ho, 1)
        ox = torch.arange(Ho).view(1, 1, 1, Ho)
        iy, ix = 2 * oy - 1 + ar // 3, 2 * ox - 1 + ar % 3
        assert bool(((iy >= 0) & (iy < 2 * Ho) & (ix >= 0) & (ix < 2 * Ho)).all()), "argmax in the padding"
        picked = _routed_pool(c, a)
        best = F.max_pool2d(c, 3, 2, 1)
        assert (best - picked).max().item() <= tol * max(1.0, c.abs().max().item())
        xs = _routed_pool(c, a)
        for b in range(2):
            h = F.conv2d(F.relu(xs), w[2 + 4 * b], w[3 + 4 * b], padding=1)
            xs = xs + F.conv2d(F.relu(h), w[4 + 4 * b], w[5 + 4 * b], padding=1)
