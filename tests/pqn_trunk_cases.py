"""Shared cases of the LayerNorm NatureCNN tests (tests/test_layernorm_twins.py on the host twins, tests/test_gpu_pqn_trunk.py on the
device kernels): shapes, seeded inputs, the float64 / float32 torch references on the NCHW view, the project's PQN bar per tensor, and
the guard-band runs on tests/guard_arena.py's arenas."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import guard_arena as GA

EPS = 1e-5
# (rows, C, HW): the FC layer's one row; conv3's, conv1's and conv2's row sizes -- every D, a ragged last quad tile, 70 rows = several
# workgroups of the forward and slabs of the backward; (257, 512, 1): the act-mask form over more than one slab
FWD_SHAPES = [(1, 512, 1), (3, 64, 49), (5, 32, 400), (70, 64, 81)]
BWD_SHAPES = FWD_SHAPES + [(257, 512, 1)]
AMAX_WORDS = 256


def inputs(rows, C, HW, seed=0, constant_row=False):
    g = torch.Generator().manual_seed(1000 * seed + rows + C + HW)
    z = torch.randn((rows, HW, C), generator=g) * 2.0 + 0.5
    if constant_row:
        z[rows // 2] = 1.7
    gamma = 1.0 + 0.2 * torch.randn((C, HW), generator=g)
    beta = 0.3 * torch.randn((C, HW), generator=g)
    dy = torch.randn((rows, HW, C), generator=g)
    return z, gamma, beta, dy


def nchw(t, rows, C, HW):
    """(rows, HW, C) rows -> torch's (rows, C, HW) view."""
    return t.view(rows, HW, C).permute(0, 2, 1)


def reference_fwd(z, gamma, beta, dtype):
    rows, HW, C = z.shape
    y = torch.relu(F.layer_norm(nchw(z, rows, C, HW).to(dtype), (C, HW), gamma.to(dtype), beta.to(dtype), EPS))
    return y.permute(0, 2, 1).contiguous()


def reference_bwd(z, gamma, beta, dy, dtype, mask_by_act):
    """(dz (rows, HW, C), dgamma (C, HW), dbeta (C, HW)) by autograd in ``dtype``.  ``mask_by_act``: dy is the gradient at relu's
    output; otherwise at the LayerNorm's output, already under the mask."""
    rows, HW, C = z.shape
    zz = nchw(z, rows, C, HW).to(dtype).detach().clone().requires_grad_(True)
    gg, bb = gamma.to(dtype).clone().requires_grad_(True), beta.to(dtype).clone().requires_grad_(True)
    y = F.layer_norm(zz, (C, HW), gg, bb, EPS)
    d = nchw(dy, rows, C, HW).to(dtype)
    (torch.relu(y) if mask_by_act else y).backward(d)
    return zz.grad.permute(0, 2, 1).contiguous(), gg.grad, bb.grad


def bar(name, got, ref64, ref32, floor=2e-6):
    """The project's PQN bar per tensor: the max-abs error against float64 is at most twice the error of torch's own f32
    result on the same inputs, plus floor * max |ref|."""
    got, ref64, ref32 = (t.detach().double().cpu().reshape(-1) for t in (got, ref64, ref32))
    err, own = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    print(f"{name}: error {err:.3e}, torch f32 {own:.3e}, max |ref| {ref64.abs().max().item():.3e}")
    assert err <= 2 * own + floor * ref64.abs().max().item(), f"{name}: error {err:.3e} against float64, torch's own f32 error {own:.3e}"


def packed_bits(a):
    """``a > 0`` packed as the ``*_bits`` forwards pack it: word w, bit b <-> flat element 32 w + b."""
    m = (a.reshape(-1, 32) > 0).to(torch.int64)
    w = (m << torch.arange(32, dtype=torch.int64, device=a.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def amax_value(rec):
    return float(rec.view(-1)[::16].contiguous().view(torch.float32).max().item())


def guarded_layernorm(mod, device, sentinel, rows, C, HW, act_mask):
    """Forward + backward through ``mod`` (ops / host_ops) with every tensor a carve of one arena: -> the results (copies), after
    asserting that no guard band was touched."""
    arena = GA.Arena(device, sentinel, words=1 << 22)
    z, gamma, beta, dy = inputs(rows, C, HW, seed=3)
    D = C * HW
    zi, gi, bi, di = (arena.input(t.to(device), n) for t, n in ((z, "z"), (gamma, "gamma"), (beta, "beta"), (dy, "dy")))
    a, mean, rstd = arena.carve((rows, HW, C), name="a"), arena.carve((rows,), name="mean"), arena.carve((rows,), name="rstd")
    bits = arena.carve((rows * D // 32,), torch.int32, "bits")
    rec_a, rec_dz = arena.carve((AMAX_WORDS,), torch.int32, "a_amax").zero_(), arena.carve((AMAX_WORDS,), torch.int32, "dz_amax").zero_()
    dz, dg, db = arena.carve((rows, HW, C), name="dz"), arena.carve((C, HW), name="dgamma"), arena.carve((C, HW), name="dbeta")
    return arena, (zi, gi, bi, di), (a, mean, rstd, bits, rec_a, dz, dg, db, rec_dz)


def run_guarded_layernorm(mod, device, sentinel, rows, C, HW, act_mask, monkeypatch):
    arena, (z, gamma, beta, dy), (a, mean, rstd, bits, rec_a, dz, dg, db, rec_dz) = guarded_layernorm(mod, device, sentinel, rows, C, HW, act_mask)
    with GA.exact_workspaces(monkeypatch, arena):
        arena.stage = "layernorm fwd: "
        mod.layernorm_relu_fwd(z, gamma, beta, C, HW, EPS, a, mean, rstd, bits, rec_a)
        arena.stage = "layernorm bwd: "
        mod.layernorm_relu_bwd(dy, z, mean, rstd, gamma, C, HW, act=a if act_mask else None, dz=dz, dgamma=dg, dbeta=db, amax=rec_dz)
    arena.assert_guards_intact()
    return [t.detach().cpu().clone() for t in (a, mean, rstd, bits, dz, dg, db)] + [amax_value(rec_a.cpu()), amax_value(rec_dz.cpu())]
