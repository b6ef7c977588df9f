"""GPU tests of ``MI355PPO_TRXL=layer`` (csrc/trxl_layer.hip around csrc/trxl_attn.hip): one TransformerLayer forward and backward against
float64 on the CPU of the reference's own formulation (the ``torch`` backend's modules on an already gathered window) under the per-row
bars of tests/row_bars.py, guard bands and refusals, the pack after an in-place weight change, a teacher-forced golden iteration and a
short script run.

Bars: c = 4 for the forward and the data gradient, ``C_WGRAD`` / ``C_BIAS_GRAD`` for the reductions (row_bars' written rule; the measured
ratios are in DESIGN.md section 3.9)."""
import copy
import ctypes
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

import trxl_cases as TC
from cleanrl_amd import _lib, ops
from cleanrl_amd.agents import MemoryWindow, TrXLTransformerLayer
from guard_arena import SENTINELS, Arena, same_bits
from row_bars import C_BIAS_GRAD, C_WGRAD, row_bar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_FORWARD = C_DGRAD = 4.0
# (D, H, B, L): d = 16 below a column tile and one row; a ragged second row tile; d = 2; the script's D on three row tiles; the LDS-limit tile
SHAPES = [(64, 4, 1, 8), (64, 1, 65, 8), (128, 64, 63, 5), (384, 4, 129, 12), (512, 8, 200, 7)]
NAMES = [n.replace("attention.", "").replace("fc_projection.0", "fc_projection") for n in ops.TRXL_LAYER_PARAMS]


def _reference(layer, x, win, mask):
    """TransformerLayer.forward on one query row per sample, keeping x1 = attention + query."""
    q = x.unsqueeze(1)
    value = layer.norm_kv(win)
    att, _ = layer.attention(value, value, layer.layer_norm_q(q), mask)
    x1 = att + q
    return x1.squeeze(1), (layer.fc_projection(layer.layer_norm_attn(x1)) + x1).squeeze(1)


def _autograd(c, n, dtype):
    layer = copy.deepcopy(c.layer).to(dtype)
    x = c.x[:n].to(dtype).requires_grad_(True)
    x1, y = _reference(layer, x, c.win[:n].to(dtype), c.mask[:n])
    (y * c.w[:n].to(dtype)).sum().backward()
    return SimpleNamespace(x1=x1.detach(), y=y.detach(), grads=[x.grad] + [p.grad for p in layer.parameters()])


@functools.lru_cache(maxsize=None)
def _case(D, H, B, L):
    """Everything on the CPU, once: ``max(B, 64)`` rows of one recipe (the kernels get the first ``B``) -- orthogonal weights, biases N(0, 0.1),
    LayerNorm gamma 1 + N(0, 0.1), x ~ N(0, 1) times a per-row factor over 2^-8 --, float64 on the first ``B`` rows and torch's f32 / f64
    pair on all rows (the yardstick)."""
    rows = max(B, 64)
    torch.manual_seed(1000 * D + 10 * H + L)
    layer = TrXLTransformerLayer(D, H)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.1)
            elif p.dim() == 1:
                p.copy_(1 + 0.1 * torch.randn(D))
            else:
                torch.nn.init.orthogonal_(p)
    g = torch.Generator().manual_seed(7 * B + D)
    x = torch.randn(rows, D, generator=g) * torch.exp2(-8 * torch.rand(rows, 1, generator=g))
    memory = torch.randn(rows, L, 2, D, generator=g) * 1.5 + 0.25
    pos = torch.randint(0, L + 3, (rows, L), generator=g)
    pe = TC.positional_table(D, L + 3)
    c = SimpleNamespace(D=D, H=H, B=B, L=L, layer=layer, x=x, memory=memory, pos=pos, pe=pe, win=memory[:, :, 1] + pe[pos],
                        mask=torch.rand(rows, L, generator=g) < 0.6, w=torch.randn(rows, D, generator=g))
    c.r64 = _autograd(c, B, torch.float64)
    c.y32, c.y64 = _autograd(c, rows, torch.float32), _autograd(c, rows, torch.float64)
    return c


def _on_device(c, B, slabs=0, grad=True):
    """The layer on the first ``B`` rows through ``forward_layer`` -> (layer, x, y)."""
    layer = copy.deepcopy(c.layer).to(DEV)
    layer._layer_pack = ops.TrXLLayerPack(c.D, c.H, DEV, slabs)
    x = c.x[:B].to(DEV).requires_grad_(grad)
    win = MemoryWindow(c.memory[:B].to(DEV), torch.arange(B, device=DEV), torch.arange(c.L, device=DEV).expand(B, c.L).contiguous())
    with torch.set_grad_enabled(grad):
        y = layer.forward_layer(x, win, 1, c.pos[:B].to(DEV), c.mask[:B].to(DEV), c.pe.to(DEV))
    return layer, x, y


@pytest.mark.parametrize("D,H,B,L", SHAPES)
def test_forward_against_float64(D, H, B, L):
    c = _case(D, H, B, L)
    layer, _, y = _on_device(c, B)
    x1 = layer._layer_pack.saved(y.grad_fn.saved_tensors[4], B)["x1"]
    ratios = {"y": row_bar(f"layer forward y {D, H, B, L}", y, c.r64.y, c.y32.y, c.y64.y, c=C_FORWARD),
              "x1": row_bar(f"layer forward x1 {D, H, B, L}", x1, c.r64.x1, c.y32.x1, c.y64.x1, c=C_FORWARD)}
    print("TrXL layer forward ratios", (D, H, B, L), {k: round(v, 2) for k, v in ratios.items()})
    _, _, y0 = _on_device(c, B, grad=False)
    assert same_bits(y, y0), "the forward without a workspace gives other bits"


def _gradients(c, B, slabs):
    layer, x, y = _on_device(c, B, slabs)
    (y * c.w[:B].to(DEV)).sum().backward()
    return [x.grad] + [p.grad for p in layer.parameters()]


@pytest.mark.parametrize("D,H,B,L,slabs", [(64, 4, 2, 8, 0), (64, 1, 65, 8, 1), (128, 64, 63, 5, 0), (384, 4, 129, 12, 0), (512, 8, 200, 7, 0)])
def test_backward_against_float64_autograd(D, H, B, L, slabs):
    """``slabs`` = 1: one slab; 0: the default of 8, so 129 and 200 rows (3 and 4 slots of 64) fold more than one."""
    c = _case(D, H, B, L)
    got = _gradients(c, B, slabs)
    ratios = {}
    for name, g, r64, y32, y64 in zip(["x"] + NAMES, got, c.r64.grads, c.y32.grads, c.y64.grads):
        if g.dim() == 2:
            ratios[name] = row_bar(f"layer d {name} {D, H, B, L}", g, r64, y32, y64, c=C_DGRAD if name == "x" else C_WGRAD)
        else:
            ratios[name] = row_bar(f"layer d {name} {D, H, B, L}", g.view(1, -1), r64.view(1, -1), y32.view(1, -1), y64.view(1, -1), c=C_BIAS_GRAD)
    print("TrXL layer gradient ratios", (D, H, B, L, slabs), {k: round(v, 2) for k, v in ratios.items()})
    assert all(same_bits(a, b) for a, b in zip(got, _gradients(c, B, slabs))), "the same call twice: not the same bits"


@pytest.mark.parametrize("D,H,B", [(64, 4, 33), (512, 8, 65)])
def test_guard_bands_and_refusals(D, H, B):
    c = _case(D, H, B, 5)
    lib, L = _lib.load(), 5
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    results = []
    for sentinel in SENTINELS:
        arena = Arena(DEV, sentinel, words=1 << 24)
        pk = ops.TrXLLayerPack(D, H, DEV)
        params = [arena.input(t.detach().to(DEV), n) for n, t in zip(NAMES, c.layer.parameters())]
        grads = [arena.carve(t.shape, name="grad " + n).zero_() for n, t in zip(NAMES, params)]
        pack = pk.pack(params, out=arena.carve(lib.mi355ppo_trxl_layer_pack_bytes(D, H), torch.uint8, "pack"))
        ws = arena.carve(lib.mi355ppo_trxl_layer_workspace_bytes(B, D, H), torch.uint8, "workspace", align=16)
        x, dy = arena.input(c.x[:B].to(DEV), "x"), arena.input(c.w[:B].to(DEV), "dy")
        out = {k: arena.carve((B, D), name=k) for k in ("qt", "y", "du", "dx")}
        att = (c.memory[:B].to(DEV), 1, torch.arange(B, device=DEV), torch.arange(L, device=DEV).expand(B, L).contiguous(), c.pos[:B].to(DEV),
               c.mask[:B].to(DEV), c.pe.to(DEV), params[7], params[8])
        ops.trxl_layer_pre_forward(x, pk, pack, ws, out["qt"])
        u, stats = ops.trxl_attn_forward(*att, out["qt"].view(B, H, D // H))
        ops.trxl_layer_post_forward(x, u.view(B, D), pk, pack, ws, out["y"])
        ops.trxl_layer_post_backward(dy, pk, pack, ws, out["du"])
        dqt, _, _ = ops.trxl_attn_backward(*att, out["qt"].view(B, H, D // H), u, stats, out["du"].view(B, H, D // H))
        ops.trxl_layer_pre_backward(dqt.view(B, D), x, pk, pack, ws, out["dx"])
        ops.trxl_layer_wgrad(u.view(B, D), dqt.view(B, D), params, grads, pk, ws)
        arena.assert_guards_intact()
        results.append([t.clone() for t in list(out.values()) + grads])
    assert all(same_bits(a, b) for a, b in zip(*results)), "the results depend on what lies outside the tensors"
    # refusals, by status alone: D = 96, a short workspace, a NULL pack -- each before any launch
    y = out["y"].clone()
    post = lambda D_, pk_, wb: lib.mi355ppo_trxl_layer_post_fwd_f32(p(x), p(u), B, D_, H, pk_, p(out["y"]), p(ws), wb, None)      # noqa: E731
    assert post(96, p(pack), ws.numel()) == -1
    assert post(D, p(pack), ws.numel() - 1) == -4
    assert post(D, None, ws.numel()) == -1
    assert lib.mi355ppo_trxl_layer_post_bwd_f32(p(dy), B, D, H, p(pack), p(out["du"]), None, 0, None) == -4
    assert b"trxl_layer" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_trxl_layer_pack_bytes(96, H) == 0 and lib.mi355ppo_trxl_layer_workspace_bytes(B, 96, H) == 0
    assert same_bits(y, out["y"])


def test_the_pack_follows_an_in_place_weight_change():
    c = _case(64, 4, 33, 5)
    layer, x, y = _on_device(c, 33, grad=False)
    win = MemoryWindow(c.memory[:33].to(DEV), torch.arange(33, device=DEV), torch.arange(5, device=DEV).expand(33, 5).contiguous())
    args = (win, 1, c.pos[:33].to(DEV), c.mask[:33].to(DEV), c.pe.to(DEV))
    with torch.no_grad():
        layer.attention.queries.weight.mul_(-1.5)
        layer.fc_projection[0].weight.add_(0.25)
        y2 = layer.forward_layer(x, *args)
        layer._layer_pack = ops.TrXLLayerPack(64, 4, DEV)              # a pack made from the changed weights
        y3 = layer.forward_layer(x, *args)
    assert same_bits(y2, y3) and not same_bits(y, y2)


@pytest.mark.parametrize("name", ["vec_discrete", "vec_multidiscrete"])
def test_layer_iteration_against_the_golden(name):
    from test_trxl_script import check_fused_iteration

    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        g = TC.golden_case(name)
        recs, metrics, agent, _ = TC.replay(g, device=DEV, backend="layer", force_actions=True)
    finally:
        torch.set_num_threads(n)
    assert agent.trxl_backend == "layer" and all(m._layer_pack is not None for m in agent.transformer.transformer_layers)
    check_fused_iteration(g, recs, metrics, agent)


def test_script_runs_layer_on_the_gpu(tmp_path):
    env = dict(os.environ, MI355PPO_TRXL="layer")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", "ppo_trxl.py"), "--num-envs", "8",
           "--num-steps", "64", "--total-timesteps", "1536", "--num-minibatches", "4", "--update-epochs", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, env=env, timeout=330)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len([ln for ln in out.stdout.splitlines() if "SPS=" in ln]) == 3
