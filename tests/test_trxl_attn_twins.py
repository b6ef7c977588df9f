"""The TrXL memory-attention host twins (mi355ppo_trxl_attn_{fwd,bwd}_f32_cpu, through ops.TrXLMemoryAttention on CPU tensors)
against float64 autograd of a transcription of the reference's window path (tests/trxl_cases.py), plus their refusals.

The bar -- at most twice the error of the reference's own f32 ops, plus a floor of a few ulps of the result -- was set here,
on the host twins, before any device run; tests/test_gpu_trxl.py holds the kernels to the same bar."""
import pytest
import torch

import trxl_cases as C
from cleanrl_amd import _lib, host_ops, ops

SHAPES = [(D, H, L) for D in (64, 384, 512) for H in (1, 4, 8) for L in (1, 7, 119, 256)]


@pytest.mark.parametrize("D,H,L", SHAPES)
def test_twins_match_float64_reference(D, H, L):
    for mask in C.MASKS:
        for pe in ("absolute", ""):
            case = C.make_case(D, H, L, 5, mask, pe)
            e_got, e_ref, scale = C.errors(C.fused_window_attention, case)
            assert C.within_bar(e_got, e_ref, scale), (mask, pe, e_got, e_ref, scale)


def test_fully_masked_window_is_uniform():
    """Step 0 of an episode: every row masked -> the reference's -1e20 fill makes the softmax uniform over all L rows, so u is
    the mean of the normalised rows and q gets no gradient."""
    case = C.make_case(64, 4, 7, 3, "all", "absolute")
    q = case["q"].clone().requires_grad_(True)
    u = ops.TrXLMemoryAttention.apply(q, case["gamma"], case["beta"], case["memory"], case["layer"], case["ep"], case["rows"],
                                      case["pos"], case["mask"], case["pe"])
    win = case["memory"][case["ep"]][torch.arange(3)[:, None], case["rows"]][:, :, case["layer"]] + case["pe"][case["pos"]]
    y = torch.nn.functional.layer_norm(win, (64,), case["gamma"], case["beta"], 1e-5).mean(1)
    assert (u.reshape(3, 64) - y).abs().max().item() < 1e-5
    u.sum().backward()
    assert q.grad.abs().max().item() == 0.0


def test_twins_are_deterministic_and_batch_invariant():
    case = C.make_case(384, 4, 119, 9, "random", "absolute")
    args = [case[k] for k in ("memory", "layer", "ep", "rows", "pos", "mask", "pe", "gamma", "beta")]
    q = case["q"]
    u1, s1 = host_ops.trxl_attn_forward(*args, q)
    u2, s2 = host_ops.trxl_attn_forward(*args, q)
    assert torch.equal(u1, u2) and torch.equal(s1, s2)
    b = 4
    one = [args[0], args[1], args[2][b:b + 1], args[3][b:b + 1], args[4][b:b + 1], args[5][b:b + 1]] + args[6:]
    u_b, _ = host_ops.trxl_attn_forward(*one, q[b:b + 1])
    assert torch.equal(u_b[0], u1[b])


def _call(D=64, H=4, L=7, **over):
    case = C.make_case(64, 4, 7, 3, "random", "absolute")
    mem, ep, rows, pos = case["memory"], case["ep"].clone(), case["rows"].clone(), case["pos"].clone()
    if D != 64:
        mem = torch.randn(mem.shape[:3] + (D,))
    gamma, beta = torch.ones(D), torch.zeros(D)
    q = torch.randn(3, H, max(D // H, 1))
    mask = case["mask"]
    pe = torch.randn(case["pe"].shape[0], D)
    if L != 7:
        rows = torch.zeros((3, L), dtype=torch.int64)
        pos = torch.zeros((3, L), dtype=torch.int64)
        mask = torch.ones((3, L), dtype=torch.bool)
    kw = dict(memory=mem, layer=1, ep=ep, rows=rows, pos=pos, mask=mask, pe=pe, gamma=gamma, beta=beta, q=q)
    kw.update(over)
    return host_ops.trxl_attn_forward(**kw)


@pytest.mark.parametrize("D,H,L", [(96, 4, 7), (576, 4, 7), (64, 3, 7), (64, 128, 7), (64, 4, 1025)])
def test_twins_refuse_unsupported_shapes(D, H, L):
    with pytest.raises((_lib.Mi355PpoError, ValueError)):
        _call(D=D, H=H, L=L)


def test_twins_refuse_out_of_range_indices():
    case = C.make_case(64, 4, 7, 3, "random", "absolute")
    E, T = case["memory"].shape[:2]
    P = case["pe"].shape[0]
    for name, bad in (("ep", torch.tensor([0, E, 0])), ("ep", torch.tensor([-1, 0, 0])),
                      ("rows", case["rows"].clone().index_fill_(1, torch.tensor([3]), T)),
                      ("pos", case["pos"].clone().index_fill_(1, torch.tensor([0]), P))):
        with pytest.raises(_lib.Mi355PpoError, match="outside"):
            _call(**{name: bad})
    _call(pe=None, pos=torch.full((3, 7), 10 ** 6))          # without a positional encoding `pos` is not read


def test_memory_gets_no_gradient():
    case = C.make_case(64, 4, 7, 3, "tril", "absolute")
    mem = case["memory"].clone().requires_grad_(True)
    q = case["q"].clone().requires_grad_(True)
    u = ops.TrXLMemoryAttention.apply(q, case["gamma"], case["beta"], mem, 1, case["ep"], case["rows"], case["pos"], case["mask"],
                                      case["pe"])
    u.sum().backward()
    assert mem.grad is None and q.grad is not None
