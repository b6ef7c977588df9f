"""Shared cases of the LSTM sequence-scan tests (tests/test_lstm_seq_twins.py on the host twins, tests/test_gpu_lstm_seq.py on the
device): the reference's ``get_states`` loop (cleanrl/ppo_atari_lstm.py:140-158) on ``nn.LSTM`` in float64 as the truth, the same
loop in float32 as the yardstick, and the bar rule: the scan's error against float64 may be at most twice the f32 reference
loop's, plus a small absolute floor (norm-relative for the weight gradients)."""
import torch
import torch.nn as nn

from cleanrl_amd import ops

H = 128
DONE_PATTERNS = ("none", "all", "random20", "first", "last", "nonbinary")
# floors of the bar rule, set from the host-twin study before any GPU run: the twins' errors are 1e-7 .. 4e-7 of O(1) values
FWD_FLOOR = 2e-6          # max |h - h64|, |hT - ..|, |cT - ..|
GRAD_FLOOR = 2e-6         # max |dgx - ..|, |dh0 - ..|, |dc0 - ..| (upstream gradients are O(1))
REL_FLOOR = 1e-6          # norm-relative error of the weight / input gradients


def done_pattern(name, T, B, gen):
    if name == "none":
        return torch.zeros(T, B)
    if name == "all":
        return torch.ones(T, B)
    if name == "random20":
        return (torch.rand(T, B, generator=gen) < 0.2).float()
    if name == "first":
        d = torch.zeros(T, B)
        d[0] = 1
        return d
    if name == "last":
        d = torch.zeros(T, B)
        d[-1] = 1
        return d
    assert name == "nonbinary"
    return torch.rand(T, B, generator=gen)


def make_case(T, B, pattern, seed=0):
    """Weights as the agent initialises them (orthogonal, here with random biases so that their gradients are exercised), inputs
    of the scale the Linear(3136, 512) + ReLU trunk produces, random state and upstream gradients."""
    gen = torch.Generator().manual_seed(seed * 1000 + T * 10 + B)
    w_ih = torch.empty(4 * H, 512)
    w_hh = torch.empty(4 * H, H)
    nn.init.orthogonal_(w_ih, 1.0, generator=gen)
    nn.init.orthogonal_(w_hh, 1.0, generator=gen)
    return dict(
        x=torch.relu(torch.randn(T, B, 512, generator=gen)),
        w_ih=w_ih, w_hh=w_hh,
        b_ih=0.1 * torch.randn(4 * H, generator=gen), b_hh=0.1 * torch.randn(4 * H, generator=gen),
        h0=0.5 * torch.randn(B, H, generator=gen), c0=torch.randn(B, H, generator=gen),
        done=done_pattern(pattern, T, B, gen),
        dh=torch.randn(T, B, H, generator=gen), dhT=torch.randn(B, H, generator=gen), dcT=torch.randn(B, H, generator=gen),
    )


def reference_loop(c, dtype, on_gx=False, with_final=True):
    """The reference's loop with nn.LSTM(512, 128) in ``dtype`` and autograd through it.  ``on_gx``: the input is the case's
    f32 gx = x W_ih^T + b_ih + b_hh with W_ih := I and zero biases, so that d input = d gx (the scan's dgx).
    Returns (h, hT, cT) and the gradients {x|gx, w_ih, w_hh, b_ih, b_hh, h0, c0} of sum(h dh) [+ hT dhT + cT dcT]."""
    lstm = nn.LSTM(512, H).to(dtype)
    with torch.no_grad():
        if on_gx:
            lstm.weight_ih_l0.copy_(torch.eye(4 * H, 512))
            lstm.bias_ih_l0.zero_()
            lstm.bias_hh_l0.zero_()
            inp = gx_of(c)
        else:
            lstm.weight_ih_l0.copy_(c["w_ih"])
            lstm.bias_ih_l0.copy_(c["b_ih"])
            lstm.bias_hh_l0.copy_(c["b_hh"])
            inp = c["x"]
        lstm.weight_hh_l0.copy_(c["w_hh"])
    inp = inp.to(dtype).requires_grad_(True)
    h0 = c["h0"].to(dtype).unsqueeze(0).requires_grad_(True)
    c0 = c["c0"].to(dtype).unsqueeze(0).requires_grad_(True)
    done = c["done"].to(dtype)
    state, hs = (h0, c0), []
    for t in range(inp.shape[0]):
        keep = (1.0 - done[t]).view(1, -1, 1)
        h, state = lstm(inp[t:t + 1], (keep * state[0], keep * state[1]))
        hs.append(h)
    h = torch.cat(hs)
    loss = (h * c["dh"].to(dtype)).sum()
    if with_final:
        loss = loss + (state[0][0] * c["dhT"].to(dtype)).sum() + (state[1][0] * c["dcT"].to(dtype)).sum()
    leaves = [inp, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, h0, c0]
    g = torch.autograd.grad(loss, leaves)
    names = ("gx" if on_gx else "x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")
    grads = {n: v.detach().double() for n, v in zip(names, g)}
    grads["h0"], grads["c0"] = grads["h0"][0], grads["c0"][0]
    return (h.detach().double(), state[0][0].detach().double(), state[1][0].detach().double()), grads


def gx_of(c):
    return nn.functional.linear(c["x"], c["w_ih"], c["b_ih"] + c["b_hh"])


def max_err(a, ref):
    return (a.double().cpu() - ref).abs().max().item()


def rel_err(a, ref):
    return ((a.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def assert_bar(name, err, ref_err, floor):
    assert err <= 2.0 * ref_err + floor, f"{name}: error {err:.3e} against float64 > 2 x the f32 reference loop's {ref_err:.3e} + {floor:.0e}"


def check_scan(c, fwd, bwd, device="cpu"):
    """Forward and backward scan (``fwd(gx, w_hh, h0, c0, done, record=True)``, ``bwd(dh, dhT, dcT, rec, w_hh, done)``, the
    host_ops / ops signatures) against float64 autograd of the reference loop on the same gx, with and without dhT / dcT."""
    gx = gx_of(c)
    to = lambda t: t.to(device)  # noqa: E731
    h, hT, cT, rec = fwd(to(gx.contiguous()), to(c["w_hh"]), to(c["h0"]), to(c["c0"]), to(c["done"]), record=True)
    for with_final in (True, False):
        (h64, hT64, cT64), g64 = reference_loop(c, torch.float64, on_gx=True, with_final=with_final)
        (h32, hT32, cT32), g32 = reference_loop(c, torch.float32, on_gx=True, with_final=with_final)
        if with_final:
            for n, a, r32, r64 in (("h", h, h32, h64), ("hT", hT, hT32, hT64), ("cT", cT, cT32, cT64)):
                assert_bar(n, max_err(a, r64), max_err(r32, r64), FWD_FLOOR)
        dhT, dcT = (to(c["dhT"]), to(c["dcT"])) if with_final else (None, None)
        dgx, dh0, dc0 = bwd(to(c["dh"]), dhT, dcT, rec, to(c["w_hh"]), to(c["done"]))
        for n, a, key in (("dgx", dgx, "gx"), ("dh0", dh0, "h0"), ("dc0", dc0, "c0")):
            assert_bar(f"{n} (final grads {with_final})", max_err(a, g64[key]), max_err(g32[key], g64[key]), GRAD_FLOOR)
        dw = ops.lstm_seq_dw_hh(dgx, rec)                      # what LSTMSeq's backward returns for W_hh
        assert_bar(f"dW_hh (final grads {with_final})", rel_err(dw, g64["w_hh"]), rel_err(g32["w_hh"], g64["w_hh"]), REL_FLOOR)
    return h, hT, cT, rec


def check_lstmseq_autograd(c, lstm_seq_apply, device):
    """x -> F.linear(x, W_ih, b_ih + b_hh) -> LSTMSeq -> sum(h dh) + hT dhT + cT dcT: every gradient against float64 autograd."""
    leaves = {k: c[k].to(device).clone().requires_grad_(True) for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0")}
    gx = nn.functional.linear(leaves["x"], leaves["w_ih"], leaves["b_ih"] + leaves["b_hh"])
    h, hT, cT = lstm_seq_apply(gx, leaves["w_hh"], leaves["h0"], leaves["c0"], c["done"].to(device))
    loss = (h * c["dh"].to(device)).sum() + (hT * c["dhT"].to(device)).sum() + (cT * c["dcT"].to(device)).sum()
    loss.backward()
    (h64, hT64, cT64), g64 = reference_loop(c, torch.float64)
    (h32, _, _), g32 = reference_loop(c, torch.float32)
    assert_bar("h", max_err(h.detach(), h64), max_err(h32, h64), FWD_FLOOR)
    for k in ("x", "w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0"):
        assert_bar(f"d{k}", rel_err(leaves[k].grad, g64[k]), rel_err(g32[k], g64[k]), REL_FLOOR)


