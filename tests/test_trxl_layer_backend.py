"""``MI355PPO_TRXL=layer`` without a GPU: the switch accepts the value, refuses the ``learned`` encoding as ``fused`` does, and on CPU
tensors is the ``fused`` path bit for bit (torch dense ops around the attention's host twins)."""
import pytest
import torch

from cleanrl_amd import envs as E
from cleanrl_amd.agents import TRXL_BACKENDS, TrXLAgent
from cleanrl_amd.ppo_trxl import Args


def test_layer_backend_on_the_host(monkeypatch):
    assert TRXL_BACKENDS == ("torch", "fused", "layer")
    monkeypatch.setenv("MI355PPO_TRXL", "layer")
    args = Args(trxl_dim=64, trxl_num_layers=2, trxl_memory_length=4, trxl_positional_encoding="learned")
    with pytest.raises(ValueError, match="learned"):
        TrXLAgent(args, E.Box(0, 1, (8,)), (3, 2), 16)
    args.trxl_positional_encoding = "absolute"
    torch.manual_seed(0)
    agent = TrXLAgent(args, E.Box(0, 1, (8,)), (3, 2), 16)
    assert agent.trxl_backend == "layer" and agent.transformer.backend == "layer"
    obs, win = torch.randn(5, 8), torch.randn(5, 4, 2, 64)
    mask, idx, act = torch.rand(5, 4) < 0.6, torch.arange(4).expand(5, 4), torch.tensor([[1, 0]] * 5)
    outs = {}
    for backend in ("layer", "fused"):
        agent.trxl_backend = backend
        agent.zero_grad()
        _, lp, ent, v, mem = agent.get_action_and_value(obs, win, mask, idx, act)
        (lp.sum() + ent.sum() + v.sum()).backward()
        outs[backend] = [lp, ent, v, mem] + [p.grad.clone() for p in agent.parameters()]
    assert all(torch.equal(a, b) for a, b in zip(outs["layer"], outs["fused"]))
