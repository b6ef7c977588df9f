"""Mint the PPG auxiliary-phase fixtures from the reference's own lines.

    python tools/mint_ppg_aux_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
It stores no reference text: it ``ast``-compiles ppg_procgen.py's ``flatten01`` / ``unflatten01`` and ``exec``s two blocks of the
script, located by their content -- the old-policy pass (from ``aux_pi = torch.zeros(`` to the ``del m_aux_obs`` that ends its loop)
and the body of one auxiliary minibatch (from ``m_aux_obs = aux_obs[:, aux_minibatch_ind].to(device)`` to ``loss.backward()``).

The kernels under test start at the 256 hidden features, so the blocks run on a stand-in ``agent`` whose "observations" ARE hidden
rows: ``aux_obs`` is a (T, R, 256) float tensor, ``get_pi`` is the actor on it, and ``get_pi_value_and_aux_value`` returns the actor's
``Categorical``, the critic on the detached rows and the auxiliary critic on the live rows, as the script's ``Agent`` does after its
encoder.  ``aux_obs`` is a leaf that requires grad, so the block's ``loss.backward()`` leaves d loss / d hidden in ``aux_obs.grad``.

Per case (T, n, R, A): random hidden rows, head tensors, returns, an unsorted ``cols`` as the first minibatch of ``aux_inds``; after
the old-policy pass one stored row gets a logit 120 below its maximum (so the row is no longer normalised, and one probability is
exactly zero in float32); then the minibatch block.  A float64 copy of everything runs the same lines in lockstep; the float32
reference's maximum deviation from it, per compared quantity, goes to tests/golden/ppg_aux_ref_sensitivity.json.  Writes
tests/golden/ppg_aux_cases.npz.
"""
from __future__ import annotations

import ast
import json
import os
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributions as td
import torch.nn as nn
from torch.distributions.categorical import Categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCRIPT = "ppg_procgen.py"
HIDDEN = 256
#        name          T  n  R  A   beta  accum  seed
CASES = {"t1n1a2": (1, 1, 3, 2, 1.0, 1, 11), "t3n2a15": (3, 2, 5, 15, 0.5, 2, 12), "t8n4a15": (8, 4, 8, 15, 1.0, 2, 13),
         "t5n3a30": (5, 3, 7, 30, 0.5, 1, 14)}
HEADS = ("actor_w", "actor_b", "critic_w", "critic_b", "aux_critic_w", "aux_critic_b")
COMPARED = ("scalars", "dh", "aux_pi_rows") + tuple("d_" + k for k in HEADS)


def blocks():
    L = R._read(SCRIPT)
    tree = ast.parse("\n".join(L))
    wanted = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("flatten01", "unflatten01")]
    assert len(wanted) == 2
    helpers = compile(ast.Module(body=wanted, type_ignores=[]), f"<reference:{SCRIPT}>", "exec")

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{SCRIPT}>", "exec")

    o0 = R._find(L, "aux_pi = torch.zeros(")
    o1 = R._find(L, "del m_aux_obs", o0) + 1
    m0 = R._find(L, "m_aux_obs = aux_obs[:, aux_minibatch_ind].to(device)", o1)
    m1 = R._find(L, "loss.backward()", m0) + 1
    assert "agent.get_pi(m_aux_obs).logits" in "".join(L[o0:o1]) and "td.kl_divergence(old_pi, new_pi)" in "".join(L[m0:m1])
    return helpers, block(o0, o1), block(m0, m1)


class HiddenAgent(nn.Module):
    """The three heads on rows that already are the encoder's 256 features."""

    def __init__(self, A):
        super().__init__()
        self.actor, self.critic, self.aux_critic = nn.Linear(HIDDEN, A), nn.Linear(HIDDEN, 1), nn.Linear(HIDDEN, 1)

    def get_pi(self, hidden):
        return Categorical(logits=self.actor(hidden))

    def get_pi_value_and_aux_value(self, hidden):
        return Categorical(logits=self.actor(hidden)), self.critic(hidden.detach()), self.aux_critic(hidden)


def head_tensors(agent):
    return (agent.actor.weight, agent.actor.bias, agent.critic.weight, agent.critic.bias, agent.aux_critic.weight, agent.aux_critic.bias)


def run(inp, dtype, helpers, old_block, mb_block):
    """The two reference blocks on one case's inputs in ``dtype`` -> the compared quantities (tensors of ``dtype``)."""
    T, R_, A = inp["aux_h"].shape[0], inp["aux_h"].shape[1], inp["actor_w"].shape[0]
    n = len(inp["cols"])
    agent = HiddenAgent(A).to(dtype)
    with torch.no_grad():
        for p, k in zip(head_tensors(agent), HEADS):
            p.copy_(torch.from_numpy(inp[k]).to(dtype))
    aux_obs = torch.from_numpy(inp["aux_h"]).to(dtype)
    ns = dict(torch=torch, np=np, td=td, Categorical=Categorical, agent=agent, device=torch.device("cpu"),
              args=SimpleNamespace(num_steps=T, aux_batch_rollouts=R_, num_aux_rollouts=n, beta_clone=float(inp["beta_clone"]),
                                   n_aux_grad_accum=int(inp["n_aux_grad_accum"])),
              envs=SimpleNamespace(single_action_space=SimpleNamespace(n=A)), aux_inds=inp["aux_inds"].copy(), aux_obs=aux_obs)
    exec(helpers, ns)
    # the script's aux_obs is u8 and its old-policy pass casts it to float32; the float64 lockstep keeps its rows in float64, and
    # its ``torch.zeros`` for aux_pi is float64 under the default dtype set by ``main``
    ns["aux_obs"] = _KeepDtype(aux_obs) if dtype == torch.float64 else aux_obs
    exec(old_block, ns)
    aux_pi = ns["aux_pi"]
    assert aux_pi.dtype == dtype
    out = {"aux_pi_rows": aux_pi[:, torch.from_numpy(inp["cols"])].clone()}
    t0, c0, j0 = (int(v) for v in inp["low_logit"])
    aux_pi[t0, c0, j0] = aux_pi[t0, c0].max() - 120.0
    out["aux_pi_in"] = aux_pi.clone()
    leaf = aux_obs.clone().requires_grad_()
    ns.update(aux_obs=leaf, aux_pi=aux_pi, aux_returns=torch.from_numpy(inp["aux_returns"]).to(dtype), aux_minibatch_ind=inp["cols"])
    exec(mb_block, ns)
    out["scalars"] = torch.stack([ns["kl_loss"], ns["aux_value_loss"], ns["real_value_loss"]]).detach()
    out["dh"] = ns["flatten01"](leaf.grad[:, torch.from_numpy(inp["cols"])])
    for p, k in zip(head_tensors(agent), HEADS):
        out["d_" + k] = p.grad.clone()
    return out


class _KeepDtype:
    """``aux_obs`` of the float64 lockstep: indexing returns float64 rows whose ``.to(torch.float32)`` is a no-op."""

    def __init__(self, t):
        self.t = t

    def __getitem__(self, idx):
        rows = self.t[idx]
        return SimpleNamespace(to=lambda *_a, **_k: SimpleNamespace(to=lambda *_b, **_c: rows), shape=rows.shape)


def make_inputs(T, n, R_, A, beta, accum, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: rs.standard_normal(s).astype(np.float32)
    aux_inds = rs.permutation(R_).astype(np.int64)
    cols = aux_inds[:n].copy()
    if n > 1 and (np.diff(cols) > 0).all():
        cols = cols[::-1].copy()
        aux_inds[:n] = cols
    return dict(aux_h=np.maximum(f(T, R_, HIDDEN), 0), actor_w=0.1 * f(A, HIDDEN), actor_b=0.1 * f(A), critic_w=0.1 * f(1, HIDDEN), critic_b=f(1),
                aux_critic_w=0.1 * f(1, HIDDEN), aux_critic_b=f(1), aux_returns=f(T, R_), aux_inds=aux_inds, cols=cols,
                beta_clone=np.float64(beta), n_aux_grad_accum=np.int64(accum),
                low_logit=np.array([rs.randint(T), cols[rs.randint(n)], rs.randint(A)], np.int64))


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    helpers, old_block, mb_block = blocks()
    out, sens = {}, {}
    for name, (T, n, R_, A, beta, accum, seed) in CASES.items():
        inp = make_inputs(T, n, R_, A, beta, accum, seed)
        r32 = run(inp, torch.float32, helpers, old_block, mb_block)
        torch.set_default_dtype(torch.float64)
        try:
            r64 = run(inp, torch.float64, helpers, old_block, mb_block)
        finally:
            torch.set_default_dtype(torch.float32)
        assert all(torch.isfinite(v).all() for v in r32.values()) and r32["aux_pi_in"].dtype == torch.float32
        t0, c0, j0 = (int(v) for v in inp["low_logit"])
        assert torch.softmax(r32["aux_pi_in"][t0, c0], -1)[j0] == 0.0, "the low logit must give an exactly zero probability"
        sens[name] = {k: float((r32[k].double() - r64[k]).abs().max()) for k in COMPARED}
        for k, v in inp.items():
            out[f"{name}/{k}"] = v
        out[f"{name}/aux_pi_in"] = r32["aux_pi_in"].numpy()
        for k in COMPARED:
            out[f"{name}/{k}"] = r32[k].numpy()
            out[f"{name}/{k}_f64"] = r64[k].numpy()
        print(name, sens[name])
    path = os.path.join(OUT, "ppg_aux_cases.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "ppg_aux_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
