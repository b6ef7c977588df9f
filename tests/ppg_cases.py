"""Case builders of the PPG auxiliary-phase tests: the minted golden cases with the project's numeric rule, seeded
random cases at the tile edges, and ``every_entry_point``, which the twin, guard-band, stream and device tests all run through
``host_ops`` or ``ops`` on plain tensors or on carves of a guard-band arena."""
import functools
import json
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = ("actor_w", "actor_b", "critic_w", "critic_b", "aux_critic_w", "aux_critic_b")
COMPARED = ("scalars", "dh", "aux_pi_rows") + tuple("d_" + k for k in HEADS)
GOLDEN_CASES = {"t1n1a2": (1, 1, 3, 2), "t3n2a15": (3, 2, 5, 15), "t8n4a15": (8, 4, 8, 15), "t5n3a30": (5, 3, 7, 30)}      # (T, n, R, A)
# one row, one below a tile of 8 rows, one exact tile, one past a tile, several tiles, many tiles
EDGE_SHAPES = ((1, 1), (7, 1), (8, 1), (3, 3), (9, 4), (64, 4))
EDGE_ACTIONS = (2, 15, 30)
HIDDEN = 256


# ---------------------------------------------------------------------------------------------- goldens and the numeric rule
@functools.lru_cache(maxsize=None)
def _golden_file():
    z = np.load(os.path.join(GOLDEN_DIR, "ppg_aux_cases.npz"))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def sensitivity():
    with open(os.path.join(GOLDEN_DIR, "ppg_aux_ref_sensitivity.json")) as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def golden(name):
    """One minted case as torch tensors (inputs, the f32 results of the reference lines, their ``_f64`` lockstep copies)."""
    g = {k.split("/", 1)[1]: v for k, v in _golden_file().items() if k.startswith(name + "/")}
    T, n, R, A = GOLDEN_CASES[name]
    assert g["aux_h"].shape == (T, R, HIDDEN) and g["cols"].shape == (n,) and g["actor_w"].shape == (A, HIDDEN)
    return {k: torch.from_numpy(v.copy()) for k, v in g.items()}


def golden_as_case(name):
    """The golden's inputs in the layout of ``case``: h are the minibatch's hidden rows in flat-row order."""
    g = golden(name)
    cols = g["cols"].contiguous()
    return dict(h=g["aux_h"].index_select(1, cols).reshape(-1, HIDDEN).contiguous(), heads=[g[k].contiguous() for k in HEADS],
                aux_pi=g["aux_pi_in"].contiguous(), aux_returns=g["aux_returns"].contiguous(), cols=cols, beta=float(g["beta_clone"]),
                accum=int(g["n_aux_grad_accum"]), low=tuple(int(v) for v in g["low_logit"]))


def assert_within_rule(name, got):
    """The project's numeric rule (tests/replay_harness.py::assert_within_sensitivity): every compared quantity's maximum deviation
    from the float64 copy is at most twice the float32 reference's own recorded deviation from it, plus 2e-6."""
    g, sens = golden(name), sensitivity()[name]
    dev = {k: float((got[k].detach().cpu().double() - g[k + "_f64"]).abs().max()) for k in got}
    print(name, {k: f"{v:.3e} (bar {2 * sens[k] + 2e-6:.3e})" for k, v in dev.items()})
    bad = {k: (v, 2 * sens[k] + 2e-6) for k, v in dev.items() if not v <= 2 * sens[k] + 2e-6}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- seeded cases
@functools.lru_cache(maxsize=None)
def case(T: int, n: int, A: int, frame=(4, 5, 3)):
    """A minibatch of n whole rollouts of T steps out of R = n + 3 stored ones, cols unsorted; one old row carries a logit 120
    below its maximum and is not normalised."""
    gen = torch.Generator().manual_seed(7000 + 97 * T + 13 * n + A)
    R, M = n + 3, T * n
    f = lambda *s: torch.randn(*s, generator=gen)
    cols = torch.randperm(R, generator=gen)[:n].contiguous()
    if n > 1 and bool((cols[1:] > cols[:-1]).all()):
        cols = cols.flip(0).contiguous()
    aux_pi = f(T, R, A)
    aux_pi = aux_pi - aux_pi.logsumexp(-1, keepdim=True)
    low = (T - 1, int(cols[0]), A - 1)
    aux_pi[low] = aux_pi[low[0], low[1]].max() - 120.0
    return dict(h=f(M, HIDDEN).relu(), heads=[0.1 * f(A, HIDDEN), 0.1 * f(A), 0.1 * f(1, HIDDEN), f(1), 0.1 * f(1, HIDDEN), f(1)],
                aux_pi=aux_pi.contiguous(), aux_returns=f(T, R), cols=cols, beta=0.5 if A % 2 else 1.0, accum=1 + (T + n) % 2, low=low,
                aux_obs=torch.randint(0, 256, (T, R) + tuple(frame), generator=gen, dtype=torch.uint8),
                prefill=[0.3 * f(A, HIDDEN), f(A), f(1, HIDDEN), f(1), f(1, HIDDEN), f(1)])


def head_shapes(A):
    return ((A, HIDDEN), (A,), (1, HIDDEN), (1,), (1, HIDDEN), (1,))


def run_gather(mod, c, put, out_of):
    obs = put(c["aux_obs"], "aux_obs")
    T, R = obs.shape[:2]
    n = c["cols"].numel()
    return mod.ppg_aux_gather(obs, put(c["cols"], "cols"), out=out_of((T * n,) + tuple(obs.shape[2:]), torch.float32, "out"))


def run_old(mod, c, put, out_of):
    """-> the written rows aux_pi[:, cols] (the rest of aux_pi is whatever it was)."""
    T, R, A = c["aux_pi"].shape
    aux_pi = out_of((T, R, A), torch.float32, "aux_pi")
    cols = put(c["cols"], "cols")
    mod.ppg_old_logits_(put(c["h"], "h"), put(c["heads"][0], "actor.weight"), put(c["heads"][1], "actor.bias"), cols, aux_pi)
    return aux_pi.index_select(1, cols).clone()


def run_aux(mod, c, put, out_of, prefill=None):
    """``prefill`` None: accumulate=0 into fresh gradients; else accumulate=1 onto these six tensors."""
    A = c["aux_pi"].shape[2]
    M = c["h"].shape[0]
    names = ("d_" + k for k in HEADS)
    if prefill is None:
        grads = [out_of(s, torch.float32, nm) for s, nm in zip(head_shapes(A), names)]
    else:
        grads = [put(t.clone(), nm) for t, nm in zip(prefill, names)]
    sc, dh = mod.ppg_aux_fwd_bwd(put(c["h"], "h"), [put(t, k) for t, k in zip(c["heads"], HEADS)], put(c["aux_pi"], "aux_pi"),
                                 put(c["aux_returns"], "aux_returns"), put(c["cols"], "cols"), c["beta"], 1.0 / c["accum"], grads,
                                 prefill is not None, scalars=out_of((3,), torch.float32, "scalars"), dh=out_of((M, HIDDEN), torch.float32, "dh"))
    out = dict(scalars=sc, dh=dh)
    out.update({"d_" + k: g for k, g in zip(HEADS, grads)})
    return out


@functools.lru_cache(maxsize=None)
def adam_case(n: int):
    gen = torch.Generator().manual_seed(900 + n)
    return dict(params=torch.randn(n, generator=gen), grads=torch.randn(n, generator=gen) * 0.3, exp_avg=torch.randn(n, generator=gen) * 0.01,
                exp_avg_sq=torch.rand(n, generator=gen) * 1e-3)


ADAM = dict(lr=5e-4, max_grad_norm=0.5, grad_scale=0.5, eps=1e-8)


def run_split(mod, c, put, out_of, n_split, step_head, step_tail):
    bufs = [put(c[k].clone(), k) for k in ("params", "grads", "exp_avg", "exp_avg_sq")]
    norm = mod.clip_adam_split_(*bufs, n_split, step_head, step_tail, ADAM["lr"], ADAM["max_grad_norm"], grad_scale=ADAM["grad_scale"],
                                eps=ADAM["eps"], total_norm_out=out_of((1,), torch.float32, "total_norm"))
    return bufs + [norm]


def run_plain_adam(mod, c, put, step):
    bufs = [put(c[k].clone(), k) for k in ("params", "grads", "exp_avg", "exp_avg_sq")]
    mod.clip_adam_(*bufs, step, ADAM["lr"], ADAM["max_grad_norm"], grad_scale=ADAM["grad_scale"], eps=ADAM["eps"])
    return bufs


# ---------------------------------------------------------------------------------------------- placement
def plain(dev):
    """(put, out_of) for ordinary tensors of ``dev``."""
    return (lambda t, name: t.to(dev).contiguous()), (lambda shape, dtype, name: torch.empty(shape, dtype=dtype, device=dev))


def carved(arena):
    """(put, out_of) for carves of a guard-band arena (tests/guard_arena.py): inputs end at their last element, outputs too."""
    return (lambda t, name: arena.input(t.contiguous(), arena.stage + name)), (lambda shape, dtype, name: arena.carve(shape, dtype, arena.stage + name))


def every_entry_point(mod, put, out_of, stage=lambda name: None, shapes=((7, 1, 2), (9, 4, 15), (3, 3, 30))):
    """Small cases of all four operators through ``mod`` -> {name: tensor}: what the guard-band tests, the stream test and the
    device-vs-twin tests compare between two runs."""
    out = {}
    for T, n, A in shapes:
        tag = f"T{T} n{n} A{A}"
        c = case(T, n, A)
        stage(f"gather {tag}")
        out[f"gather {tag}"] = run_gather(mod, c, put, out_of)
        stage(f"old {tag}")
        out[f"old {tag}"] = run_old(mod, c, put, out_of)
        for acc in (False, True):
            stage(f"aux {tag} accumulate={acc}")
            for k, v in run_aux(mod, c, put, out_of, c["prefill"] if acc else None).items():
                out[f"aux {tag} {acc} {k}"] = v
    stage("gather two column blocks")
    out["gather wide"] = run_gather(mod, case(2, 2, 2, frame=(36, 38, 3)), put, out_of)            # 4,104 bytes: 1,026 dwords
    for n, n_split in ((1001, 700), (1001, 1001), (4100, 4)):
        stage(f"split n={n} n_split={n_split}")
        for k, v in zip(("params", "grads", "exp_avg", "exp_avg_sq", "norm"), run_split(mod, adam_case(n), put, out_of, n_split, 7, 3)):
            out[f"split {n} {n_split} {k}"] = v
    return out
