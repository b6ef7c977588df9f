"""The case table of the guard-band tests (tests/guard_arena.py): one list, run on the device by test_gpu_bounds.py and, for
the entry points that have a host twin, on the CPU by test_bounds_twins.py.

A case names its entry points, builds its inputs once on the CPU (with the generators of the families' own ``*_cases`` modules)
and runs them through ``mod`` -- ``cleanrl_amd.ops`` (with ``cleanrl_amd.cnn``) or ``cleanrl_amd.host_ops``.  ``check`` runs it
three times: the ordinary way (the reference bits), then with every input, every caller-owned output, every buffer the wrapper
allocates itself and every workspace carved at its exact size out of a NaN-sentinel arena, then out of a finite-sentinel one.

Row counts: 1; one below and one above the tile / vector / group width that the kernel's source names; one that leaves the last
group or block ragged.  The reason stands beside each list.  The other dimensions: their smallest and the largest accepted.
"""
from __future__ import annotations

from collections import namedtuple

import torch

import dist_cases as D
import guard_arena as GA
import impala_cases as I
import lstm_cases as L
import offpolicy_cases as C
import pqn_cases as P
import pqn_lstm_cases as PL
import sac_cases as S
import trxl_cases as X

Case = namedtuple("Case", "name build run outs workspace twin carves twin_outs")
CASES: list = []


def case(name, outs, workspace=False, twin=False, carves=None, twin_outs=None):
    """``case(...)((build, run))`` adds one row: ``build()`` -> dict of CPU inputs, ``run(mod, dev, T, K)`` -> dict of outputs, with
    ``T`` the inputs on the device (plain or carved) and ``K`` the allocator of the caller-owned outputs (``Plain`` / ``Carved``).
    ``outs``: outputs that a kernel (or twin) writes and that the run must return -- in a carved run each of them must lie inside the
    arena; ``workspace``: the wrapper takes one from ``_workspace``; ``twin``: host_ops has it; ``carves()`` -> byte counts that the
    wrapper must have asked torch for itself on the device (a workspace it allocates without ``_workspace``); ``twin_outs``: the
    outputs held to the arena on the twin, where they are not ``outs`` (a twin whose gradients come back through autograd's own
    multiply by the upstream gradient)."""
    def deco(pair):
        build, run = pair
        CASES.append(Case(name, build, run, tuple(outs), workspace, twin, carves, twin_outs))
        return pair
    return deco


def is_twin(mod):
    return mod.__name__.endswith("host_ops")


class Plain:
    """The ordinary way: inputs are torch's own tensors on the device, outputs ``torch.empty``."""

    def __init__(self, dev):
        self.dev = dev

    def input(self, t, name=None):
        return t.to(self.dev).clone()

    def new(self, name, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.dev)

    def stage(self, name):
        pass


class Carved:
    """Inputs and caller-owned outputs carved from an arena; ``stage`` names the entry point in the carves that follow."""

    def __init__(self, arena):
        self.arena, self.dev, self._stage = arena, arena.device, ""

    def input(self, t, name=None):
        return self.arena.input(t, f"{self._stage}input {name}")

    def new(self, name, shape, dtype=torch.float32):
        return self.arena.carve(shape, dtype, f"{self._stage}output {name}")

    def stage(self, name):
        self._stage = self.arena.stage = name + ": "


def _place(v, K, name):
    if isinstance(v, torch.Tensor):
        return K.input(v, name)
    if isinstance(v, (tuple, list)) and v and all(isinstance(t, torch.Tensor) for t in v):
        return type(v)(K.input(t, f"{name}[{i}]") for i, t in enumerate(v))
    return v


_built: dict = {}


def inputs_of(c: Case):
    """The case's CPU inputs, built once and shared by every run of it (never modified: each run gets copies)."""
    if c.name not in _built:
        _built[c.name] = c.build()
    return _built[c.name]


def _modules(mod):
    import cleanrl_amd.cnn as cnn
    import cleanrl_amd.ops as ops

    return (mod,) if is_twin(mod) else (ops, cnn)


def run_plain(c: Case, mod, dev):
    K = Plain(dev)
    T = {k: _place(v, K, k) for k, v in inputs_of(c).items()}
    out = c.run(mod, dev, T, K)
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def run_carved(c: Case, mod, dev, monkeypatch, sentinel):
    """-> (outputs as CPU tensors, the arena after the run, the workspace sizes requested)."""
    words = 1 << 22
    while True:
        arena = GA.Arena(dev, sentinel, words)
        K = Carved(arena)
        try:
            with GA.exact_workspaces(monkeypatch, arena) as requested, GA.carved_allocations(monkeypatch, arena, *_modules(mod)):
                T = {k: _place(v, K, k) for k, v in inputs_of(c).items()}
                out = c.run(mod, dev, T, K)
            lo, hi = arena.buf.data_ptr(), arena.buf.data_ptr() + 4 * arena.buf.numel()
            for k in (c.twin_outs if is_twin(mod) and c.twin_outs is not None else c.outs):                     # a wrapper that allocates some other way would leave the arena, and the check, unnoticed
                assert lo <= out[k].data_ptr() and out[k].data_ptr() + out[k].numel() * out[k].element_size() <= hi, \
                    f"{c.name}: output '{k}' was not allocated from the arena"
            return {k: v.detach().cpu().clone() for k, v in out.items()}, arena, list(requested)
        except MemoryError:                      # raised by ``carve`` BEFORE the call that would not fit: start over with more room
            if words >= 1 << 29:
                raise
            words *= 4


def check(c: Case, mod, dev, monkeypatch):
    ref = run_plain(c, mod, dev)
    assert set(c.outs) <= set(ref), f"{c.name}: the run returned {sorted(ref)}, the table lists {c.outs}"
    runs = [run_carved(c, mod, dev, monkeypatch, s) for s in GA.SENTINELS]
    for (out, arena, _), s in zip(runs, GA.SENTINELS):
        hit = arena.first_touched()
        assert hit is None, f"{c.name}, sentinel 0x{s:08X}: {hit[2]}"
    for (out, _, _), s in zip(runs, GA.SENTINELS):
        for k, v in ref.items():
            assert GA.same_bits(out[k], v), (f"{c.name}, sentinel 0x{s:08X}: output '{k}' differs from the ordinary run in "
                                             f"{int((~_eq(out[k], v)).sum())} of {v.numel()} elements (a read of memory nobody wrote?)")
    if c.workspace and not is_twin(mod):
        for _, _, requested in runs:
            assert requested and max(requested) > 0, f"{c.name}: no workspace was requested"
    if c.carves is not None and not is_twin(mod):
        for _, arena, _ in runs:
            own = [n for name, _, n in arena.carves if "wrapper's own" in name]
            for nbytes in c.carves():
                assert nbytes > 0 and nbytes in own, f"{c.name}: the wrapper carved no buffer of {nbytes} bytes of its own"


def _eq(a, b):
    if a.shape != b.shape:
        return torch.zeros(b.shape, dtype=torch.bool)
    if not a.is_floating_point():
        return a == b
    return (a == b) | (a.isnan() & b.isnan())


# ================================================================================================== DDPG / TD3 (csrc/offpolicy.hip)
# kOpRows = 8 rows per tile, kOpMaxGroups = 64 weight-gradient partials: 1; 7 and 9 (one below / above a tile: a ragged only
# tile, a ragged second tile); 70 (9 tiles, every group one tile, the last ragged); 513 (65 tiles: group 0 alone has a second
# tile, and that tile holds one row).  (O, A): the smallest, the workload's, the largest (kOpMaxObs = 512, kOpMaxAct = 20).
OP_M = (1, 7, 9, 70, 513)
OP_OA = ((5, 1), (17, 6), (512, 20))


def _offpolicy(O, A, M):
    def build():
        c = C.make_case(O, A, M, N=3, slots=5)
        g = torch.Generator().manual_seed(M + O)
        pq = c.critics.numel() // 2
        Nr = min(M, 11)
        return dict(ring=c.ring, bi=c.bi, ei=c.ei, noise=c.noise, actor=c.actor, target_actor=c.target_actor, critics=c.critics,
                    target_critics=c.target_critics, qf1=c.critics[:pq].clone(), qt1=c.target_critics[:pq].clone(), scale=c.scale, bias=c.bias,
                    obs_rows=c.ring[0][c.bi[:Nr], c.ei[:Nr]].contiguous(), noise_row=c.noise[0].contiguous() * 0.1,
                    lo=torch.full((A,), -0.9), hi=torch.full((A,), 0.9), src=torch.cat([c.actor, c.critics]),
                    tgt=torch.cat([c.target_actor, c.target_critics]), step=(torch.randn((3, O), generator=g), torch.randn((3, O), generator=g),
                                                                             torch.randn((3, A), generator=g), torch.randn(3, generator=g),
                                                                             torch.ones(3)),
                    hp=c.hp, dims=(O, A, M, Nr))

    def run(mod, dev, T, K):
        O, A, M, Nr = T["dims"]
        hp, ring = T["hp"], T["ring"]
        out = {}
        K.stage("td3_target")
        y, na = K.new("next_q_value", (M,)), K.new("next_actions", (M, A))
        mod.td3_target(ring, T["bi"], T["ei"], T["target_actor"], T["target_critics"], 2, T["scale"], T["bias"], T["noise"], hp["policy_noise"],
                       hp["noise_clip"], -1.0, 1.0, hp["gamma"], y, na)
        y1 = K.new("next_q_value (ddpg)", (M,))
        mod.td3_target(ring, T["bi"], T["ei"], T["target_actor"], T["qt1"], 1, T["scale"], T["bias"], None, 0.0, 0.0, -1.0, 1.0, hp["gamma"], y1)
        out.update(y=y, next_actions=na, y_ddpg=y1)
        K.stage("td3_critic_fwd_bwd, 2 critics")
        g2, s2 = K.new("grads", (T["critics"].numel(),)), K.new("scalars", (4,))
        mod.td3_critic_fwd_bwd(ring, T["bi"], T["ei"], T["critics"], 2, y, g2, s2)
        K.stage("td3_critic_fwd_bwd, 1 critic")
        g1, s1 = K.new("grads", (T["qf1"].numel(),)), K.new("scalars", (2,))
        mod.td3_critic_fwd_bwd(ring, T["bi"], T["ei"], T["qf1"], 1, y1, g1, s1)
        out.update(critic2_grads=g2, critic2_scalars=s2, critic1_grads=g1, critic1_scalars=s1)
        K.stage("td3_actor_fwd_bwd")
        ga, la, da = K.new("grads", (T["actor"].numel(),)), K.new("actor_loss", (1,)), K.new("dq_daction", (M, A))
        mod.td3_actor_fwd_bwd(ring, T["bi"], T["ei"], T["actor"], T["qf1"], T["scale"], T["bias"], ga, la, da)
        out.update(actor_grads=ga, actor_loss=la, dq_daction=da)
        K.stage("ddpg_act")
        acts = K.new("actions", (Nr, A))
        mod.ddpg_act(T["obs_rows"], T["actor"], T["scale"], T["bias"], T["noise_row"], T["lo"], T["hi"], acts)
        K.stage("polyak_")
        mod.polyak_(T["src"], T["tgt"], 0.005)
        K.stage("replay_add")                                   # the ring is carved; the step goes into its LAST slot
        mod.replay_add(ring, ring[0].shape[0] - 1, *T["step"])
        out.update(act=acts, polyak=T["tgt"], **{f"ring{i}": t for i, t in enumerate(ring)})
        return out

    return build, run


for _O, _A in OP_OA:
    for _M in OP_M:
        case(f"offpolicy O={_O} A={_A} M={_M}",
             ("y", "next_actions", "y_ddpg", "critic2_grads", "critic2_scalars", "critic1_grads", "critic1_scalars", "actor_grads", "actor_loss",
              "dq_daction", "act", "polyak", "ring0", "ring1", "ring2", "ring3", "ring4"), workspace=True, twin=True)(_offpolicy(_O, _A, _M))


# ================================================================================================== SAC (csrc/sac.hip): the same tiles
def _sac(O, A, M):
    def build():
        c = S.make_case(O, A, M, N=3, slots=5)
        return dict(ring=c.ring, bi=c.bi, ei=c.ei, actor=c.actor, critics=c.critics, target_critics=c.target_critics, scale=c.scale, bias=c.bias,
                    eps0=c.eps[0], eps1=c.eps[1], eps2=c.eps[2], alpha=c.alpha, dense=c.ring[0][c.bi, c.ei].contiguous(),
                    state=torch.tensor([-0.3, 0.0, 0.0, 0.0, 0.0]), target_entropy=c.target_entropy, dims=(O, A, M))

    def run(mod, dev, T, K):
        O, A, M = T["dims"]
        ring, bi, ei, actor, scale, bias, alpha = T["ring"], T["bi"], T["ei"], T["actor"], T["scale"], T["bias"], T["alpha"]
        K.stage("sac_target")
        y, na, nlp = K.new("next_q_value", (M,)), K.new("next_actions", (M, A)), K.new("next_log_pi", (M,))
        mod.sac_target(ring, bi, ei, actor, T["target_critics"], scale, bias, T["eps0"], alpha, S.GAMMA, y, na, nlp)
        K.stage("sac_actor_fwd_bwd")
        ga, la, lp, dm, du = K.new("grads", (actor.numel(),)), K.new("actor_loss", (1,)), K.new("log_pi", (M,)), K.new("dmean", (M, A)), K.new("du", (M, A))
        mod.sac_actor_fwd_bwd(ring, bi, ei, actor, T["critics"], scale, bias, T["eps1"], alpha, ga, la, lp, dm, du)
        K.stage("sac_policy, ring rows")
        pi, lp1 = K.new("actions", (M, A)), K.new("log_pi", (M,))
        mod.sac_policy(ring[0], actor, scale, bias, T["eps1"], actions_out=pi, log_pi_out=lp1, batch_inds=bi, env_inds=ei)
        K.stage("sac_policy, dense rows")
        pid, lp2 = K.new("actions", (M, A)), K.new("log_pi", (M,))
        mod.sac_policy(T["dense"], actor, scale, bias, T["eps2"], actions_out=pid, log_pi_out=lp2)
        K.stage("sac_alpha_")
        s = [T["state"][i:i + 1] for i in range(5)]
        mod.sac_alpha_(lp2, T["target_entropy"], s[0], s[1], s[2], 1, 1e-3, s[3], s[4])
        return dict(y=y, next_actions=na, next_log_pi=nlp, actor_grads=ga, actor_loss=la, log_pi=lp, dmean=dm, du=du, pi=pi, log_pi_policy=lp1,
                    pi_dense=pid, log_pi2=lp2, alpha_state=T["state"])

    return build, run


for _O, _A in OP_OA:
    for _M in OP_M:
        case(f"sac O={_O} A={_A} M={_M}", ("y", "next_actions", "next_log_pi", "actor_grads", "actor_loss", "log_pi", "dmean", "du", "pi",
                                          "log_pi_policy", "pi_dense", "log_pi2", "alpha_state"), workspace=True, twin=True)(_sac(_O, _A, _M))


# ================================================================================================== PQN (csrc/pqn.hip)
# kPqnRows = 256 rows per workgroup of the fwd_bwd kernel and per weight-gradient partial: 1; 255 and 257; 600 (three partials, the
# last of 88 rows).  (O, A): (1, 1), CartPole's (4, 2), the largest (kPqnMaxObs = 64, kPqnMaxA = 18).
PQN_M = (1, 255, 257, 600)
PQN_OA = ((1, 1), (4, 2), (64, 18))


def _pqn(O, A, M):
    def build():
        g = torch.Generator().manual_seed(7 * M + O)
        B = M + 9
        T_, N = 5, max(1, min(M, 67))
        return dict(params=P.random_mlp_params(O, A, seed=M + O + A), b_obs=torch.randn((B, O), generator=g), mb=torch.randperm(B, generator=g)[:M],
                    b_actions=torch.randint(0, A, (B,), generator=g).float(), b_returns=torch.randn(B, generator=g) * 2,
                    obs=torch.randn((M, O), generator=g), rnd=torch.randint(0, A, (M,), generator=g), u=torch.rand(M, generator=g),
                    done_in=(torch.rand(M, generator=g) < 0.3).float(), rewards=torch.randn((T_, N), generator=g),
                    dones=(torch.rand((T_, N), generator=g) < 0.2).float(), values=torch.randn((T_, N), generator=g),
                    next_done=(torch.rand(N, generator=g) < 0.2).float(), next_q=torch.randn((N, A), generator=g), dims=(O, A, M, B, T_, N))

    def run(mod, dev, T, K):
        O, A, M, B, T_, N = T["dims"]
        K.stage("pqn_mlp_forward")
        q = K.new("q", (M, A))
        mod.pqn_mlp_forward(T["obs"], T["params"], A, q)
        K.stage("pqn_egreedy")
        a0, v0, i0 = K.new("actions", (M,)), K.new("values", (M,)), K.new("action_i64", (M,), torch.int64)
        mod.pqn_egreedy(q, T["rnd"], T["u"], 0.3, a0, v0, i0)
        K.stage("pqn_mlp_act")
        a1, v1, i1, orow, drow = K.new("actions", (M,)), K.new("values", (M,)), K.new("action_i64", (M,), torch.int64), K.new("obs_row", (M, O)), K.new("done_row", (M,))
        mod.pqn_mlp_act(T["obs"], T["params"], A, T["rnd"], T["u"], 0.3, a1, v1, i1, orow, T["done_in"], drow)
        K.stage("pqn_qlambda")
        ret = K.new("returns", (T_, N))
        mod.pqn_qlambda(T["rewards"], T["dones"], T["values"], T["next_done"], T["next_q"], 0.99, 0.65, ret)
        K.stage("pqn_td_loss")
        qm = K.new("q rows", (M, A))
        mod.pqn_mlp_forward(K.input(T["b_obs"][T["mb"]], "minibatch obs"), T["params"], A, qm)
        dq, sc = K.new("dq", (M, A)), K.new("scalars", (2,))
        mod.pqn_td_loss(qm, T["mb"], T["b_actions"], T["b_returns"], dq, sc)
        K.stage("pqn_mlp_td_fwd_bwd")
        grads, sc2 = K.new("grads", (T["params"].numel(),)), K.new("scalars", (2,))
        mod.pqn_mlp_td_fwd_bwd(T["b_obs"], T["mb"], T["params"], T["b_actions"], T["b_returns"], grads, A, sc2)
        return dict(q=q, eg_actions=a0, eg_values=v0, eg_i64=i0, act_actions=a1, act_values=v1, act_i64=i1, obs_row=orow, done_row=drow, returns=ret,
                    dq=dq, td_scalars=sc, grads=grads, scalars=sc2)

    return build, run


for _O, _A in PQN_OA:
    for _M in PQN_M:
        case(f"pqn O={_O} A={_A} M={_M}", ("q", "eg_actions", "eg_values", "eg_i64", "act_actions", "act_values", "act_i64", "obs_row", "done_row",
                                          "returns", "dq", "td_scalars", "grads", "scalars"), workspace=True, twin=True)(_pqn(_O, _A, _M))


# ================================================================================================== the RAdam / Adam steps (csrc/optim.hip, pqn.hip)
# 256 threads x 4 floats per pass (1,024 elements), kNormMaxBlocks = 256 norm partials: 1; 1,023 and 1,025; 262,144 + 3 elements
# (more blocks' worth than partials, the last vector ragged).
OPT_N = (1, 1023, 1025, 256 * 1024 + 3)


def _optim(n):
    def build():
        g = torch.Generator().manual_seed(n)
        return dict(p=torch.randn(n, generator=g), g=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.1,
                    n=n)

    def run(mod, dev, T, K):
        from cleanrl_amd import ops

        out = {}
        flavours = ("clip_radam_", "clip_adam_") if is_twin(mod) else ("clip_adam_", "clip_adam_sched_", "clip_radam_", "clip_radam_sched_")
        for f in flavours:
            K.stage(f)
            p, g, m, v = (K.input(T[k], k) for k in "pgmv")
            if is_twin(mod):
                norm = getattr(mod, f)(p, g, m, v, 7, 2.5e-4, 0.5)
            else:
                norm = K.new("total_norm", (1,))
                if f == "clip_adam_":
                    mod.clip_adam_(p, g, m, v, 7, 2.5e-4, 0.5, total_norm_out=norm)
                elif f == "clip_adam_sched_":
                    mod.clip_adam_sched_(p, g, m, v, K.input(torch.tensor(ops.adam_schedule(2.5e-4, 7)), "sched2"), 0.5, total_norm_out=norm)
                elif f == "clip_radam_":
                    mod.clip_radam_(p, g, m, v, 7, 2.5e-4, 0.5, total_norm_out=norm)
                else:
                    mod.clip_radam_sched_(p, g, m, v, K.input(torch.tensor(ops.radam_schedule(2.5e-4, 7)), "sched8"), 0.5, total_norm_out=norm)
            out.update({f + "p": p, f + "g": g, f + "m": m, f + "v": v, f + "norm": norm})
        return out

    return build, run


for _n in OPT_N:
    case(f"optim n={_n}", ("clip_adam_p", "clip_radam_p"), workspace=True, twin=True)(_optim(_n))


# ================================================================================================== recurrent PQN (csrc/pqn_lstm.hip)
# act: one workgroup owns E envs (lstm_rows.h: E = 1 up to 256 envs, then 2, 4, 8): 1; 255 and 257 (E = 1 | 2); 515 (E = 4, the last
# workgroup holds 3 envs); 1,027 (E = 8 from 1,025 envs on, the last workgroup holds 3).  td: 256 rows per workgroup and partial: 1;
# 255 and 257; 600.  A: 1 and the largest, 18.
PL_N = (1, 255, 257, 515, 1027)
PL_M = (1, 255, 257, 600)


def _pqn_lstm_act(N, A):
    def build():
        c = PL.make_act_case(N, A, "random20", seed=N)
        return dict(gx=c["gx"], w_hh=c["w_hh"], h0=c["h0"], c0=c["c0"], done=c["done"][0].contiguous(), wq=c["wq"], bq=c["bq"], rnd=c["rnd"], u=c["u"],
                    dims=(N, A))

    def run(mod, dev, T, K):
        N, A = T["dims"]
        H = PL.H
        K.stage("pqn_lstm_act")
        h, c, q, act, val = K.new("h", (N, H)), K.new("c", (N, H)), K.new("q", (N, A)), K.new("actions", (N,)), K.new("values", (N,))
        a64, drow = K.new("action_i64", (N,), torch.int64), K.new("done_row", (N,))
        mod.pqn_lstm_act(T["gx"], T["w_hh"], T["h0"], T["c0"], T["done"], T["wq"], T["bq"], T["rnd"], T["u"], 0.3, h_out=h, c_out=c, q_out=q,
                         actions_out=act, values_out=val, action_i64_out=a64, done_row_out=drow)
        K.stage("pqn_lstm_act, bootstrap (q only) and aliased state")
        qb = K.new("q", (N, A))
        mod.pqn_lstm_act(T["gx"], T["w_hh"], T["h0"], T["c0"], T["done"], T["wq"], T["bq"], q_out=qb)
        mod.pqn_lstm_act(T["gx"], T["w_hh"], T["h0"], T["c0"], T["done"], T["wq"], T["bq"], h_out=T["h0"], c_out=T["c0"])
        return dict(h=h, c=c, q=q, actions=act, values=val, a64=a64, done_row=drow, q_bootstrap=qb, h_alias=T["h0"], c_alias=T["c0"])

    return build, run


def _pqn_lstm_td(M, A):
    def build():
        c = PL.make_td_case(M, A, seed=M)
        return dict(h=c["h"], mb=c["mb"], b_actions=c["b_actions"], b_returns=c["b_returns"], wq=c["wq"], bq=c["bq"], dims=(M, A))

    def run(mod, dev, T, K):
        M, A = T["dims"]
        K.stage("pqn_lstm_td_fwd_bwd")
        dwq, dbq, dh, sc = K.new("dwq", (A, PL.H)), K.new("dbq", (A,)), K.new("dh", (M, PL.H)), K.new("scalars", (2,))
        mod.pqn_lstm_td_fwd_bwd(T["h"], T["mb"], T["b_actions"], T["b_returns"], T["wq"], T["bq"], dwq, dbq, dh, sc)
        return dict(dwq=dwq, dbq=dbq, dh=dh, scalars=sc)

    return build, run


for _A in (1, 18):
    for _N in PL_N:
        case(f"pqn_lstm_act N={_N} A={_A}", ("h", "c", "q", "actions", "values", "a64", "done_row", "q_bootstrap", "h_alias", "c_alias"),
             twin=True)(_pqn_lstm_act(_N, _A))
    for _M in PL_M:
        case(f"pqn_lstm_td M={_M} A={_A}", ("dwq", "dbq", "dh", "scalars"), workspace=True, twin=True)(_pqn_lstm_td(_M, _A))


# ================================================================================================== LSTM scans (csrc/lstm.hip)
# E envs per workgroup (lstm_rows.h): B = 1; 255 and 257 (E = 1 | 2, the last workgroup of 257 holds one env); 515 (E = 4, ragged);
# 1,027 (E = 8 from 1,025 envs on, the last workgroup holds 3).  T: 1 and 3 (the record's planes are T B H apart).
LSTM_TB = ((1, 1), (3, 255), (3, 257), (2, 515), (1, 1027))


def _lstm(T_, B):
    def build():
        c = L.make_case(T_, B, "random20", seed=B)
        return dict(gx=L.gx_of(c).contiguous(), w_hh=c["w_hh"], h0=c["h0"], c0=c["c0"], done=c["done"], dh=c["dh"], dhT=c["dhT"], dcT=c["dcT"])

    def run(mod, dev, T, K):
        K.stage("lstm_seq_forward, no record")
        h1, hT1, cT1, _ = mod.lstm_seq_forward(T["gx"], T["w_hh"], T["h0"], T["c0"], T["done"], record=False)
        K.stage("lstm_seq_forward")
        h, hT, cT, rec = mod.lstm_seq_forward(T["gx"], T["w_hh"], T["h0"], T["c0"], T["done"], record=True)
        K.stage("lstm_seq_backward")
        dgx, dh0, dc0 = mod.lstm_seq_backward(T["dh"], T["dhT"], T["dcT"], rec, T["w_hh"], T["done"])
        dgx2, _, _ = mod.lstm_seq_backward(T["dh"], None, None, rec, T["w_hh"], T["done"], want_dh0=False, want_dc0=False)
        out = dict(h=h, hT=hT, cT=cT, record=rec, h_norec=h1, hT_norec=hT1, cT_norec=cT1, dgx=dgx, dh0=dh0, dc0=dc0, dgx_nofinal=dgx2)
        if not is_twin(mod):
            K.stage("lstm_seq_dw_hh")
            out["dw_hh"] = mod.lstm_seq_dw_hh(dgx, rec)
        return out

    return build, run


for _T, _B in LSTM_TB:
    case(f"lstm T={_T} B={_B}", ("h", "hT", "cT", "record", "dgx", "dh0", "dc0"), twin=True)(_lstm(_T, _B))


# ================================================================================================== TrXL attention (csrc/trxl_attn.hip)
# One workgroup of kTrxlWaves = 4 waves per sample, the window dealt to the waves: B = 1 and 5; L = 1, 3 and 5 (below / above
# the four waves), 67 (ragged over 4 waves of rows).  (D, H): (64, 1) the smallest D the kernel takes, (384, 4) the workload's, (512, 8) the largest D.
TRXL = ((64, 1, 1, 1), (64, 1, 3, 5), (384, 4, 5, 5), (384, 4, 67, 3), (512, 8, 67, 2))


def _trxl(D_, H, L_, B, pe_kind):
    def build():
        c = X.make_case(D_, H, L_, B, "random", pe_kind, seed=L_ + B)
        c["mask"] = c["mask"].to(torch.uint8)
        c["pos"] = c["pos"] if c["pe"] is not None else None
        return c

    def run(mod, dev, T, K):
        a = (T["memory"], T["layer"], T["ep"], T["rows"], T["pos"], T["mask"], T["pe"], T["gamma"], T["beta"], T["q"])
        K.stage("trxl_attn_forward")
        u, stats = mod.trxl_attn_forward(*a)
        K.stage("trxl_attn_backward")
        dq, dgamma, dbeta = mod.trxl_attn_backward(*a, u, stats, T["dout"])
        return dict(u=u, stats=stats, dq=dq, dgamma=dgamma, dbeta=dbeta)

    return build, run


for _D, _H, _L, _B in TRXL:
    for _pe in ("absolute", "none"):
        case(f"trxl D={_D} H={_H} L={_L} B={_B} pe={_pe}", ("u", "stats", "dq", "dgamma", "dbeta"), twin=True)(_trxl(_D, _H, _L, _B, _pe))


# ================================================================================================== IMPALA trunk (csrc/impala.hip)
# The conv launches deal (image, band) items to workgroups and kImpMaxParts = 512 weight-gradient partials to bands: B = 1, 2 and 3
# (the pool's and the partials' per-image strides), 9 (an odd count past one band group).  saved / argmax / workspace are the
# wrapper's own allocations of exactly ``impala_saved_floats`` / ``impala_argmax_bytes`` / ``impala_workspace_bytes``.
IMPALA_B = (1, 2, 3, 9)


def _impala(B):
    def build():
        agent = I.make_agent("procgen", seed=B)
        return dict(x=I.make_frames("noise", B, seed=B), params=[p.detach().clone() for p in I.trunk_params(agent)], dy=I.upstream(B))

    def run(mod, dev, T, K):
        K.stage("impala_forward")
        y, saved, arg = mod.impala_forward(T["x"], T["params"])
        K.stage("impala_backward")
        grads = mod.impala_backward(T["x"], T["params"], saved, arg, T["dy"])
        out = dict(y=y, saved=saved, argmax=arg)
        out.update({f"grad{i}": g for i, g in enumerate(grads)})
        return out

    def carves():
        from cleanrl_amd import _lib

        lib = _lib.load()
        return [int(lib.mi355ppo_impala_workspace_bytes(B, 0)), int(lib.mi355ppo_impala_workspace_bytes(B, 1))]

    return build, run, carves


def _maxpool(B, H, C_):
    def build():
        return dict(x=torch.randn((B, H, H, C_), generator=torch.Generator().manual_seed(B + H)), dy=torch.randn((B, H // 2, H // 2, C_),
                                                                                                                 generator=torch.Generator().manual_seed(B)))

    def run(mod, dev, T, K):
        K.stage("impala_maxpool_forward")
        y, arg = mod.impala_maxpool_forward(T["x"])
        K.stage("impala_maxpool_backward")
        dx = mod.impala_maxpool_backward(T["dy"], arg)
        return dict(y=y, argmax=arg, dx=dx)

    return build, run


for _B in IMPALA_B:
    _b, _r, _c = _impala(_B)                      # (its workspace is the wrapper's own ``torch.empty``, not ``_workspace``'s)
    case(f"impala B={_B}", ("y", "saved", "argmax") + tuple(f"grad{i}" for i in range(30)), twin=True, carves=_c)((_b, _r))
for _B, _H, _C in ((1, 16, 32), (3, 64, 16), (5, 32, 32)):            # the trunk's three pools: (64, 16), (32, 32), (16, 32)
    case(f"impala_maxpool B={_B} H={_H} C={_C}", ("y", "argmax", "dx"), twin=True)(_maxpool(_B, _H, _C))


# ================================================================================================== GAE, distributions, losses, observations
# gae.hip: one thread per env column, staged in chunks of kStageFloats = 2,048 elements: N = 1; 255 and 257 (the 256-thread block);
# 2,049 (past one stage row); 2,052 (the same in whole float4s, which variant 3 needs).  T = 1 and 5.
def _gae(T_, N):
    def build():
        g = torch.Generator().manual_seed(T_ + N)
        return dict(r=torch.randn((T_, N), generator=g), d=(torch.rand((T_, N), generator=g) < 0.2).float(), v=torch.randn((T_, N), generator=g),
                    nd=(torch.rand(N, generator=g) < 0.2).float(), nv=torch.randn(N, generator=g), dims=(T_, N))

    def run(mod, dev, T, K):
        K.stage("gae")
        if is_twin(mod):
            adv, ret = mod.gae(T["r"], T["d"], T["v"], T["nd"], T["nv"], 0.99, 0.95)
            return dict(adv=adv, ret=ret)
        out = {}
        for variant in (0, 1, 6) + ((3,) if T["dims"][1] % 4 == 0 else ()):        # auto; per-column; staged; the vec4 one (N % 4 == 0)
            adv, ret = K.new("advantages", T["dims"]), K.new("returns", T["dims"])
            mod.gae(T["r"], T["d"], T["v"], T["nd"], T["nv"], 0.99, 0.95, adv, ret, variant=variant)
            out.update({f"adv{variant}": adv, f"ret{variant}": ret})
        out.update(adv=out["adv0"], ret=out["ret0"])
        return out

    return build, run


for _T, _N in ((1, 1), (5, 255), (5, 257), (3, 2049), (3, 2052)):
    case(f"gae T={_T} N={_N}", ("adv", "ret"), twin=True)(_gae(_T, _N))


# distributions.hip: a row per lane group, 256-thread blocks: B = 1; 255 and 257; 1,031 (five blocks, the last of 7 rows).  A / D: 1
# and the widest the tests of the family use (64 / 100), plus an odd one.
DIST_B = (1, 255, 257, 1031)


def _categorical(B, A):
    def build():
        x, action, g_lp, g_ent = D.categorical_case(B, A, "randn", seed=B)
        g = torch.Generator().manual_seed(B * A)
        return dict(x=x, action=action, action_f=action.float(), g_lp=g_lp, g_ent=g_ent, noise=-torch.log(torch.rand((B, A), generator=g).clamp_min(1e-30)),
                    dims=(B, A))

    def run(mod, dev, T, K):
        B, A = T["dims"]
        K.stage("categorical_sample")
        if is_twin(mod):
            a, lp, ent = mod.categorical_sample(T["x"], T["noise"])
            a2, lp2, ent2 = mod.categorical_sample(T["x"], None, seed=3, offset=5)
            lpe, ente = mod.categorical_logprob_entropy(T["x"], T["action"])
            dl = mod.categorical_logprob_entropy_bwd(T["x"], T["action"], T["g_lp"], T["g_ent"])
            return dict(a=a, lp=lp, ent=ent, a_philox=a2, lp_philox=lp2, ent_philox=ent2, lp_given=lpe, ent_given=ente, dlogits=dl)
        a, af, lp, ent = mod.categorical_sample(T["x"], T["noise"], action_f32_out=K.new("action_f32", (B,)), logprob_out=K.new("logprob", (B,)))
        a2, _, lp2, ent2 = mod.categorical_sample(T["x"], None, seed=3, offset=5)
        _, af3, lp3, _ = mod.categorical_sample(T["x"], None, seed=3, offset=5, want_entropy=False, want_i64=False)
        K.stage("categorical_logprob_entropy")
        lpe, ente = mod.categorical_logprob_entropy(T["x"], T["action"])
        lpf, entf = mod.categorical_logprob_entropy(T["x"], T["action_f"])
        K.stage("categorical_logprob_entropy backward")
        x = T["x"].detach().requires_grad_(True)
        l, e = mod.CategoricalLogProbEntropy.apply(x, T["action"])
        (dl,) = torch.autograd.grad([l, e], [x], [T["g_lp"], T["g_ent"]])
        return dict(a=a, af=af, lp=lp, ent=ent, a_philox=a2, lp_philox=lp2, ent_philox=ent2, af_lean=af3, lp_lean=lp3, lp_given=lpe, ent_given=ente,
                    lp_given_f=lpf, ent_given_f=entf, dlogits=dl)

    return build, run


def _normal(B, D_):
    def build():
        mean, logstd, action, g_lp, g_ent = D.normal_case(B, D_, seed=B)
        return dict(mean=mean, logstd=logstd, action=action, g_lp=g_lp, g_ent=g_ent, noise=torch.randn((B, D_), generator=torch.Generator().manual_seed(B)),
                    dims=(B, D_))

    def run(mod, dev, T, K):
        B, D_ = T["dims"]
        K.stage("normal_sample")
        if is_twin(mod):
            act, lp, ent = mod.normal_sample(T["mean"], T["logstd"], T["noise"])
            act2, lp2, ent2 = mod.normal_sample(T["mean"], T["logstd"], None, seed=3, offset=5)
            lpe, ente = mod.normal_logprob_entropy(T["mean"], T["logstd"], T["action"])
            dmean, drows = mod.normal_logprob_entropy_bwd(T["mean"], T["logstd"], T["action"], T["g_lp"], T["g_ent"])
            return dict(act=act, lp=lp, ent=ent, act_philox=act2, lp_philox=lp2, ent_philox=ent2, lp_given=lpe, ent_given=ente, dmean=dmean, drows=drows)
        act, lp, ent = mod.normal_sample(T["mean"], T["logstd"], T["noise"], action_out=K.new("action", (B, D_)), logprob_out=K.new("logprob", (B,)))
        act2, lp2, ent2 = mod.normal_sample(T["mean"], T["logstd"], None, seed=3, offset=5)
        K.stage("normal_logprob_entropy")
        lpe, ente = mod.normal_logprob_entropy(T["mean"], T["logstd"], T["action"])
        K.stage("normal_logprob_entropy backward")
        mean, logstd = T["mean"].detach().requires_grad_(True), T["logstd"].detach().requires_grad_(True)
        l, e = mod.NormalLogProbEntropy.apply(mean, logstd, T["action"])
        dmean, dls = torch.autograd.grad([l, e], [mean, logstd], [T["g_lp"], T["g_ent"]])
        return dict(act=act, lp=lp, ent=ent, act_philox=act2, lp_philox=lp2, ent_philox=ent2, lp_given=lpe, ent_given=ente, dmean=dmean, dlogstd=dls)

    return build, run


for _B in DIST_B:
    for _A in (1, 7, 64):
        case(f"categorical B={_B} A={_A}", ("a", "lp", "ent", "lp_given", "ent_given", "dlogits"), twin=True)(_categorical(_B, _A))
    for _D in (1, 6, 100):
        case(f"normal B={_B} D={_D}", ("act", "lp", "ent", "lp_given", "ent_given", "dmean"), twin=True)(_normal(_B, _D))


# loss.hip: 256 lanes x 4 rows per sweep (1,024 rows), kStatsMaxBlocks = 1,024 partial pairs: M = 1; 1,023 and 1,025; 2,500 (three
# sweeps, the last ragged).  A = 1 and 18; D = 1 and kMaxD = 64.  The flat batch has 4 M rows, the minibatch is a permutation's head.
LOSS_M = (1, 1023, 1025, 2500)


def _loss_categorical(M, A):
    def build():
        g = torch.Generator().manual_seed(M * 3 + A)
        Bf = 4 * M
        return dict(logits=torch.randn((M, A), generator=g), value=torch.randn(M, generator=g), mb=torch.randperm(Bf, generator=g)[:M],
                    perm=torch.randperm(Bf, generator=g), b_actions=torch.randint(0, A, (Bf,), generator=g).float(), b_logprobs=-torch.rand(Bf, generator=g) * 2,
                    b_adv=torch.randn(Bf, generator=g), b_ret=torch.randn(Bf, generator=g), b_val=torch.randn(Bf, generator=g), dims=(M, A, Bf))

    def run(mod, dev, T, K):
        M, A, Bf = T["dims"]
        b = (T["b_actions"], T["b_logprobs"], T["b_adv"], T["b_ret"], T["b_val"])
        if is_twin(mod):
            K.stage("ppo_loss_categorical twin")
            lg, vl = T["logits"].detach().requires_grad_(True), T["value"].detach().requires_grad_(True)
            loss, sc = mod.ppo_loss_categorical(lg, vl, T["mb"], *b, 0.1, 0.01, 0.5, M > 1, True)
            dl, dv = torch.autograd.grad(loss, [lg, vl])
            return dict(scalars=sc, dlogits=dl, dvalue=dv)
        mbs = max(M, 2)                                          # (the unbiased std needs two rows: M = 1 normalises nothing)
        nseg = (Bf + mbs - 1) // mbs
        K.stage("adv_stats")
        st = mod.adv_stats(T["b_adv"], T["perm"], mbs, out=K.new("stats", (nseg, 2)))
        st1 = mod.adv_stats(T["b_adv"], T["mb"] if M > 1 else K.input(T["perm"][:2], "two rows"), mbs, out=K.new("stats", (1, 2)))
        st0 = mod.adv_stats(T["b_adv"], None, Bf, out=K.new("stats", (1, 2)))
        K.stage("batch_pack")
        pack = mod.batch_pack(*b, out=K.new("pack", (Bf, 8)))
        K.stage("adv_stats_packed")
        stp = mod.adv_stats_packed(pack, T["perm"], mbs, out=K.new("stats", (nseg, 2)))
        K.stage("ppo_loss_categorical")
        sc, dl, dv = mod.ppo_loss_categorical(T["logits"], T["value"], T["mb"], *b, 0.1, 0.01, 0.5, M > 1, True, scalars_out=K.new("scalars", (7,)),
                                              dlogits_out=K.new("dlogits", (M, A)), dvalue_out=K.new("dvalue", (M,)), adv_mean_den=st1[0] if M > 1 else None)
        K.stage("ppo_loss_categorical_packed")
        scp, dlp, dvp = mod.ppo_loss_categorical_packed(T["logits"], T["value"], T["mb"], pack, 0.1, 0.01, 0.5, M > 1, False,
                                                        scalars_out=K.new("scalars", (7,)), dlogits_out=K.new("dlogits", (M, A)),
                                                        dvalue_out=K.new("dvalue", (M,)), adv_mean_den=st1[0] if M > 1 else None)
        K.stage("loss_scalars (the deferred fold of two slots)")
        slots = mod.LossSlots(2, dev)                            # (its buffer is the wrapper's own ``torch.empty`` of 2 strides)
        for k in (0, 1):
            mod.ppo_loss_categorical(T["logits"], T["value"], T["mb"], *b, 0.1, 0.01, 0.5, M > 1, k == 0, dlogits_out=K.new("dlogits", (M, A)),
                                     dvalue_out=K.new("dvalue", (M,)), adv_mean_den=st1[0] if M > 1 else None, slot=(slots, k))
        folded = slots.fold(2, K.new("scalar table", (2, 7)))
        return dict(stats=st, stats_mb=st1, stats_all=st0, pack=pack, stats_packed=stp, scalars=sc, dlogits=dl, dvalue=dv, scalars_packed=scp,
                    dlogits_packed=dlp, dvalue_packed=dvp, folded=folded)

    return build, run


def _loss_normal(M, D_):
    def build():
        c = D.loss_normal_case(M, D_, seed=M)
        c["dims"] = (M, D_)
        return c

    def run(mod, dev, T, K):
        M = T["dims"][0]
        b = (T["b_actions"], T["b_logprobs"], T["b_advantages"], T["b_returns"], T["b_values"])
        K.stage("ppo_loss_normal")
        if is_twin(mod):
            mu, ls, vl = (T[k].detach().requires_grad_(True) for k in ("new_mean", "logstd", "new_value"))
            loss, sc = mod.ppo_loss_normal(mu, ls, vl, T["mb_inds"], *b, D.CLIP, 0.01, D.VF, M > 1, True)
            dm, dls, dv = torch.autograd.grad(loss, [mu, ls, vl])
            return dict(scalars=sc, dmean=dm, dlogstd=dls, dvalue=dv)
        sc, dm, dls, dv = mod.ppo_loss_normal(T["new_mean"], T["logstd"], T["new_value"], T["mb_inds"], *b, D.CLIP, 0.01, D.VF, M > 1, True,
                                              scalars_out=K.new("scalars", (7,)))
        return dict(scalars=sc, dmean=dm, dlogstd=dls, dvalue=dv)

    return build, run


for _M in LOSS_M:
    for _A in (1, 18):
        case(f"loss_categorical M={_M} A={_A}", ("scalars", "dlogits", "dvalue"), workspace=True, twin=True, twin_outs=("scalars",))(_loss_categorical(_M, _A))
    for _D in (1, 64):
        case(f"loss_normal M={_M} D={_D}", ("scalars", "dmean", "dlogstd", "dvalue"), workspace=True, twin=True, twin_outs=("scalars",))(_loss_normal(_M, _D))


# obs.hip: 16-byte vectors, kObsUnroll = 4 of them per lane: rows of 1 pixel (4 bytes), 15 and 20 pixels (an odd count: the relayout's
# generic path; whole quads past one vector), 84 x 84 (the workload's), 4 (one quad); 1, 3 and 257 rows (one row; a ragged few;
# past one 256-thread block).  (1, 2, 2) is the one-row case of obs_shift_append_u8, which takes whole pixel quads only.
def _obs(rows, H, W):
    def build():
        g = torch.Generator().manual_seed(rows + H + W)
        R = rows + 3
        return dict(src=torch.randint(0, 256, (R, H, W, 4), dtype=torch.uint8, generator=g), inds=torch.randperm(R, generator=g)[:rows],
                    nchw=torch.randint(0, 256, (rows, 4, H, W), dtype=torch.uint8, generator=g),
                    newest=torch.randint(0, 256, (rows, H, W), dtype=torch.uint8, generator=g), dims=(rows, H, W, R))

    def run(mod, dev, T, K):
        rows, H, W, R = T["dims"]
        K.stage("obs_u8_to_f32")
        if is_twin(mod):
            return dict(f32=mod.obs_u8_to_f32(T["src"], T["inds"]), f32_all=mod.obs_u8_to_f32(T["src"], None, scale_255=False))
        f = mod.obs_u8_to_f32(T["src"], T["inds"], out=K.new("out", (rows, H, W, 4)))
        fa = mod.obs_u8_to_f32(T["src"], None, out=K.new("out", (R, H, W, 4)), scale_255=False)
        K.stage("obs_nchw_to_nhwc_u8")
        hwc = mod.obs_nchw_to_nhwc_u8(T["nchw"], out=K.new("out", (rows, H, W, 4), torch.uint8))
        out = dict(f32=f, f32_all=fa, nhwc=hwc)
        if H * W % 4 == 0:                                       # (the delta store takes whole pixel quads only)
            K.stage("obs_shift_append_u8")
            out["shifted"] = mod.obs_shift_append_u8(hwc, T["newest"], K.new("out", (rows, H, W, 4), torch.uint8))
        return out

    return build, run


for _rows, _H, _W in ((1, 1, 1), (1, 2, 2), (3, 3, 5), (257, 4, 5), (3, 84, 84), (257, 2, 2)):
    case(f"obs rows={_rows} H={_H} W={_W}", ("f32", "f32_all"), twin=True)(_obs(_rows, _H, _W))


# ================================================================================================== the fused MLP agents (csrc/mlp.hip), device only
# Narrow kernels: up to 64 rows per block; wide ones (O > 32 or n_out > 8): kWideRows = 32.  B / M = 1; 63 and 65; 31 and 33 for the
# wide tile; 200 (ragged last block of either).  rows_per_block 0 (the library's pick) and 16.  (O, n_out): (1, 1), (4, 2) narrow,
# (376, 17) the wide workload, (512, 20) the largest.
MLP_ROWS = (1, 31, 33, 63, 65, 200)
MLP_ON = ((1, 1), (4, 2), (376, 17), (512, 20))


def _mlp_shell(O, n):
    """The agent's Sequential with uninitialised parameters (``MlpNetPtrs`` reads its structure; the values are set by the caller)."""
    with torch.device("meta"):
        seq = torch.nn.Sequential(torch.nn.Linear(O, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(), torch.nn.Linear(64, n))
    return seq


def _mlp_params(O, n, g):
    """Linear's default initialisation from a generator of its own: the global RNG is left alone."""
    out = []
    for fan_in, fan_out in ((O, 64), (64, 64), (64, n)):
        b = 1.0 / fan_in ** 0.5
        out += [(torch.rand((fan_out, fan_in), generator=g) * 2 - 1) * b, (torch.rand(fan_out, generator=g) * 2 - 1) * b]
    return out


def _mlp(O, nout, M):
    def build():
        g = torch.Generator().manual_seed(M * 5 + O)
        Bf = M + 5
        return dict(actor=_mlp_params(O, nout, g), critic=_mlp_params(O, 1, g),
                    obs=torch.randn((M, O), generator=g), b_obs=torch.randn((Bf, O), generator=g), mb=torch.randperm(Bf, generator=g)[:M],
                    noise1=-torch.log(torch.rand((M, nout), generator=g).clamp_min(1e-30)), noise=torch.randn((M, nout), generator=g),
                    logstd=torch.randn(nout, generator=g) * 0.3, a_cat=torch.randint(0, nout, (Bf,), generator=g).float(),
                    a_nrm=torch.randn((Bf, nout), generator=g), b_lp=-torch.rand(Bf, generator=g) * 2, b_adv=torch.randn(Bf, generator=g),
                    b_ret=torch.randn(Bf, generator=g), b_val=torch.randn(Bf, generator=g), dims=(O, nout, M, Bf))

    def run(mod, dev, T, K):
        O, nout, M, Bf = T["dims"]
        nets = []
        for name, n in (("actor", nout), ("critic", 1)):
            seq = _mlp_shell(O, n)
            for (pname, _), t in zip(list(seq.named_parameters()), T[name]):
                mod_, attr = seq.get_submodule(pname.rsplit(".", 1)[0]), pname.rsplit(".", 1)[1]
                setattr(mod_, attr, torch.nn.Parameter(t))
                getattr(mod_, attr).grad = K.new(f"{name} grad", tuple(t.shape)).zero_()
            nets.append(mod.MlpNetPtrs(seq))
        actor, critic = nets
        out = {}
        K.stage("mlp_forward")
        out["logits"], out["value"] = mod.mlp_forward(T["obs"], actor, critic, K.new("actor_out", (M, nout)), K.new("value", (M,)))
        K.stage("mlp_act_categorical")
        r = mod.mlp_act_categorical(T["obs"], actor, critic, T["noise1"], action_f32_out=K.new("action_f32", (M,)), logprob_out=K.new("logprob", (M,)),
                                    value_out=K.new("value", (M,)), want_entropy=True, want_logits=True)
        out.update({f"cat{i}": t for i, t in enumerate(r)})
        r = mod.mlp_act_categorical(T["obs"], actor, critic, None, seed=3, offset=9, want_i64=False)
        out.update({f"cat_lean{i}": t for i, t in enumerate(r) if t is not None})
        K.stage("mlp_act_normal")
        r = mod.mlp_act_normal(T["obs"], actor, critic, T["logstd"], T["noise"], action_out=K.new("action", (M, nout)), logprob_out=K.new("logprob", (M,)),
                               value_out=K.new("value", (M,)), want_entropy=True, want_mean=True)
        out.update({f"nrm{i}": t for i, t in enumerate(r)})
        b = (T["b_lp"], T["b_adv"], T["b_ret"], T["b_val"])
        for rpb in (0, 16):
            K.stage(f"mlp_ppo_fwd_bwd categorical, rows_per_block={rpb}")
            out[f"ppo_cat_scalars{rpb}"] = mod.mlp_ppo_fwd_bwd(T["b_obs"], T["mb"], actor, critic, T["a_cat"], *b, 0.2, 0.01, 0.5, norm_adv=M > 1,
                                                               scalars_out=K.new("scalars", (7,)), rows_per_block=rpb)
            K.stage(f"mlp_ppo_fwd_bwd normal, rows_per_block={rpb}")
            lg = K.new("logstd grad", (nout,)).zero_()
            out[f"ppo_nrm_scalars{rpb}"] = mod.mlp_ppo_fwd_bwd(T["b_obs"], T["mb"], actor, critic, T["a_nrm"], *b, 0.2, 0.01, 0.5, norm_adv=M > 1,
                                                               scalars_out=K.new("scalars", (7,)), logstd=T["logstd"], logstd_grad=lg, rows_per_block=rpb)
            out[f"logstd_grad{rpb}"] = lg
        for name, net in (("actor", actor), ("critic", critic)):
            out.update({f"{name}_grad{i}": t.grad for i, t in enumerate(net.tensors)})
        return out

    return build, run


for _O, _n in MLP_ON:
    for _M in MLP_ROWS:
        case(f"mlp O={_O} n_out={_n} M={_M}", ("logits", "value", "ppo_cat_scalars0", "ppo_nrm_scalars16", "actor_grad0", "critic_grad5"),
             workspace=True)(_mlp(_O, _n, _M))


# ================================================================================================== synth_continuous_step, device only
# Eight envs per 256-thread block, one half-wave each: N = 1; 8 and 9; 300 (38 blocks, the last of 4 envs).
def _synth(N, O, Dm):
    def build():
        g = torch.Generator().manual_seed(N + O)
        return dict(state=torch.randn((N, O), generator=g), reset=torch.randn((N, O), generator=g), At=torch.randn((O, O), generator=g) * 0.3,
                    Bm=torch.randn((Dm, O), generator=g), w=torch.randn(O, generator=g), noise=torch.randn((3, N, O), generator=g) * 0.1,
                    steps=torch.full((N,), 3.0), action=torch.randn((N, Dm), generator=g) * 1.5, dims=(N, O, Dm))

    def run(mod, dev, T, K):
        N, O, Dm = T["dims"]
        K.stage("synth_continuous_step")
        obs, rew, done = K.new("obs", (N, O)), K.new("reward", (N,)), K.new("done", (N,))
        mod.synth_continuous_step(T["state"], T["reset"], T["At"], T["Bm"], T["w"], T["noise"], 4, T["steps"], 5.0, T["action"], obs, rew, done)
        mod.synth_continuous_step(T["state"], T["reset"], T["At"], T["Bm"], T["w"], T["noise"], 5, T["steps"], 5.0, T["action"], T["state"], rew, done)
        return dict(state=T["state"], steps=T["steps"], obs=obs, reward=rew, done=done)

    return build, run


for _N in (1, 8, 9, 300):
    for _O, _D in ((1, 1), (17, 6), (32, 8)):
        case(f"synth N={_N} O={_O} D={_D}", ("state", "steps", "obs", "reward", "done"))(_synth(_N, _O, _D))


# ================================================================================================== cnn.py's workspace users, device only
# conv weight gradient (layers 1-3), the FC forward in its K-split workspace form, the FC weight gradient, the heads' backward with
# and without the ReLU variant.  Images / rows: 1; 31 and 33 (kernel tiles of 32 rows / pixels); 130 (ragged past the 128-row wave
# tiles of kernel W).
CNN_ROWS = (1, 31, 33, 130)


def _cnn_wgrad(layer, images):
    def build():
        import cleanrl_amd.cnn as cnn

        cin, cout, k, _, hin, hout = cnn.LAYERS[layer]
        g = torch.Generator().manual_seed(layer * 100 + images)
        src = torch.randint(0, 256, (images + 2, 84, 84, 4), dtype=torch.uint8, generator=g) if layer == 1 else torch.relu(torch.randn((images, hin, hin, cin), generator=g))
        return dict(src=src, inds=torch.randperm(images + 2, generator=g)[:images] if layer == 1 else None,
                    dz=torch.randn((images, hout, hout, cout), generator=g), dims=(cout, cin, k))

    def run(mod, dev, T, K):
        import cleanrl_amd.cnn as cnn

        cout, cin, k = T["dims"]
        K.stage(f"conv_wgrad layer {layer}")
        dW, db = cnn.conv_wgrad(T["src"], T["dz"], layer, T["inds"], out=(K.new("dW", (cout, cin, k, k)), K.new("db", (cout,))))
        return dict(dW=dW, db=db)

    return build, run


def _cnn_fc(M, A):
    def build():
        g = torch.Generator().manual_seed(M + A)
        return dict(a=torch.relu(torch.randn((M, 3136), generator=g)), W=torch.randn((512, 3136), generator=g) * 0.02, bias=torch.randn(512, generator=g) * 0.1,
                    dz=torch.randn((M, 512), generator=g), Wa=torch.randn((A, 512), generator=g) * 0.05, ba=torch.randn(A, generator=g) * 0.1,
                    Wc=torch.randn((1, 512), generator=g) * 0.05, bc=torch.randn(1, generator=g), dlogits=torch.randn((M, A), generator=g),
                    dvalue=torch.randn((M, 1), generator=g), noise1=-torch.log(torch.rand((M, A), generator=g).clamp_min(1e-30)),
                    a_small=torch.randn((M, 64), generator=g), W_small=torch.randn((64, 64), generator=g), dims=(M, A))

    def run(mod, dev, T, K):
        import cleanrl_amd.cnn as cnn

        M, A = T["dims"]
        T["Wt"] = K.input(T["W"].t().contiguous(), "W transposed")
        if M * 3136 % 32 == 0:
            T["a_bits"] = K.input(_mask_bits(T["a"]), "a's mask bits")
        K.stage("fc_pack")
        pack = cnn.fc_pack(T["W"])
        K.stage("fc_fwd_relu_packed (workspace form)")
        assert cnn.fc_heads_act_supported_rows(M), "these row counts take the K-split route, whose partials live in the workspace"
        h = cnn.fc_fwd_relu_packed(T["a"], pack, T["bias"], 512, out=K.new("out", (M, 512)))
        K.stage("fc_wgrad")
        dWfc = cnn.fc_wgrad(T["dz"], T["a"], out=K.new("out", (512, 3136)))
        dWhwc = cnn.fc_wgrad(T["dz"], T["a"], hwc_channels=64, out=K.new("out", (512, 3136)))
        K.stage("heads forward / backward")
        hh, Wa, ba, Wc, bc = (t.detach().requires_grad_(True) for t in (h, T["Wa"], T["ba"], T["Wc"], T["bc"]))
        logits, value = cnn.HeadsFn.apply(hh, Wa, ba, Wc, bc)
        grads = torch.autograd.grad([logits, value], [hh, Wa, ba, Wc, bc], [T["dlogits"], T["dvalue"]])
        K.stage("heads backward, ReLU variant")
        bufs = _HeadsBufs(K)
        logits2, value2 = cnn.HeadsFn.apply(hh, Wa, ba, Wc, bc, bufs)
        grads2 = torch.autograd.grad([logits2, value2], [hh, Wa, ba, Wc, bc], [T["dlogits"], T["dvalue"]])
        out = dict(pack=pack, h=h, dW_fc=dWfc, dW_fc_hwc=dWhwc, logits=logits, value=value, dbh=bufs.fc_dz_from_heads[1])
        out.update({f"heads_grad{i}": t for i, t in enumerate(grads)})
        out.update({f"heads_relu_grad{i}": t for i, t in enumerate(grads2)})
        rec = lambda name, x=None: _amax(cnn, K, name, x)  # noqa: E731
        K.stage("fc_heads_act_categorical")
        a64, af, lp, val = cnn.fc_heads_act_categorical(T["a"], pack, T["bias"], T["Wa"], T["ba"], T["Wc"].view(-1), T["bc"], 3, 11,
                                                        action_f32_out=K.new("action_f32", (M,)), logprob_out=K.new("logprob", (M,)),
                                                        value_out=K.new("value", (M,)), noise_exp1=T["noise1"])
        out.update(act_i64=a64, act_f32=af, act_logprob=lp, act_value=val)
        K.stage("fc_dgrad_mask_packed / maskbits")               # B = the transposed weight (3136, 512); the mask is a's sign
        packT = cnn.fc_pack(T["Wt"])
        out["da"] = cnn.fc_dgrad_mask_packed(T["dz"], packT, T["a"], out=K.new("da", (M, 3136)))
        if M * 3136 % 32 == 0:
            out["da_bits"] = cnn.fc_dgrad_mask_packed(T["dz"], packT, T["a"], out=K.new("da", (M, 3136)), bits=T["a_bits"])
        K.stage("f16x2: absmax, fc_pack_f16x2")
        a_rec, dz_rec = rec("a", T["a"]), rec("dz", T["dz"])
        pack16 = cnn.fc_pack_f16x2(T["W"], rec("W", T["W"]))
        pack16T = cnn.fc_pack_f16x2(T["Wt"])
        K.stage("fc_fwd_relu_packed f16x2 (workspace form)")
        out["h16"] = cnn.fc_fwd_relu_packed(T["a"], pack16, T["bias"], 512, out=K.new("out", (M, 512)), amax=(a_rec, None))
        K.stage("fc_heads_act_categorical f16x2")
        r = cnn.fc_heads_act_categorical(T["a"], pack16, T["bias"], T["Wa"], T["ba"], T["Wc"].view(-1), T["bc"], 3, 11, want_i64=False, amax=a_rec)
        out.update(act16_f32=r[1], act16_logprob=r[2], act16_value=r[3])
        K.stage("fc_dgrad_packed f16x2")
        da_rec = rec("da")
        out["da16"] = cnn.fc_dgrad_mask_packed(T["dz"], pack16T, T["a"], out=K.new("da", (M, 3136)), amax=(dz_rec, da_rec))
        if M * 3136 % 32 == 0:
            out["da16_bits"] = cnn.fc_dgrad_mask_packed(T["dz"], pack16T, T["a"], out=K.new("da", (M, 3136)), bits=T["a_bits"], amax=(dz_rec, None))
        K.stage("fc_wgrad f16x2")
        out["dW_fc16"] = cnn.fc_wgrad(T["dz"], T["a"], hwc_channels=64, out=K.new("out", (512, 3136)), amax=(dz_rec, a_rec))
        K.stage("heads_bwd_relu_amax")
        bufs16 = _HeadsBufs(K, rec("dz from the heads"))
        logits3, value3 = cnn.HeadsFn.apply(hh, Wa, ba, Wc, bc, bufs16)
        grads3 = torch.autograd.grad([logits3, value3], [hh, Wa, ba, Wc, bc], [T["dlogits"], T["dvalue"]])
        out.update({f"heads_amax_grad{i}": t for i, t in enumerate(grads3)})
        out.update(pack_t=packT, pack16=pack16, pack16_t=pack16T, a_rec=a_rec, dz_rec=dz_rec, da_rec=da_rec, dh_rec=bufs16.rec, dbh16=bufs16.fc_dz_from_heads[1])
        # the whole-K route of the plain forward: shapes whose fc_fwd_workspace_bytes is 0 (N = 64; K = 16, one k-step, and 64)
        K.stage("fc_fwd_relu_packed (whole K, no workspace)")
        for Kd in (16, 64):
            assert cnn._lib.load().mi355ppo_fc_fwd_workspace_bytes(M, 64, Kd) == 0
            a_s, W_s = K.input(T["a_small"][:, :Kd].contiguous(), "a"), K.input(T["W_small"][:, :Kd].contiguous(), "B")
            out[f"h_whole_k{Kd}"] = cnn.fc_fwd_relu_packed(a_s, cnn.fc_pack(W_s), K.input(T["bias"][:64].clone(), "bias"), 64, out=K.new("out", (M, 64)))
        return out

    return build, run


class _HeadsBufs:
    """What ``HeadsFn.backward`` asks of the trunk's buffers for its ReLU variant: the padded-pitch dz rows, nothing else."""
    direct_grads = False
    fc_dz_from_heads = None

    def __init__(self, K, rec=None):
        self.K, self.rec = K, rec              # ``rec``: the amax record of dz -> the f16 form, mi355ppo_heads_bwd_relu_amax_f32

    def fc_dz(self, M, H, dev):
        from cleanrl_amd.cnn import FC_PAD

        return self.K.new("dz rows, padded pitch", (M, H + FC_PAD))[:, :H]

    def f16(self, h):
        return self.rec is not None

    def has_pass(self, M, dev):
        return self.rec is not None

    def owns(self, idx, t):
        return self.rec


def _amax(cnn, K, name, x=None):
    """A zeroed amax record carved from the arena; with ``x``, holding ``max |x|`` (``absmax``)."""
    rec = K.new(f"amax record of {name}", (cnn.AMAX_WORDS,), torch.int32).zero_()
    return rec if x is None else cnn.absmax(x, rec)


def _mask_bits(a):
    """``a > 0`` as the ``*_bits`` forwards write it: bit b of word w <-> flat element 32 w + b."""
    w = ((a.reshape(-1, 32) > 0).to(torch.int64) << torch.arange(32, device=a.device)).sum(1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


for _layer in (1, 2, 3):
    for _images in CNN_ROWS:
        case(f"cnn conv_wgrad layer={_layer} images={_images}", ("dW", "db"), workspace=True)(_cnn_wgrad(_layer, _images))
for _M, _A in ((1, 1), (31, 6), (33, 18), (130, 6)):
    case(f"cnn fc/heads M={_M} A={_A}", ("h", "dW_fc", "dW_fc_hwc", "logits", "value", "heads_grad0", "heads_relu_grad0", "dbh"), workspace=True)(_cnn_fc(_M, _A))


# ================================================================================================== the Nature-CNN convolutions, device only
# Forward, data gradient and the weight packs of every route: the f32-pipe kernels (conv.hip), kernel Q (conv1q.hip), kernel Z / R
# on the packs (gemmz.hip, convr.hip) plain, with mask bits and on the f16 split, the fused pack launches.  A GEMM row is an output
# pixel: 1 image (400 / 81 / 49 rows: ragged against the 32- and 64-row tiles); 3 (a ragged few); 16 (kernel V's / U's multiple of
# 16 images); 33 (one past two of them: 1,617 rows of layer 3).
NATURE_IMAGES = (1, 3, 16, 33)


def _nature(images):
    def build():
        g = torch.Generator().manual_seed(images)
        r = lambda *s_: torch.randn(s_, generator=g)  # noqa: E731
        return dict(obs=torch.randint(0, 256, (images + 2, 84, 84, 4), dtype=torch.uint8, generator=g), inds=torch.randperm(images + 2, generator=g)[:images],
                    W1=r(32, 4, 8, 8) * 0.06, b1=r(32) * 0.1, W2=r(64, 32, 4, 4) * 0.04, b2=r(64) * 0.1, W3=r(64, 64, 3, 3) * 0.04, b3=r(64) * 0.1,
                    Wfc=r(512, 3136) * 0.02, dz3=r(images, 7, 7, 64), dz2=r(images, 9, 9, 64), dz1=r(images, 20, 20, 32), n=images)

    def run(mod, dev, T, K):
        import cleanrl_amd.cnn as cnn
        from cleanrl_amd.ops import _launch, _ptr

        n, lib = T["n"], cnn._lib.load()
        obs, inds, W, b = T["obs"], T["inds"], {l: T[f"W{l}"] for l in (1, 2, 3)}, {l: T[f"b{l}"] for l in (1, 2, 3)}
        shape = {l: (n, cnn.LAYERS[l][5], cnn.LAYERS[l][5], cnn.LAYERS[l][1]) for l in (1, 2, 3)}
        f32, u8 = (lambda name, sh: K.new(name, sh)), (lambda name, nbytes: K.new(name, (int(nbytes),), torch.uint8))
        bits = lambda name, l: K.new(name, (n * shape[l][1] * shape[l][2] * shape[l][3] // 32,), torch.int32)  # noqa: E731
        rec = lambda name, x=None: _amax(cnn, K, name, x)  # noqa: E731
        out = {}
        K.stage("cnn_repack_weights")
        numel = {0: None, 1: None, 2: None, 3: cnn.BT_CLASSES_NUMEL, 4: cnn.QPACK_NUMEL, 5: cnn.BT2_CLASSES_NUMEL}
        bt = {}
        for l, mode in ((1, 0), (1, 4), (2, 0), (2, 2), (2, 5), (3, 0), (3, 1), (3, 3)):
            bt[l, mode] = cnn.repack_weights(W[l], l, mode, out=f32(f"Bt layer {l} mode {mode}", (numel[mode] or W[l].numel(),)))
            out[f"bt{l}_{mode}"] = bt[l, mode]
        K.stage("cnn_conv1q_pack")
        qpack = f32("pack", (int(lib.mi355ppo_cnn_conv1q_pack_bytes()) // 4,))
        _launch("mi355ppo_cnn_conv1q_pack", dev, _ptr(W[1]), _ptr(qpack))
        out["qpack"] = qpack
        K.stage("cnn_conv_fwd_f32 / _variant")
        a1 = cnn.conv_fwd(obs, bt[1, 0], b[1], 1, inds, out=f32("a1", shape[1]))
        a1q = cnn.conv_fwd(obs, bt[1, 4], b[1], 1, inds, out=f32("a1", shape[1]), variant=cnn.VARIANT_Q)
        a1s = cnn.conv_fwd(obs, bt[1, 0], b[1], 1, None, out=f32("a1", (n + 2, 20, 20, 32)), variant=4)
        a2 = cnn.conv_fwd(a1, bt[2, 0], b[2], 2, out=f32("a2", shape[2]))
        a3 = cnn.conv_fwd(a2, bt[3, 0], b[3], 3, out=f32("a3", shape[3]), variant=4)
        a3p = f32("a3", shape[3])
        _launch("mi355ppo_cnn_conv_fwd_f32", dev, _ptr(a2), None, _ptr(bt[3, 0]), _ptr(b[3]), _ptr(a3p), n, 3)
        a1p = f32("a1", shape[1])
        _launch("mi355ppo_cnn_conv1q_fwd", dev, _ptr(obs), _ptr(inds), _ptr(qpack), _ptr(b[1]), _ptr(a1p), n)
        out.update(a1=a1, a1q=a1q, a1_all_rows=a1s, a2=a2, a3=a3, a3_plain=a3p, a1_q_plain=a1p)
        K.stage("cnn_trunk_fwd")
        for v in (0, cnn.VARIANT_Q):
            t = [f32(f"a{l}", shape[l]) for l in (1, 2, 3)]
            cnn.trunk_fwd(obs, inds, bt[1, 4 if v else 0], b[1], bt[2, 0], b[2], bt[3, 0], b[3], *t, conv1_variant=v)
            out.update({f"trunk{v}_a{l + 1}": x for l, x in enumerate(t)})
        K.stage("cnn_conv_dgrad_f32 / _variant")
        out["da2"] = cnn.conv_dgrad(T["dz3"], bt[3, 1], a2, 3, out=f32("dsrc", shape[2]))
        out["da2_classes"] = cnn.conv_dgrad(T["dz3"], bt[3, 3], a2, 3, out=f32("dsrc", shape[2]), variant=5)
        out["da1"] = cnn.conv_dgrad(T["dz2"], bt[2, 2], a1, 2, out=f32("dsrc", shape[1]))
        out["da1_parity"] = cnn.conv_dgrad(T["dz2"], bt[2, 2], a1, 2, out=f32("dsrc", shape[1]), variant=3)
        out["da1_classes"] = cnn.conv_dgrad(T["dz2"], bt[2, 5], a1, 2, out=f32("dsrc", shape[1]), variant=6)
        out["da1_s"] = cnn.conv_dgrad(T["dz2"], bt[2, 2], a1, 2, out=f32("dsrc", shape[1]), variant=4)
        da2p = f32("dsrc", shape[2])
        _launch("mi355ppo_cnn_conv_dgrad_f32", dev, _ptr(T["dz3"]), _ptr(bt[3, 1]), _ptr(a2), _ptr(da2p), n, 3)
        out["da2_plain"] = da2p
        # ------------------------------------------------------------------------------------------ kernel Z / R on the packs
        modes = ((2, cnn.MODE_FWD), (3, cnn.MODE_FWD), (3, cnn.MODE_DGRAD_S1), (2, cnn.MODE_DGRAD_S2))
        K.stage("fc_pack of the conv matrices")
        zp = {k: cnn.conv_zpack(W[k[0]], *k, out=u8("pack", lib.mi355ppo_fc_pack_bytes(*cnn.ZPACK_SHAPE[k]))) for k in modes}
        K.stage("cnn_conv1q_fwd_bits")
        m1, m2, m3 = bits("a1 bits", 1), bits("a2 bits", 2), bits("a3 bits", 3)
        out["a1_bits_f32"] = cnn.conv1q_fwd_bits(obs, bt[1, 4], b[1], inds, f32("a1", shape[1]), m1)
        K.stage("cnn_conv_fwd_packed / _bits")
        out["a2z"] = cnn.conv_fwd_packed(a1, zp[2, 0], b[2], 2, out=f32("a2", shape[2]))
        out["a3z"] = cnn.conv_fwd_packed(a2, zp[3, 0], b[3], 3, out=f32("a3", shape[3]))
        out["a2z_bits"] = cnn.conv_fwd_packed(a1, zp[2, 0], b[2], 2, out=f32("a2", shape[2]), bits=m2)
        out["a3z_bits"] = cnn.conv_fwd_packed(a2, zp[3, 0], b[3], 3, out=f32("a3", shape[3]), bits=m3)
        K.stage("cnn_conv_dgrad_packed / _bits")
        out["da2z"] = cnn.conv_dgrad_packed(T["dz3"], zp[3, 1], a2, 3, out=f32("dsrc", shape[2]))
        out["da1z"] = cnn.conv_dgrad_packed(T["dz2"], zp[2, 2], a1, 2, out=f32("dsrc", shape[1]))
        out["da2z_bits"] = cnn.conv_dgrad_packed(T["dz3"], zp[3, 1], None, 3, out=f32("dsrc", shape[2]), bits=m2)
        out["da1z_bits"] = cnn.conv_dgrad_packed(T["dz2"], zp[2, 2], None, 2, out=f32("dsrc", shape[1]), bits=m1)
        out.update(m1=m1, m2=m2, m3=m3, **{f"zpack{l}_{m}": t for (l, m), t in zp.items()})
        # ------------------------------------------------------------------------------------------ the f16 split
        K.stage("f16x2 packs")
        zp16 = {k: cnn.conv_zpack_f16x2(W[k[0]], *k, out=u8("pack", lib.mi355ppo_fc_pack_f16x2_bytes(*cnn.ZPACK_SHAPE[k]))) for k in modes}
        K.stage("cnn_conv1q_fwd_amax")
        r1, r2, r3 = rec("a1"), rec("a2"), rec("a3")
        b1m, b2m = bits("a1 bits", 1), bits("a2 bits", 2)
        a1h = cnn.conv1q_fwd_amax(obs, bt[1, 4], b[1], inds, f32("a1", shape[1]), b1m, r1)
        out["a1h_nobits"] = cnn.conv1q_fwd_amax(obs, bt[1, 4], b[1], inds, f32("a1", shape[1]), None, rec("a1 again"))
        K.stage("cnn_conv_fwd_packed_f16x2")
        a2h = cnn.conv_fwd_packed(a1h, zp16[2, 0], b[2], 2, out=f32("a2", shape[2]), bits=b2m, amax=(r1, r2))
        a3h = cnn.conv_fwd_packed(a2h, zp16[3, 0], b[3], 3, out=f32("a3", shape[3]), amax=(r2, r3))
        K.stage("cnn_conv_dgrad_packed_f16x2")
        rz3, rz2, rd2, rd1 = rec("dz3", T["dz3"]), rec("dz2", T["dz2"]), rec("da2"), rec("da1")
        out["da2h"] = cnn.conv_dgrad_packed(T["dz3"], zp16[3, 1], None, 3, out=f32("dsrc", shape[2]), bits=b2m, amax=(rz3, rd2))
        out["da1h"] = cnn.conv_dgrad_packed(T["dz2"], zp16[2, 2], None, 2, out=f32("dsrc", shape[1]), bits=b1m, amax=(rz2, rd1))
        out["da2h_act"] = cnn.conv_dgrad_packed(T["dz3"], zp16[3, 1], a2h, 3, out=f32("dsrc", shape[2]), amax=(rz3, None))
        out["da1h_act"] = cnn.conv_dgrad_packed(T["dz2"], zp16[2, 2], a1h, 2, out=f32("dsrc", shape[1]), amax=(rz2, None))
        out.update(a1h=a1h, a2h=a2h, a3h=a3h, b1m=b1m, b2m=b2m, r1=r1, r2=r2, r3=r3, rz3=rz3, rz2=rz2, rd2=rd2, rd1=rd1,
                   **{f"zpack16_{l}_{m}": t for (l, m), t in zp16.items()})
        K.stage("cnn_conv_wgrad f16x2")
        rz1 = rec("dz1", T["dz1"])
        for l, src, dz, am in ((1, obs, T["dz1"], (None, rz1)), (2, a1h, T["dz2"], (r1, rz2)), (3, a2h, T["dz3"], (r2, rz3))):
            cin, cout, k = cnn.LAYERS[l][:3]
            dW, db = cnn.conv_wgrad(src, dz, l, inds if l == 1 else None, out=(f32("dW", (cout, cin, k, k)), f32("db", (cout,))), amax=am)
            out.update({f"dW{l}h": dW, f"db{l}h": db})
        # ------------------------------------------------------------------------------------------ every pack in one launch
        sizes = [(64, 512), (64, 576), (64, 576), (128, 256), (512, 3136), (3136, 512)]
        K.stage("nature_packs")
        packs = [f32("qpack", (cnn.QPACK_NUMEL,))] + [u8("pack", lib.mi355ppo_fc_pack_bytes(*s_)) for s_ in sizes]
        _launch("mi355ppo_nature_packs_f32", dev, _ptr(W[1]), _ptr(W[2]), _ptr(W[3]), _ptr(T["Wfc"]), *[_ptr(t) for t in packs])
        K.stage("nature_packs_f16x2")
        packs16 = [f32("qpack", (cnn.QPACK_NUMEL,))] + [u8("pack", lib.mi355ppo_fc_pack_f16x2_bytes(*s_)) for s_ in sizes]
        w_amax = K.new("w_amax", (3, cnn.AMAX_WORDS), torch.int32)            # (every slot written by the call: not zeroed here)
        _launch("mi355ppo_nature_packs_f16x2_f32", dev, _ptr(W[1]), _ptr(W[2]), _ptr(W[3]), _ptr(T["Wfc"]), *[_ptr(t) for t in packs16], _ptr(w_amax))
        out.update({f"packs{i}": t for i, t in enumerate(packs)})
        out.update({f"packs16_{i}": t for i, t in enumerate(packs16)})
        out["w_amax"] = w_amax.view(-1)[::16]                                   # the records' 16 slots, 64 bytes apart: the words between are padding
        return out

    return build, run


for _images in NATURE_IMAGES:
    case(f"cnn nature images={_images}", ("a1", "a1q", "a2", "a3", "a3_plain", "a1_q_plain", "trunk6_a3", "da2", "da1", "da1_classes", "qpack", "a2z",
                                         "a3z_bits", "da2z", "da1z_bits", "m1", "m3", "a1h", "a3h", "da2h", "da1h", "r3", "rd1", "dW1h", "dW3h",
                                         "db2h", "packs0", "packs6", "packs16_6", "w_amax", "zpack16_2_2"), workspace=True)(_nature(_images))


# ================================================================================================== the synthetic Atari env step, device only
# synth_env.hip: one launch draws reward / done / cursor per env, one copies four 84 x 84 planes per env: N = 1; 3; 257 (past one
# 256-thread block of the per-env launch).  The pool is the smallest that still wraps (5 planes: cursor + 3 runs past its end).
def _synth_atari(N):
    def build():
        g = torch.Generator().manual_seed(N)
        return dict(planes=torch.randint(0, 256, (5, 84, 84), dtype=torch.uint8, generator=g), cursor=torch.randint(0, 5, (N,), generator=g),
                    base=torch.tensor([7]), N=N)

    def run(mod, dev, T, K):
        from cleanrl_amd.ops import _launch, _ptr

        N, out = T["N"], {}
        for name, layout, ctr in (("mi355ppo_synth_atari_step_u8", (N, 4, 84, 84), False), ("mi355ppo_synth_atari_step_ctr_u8", (N, 4, 84, 84), True),
                                  ("mi355ppo_synth_atari_step_hwc_ctr_u8", (N, 84, 84, 4), True)):
            K.stage(name)
            cursor = K.input(T["cursor"], "cursor")
            for advance in (1, 0):                               # a step, then the observation alone (reward / done null)
                obs, rew, done = K.new("obs", layout, torch.uint8), K.new("reward", (N,)), K.new("done", (N,))
                _launch(name, dev, _ptr(T["planes"]), 5, _ptr(cursor), 11, 3, *((_ptr(T["base"]),) if ctr else ()), _ptr(obs),
                        _ptr(rew) if advance else None, _ptr(done) if advance else None, N, 0.3, advance)
                out[f"{name} obs{advance}"] = obs
                if advance:
                    out.update({f"{name} reward": rew, f"{name} done": done})
            out[f"{name} cursor"] = cursor
        return out

    return build, run


for _N in (1, 3, 257):
    case(f"synth_atari N={_N}", ("mi355ppo_synth_atari_step_u8 obs1", "mi355ppo_synth_atari_step_ctr_u8 done", "mi355ppo_synth_atari_step_hwc_ctr_u8 obs0",
                                 "mi355ppo_synth_atari_step_hwc_ctr_u8 cursor"))(_synth_atari(_N))


TWIN_CASES = [c for c in CASES if c.twin]
