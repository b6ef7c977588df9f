"""Mint the qdagger_dqn_atari_impalacnn fixtures from the reference's own lines.

    python tools/mint_qdagger_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
It stores no reference text: as tools/mint_dqn_atari_goldens.py does, it ``ast``-compiles the script's ``ResidualBlock``,
``ConvSequence``, ``QNetwork``, ``linear_schedule`` and ``kl_divergence_with_logits``, dqn_atari.py's ``QNetwork`` (the script's
``TeacherModel``) and ``ReplayBuffer`` of cleanrl_utils/buffers.py, and ``exec``s the script's setup lines and the bodies of its three
loops (teacher, offline, online), located by their lines, against ``AtariReplayVecEnv`` (6 actions) on one CPU thread, batch 8, a
16-slot ring that wraps in the teacher phase and again in the online phase.  What the reference downloads or imports from packages
that are not here is stated instead: the teacher is ``TeacherModel`` initialised from ``TEACHER_SEED`` (both sides build it the same
way), ``teacher_episodic_returns`` is the list ``TEACHER_RETURNS``, and the ``evaluate`` / model-saving legs inside the offline loop
are not run (they sit behind the logging line where the offline block ends).  Frames are never stored: both sides regenerate them
from the seed.  A float64 copy of the three networks runs the offline and online training lines in lockstep on the float32 run's
batches; the float32 reference's maximum deviation from it, per compared quantity, goes to
tests/golden/qdagger_iteration_ref_sensitivity.json.  Writes tests/golden/qdagger_iteration.npz and
tests/golden/qdagger_cli_surface.json.
"""
from __future__ import annotations

import ast
import json
import os
import random
import sys
import textwrap
import time
from collections import deque
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mint_dqn_atari_goldens as D  # noqa: E402
import mint_td3_goldens as T  # noqa: E402
from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCRIPT = "qdagger_dqn_atari_impalacnn.py"
STRIDE = 997
N_ACTIONS = 6
HORIZON = 4
TEACHER_SEED = 77
TEACHER_RETURNS = [2.0, 1.0, 3.0, 2.0, 1.0, 3.0, 2.0, 2.0, 1.0, 3.0]
# learning_rate: at the script's 1e-4 this short run on byte-noise frames (batch 8, the KL summed over the batch) is numerically
# unstable in the reference itself -- its float32 lines drift 1e-3 from their float64 lockstep copy in the loss and in the final
# parameters over the 39 Adam steps, which is the size of the whole-run bar the replays are held to (rtol 1e-3), so such a run
# measures the reference's chaos, not a backend.  At 1e-5 the same steps drift below 1e-6.  MAX_SENSITIVITY holds the minted run to
# that: the reference's own float32-vs-float64 deviation of every logged scalar must stay two orders below the bar, or the tool refuses
# to write (single parameters still move by an Adam step or two, 1e-5, where a gradient element is rounding noise).
_COMMON = dict(buffer_size=16, batch_size=8, teacher_steps=24, offline_steps=12, total_timesteps=60, learning_starts=16, train_frequency=2,
               target_network_frequency=6, exploration_fraction=0.5, end_e=0.3, learning_rate=1e-5)
MAX_SENSITIVITY = 1e-5
CASES = {"qdagger": dict(_COMMON, seed=3), "qdagger_t07": dict(_COMMON, seed=4, temperature=0.7)}
SCALARS = ("loss", "q_loss", "distill_loss", "q_values")
NETS = ("q_network", "target_network", "teacher_model")


def load_reference_classes():
    ns = T.load_reference_classes("dqn_atari.py")                 # dqn_atari.py's QNetwork and ReplayBuffer
    ns["TeacherModel"] = ns.pop("QNetwork")
    tree = ast.parse("\n".join(R._read(SCRIPT)))
    names = ("ResidualBlock", "ConvSequence", "QNetwork", "linear_schedule", "kl_divergence_with_logits")
    wanted = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in names]
    assert len(wanted) == len(names)
    exec(compile(ast.Module(body=wanted, type_ignores=[]), f"<reference:{SCRIPT}>", "exec"), ns)
    return ns


def blocks():
    L = R._read(SCRIPT)

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{SCRIPT}>", "exec")

    s0 = R._find(L, "q_network = QNetwork(envs")
    s1 = R._find(L, "# QDAGGER LOGIC:", s0)
    r0 = R._find(L, "teacher_rb = ReplayBuffer(", s1)
    r1 = R._find(L, "obs, _ = envs.reset(seed=args.seed)", r0)
    t0 = R._find(L, "epsilon = linear_schedule(args.start_e, args.end_e, args.teacher_steps, global_step)", r1)
    t1 = R._find(L, "# offline training phase", t0)
    o0 = R._find(L, "data = teacher_rb.sample(args.batch_size)", t1)
    o1 = R._find(L, "if global_step % 100 == 0:", o0)
    b0 = R._find(L, "rb = ReplayBuffer(", o1)
    b1 = R._find(L, "start_time = time.time()", b0)
    n0 = R._find(L, "global_step += args.offline_steps", b1)
    tr = R._find(L, "if global_step % args.train_frequency == 0:", n0)
    n1 = R._find(L, "if args.save_model:", tr)
    assert "optimize_memory_usage=True" in "".join(L[r0:r1]) and "optimize_memory_usage=True" in "".join(L[b0:b1])
    return dict(setup=block(s0, s1), teacher_rb=block(r0, r1), teacher=block(t0, t1), offline=block(o0, o1), rb=block(b0, b1),
                online=block(n0, n1), train=block(tr, n1))


def make_args(over):
    d = T.reference_args_defaults(SCRIPT)
    d.update(over)
    return SimpleNamespace(**d)


def _draw_indices(np_state, rb, B):
    """``ReplayBuffer.sample`` of the memory-optimised buffer from the saved ``np.random`` state (never slot ``pos`` once full)."""
    rs = np.random.RandomState()
    rs.set_state(np_state)
    size = rb.buffer_size
    bi = (rs.randint(1, size, size=B) + rb.pos) % size if rb.full else rs.randint(0, rb.pos, size=B)
    return bi, rs.randint(0, high=1, size=(B,))


def _scalars(ns):
    return tuple(float(ns[k].item()) for k in ("loss", "q_loss", "distill_loss")) + (float(ns["old_val"].mean().item()),)


def mint_case(name):
    over = CASES[name]
    args = make_args(over)
    blk = blocks()
    B = args.batch_size

    def seeded_setup():
        classes = load_reference_classes()
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        envs = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=N_ACTIONS, horizon=HORIZON)
        classes["envs"] = envs                                   # the reference's QNetwork reads the module's ``envs``
        ns = classes
        ns.update(args=args, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, random=random,
                  deque=deque, writer=T._Writer(), teacher_episodic_returns=list(TEACHER_RETURNS))
        exec(blk["setup"], ns)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(TEACHER_SEED)
            ns["teacher_model"] = ns["TeacherModel"](envs)
        ns["teacher_model"].eval()
        return ns

    ns64 = seeded_setup()
    for k in NETS:
        ns64[k].double()
    ns = seeded_setup()                                          # the float32 run owns the global random streams from here on
    envs = ns["envs"]
    rec = {"init_checksum": np.float64(T.flat(ns["q_network"]).double().sum()),
           "teacher_checksum": np.float64(T.flat(ns["teacher_model"]).double().sum())}
    dev = {k: 0.0 for k in SCALARS}

    def compare(sc32, sc64):
        for k, a, b in zip(SCALARS, sc32, sc64):
            dev[k] = max(dev[k], abs(a - b))

    # ---------------------------------------------------------------- the teacher fills its buffer
    exec(blk["teacher_rb"], ns)
    ns["obs"], _ = envs.reset(seed=args.seed)
    t_actions, t_random = [], []
    for global_step in range(args.teacher_steps):
        ns["global_step"] = global_step
        pr = random.Random()
        pr.setstate(random.getstate())
        exec(blk["teacher"], ns)
        t_actions.append(np.asarray(ns["actions"], np.int64).reshape(1))
        t_random.append(np.int64(pr.random() < ns["epsilon"]))
    rec["teacher_actions"], rec["teacher_random_branch"] = np.stack(t_actions), np.asarray(t_random)
    assert ns["teacher_rb"].full and 0 < rec["teacher_random_branch"].sum() < args.teacher_steps

    # ---------------------------------------------------------------- offline: the student on the teacher's buffer
    rb64 = D._Rb64(ns["teacher_rb"])
    ns64["teacher_rb"] = rb64
    off = {k: [] for k in ("batch_inds", "env_inds") + SCALARS}
    for global_step in range(args.offline_steps):
        ns["global_step"] = ns64["global_step"] = global_step
        bi, ei = _draw_indices(np.random.get_state(), ns["teacher_rb"], B)
        exec(blk["offline"], ns)
        assert torch.equal(ns["data"].observations, torch.tensor(ns["teacher_rb"].observations[bi, ei, :])), "index recovery is off"
        rb64.inds = (bi, ei)
        exec(blk["offline"], ns64)
        sc = _scalars(ns)
        compare(sc, _scalars(ns64))
        off["batch_inds"].append(bi), off["env_inds"].append(ei)
        for k, v in zip(SCALARS, sc):
            off[k].append(v)
    for k, v in off.items():
        rec["offline_" + k] = np.stack(v) if k.endswith("inds") else np.asarray(v)

    # ---------------------------------------------------------------- online
    exec(blk["rb"], ns)
    rb64 = D._Rb64(ns["rb"])
    ns64["rb"] = rb64
    envs = ns["envs"] = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=N_ACTIONS, horizon=HORIZON)     # the reference makes its envs again
    ns["obs"], _ = envs.reset(seed=args.seed)
    ns["episodic_returns"] = ns64["episodic_returns"] = deque(maxlen=10)
    ns["start_time"] = ns64["start_time"] = time.time() - 1.0
    per = {k: [] for k in ("actions", "batch_inds", "env_inds", "random_branch", "target_update", "distill_coeff") + SCALARS}
    truncs = 0
    for step in range(args.total_timesteps):
        ns["global_step"] = step
        global_step = step + args.offline_steps
        ns64["global_step"] = global_step                       # the train block alone: already shifted
        pr = random.Random()
        pr.setstate(random.getstate())
        np_state = np.random.get_state()
        pos, full = ns["rb"].pos, ns["rb"].full
        n_eps = len(ns["episodic_returns"])
        exec(blk["online"], ns)
        truncs += int(np.asarray(ns["truncations"]).sum())
        per["actions"].append(np.asarray(ns["actions"], np.int64).reshape(1))
        per["random_branch"].append(np.int64(pr.random() < ns["epsilon"]))
        learning = global_step > args.learning_starts
        trained = learning and global_step % args.train_frequency == 0
        bi, ei = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
        sc, coeff = {k: np.nan for k in SCALARS}, np.nan
        if trained:
            after = SimpleNamespace(buffer_size=ns["rb"].buffer_size, pos=(pos + 1) % ns["rb"].buffer_size,
                                    full=full or pos + 1 == ns["rb"].buffer_size)              # rb.add ran before rb.sample
            bi, ei = _draw_indices(np_state, after, B)
            assert torch.equal(ns["data"].observations, torch.tensor(ns["rb"].observations[bi, ei, :])), "index recovery is off"
            rb64.inds = (bi, ei)
            coeff = float(ns["distill_coeff"])
        if learning:
            exec(blk["train"], ns64)
        if trained:
            s32 = _scalars(ns)
            compare(s32, _scalars(ns64))
            sc = dict(zip(SCALARS, s32))
        per["batch_inds"].append(bi), per["env_inds"].append(ei)
        per["target_update"].append(np.int64(learning and global_step % args.target_network_frequency == 0))
        per["distill_coeff"].append(coeff)
        for k in SCALARS:
            per[k].append(sc[k])
        del n_eps
    for k, v in per.items():
        rec[k] = np.stack(v) if k in ("actions", "batch_inds", "env_inds") else np.asarray(v)
    for nm, key in (("online", "q_network"), ("target", "target_network")):
        f32, f64 = T.flat(ns[key]), T.flat(ns64[key])
        rec[f"final_{nm}_sub"] = f32[::STRIDE].numpy()
        rec[f"final_{nm}_checksum"] = np.float64(f32.double().sum())
        dev[f"final_{nm}"] = float((f32.double() - f64).abs().max())
    rec["stride"] = np.int64(STRIDE)
    rec["config"] = np.frombuffer(json.dumps({"script": SCRIPT, "args": over, "horizon": HORIZON, "n_actions": N_ACTIONS,
                                              "teacher_seed": TEACHER_SEED, "teacher_returns": TEACHER_RETURNS}).encode(), np.uint8)
    coeffs = rec["distill_coeff"][~np.isnan(rec["distill_coeff"])]
    first_full = next(i for i, c in enumerate(coeffs) if c != 1.0)
    assert first_full > 0 and (coeffs[:first_full] == 1.0).all(), "both distill_coeff branches must occur: the short deque first"
    assert truncs >= 10 and ns["rb"].full, "ten episodes must end and the online ring must wrap"
    assert 0 < rec["random_branch"].sum() < args.total_timesteps, "both action branches must occur"
    assert max(dev[k] for k in SCALARS) <= MAX_SENSITIVITY, f"the reference's own f32-vs-f64 deviation {dev} is too close to the whole-run bars"
    print(f"{name}: truncations {truncs}, random actions {int(rec['random_branch'].sum())}, trained steps {len(coeffs)} "
          f"({first_full} with the short deque), distill_coeff after {sorted(set(np.round(coeffs[first_full:], 4)))}, target updates "
          f"{int(rec['target_update'].sum())}, deviations {dev}")
    return rec, dev


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out, sens = {}, {}
    for name in CASES:
        rec, dev = mint_case(name)
        sens[name] = dev
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
    path = os.path.join(OUT, "qdagger_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "qdagger_iteration_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "qdagger_cli_surface.json"), "w") as fh:
        surf = {SCRIPT[: -len(".py")]: {"defaults": T.reference_args_defaults(SCRIPT), "order": T.reference_args_order(SCRIPT)}}
        json.dump(surf, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
