"""``MI355PPO_RND_TRUNK=fused`` on the MI355X: the LeakyReLU kernels against their twins, the normalising one-frame conv1 (csrc/rnd_conv1.hip)
against a one-hot tap probe and per-row float64 bars (tests/row_bars.py), the predictor / target nodes (cleanrl_amd/leaky_cnn.py) and the
agent seam ``heads3_u8`` against float64 autograd of the modules themselves -- with the ``torch`` trunk held to the same bars --, guard
bands, determinism, a non-default stream, and the learner with both switches.

Bars.  The probe's ``2^-22 * 8`` is derived from the split: two f16 terms keep 22 bits of a value below 8.  conv1's forward and gradients
start at the project's c = 4 (``row_bars.C_CONV_FORWARD`` / ``C_WGRAD`` / ``C_BIAS_GRAD``).  A whole node is a chain of kernels of several
families; its yardstick -- torch f32 on the CPU through the same chain -- compounds the same way, so the node is held to the largest
family constant along its chain, ``row_bars.C_FC_FORWARD`` = 9 (the whole-K FC forward) -- this file's choice, not ``row_bar``'s default
4 (DESIGN 3.22.1 says what would change at 4).  Every test prints its worst ratio.

Image counts.  1, 5, 8 and 67 images give every workgroup of the conv1 kernels ONE image (the forward's grid is min(CUs, M), the gradient's
min(images, 512)); the loops over images -- the second staging pass, the barriers between images, the dz ring carried across images,
accumulators and the record's maximum over several images -- run in the cases with 2 CUs + 3 and with 1,030 images."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
import rnd_cases as R
import row_bars as RB
from cleanrl_amd import envs as E
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops
from test_rnd_trunk_twins import SIZES, _bits_of, _record, leaky_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
IMAGES = (1, 5, 67)            # one image; a few; more than one workgroup's share on no group size's multiple
PROBE_BAR = 2.0 ** -22 * 8     # two f16 terms keep 22 bits of |x| <= 5 < 8
C_NODE = RB.C_FC_FORWARD


def _same(a, b, what):
    assert GA.same_bits(a, b), f"{what}: bits differ"


def _rows(c, nhwc):
    return (R.to_nhwc(c["rows"]) if nhwc else c["rows"]).to(DEV).contiguous()


# ---------------------------------------------------------------------------------------------- LeakyReLU: the device equals its twin
def _cus() -> int:
    return torch.cuda.get_device_properties(DEV).multi_processor_count


# "stride": one element more than a quad past what the capped grid (8 workgroups per CU, 1,024 elements each) covers in one pass, so the
# grid-stride loop of both kernels iterates and its last pass is ragged
@pytest.mark.parametrize("n", SIZES + (4 * 256 * 3 + 5, 1 << 20, "stride"))
def test_leaky_kernels_equal_their_twins(n):
    if n == "stride":
        n = _cus() * 8 * 1024 + 1029
    z, da = leaky_case(n)
    words = (n + 31) // 32
    hb, hr = torch.zeros(words, dtype=torch.int32), torch.zeros(256, dtype=torch.int32)
    ha = H.leaky_relu_fwd(z, bits=hb, amax=hr)
    hr2 = torch.zeros(256, dtype=torch.int32)
    hdz = H.leaky_relu_bwd(da, hb, amax=hr2)
    for in_place in (False, True):
        arena = GA.Arena(DEV, GA.SENTINELS[0], words=1 << 24)
        zz, dd = arena.input(z, "z"), arena.input(da, "da")
        db, dr, dr2 = arena.carve((words,), torch.int32, "bits"), arena.input(torch.zeros(256, dtype=torch.int32), "rec", 64), \
            arena.input(torch.zeros(256, dtype=torch.int32), "rec2", 64)
        a = ops.leaky_relu_fwd(zz, out=zz if in_place else arena.carve((n,), torch.float32, "a"), bits=db, amax=dr)
        dz = ops.leaky_relu_bwd(dd, db, out=dd if in_place else arena.carve((n,), torch.float32, "dz"), amax=dr2)
        arena.assert_guards_intact()
        _same(a.cpu(), ha, "leaky forward")
        _same(dz.cpu(), hdz, "leaky backward")
        assert torch.equal(db.cpu(), hb) and torch.equal(hb, _bits_of(z > 0))
        assert _record(dr.cpu()) == _record(hr) and _record(dr2.cpu()) == _record(hr2)


# ---------------------------------------------------------------------------------------------- conv1 forward
def _pack(W1):
    from cleanrl_amd import cnn

    return cnn.fc_pack_f16x2(W1.to(DEV).view(32, 64))


def _conv1(c, nhwc, W1, b1, slope, bits=True, put=None, out_of=None):
    from cleanrl_amd import leaky_cnn as LC

    put = put or (lambda t, name: t.to(DEV).contiguous())
    M = c["want"].shape[0]
    out_of = out_of or (lambda shape, dtype, name: torch.empty(shape, dtype=dtype, device=DEV))
    rows = put(R.to_nhwc(c["rows"]) if nhwc else c["rows"], "rows")
    idx = None if c["idx"] is None else put(c["idx"], "idx")
    rec = put(torch.zeros(256, dtype=torch.int32), "rec")
    mb = out_of((M * 400,), torch.int32, "bits") if bits else None
    out = LC.rnd_conv1_fwd(rows, put(c["mean"], "mean"), put(c["sd"], "sd"), _pack(W1), put(b1, "bias"), idx, out_of((M, 20, 20, 32), torch.float32, "a1"),
                           mb, rec, nhwc=nhwc, slope=slope)
    return out, mb, rec


def _onehot():
    """Channel n reads tap (n % 8, 2 (n // 8) + n % 2): every tap row, every tap column -- all four x mod 4 classes, both column halves."""
    W = torch.zeros(32, 1, 8, 8)
    taps = [(n % 8, 2 * (n // 8) + n % 2) for n in range(32)]
    for n, (kh, kw) in enumerate(taps):
        W[n, 0, kh, kw] = 1.0
    assert {kw for _, kw in taps} == set(range(8)) and {kh for kh, _ in taps} == set(range(8))
    return W, taps


@pytest.mark.parametrize("M", IMAGES)
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_conv1_forward_one_hot_taps_return_the_normalised_pixels(M, gather, nhwc):
    c = R.normalize_case(M, gather)
    W, taps = _onehot()
    out, mb, rec = _conv1(c, nhwc, W, torch.zeros(32), 1.0)          # slope 1: the activation is the identity, the bits still say x > 0
    x = c["want"][:, 0]                                             # rnd_normalize's f32 value (M, 84, 84)
    want = torch.stack([x[:, kh:kh + 77:4, kw:kw + 77:4] for kh, kw in taps], dim=-1)      # (M, 20, 20, 32)
    err = (out.cpu().double() - want.double()).abs().max().item()
    print(f"conv1 one-hot probe M={M} gather={gather} nhwc={nhwc}: max |out - x| = {err:.3e} (bar {PROBE_BAR:.3e})")
    assert err <= PROBE_BAR
    assert bool((want.abs() == 5.0).any()) and bool((want == 5.0).any()) and bool((want == -5.0).any())      # the clips fired in the window
    assert torch.equal(mb.cpu(), RB.packed_bits(out.cpu() > 0))
    assert _record(rec.cpu()) == float(out.abs().max())


@functools.lru_cache(maxsize=None)
def conv1_params():
    """Conv2d(1, 32, 8, stride=4) with a per-output-channel factor over 2^-12 on the weight's rows (and the bias with them)."""
    g = torch.Generator().manual_seed(4100)
    f = torch.exp2(-12 * torch.rand(32, generator=g))
    W = torch.randn(32, 1, 8, 8, generator=g) / 8.0 * f.view(32, 1, 1, 1)
    b = torch.randn(32, generator=g) * 0.1 * 2.0 ** -8 * f
    return W, b


def _conv1_ref(c, dtype):
    W, b = conv1_params()
    y = F.leaky_relu(F.conv2d(c["want"].to(dtype), W.to(dtype), b.to(dtype), stride=4), 0.01)
    return y.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv1_yard():
    c = R.normalize_case(RB.CONV_IMAGES_MIN, False)
    return _conv1_ref(c, torch.float32), _conv1_ref(c, torch.float64)


@pytest.mark.parametrize("M", IMAGES)
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_conv1_forward_rows_against_float64(M, gather, nhwc):
    c = R.normalize_case(M, gather)
    W, b = conv1_params()
    out, mb, rec = _conv1(c, nhwc, W, b, 0.01)
    y32, y64 = conv1_yard()
    ratio = RB.row_bar(f"rnd conv1 forward M={M}", out.cpu(), _conv1_ref(c, torch.float64), y32, y64, c=RB.C_CONV_FORWARD)
    print(f"rnd conv1 forward M={M} gather={gather} nhwc={nhwc}: worst ratio {ratio:.2f} against c = {RB.C_CONV_FORWARD:g}")
    assert _record(rec.cpu()) == float(out.abs().max())


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_conv1_forward_walks_several_images_per_workgroup(gather, nhwc):
    """The forward launches min(CUs, M) workgroups: with 2 CUs + 3 images every workgroup stages a second image over the first (the barrier at
    an image's end, the record's maximum over several images) and three of them a third.  Same row bar, sign bits, record, guard bands and bits on
    a second run as the one-image-per-workgroup cases."""
    M = 2 * _cus() + 3
    c = R.normalize_case(M, gather)
    W, b = conv1_params()
    arena = GA.Arena(DEV, GA.SENTINELS[0], words=1 << 24)
    out, mb, rec = _conv1(c, nhwc, W, b, 0.01, put=lambda t, name: arena.input(t.contiguous(), name, 64),
                          out_of=lambda shape, dtype, name: arena.carve(shape, dtype, name))
    arena.assert_guards_intact()
    again = _conv1(c, nhwc, W, b, 0.01)
    _same(out, again[0], "two runs of the forward")
    _same(mb, again[1], "two runs of the sign bits")
    y32, y64 = conv1_yard()
    ref64 = _conv1_ref(c, torch.float64)
    ratio = RB.row_bar(f"rnd conv1 forward M={M}", out.cpu(), ref64, y32, y64, c=RB.C_CONV_FORWARD)
    print(f"rnd conv1 forward M={M} (several images per workgroup) gather={gather} nhwc={nhwc}: worst ratio {ratio:.2f} against c = {RB.C_CONV_FORWARD:g}")
    assert _record(rec.cpu()) == float(out.abs().max()) == _record(again[2].cpu())
    assert torch.equal(mb.cpu(), RB.packed_bits(out.cpu() > 0))      # leaky(z) > 0 exactly where z > 0


# ---------------------------------------------------------------------------------------------- conv1 weight / bias gradient
@functools.lru_cache(maxsize=None)
def wgrad_case(M: int, gather: bool):
    c = R.normalize_case(M, gather)
    g = torch.Generator().manual_seed(4200 + M + gather)
    dz = (torch.randn(M, 20, 20, 32, generator=g) * torch.exp2(-10 * torch.rand(M, 1, 1, 1, generator=g)) * 1e-3
          * (torch.rand(M, 20, 20, 32, generator=g) > 0.5) * torch.exp2(-12 * torch.rand(32, generator=g)))
    z = dz.permute(0, 3, 1, 2)
    refs = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        refs["dW" + name] = torch.nn.grad.conv2d_weight(c["want"].to(dt), (32, 1, 8, 8), z.to(dt), stride=4)
        refs["db" + name] = dz.to(dt).sum((0, 1, 2))
    return SimpleNamespace(c=c, dz=dz, **refs)


# 1,030 images: the gradient's grid is min(images, 512) workgroups, so every workgroup walks a second image (the second staging pass, the
# barriers between images, the dz ring carried across images, accumulators over several images) and workgroups 0 .. 5 a third
WGRAD_WALK = 2 * 512 + 6


@pytest.mark.parametrize("M", (8, 67, WGRAD_WALK))
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
@pytest.mark.parametrize("sentinel", GA.SENTINELS[:1])
def test_conv1_gradient_rows_against_float64_inside_guard_bands(M, gather, nhwc, sentinel, monkeypatch):
    from cleanrl_amd import cnn
    from cleanrl_amd import leaky_cnn as LC

    w = wgrad_case(M, gather)
    c = w.c
    arena = GA.Arena(DEV, sentinel, words=1 << (26 if M > 512 else 24))
    put = lambda t, name: arena.input(t.contiguous(), name)      # noqa: E731
    rows = put(R.to_nhwc(c["rows"]) if nhwc else c["rows"], "rows")
    idx = None if c["idx"] is None else put(c["idx"], "idx")
    dz = put(w.dz, "dz")
    rec = arena.input(torch.zeros(256, dtype=torch.int32), "rec", 64)
    cnn.absmax(dz, rec)
    with GA.exact_workspaces(monkeypatch, arena) as requested:
        dW, db = LC.rnd_conv1_wgrad(rows, put(c["mean"], "mean"), put(c["sd"], "sd"), dz, rec, idx,
                                    out=(arena.carve((32, 1, 8, 8), torch.float32, "dW"), arena.carve((32,), torch.float32, "db")), nhwc=nhwc)
        again = LC.rnd_conv1_wgrad(rows, put(c["mean"], "mean2"), put(c["sd"], "sd2"), dz, rec, idx, nhwc=nhwc)
    arena.assert_guards_intact()
    assert requested and max(requested) > 0
    _same(dW, again[0], "two runs of the weight gradient")
    _same(db, again[1], "two runs of the bias gradient")
    rw = RB.row_bar(f"rnd conv1 dW M={M}", dW.cpu(), w.dW64, w.dW32, w.dW64, c=RB.C_WGRAD)
    rb = RB.row_bar(f"rnd conv1 db M={M}", db.cpu(), w.db64, w.db32, w.db64, c=RB.C_BIAS_GRAD)
    print(f"rnd conv1 gradient M={M} gather={gather} nhwc={nhwc}: worst ratios dW {rw:.2f}, db {rb:.2f} against c = {RB.C_WGRAD:g}")


@pytest.mark.parametrize("sentinel", GA.SENTINELS, ids=[f"0x{s:08X}" for s in GA.SENTINELS])
def test_conv1_forward_stays_inside_its_outputs(sentinel):
    W, b = conv1_params()
    ref = {}
    for nhwc in (True, False):
        for gather in (False, True):
            c = R.normalize_case(5, gather)
            ref[(nhwc, gather)] = _conv1(c, nhwc, W, b, 0.01)
            arena = GA.Arena(DEV, sentinel, words=1 << 22)
            got = _conv1(c, nhwc, W, b, 0.01, put=lambda t, name: arena.input(t.contiguous(), name, 64),
                         out_of=lambda shape, dtype, name: arena.carve(shape, dtype, name))
            arena.assert_guards_intact()
            for g, r, what in zip(got[:2], ref[(nhwc, gather)][:2], ("a1", "bits")):
                _same(g, r, f"sentinel 0x{sentinel:08X} nhwc={nhwc} gather={gather} {what}")


# ---------------------------------------------------------------------------------------------- the nodes
@functools.lru_cache(maxsize=None)
def node_case(M: int):
    from cleanrl_amd.agents import RNDModel

    torch.manual_seed(4300 + M)
    model = RNDModel(4, 6)
    c = R.normalize_case(M, True)
    g = torch.Generator().manual_seed(4400 + M)
    cot = torch.randn(M, 512, generator=g) * 1e-3
    refs = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        m = copy.deepcopy(model).to(dt)
        x = c["want"].to(dt)
        out = m.predictor(x)
        out.backward(cot.to(dt))
        refs["p" + name] = out.detach()
        refs["g" + name] = [m.predictor[i].weight.grad if k == 0 else m.predictor[i].bias.grad for i in (0, 2, 4, 7) for k in (0, 1)]
        refs["t" + name] = m.target(x).detach()
    return SimpleNamespace(model=model, c=c, cot=cot, **refs)


def _node_run(n, fused: bool):
    from cleanrl_amd import leaky_cnn as LC

    model = copy.deepcopy(n.model).to(DEV)
    c = n.c
    rows, idx, mean, sd = _rows(c, True), c["idx"].to(DEV), c["mean"].to(DEV), c["sd"].to(DEV)
    if fused:
        pred, targ = LC.LeakyNatureTrunk(model.predictor, head=True), LC.LeakyNatureTrunk(model.target, head=False)
        out = model.predictor[9:](pred(rows, idx, mean, sd))
        t = targ(rows, idx, mean, sd)
    else:
        x = ops.rnd_normalize(rows, mean, sd, idx=idx)
        out, t = model.predictor(x), model.target(x)
    out.backward(n.cot.to(DEV))
    grads = [model.predictor[i].weight.grad if k == 0 else model.predictor[i].bias.grad for i in (0, 2, 4, 7) for k in (0, 1)]
    torch.cuda.synchronize()
    return out.detach(), [g.clone() for g in grads], t.detach()


@pytest.mark.parametrize("M", (8, 67))
def test_predictor_and_target_nodes_against_float64_autograd(M):
    n = node_case(M)
    names = ("dW1", "db1", "dW2", "db2", "dW3", "db3", "dWfc", "dbfc")
    for trunk in ("torch", "fused"):
        out, grads, t = _node_run(n, trunk == "fused")
        ratios = {"predictor": RB.row_bar(f"{trunk} predictor", out.cpu(), n.p64, n.p32, n.p64, c=C_NODE),
                  "target": RB.row_bar(f"{trunk} target", t.cpu(), n.t64, n.t32, n.t64, c=C_NODE)}
        for name, g, g32, g64 in zip(names, grads, n.g32, n.g64):
            ratios[name] = RB.row_bar(f"{trunk} {name}", g.cpu(), g64, g32, g64, c=C_NODE)
        print(f"RND nodes M={M} trunk={trunk}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()) + f" against c = {C_NODE:g}")


def test_nodes_give_the_same_bits_twice_and_on_another_stream():
    n = node_case(67)
    ref = _node_run(n, True)
    again = _node_run(n, True)
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        other = _node_run(n, True)
    s.synchronize()
    for run, what in ((again, "second run"), (other, "non-default stream")):
        _same(run[0], ref[0], f"{what}: predictor")
        _same(run[2], ref[2], f"{what}: target")
        for a, b in zip(run[1], ref[1]):
            _same(a, b, f"{what}: gradient")


@pytest.mark.parametrize("M", (8, 67))
def test_agent_seam_heads3_u8_against_float64(M):
    from cleanrl_amd.agents import RNDAgent

    torch.manual_seed(4500 + M)
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (4, 84, 84), np.uint8), single_action_space=E.Discrete(6))
    agent = RNDAgent(envs)
    c = R.normalize_case(M, True)
    rows_nhwc, idx = R.to_nhwc(c["rows"]), c["idx"]
    g = torch.Generator().manual_seed(4600 + M)
    cots = [torch.randn(M, 6, generator=g) * 1e-3, torch.randn(M, 1, generator=g) * 1e-3, torch.randn(M, 1, generator=g) * 1e-3]
    layers = (0, 2, 4, 7)

    def run(ag, outs):
        torch.autograd.backward(list(outs), [ct.to(outs[0].dtype).to(outs[0].device) for ct in cots])
        # one row per sample: its logits and both values side by side (a lone value near zero has no scale of its own)
        return [torch.cat([o.detach().cpu() for o in outs], dim=1)], [(ag.network[i].weight.grad if k == 0 else ag.network[i].bias.grad).detach().cpu()
                                                  for i in layers for k in (0, 1)]

    refs = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        a = copy.deepcopy(agent).to(dt)
        refs[name] = run(a, a.heads3(rows_nhwc[idx].permute(0, 3, 1, 2).to(dt) / 255.0))
    for trunk in ("torch", "fused"):
        a = copy.deepcopy(agent).to(DEV)
        rows_d, idx_d = rows_nhwc.to(DEV), idx.to(DEV)
        outs = a.heads3_u8(rows_d, idx_d) if trunk == "fused" else a.heads3(ops.obs_u8_to_f32(rows_d, idx_d).permute(0, 3, 1, 2))
        got = run(a, outs)
        ratios = []
        for k, what in enumerate(("heads",)):
            ratios.append((what, RB.row_bar(f"{trunk} {what}", got[0][k], refs["64"][0][k], refs["32"][0][k], refs["64"][0][k], c=C_NODE)))
        for k, what in enumerate(("dW1", "db1", "dW2", "db2", "dW3", "db3", "dWfc", "dbfc")):
            ratios.append((what, RB.row_bar(f"{trunk} {what}", got[1][k], refs["64"][1][k], refs["32"][1][k], refs["64"][1][k], c=C_NODE)))
        print(f"heads3_u8 M={M} trunk={trunk}: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in ratios) + f" against c = {C_NODE:g}")


# ---------------------------------------------------------------------------------------------- the learner with both switches
def test_learner_teacher_forced_with_both_switches(monkeypatch):
    """tests/test_gpu_rnd.py::test_fused_rnd_teacher_forced_against_reference_iteration itself, at its bars, with the trunk switch set."""
    import test_gpu_rnd as T
    from cleanrl_amd.learner_rnd import RNDPPOLearner

    monkeypatch.setenv("MI355PPO_RND_TRUNK", "fused")
    built, real_init = [], RNDPPOLearner.init_rnd_trunk_fused
    monkeypatch.setattr(RNDPPOLearner, "init_rnd_trunk_fused", lambda self: (real_init(self), built.append(self))[0])
    # the torch trunk's two conversions must never launch: the RND input's normalise kernel and K5
    launched = []
    for name in ("rnd_normalize", "obs_u8_to_f32"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: launched.append(_n) or pytest.fail(f"ops.{_n} ran under MI355PPO_RND_TRUNK=fused"))
    T.test_fused_rnd_teacher_forced_against_reference_iteration(monkeypatch)
    assert len(built) == 1 and built[0].rnd_trunk_fused and launched == []
    L = built[0]
    assert L._rnd_x_mb is None and L._x_mb is None and L._rnd_x_step is None
    assert L.agent._trunk.bufs.weights_version == 2 and L._rnd_pred.bufs.weights_version == 2      # two optimizer steps


def test_script_runs_with_both_switches_and_allocates_no_f32_frames(monkeypatch):
    from cleanrl_amd import ppo_rnd_envpool

    monkeypatch.setenv("MI355PPO_RND", "fused")
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "fused")
    L = ppo_rnd_envpool.main(["--num-envs", "8", "--num-steps", "16", "--total-timesteps", "256", "--num-minibatches", "4",
                              "--num-iterations-obs-norm-init", "1"])
    assert L.hip and L.rnd_fused and L.rnd_trunk_fused
    assert L._rnd_x_mb is None and L._x_mb is None and L._rnd_x_step is None      # no (M, 1, 84, 84) / (M, 4, 84, 84) f32 tensors
    assert np.isfinite(L.last_metrics["loss"]) and np.isfinite(L.last_metrics["fwd_loss"])
    assert L.int_returns.abs().sum().item() > 0 and L.curiosity_rewards.min().item() >= 0.0
    assert L.agent._trunk.bufs.weights_version > 0 and L._rnd_pred.bufs.weights_version > 0 and L._rnd_targ.bufs.weights_version == 0
    L.flat.check_views()


def test_fused_trunk_without_the_fused_rnd_backend_is_refused_on_the_device(monkeypatch):
    from cleanrl_amd import ppo_rnd_envpool

    monkeypatch.delenv("MI355PPO_RND", raising=False)
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "fused")
    with pytest.raises(ValueError, match="MI355PPO_RND=fused"):
        ppo_rnd_envpool.main(["--num-envs", "8", "--num-steps", "16", "--total-timesteps", "256", "--num-minibatches", "4",
                              "--num-iterations-obs-norm-init", "1"])
