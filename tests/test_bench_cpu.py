"""bench.py's host-side bookkeeping (no GPU): one named workload per BASELINE.json config, work accounting."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_one_named_workload_per_baseline_config():
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    names = ["cfg1", "cfg2", "cfg3", "cfg4", "cfg5"]
    assert len(base["configs"]) == len(names)
    for i, n in enumerate(names):
        assert n in bench.WORKLOADS and bench.WORKLOAD_INFO[n][0] == f"BASELINE configs[{i}]"
    assert set(bench.WORKLOAD_INFO) == set(bench.WORKLOADS)
    # configs[2]: batch 256 on 8 GPUs; configs[3]: batch 64, 6 channels, 4 GPUs; configs[4]: batch 128 fp8 on 8 GPUs
    assert bench.WORKLOADS["cfg3"][0] * bench.WORKLOAD_INFO["cfg3"][1] == 256 and bench.WORKLOAD_INFO["cfg3"][2] == "bf16"
    assert bench.WORKLOADS["cfg4"][0] * bench.WORKLOAD_INFO["cfg4"][1] == 64 and bench.WORKLOADS["cfg4"][3] == 6
    assert bench.WORKLOADS["cfg5"][0] * bench.WORKLOAD_INFO["cfg5"][1] == 128 and bench.WORKLOAD_INFO["cfg5"][2] == "fp8"
    assert bench.WORKLOADS["cfg2"][:1] == (32,) and bench.WORKLOAD_INFO["cfg2"][1:] == (1, "bf16")
    for n in ("cfg2", "cfg3", "cfg4", "cfg5"):        # the full 128 -> 1024 tile, filters 128, 16 RRDBs
        assert bench.WORKLOADS[n][1:3] == (128, 128) and bench.WORKLOADS[n][4] == 16


def test_algorithmic_flops_of_the_headline_workload():
    """Gf 4203.8, Cf 778.8 GFLOP per sample at configs[1] shapes with real channel counts."""
    gf, cf = bench.conv_flops_per_sample(128, 128, 2, 2, 16)
    assert abs(gf / 1e9 - 4203.8) < 0.5 and abs(cf / 1e9 - 778.8) < 0.5, (gf, cf)


def test_full_and_dump_outputs_options_exist():
    import subprocess
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr


def test_dump_outputs_writes_floats_and_a_fixed_sample(tmp_path, monkeypatch):
    """dump_outputs on host tensors: float64 scalars, arrays above their cap sampled at the same indices every time."""
    from types import SimpleNamespace
    import numpy as np
    import torch
    monkeypatch.setattr(bench, "DUMP_SAMPLE", {"generated": 1 << 20, "generator_params": 1000, "critic_params": 1 << 20})
    store = lambda n: SimpleNamespace(p=torch.arange(n, dtype=torch.float32), sync=lambda: None)
    fake = torch.randn(2, 8, 8, 16).to(torch.bfloat16)
    eng = SimpleNamespace(G=SimpleNamespace(fake=fake, P=store(5000)), C=SimpleNamespace(P=store(3000)))
    outs = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), eng, {"critic_loss": 1.5, "g_loss": -2.25})
        outs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a = outs[0]
    assert sorted(a) == ["critic_loss.npy", "critic_params.npy", "g_loss.npy", "generated.npy", "generator_params.npy"]
    assert a["critic_loss.npy"].dtype == np.float64 and a["critic_loss.npy"].tolist() == [1.5] and a["g_loss.npy"].tolist() == [-2.25]
    assert np.array_equal(a["generated.npy"], fake[..., :2].float().reshape(-1).numpy())          # under the cap: whole
    assert np.array_equal(a["critic_params.npy"], np.arange(3000, dtype=np.float32))
    g = a["generator_params.npy"]                                                                 # over the cap: sampled
    assert g.dtype == np.float32 and g.shape == (1000,) and (np.diff(g) >= 0).all() and g.max() < 5000
    assert all(np.array_equal(outs[0][f], outs[1][f]) for f in a)
