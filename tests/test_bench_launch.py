"""bench.py's launch logic (no GPU): `python bench.py --gpus N` must work however it is started -- as a plain process it
takes the library's single-process multi-device path (pt_multi_*), under torch.distributed.run the one-process-per-GPU
path -- and never exits just because no launcher environment is present."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_plain_process_launches(bench):
    assert bench.launch_mode(1, {}) == ("single", 1, 0, 0)
    for n in (2, 4, 8):
        assert bench.launch_mode(n, {}) == ("multi", n, 0, 0)              # the driver's `python3 bench.py --gpus N` form
    assert bench.launch_mode(1, {}, force_multi=True) == ("multi", 1, 0, 0)
    assert bench.launch_mode(1, {}, force_dist=True) == ("dist", 1, 0, 0)
    assert bench.launch_mode(1, {"WORLD_SIZE": "1", "RANK": "0"}) == ("single", 1, 0, 0)


def test_torchrun_environment_wins_over_the_flag(bench):
    env = {"WORLD_SIZE": "8", "RANK": "5", "LOCAL_RANK": "5"}
    assert bench.launch_mode(8, env) == ("dist", 8, 5, 5)
    assert bench.launch_mode(1, env) == ("dist", 8, 5, 5)
    with pytest.raises(SystemExit):
        bench.launch_mode(8, env, force_multi=True)
    with pytest.raises(SystemExit):
        bench.launch_mode(1, {}, force_dist=True, force_multi=True)


def test_workloads_name_the_baseline_configs(bench):
    assert bench.WORKLOADS["c2"][2:5] == (1024, 1024, 64)                   # BASELINE.json configs[1]: the headline
    assert bench.WORKLOADS["c3"][4] == 4096 and bench.WORKLOADS["c4"][1] == 10000 and bench.WORKLOADS["c5"][2:5] == (3840, 2160, 1024)


def test_cpu_baseline_leg_on_a_tiny_workload(bench, pt):
    """The bounded CPU sample: figures for the 16-thread share, for every visible CPU, and BASELINE configs[0]."""
    out = bench.cpu_baseline(pt, pt.builtin_scene(2), 64, 64, 2, "C2 scene")
    assert out["kind"] == "port" and out["value"] > 0 and out["cores"] >= 1
    assert out["all_cores"]["cores"] == len(os.sched_getaffinity(0)) and out["all_cores"]["value"] > 0
    assert out["config0_single_thread"]["cores"] == 1


def test_the_timed_regions_counters_are_checked_against_the_job(bench):
    """bench.py's own verification of its overlapped timed region: exact device counters, or a problem."""
    per3 = {"vertices": 3 * 329_000_001, "shadow_rays": 3 * 250_000_007}
    good = {"samples": 20 * 67_108_864, "samples_expected": 20 * 67_108_864, "vertices": 20 * 329_000_001, "shadow_rays": 20 * 250_000_007}
    assert bench.counter_problems("t", good, 20 * 67_108_864, 20, per3, 3) == []
    assert bench.counter_problems("t", good, 20 * 67_108_864, 20) == []
    lost = dict(good, samples=int(good["samples"] * 0.97))                      # round 4's race: 3 % of the samples lost
    assert any("finished" in p for p in bench.counter_problems("t", lost, 20 * 67_108_864, 20, per3, 3))
    off = dict(good, vertices=good["vertices"] - 64)
    assert any("vertices" in p for p in bench.counter_problems("t", off, 20 * 67_108_864, 20, per3, 3))
    assert any("vertices" in p for p in bench.counter_problems("t", dict(good, vertices=good["vertices"] + 1), 20 * 67_108_864, 20))
    wrong_job = bench.counter_problems("t", good, 19 * 67_108_864, 20, per3, 3)
    assert wrong_job and "renders of the job" in wrong_job[0]


def test_dump_outputs_writes_float32_planes_and_samples_large_frames(bench, tmp_path, monkeypatch):
    """--dump-outputs: both film planes as float32; above the size cap, the same seeded pixels of both planes and their indices."""
    import numpy as np
    import torch
    lin = torch.rand((48, 40, 3), dtype=torch.float32, generator=torch.Generator().manual_seed(1))
    rgba = torch.randint(0, 256, (48, 40, 4), dtype=torch.uint8, generator=torch.Generator().manual_seed(2))
    bench.dump_outputs(str(tmp_path / "full"), lin, rgba)
    got_lin, got_rgba = np.load(tmp_path / "full" / "linear.npy"), np.load(tmp_path / "full" / "rgba8.npy")
    assert got_lin.dtype == np.float32 and got_rgba.dtype == np.float32
    assert np.array_equal(got_lin, lin.numpy()) and np.array_equal(got_rgba, rgba.numpy().astype(np.float32))
    assert not (tmp_path / "full" / "pixel_index.npy").exists()

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_PIXELS", 100)
    runs = []
    for k in range(2):
        out = tmp_path / f"sampled{k}"
        bench.dump_outputs(str(out), lin, rgba)
        runs.append({n: np.load(out / f"{n}.npy") for n in ("linear", "rgba8", "pixel_index")})
    a, b = runs
    assert all(np.array_equal(a[n], b[n]) for n in a)                    # the same sample in every run
    idx = a["pixel_index"]
    assert idx.dtype == np.float64 and idx.shape == (100,) and len(np.unique(idx)) == 100
    i = idx.astype(np.int64)
    assert np.array_equal(a["linear"], lin.numpy().reshape(-1, 3)[i]) and np.array_equal(a["rgba8"], rgba.numpy().reshape(-1, 4)[i].astype(np.float32))
    assert sum(v.nbytes for v in a.values()) <= 64 << 20


def test_the_largest_workload_dumps_under_the_cap(bench):
    """C5 (3840 x 2160) is above 64 MB as float32 planes: its sample, with the index, must fit."""
    w, h = bench.WORKLOADS["c5"][2:4]
    assert w * h * (3 + 4) * 4 > bench.DUMP_MAX_BYTES
    assert bench.DUMP_SAMPLE_PIXELS * ((3 + 4) * 4 + 8) <= bench.DUMP_MAX_BYTES
    for name, (_, _, w, h, _, _) in bench.WORKLOADS.items():
        assert min(w * h, bench.DUMP_SAMPLE_PIXELS) * ((3 + 4) * 4 + 8) <= bench.DUMP_MAX_BYTES, name
