"""bench.py's own multi-rank launch (`python bench.py --gpus N` with no torchrun around it), rehearsed on the CPU with
a stand-in step: N rank processes are started, meet at the barriers, and rank 0 reports n_gpus = N with the MAX over
ranks as the step time."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=180)


def test_self_launch_two_ranks_stub():
    p = _run(["--gpus", "2", "--steps", "5", "--warmup", "1"], ARREAU_BENCH_STUB="1")
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout  # ONE line on stdout: rank 0's result, nothing a library printed (gloo announces itself)
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 5 and len(d["per_rank_ms"]) == 2
    assert d["per_rank_ms"][1] > d["per_rank_ms"][0]  # the stub's rank 1 is slower ...
    assert d["ms_per_step"] >= max(d["per_rank_ms"])  # ... and the reported time covers the slowest rank
    # the line proves its ranks: backend and size as the process group sees them, one record per rank from distinct processes
    r = d["ranks"]
    assert r["backend"] == "gloo" and r["world_size"] == 2 and r["data_path_collectives"] == 0
    assert [x["rank"] for x in r["per_rank"]] == [0, 1] and len({x["pid"] for x in r["per_rank"]}) == 2


def test_self_launch_refuses_when_gpus_are_missing():
    """Without the stub, asking for more GPUs than are visible must fail loudly (never a silent 1-GPU run)."""
    sys.path.insert(0, ROOT)
    import bench
    want = bench.visible_gpu_count() + 2
    p = _run(["--gpus", str(want), "--steps", "1", "--warmup", "0"])
    assert p.returncode != 0
    assert "GPU(s) are visible" in p.stderr and not p.stdout.strip()


def test_gpu_count_comes_from_sysfs_and_visibility_lists(monkeypatch):
    """The launcher parent counts devices without calling into HIP: KFD topology + *_VISIBLE_DEVICES."""
    sys.path.insert(0, ROOT)
    import bench
    base = bench.visible_gpu_count()
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0")
    assert bench.visible_gpu_count() == min(base, 1)
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    assert bench.visible_gpu_count() == 0
    src = open(BENCH).read()
    body = src[src.index("def launch_ranks"):src.index("def main()")]
    assert "import torch" not in body and "device_count" not in body


def test_dump_outputs_files_dtypes_and_budget(tmp_path):
    """--dump-outputs: one <name>.npy per output in float32 (float64 kept); over the budget every array keeps the same seeded
    sample of its rows, identical from call to call; rank r > 0 writes <name>.rank<r>.npy within its share of the budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    frac = np.arange(3000, dtype=np.float32).reshape(1000, 3)
    types = np.arange(1000, dtype=np.int32)
    loss = np.array([0.25])
    bench.dump_outputs(str(tmp_path / "all"), {"frac": frac, "types": types, "loss": loss})
    got = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in ("frac", "types", "loss")}
    assert got["frac"].dtype == np.float32 and got["types"].dtype == np.float32 and got["loss"].dtype == np.float64
    np.testing.assert_array_equal(got["frac"], frac)
    np.testing.assert_array_equal(got["types"], types)
    assert float(got["loss"][0]) == 0.25
    budget = 8000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"frac": frac, "types": types}, budget=budget)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("frac", "types")}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in ("frac", "types")}
    assert 0 < sum(v.nbytes for v in a.values()) <= budget
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["frac"], frac[a["types"].astype(np.int64)])  # the same rows of every array
    bench.dump_outputs(str(tmp_path / "r1"), {"frac": frac}, rank=1, world=2, budget=budget)
    r1 = np.load(tmp_path / "r1" / "frac.rank1.npy")
    assert os.listdir(tmp_path / "r1") == ["frac.rank1.npy"] and 0 < r1.nbytes <= budget // 2


def test_world_size_mismatch_is_an_error():
    p = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], ARREAU_BENCH_STUB="1", WORLD_SIZE="2", RANK="0")
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr
