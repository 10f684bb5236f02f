"""bench.py contract: `--gpus N` without a launcher spawns N ranks itself, with `--full` both
halves of the metric (BERT tokens/s + ResNet-50 images/s) land in ONE JSON line, and the world
size seen by the process group is N.  A plain run is the headline half alone; `--dump-outputs`
writes what its last timed step computed."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--model", "tiny",
                          "--steps", "2", "--warmup", "1", "--full", *extra], capture_output=True, text=True,
                         env=env, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_spawns_two_ranks_and_reports_both_metrics():
    r = _run("--gpus", "2")
    # CPU/gloo: no GPU behind the ranks; the world size comes from a real collective
    assert r["n_gpus"] == 0 and r["world_size"] == 2 and r["backend"] == "gloo"
    assert r["env"]["world_size_seen_by_collective"] == 2 and r["world_size_seen_by_rccl"] is None
    assert r["step_ms_mean"] > 0 and r["step_ms_ci95"] >= 0 and r["value_ci95"] >= 0
    assert r["bucket_plan"]["buckets"] >= 1 and r["resnet50_bucket_plan"]["buckets"] >= 1
    assert r["metric"] == "bert_large_pretrain_tokens_per_sec" and r["value"] > 0
    assert r["resnet50_images_per_sec"] > 0
    assert len(r["per_rank_ms_per_step"]) == 2
    assert r["config"]["parallelism"] == "dp2" and r["config"]["global_batch"] == 8
    assert r["steps"] == 2 and r["warmup"] == 1


def _plain(*extra):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--model", "tiny",
                          "--gpus", "1", "--steps", "3", "--warmup", "1", *extra], capture_output=True, text=True,
                         env=env, timeout=600, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_dumps_reproducible_outputs(tmp_path):
    """Without --full: the BERT half alone, no baseline; --dump-outputs writes the last timed
    step's loss and updated weights as float32, identical from run to run."""
    import numpy as np
    runs = []
    for d in ("a", "b"):
        r = _plain("--dump-outputs", str(tmp_path / d))
        assert r["metric"] == "bert_large_pretrain_tokens_per_sec" and r["unit"] == "tokens/s" and r["value"] > 0
        assert r["higher_is_better"] is True and r["dtype"] == "fp32" and r["steps"] == 3
        assert r["ms_per_step"] > 0 and len(r["step_ms"]) == 3
        # value is items over the timed steps' wall time, ms_per_step that time per step
        tokens = r["config"]["global_batch"] * r["config"]["seq_len"]
        assert abs(r["value"] - tokens / (r["ms_per_step"] / 1e3)) <= 0.01 * r["value"]
        assert not any(k.startswith("resnet50") or k.startswith("eager") for k in r) and r["vs_baseline"] is None
        assert sorted(os.listdir(tmp_path / d)) == ["bert_tiny_loss.npy", "bert_tiny_weights.npy"]
        arrs = {f: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
        assert arrs["bert_tiny_loss.npy"].shape == (1,) and arrs["bert_tiny_weights.npy"].ndim == 1
        assert abs(float(arrs["bert_tiny_loss.npy"][0]) - r["config"]["loss_last_step"]) < 1e-3
        runs.append(arrs)
    for f in runs[0]:
        np.testing.assert_array_equal(runs[0][f], runs[1][f])


def test_baseline_options_need_full():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--model", "tiny",
                          "--baseline-steps", "2"], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 2 and "--full" in out.stderr


def test_bench_single_process_eager_impl():
    r = _run("--gpus", "1", "--impl", "eager")
    assert r["world_size"] == 1 and r["config"]["impl"] == "eager"
    assert r["value"] > 0 and r["resnet50_images_per_sec"] > 0


def test_bench_eight_ranks_one_node_layout():
    """The N = 8 launch of the driver's scaling run, rehearsed on gloo: 8 ranks, one JSON
    line, the max over 8 ranks, both halves through the same bucketed data-parallel path."""
    r = _run("--gpus", "8")
    assert r["world_size"] == 8 and r["env"]["world_size_seen_by_collective"] == 8
    assert len(r["per_rank_ms_per_step"]) == 8 and len(r["resnet50_per_rank_ms_per_step"]) == 8
    assert r["ms_per_step"] >= max(r["per_rank_ms_per_step"]) * 0.999
    assert r["config"]["parallelism"] == "dp8" and r["config"]["global_batch"] == 32
    assert r["value"] > 0 and r["resnet50_images_per_sec"] > 0
