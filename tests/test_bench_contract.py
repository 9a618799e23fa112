"""bench.py's output contract: ONE JSON line on stdout with the driver's keys, values that are consistent with each other
(value = rays per step / time per step), the roofline and cpu_baseline objects of a --full run, and the outputs a plain run
writes with --dump-outputs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_default_shape_bench_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--full"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines  # exactly one line, and it is JSON
    d = json.loads(lines[0])
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["metric"] == "training rays/sec" and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["dtype"].startswith("f32 (f16x3") and d["world_size_observed"] == 1
    assert d["config"]["launch"].startswith("HIP graph replay") and d["graph_stats"]["replays"] >= 4 + 2
    assert d["host_issue_ms_per_step"] < 6.0  # the host no longer paces the step
    assert set(d["phases"]) == {"0.05", "0.3", "0.8"} and all(v["value"] > 50_000 for v in d["phases"].values())
    assert d["phases"]["0.3"]["value"] == d["value"]
    assert d["strict_f32"]["dtype"] == "f32" and 50_000 < d["strict_f32"]["value"] < d["value"]
    assert d["wgrad_f16"]["value"] > 0.95 * d["value"] and "option" in d["wgrad_f16"]["note"]
    rays = d["config"]["rays_per_gpu"]
    assert rays == 4096 and d["config"]["N_samples"] == 64 and d["config"]["N_importance"] == 128
    assert abs(d["value"] - rays / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert 50_000 < d["value"] < 5_000_000
    r = d["roofline"]
    assert r["bound"] in ("mfma", "hbm") and r["unit"] in ("TFLOP/s", "GB/s") and r["peak"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.05 < r["frac"] < 1.0
    assert r["traffic"] is None or (r["traffic"] > 0 and r["traffic_source"])
    # the executed fraction (composite-then-project removed ~20 % of the reference's per-sample MACs) and
    # the step-level floors ride in the line
    assert 0.7 * r["frac"] < r["executed_frac"] < r["frac"]
    st = r["step"]
    assert abs(st["algorithmic_tflop"] - d["algorithmic_tflop_per_step"]) < 1e-9 and 4.0 < st["algorithmic_tflop"] < 6.0
    assert abs(st["mfma_floor_ms"] - st["algorithmic_tflop"] / r["peak"] * 1e3) < 1e-9
    assert abs(st["algorithmic_tflops"] - st["algorithmic_tflop"] / (d["ms_per_step"] * 1e-3)) < 1e-6 * st["algorithmic_tflops"]
    assert (st["hbm_floor_ms"] is None) == (r["hbm_bytes_per_step"] is None)
    if st["hbm_floor_ms"] is not None:
        assert abs(st["hbm_floor_ms"] - r["hbm_bytes_per_step"] / 6.29e12 * 1e3) < 1e-9 and st["binding_floor"] in ("hbm", "mfma")
    assert abs(st["frac_of_floor"] - max(st["mfma_floor_ms"], st["hbm_floor_ms"] or 0.0) / d["ms_per_step"]) < 1e-9
    assert 0.1 < st["frac_of_floor"] < 1.0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["unit"] == "rays/s" and c["cores"] >= 1 and c["value"] > 0
    assert isinstance(c["sample"], str) and c["sample"]
    assert d["value"] / c["value"] > 10  # north_star: >= 10x the CPU path
    # BASELINE.json configs[3] and configs[4] ride in the same line
    t = d["trevi"]
    assert t["config"]["rays_per_gpu"] == 8192 and t["config"]["n_images"] == 1689 and t["dtype"].startswith("f16")
    assert abs(t["value"] - 8192 / (t["ms_per_step"] * 1e-3)) < 1e-6 * t["value"] and t["value"] > 100_000
    assert t["roofline"]["peak"] > 2000 and 0.02 < t["roofline"]["frac"] < 1.0
    assert 0.7 * t["roofline"]["frac"] < t["roofline"]["executed_frac"] < t["roofline"]["frac"] and "frac_of_floor" in t["roofline"]["step"]
    o = d["tto"]
    for st in ("pose_stage", "appearance_stage"):
        assert o["rays_per_step"] == 1024 and abs(o[st]["value"] - 1024 / (o[st]["ms_per_step"] * 1e-3)) < 1e-6 * o[st]["value"]
        assert o[st]["value"] > 20_000
    assert o["render"]["no_grad"] is True and o["render"]["value"] > 100_000 and o["render"]["chunk"] == 4096


@pytest.mark.gpu
def test_plain_bench_line_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps replayed steps and nothing else; --dump-outputs writes the loss and its
    terms, the parameters after the update and the gradients of the last timed step, float32, within 64 MB.  The same
    arguments give the same outputs bit for bit (seeded inputs, deterministic step); one more timed step changes them."""
    import numpy as np

    def plain(name, steps):
        d = tmp_path / name
        out = _run(["--gpus", "1", "--steps", str(steps), "--warmup", "2", "--dump-outputs", str(d)], timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        assert all(f.endswith(".npy") for f in os.listdir(d))
        return json.loads(lines[0]), {f[:-len(".npy")]: np.load(d / f) for f in os.listdir(d)}

    d, files = plain("a", 3)
    assert d["metric"] == "training rays/sec" and d["unit"] == "rays/s" and d["higher_is_better"] is True
    assert d["dtype"].startswith("f32 (f16x3") and d["steps"] == 3 and d["warmup"] == 2
    assert abs(d["value"] - 4096 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    # the first call runs eagerly, the second is captured and replayed, then warm-up and timed steps replay
    assert d["graph_stats"] == {"eager": 1, "captures": 1, "replays": 1 + 2 + 3}
    for k in ("value_spread", "phases", "strict_f32", "wgrad_f16", "trevi", "tto", "kernels", "roofline", "cpu_baseline"):
        assert d.get(k) is None, k
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert files["loss"].size == 1 and "param.nerf_fine.xyz_encoding_1.0.weight" in files
    assert np.abs(files["grad.nerf_fine.xyz_encoding_1.0.weight"]).max() > 0 and np.abs(files["grad.se3_refine.weight"]).max() > 0
    terms = [float(a.sum()) for k, a in files.items() if k.startswith("loss.")]
    loss = float(files["loss"].reshape(()))
    assert terms and abs(sum(terms) - loss) <= 1e-4 * max(1e-2, abs(loss))  # the terms of the same step as the loss
    _, again = plain("b", 3)
    assert sorted(again) == sorted(files) and all(np.array_equal(files[k], again[k]) for k in files)
    _, later = plain("c", 4)
    assert sorted(later) == sorted(files)
    w = "param.nerf_fine.xyz_encoding_1.0.weight"
    assert not np.array_equal(files[w], later[w]) and not np.array_equal(files["loss"], later["loss"])


def _run(args, env=None, timeout=300):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT, env=e)


def test_gpus_n_without_torchrun_spawns_n_ranks():
    """`python bench.py --gpus 2` with no torchrun environment must start two ranks itself (fresh processes) -- never run
    one rank silently; checked on the plumbing-only path (gloo, no GPU needed)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["UPNERF_DIST_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                          "--dry-run"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_observed"] == 2 and d["backend"] == "gloo" and d["dry_run"] is True
    assert d["config"]["parallelism"] == "dp2" and d["steps"] == 3


def test_eight_ranks_dry_run_is_the_line_the_scale_run_expects():
    """what the driver's 8-GPU run will do first -- spawn eight ranks, rendezvous, barrier, max over ranks,
    ONE line from rank 0 that says dp8 -- on the plumbing-only path (gloo on CPU)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["UPNERF_DIST_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "2", "--warmup", "1",
                          "--dry-run"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["world_size_observed"] == 8 and d["config"]["parallelism"] == "dp8" and d["scaling"] == "weak"
    assert d["backend"] == "gloo" and d["dry_run"] is True and d["steps"] == 2
    # an N > 1 line attributes its communication -- time inside the all-reduces, bytes per rank and step, how
    # often the early (fine-field) bucket went out -- and roofline.step subtracts it
    c = d["comm"]
    assert set(c) >= {"allreduce_ms", "bytes", "allreduces_per_step", "early_launches", "late_only", "clock", "placement"}
    assert c["bytes"] == 4 * (823_000 + 1_426_577) and c["allreduce_ms"] > 0
    # the first step of a phase learns the early count (late only), the second launches the early bucket
    assert c["late_only"] == 1 and c["early_launches"] == 1 and c["allreduces_per_step"] == 1.5
    st = d["roofline"]["step"]
    assert abs(st["compute_ms"] - (d["ms_per_step"] - c["allreduce_ms"])) < 1e-9 and st["comm_ms"] == c["allreduce_ms"]


def test_a_dead_rank_is_a_nonzero_exit():
    """A rank that dies before the rendezvous completes must fail the whole run (non-zero exit, no JSON line that looks like a
    measurement) instead of hanging or reporting the survivors."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["UPNERF_DIST_BACKEND"] = "gloo"
    env["UPNERF_BENCH_KILL_RANK"] = "1"  # test hook of bench.py: this rank exits(3) right after parsing its arguments
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--dry-run"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert out.returncode != 0
    assert not [l for l in out.stdout.splitlines() if l.strip().startswith("{")], out.stdout


def test_strong_scaling_dry_run_splits_the_batch():
    """--strong: the configuration's 4096 rays are split over the ranks; the line says so."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["UPNERF_DIST_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--dry-run", "--strong"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.strip().startswith("{")][0])
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 and d["world_size_observed"] == 2


def test_world_size_mismatch_is_an_error():
    """A launcher environment that disagrees with --gpus must fail, not measure something else."""
    out = _run(["--gpus", "2", "--dry-run"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0 and "WORLD_SIZE=1" in (out.stderr + out.stdout)


@pytest.mark.gpu
def test_two_ranks_spawned_on_one_device_run_the_real_step():
    """The spawn path with the real workload: two ranks share cuda:0 through gloo (diagnostic switches of parallel.py),
    graph replay with the all-reduce between the two graphs of a step."""
    args, env = ["--gpus", "2", "--steps", "3", "--warmup", "1", "--no-extras", "--no-kernel-timing"], \
        {"UPNERF_DIST_BACKEND": "gloo", "UPNERF_SHARE_DEVICE": "1"}
    try:  # (the run takes ~5 s; a rendezvous that never completes was seen once in a round of runs: one retry on a fresh port)
        out = _run(args, env=env, timeout=240)
    except subprocess.TimeoutExpired:
        out = _run(args, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["world_size_observed"] == 2 and d["graph_stats"]["replays"] >= 4
    assert abs(d["value"] - 2 * 4096 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    c = d["comm"]  # the exchange of the replayed step: one flat all-reduce between the two graphs
    assert 8.0e6 < c["bytes"] < 9.5e6 and c["allreduces_per_step"] == 1.0 and 0 < c["allreduce_ms"] < d["ms_per_step"]
    assert c["placement"].startswith("between the two HIP graphs")
