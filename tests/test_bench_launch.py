"""bench.py's launching paths on CPU (`--dry-run`: gloo, CPU tensors, numpy stand-ins
of the device steps — tests/numpy_ops.py). What is under test: that
`python bench.py --gpus N` with no launcher around it starts N fresh ranks by
itself, that the driver's `python -m torch.distributed.run ... bench.py --gpus N`
form works too, and that the one JSON line carries the weak / strong / uint64
legs with the rank count really seen. Nothing here is a measurement."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _line(proc):
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0: %r" % proc.stdout[-500:]
    return json.loads(lines[0])


def _check(d, world):
    assert d["n_gpus"] == world and d["correct"] is True and d["scaling"] == "weak"
    assert d["ranks_seen"] == {"world_size": world, "allreduce_of_ones": world}
    assert d["data"].startswith("dry-run")
    assert set(d["phases_ms"]) == {"partition", "count_exchange", "key_exchange", "local_sort"}
    for leg in ("strong", "config5_u64"):
        assert d[leg]["correct"] is True and d[leg]["ranks_seen"]["allreduce_of_ones"] == world
    # every leg says what it sent over the links and how the local sort stands against the HBM peak
    for leg in (d, d["strong"], d["config5_u64"]):
        x = leg["exchange_stats"]
        assert x["bytes_out_per_gpu"] > 0 and x["xgmi_peak_GBps"] == round((world - 1) * 153.0, 1)
        assert x["key_exchange_GBps"] > 0 and x["xgmi_frac"] > 0 and x["slices"] >= 1
    assert d["roofline"]["bound"] == "hbm" and d["roofline"]["bytes"] > 0 and d["roofline"]["frac"] > 0
    assert d["strong"]["local_sort_roofline"]["bytes"] > 0
    assert d["strong"]["elements_total"] == d["config"]["elements_per_gpu"]           # the same array, split N ways
    assert d["config5_u64"]["dtype"] == "u64" and d["config5_u64"]["elements_per_gpu"] == d["config"]["elements_per_gpu"]


@pytest.mark.parametrize("world", [2, 8])
def test_plain_invocation_launches_its_own_ranks(world):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(world), "--steps", "2", "--warmup", "1", "--dry-run",
                        "--log2n", "11"], capture_output=True, text=True, env=env, timeout=600)
    _check(_line(p), world)


def test_drivers_torchrun_form():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--steps", "2",
                        "--warmup", "1", "--dry-run", "--log2n", "11"], capture_output=True, text=True, timeout=600)
    _check(_line(p), 2)


def test_reference_round_trip_yardstick():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.reference_bitonic_round_trips(26) == 58           # G_ref at 2^26, lws 1024
    assert bench.reference_bitonic_round_trips(12) == 12
    assert bench.contract_bytes_per_elem("satradix_u32", 16, 28) == 96
    assert bench.contract_bytes_per_elem("sbitonic", 16, 16) == 8 * 136


def test_dump_outputs_are_exact_float64_within_the_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    small = np.sort(bench.make_input("satradix_u32", 5000, 1))
    d = bench.dump_outputs(str(tmp_path / "u32"), "satradix_u32", small)
    got = np.load(tmp_path / "u32" / "keys.npy")
    assert d["files"] == ["keys.npy"] and d["sample"] is None
    assert got.dtype == np.float64 and np.array_equal(got.astype(np.uint32), small)
    # larger than the budget: the same seeded positions every time, both 32-bit words of every sampled pair exact
    pairs = np.sort(bench.make_input("satradix_pairs", 3 << 20, 2))
    for sub in ("a", "b"):
        d = bench.dump_outputs(str(tmp_path / sub), "satradix_pairs", pairs)
    assert d["files"] == ["keys.npy", "values.npy"] and d["sample"]["positions"] == bench.DUMP_VALUES // 2
    k, v = (np.load(tmp_path / "a" / f) for f in d["files"])
    assert np.array_equal(k, np.load(tmp_path / "b" / "keys.npy")) and np.array_equal(v, np.load(tmp_path / "b" / "values.npy"))
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(pairs.size, bench.DUMP_VALUES // 2, replace=False))
    assert np.array_equal(k, (pairs[idx] >> np.uint64(32)).astype(np.float64))
    assert np.array_equal(v, (pairs[idx] & np.uint64(0xFFFFFFFF)).astype(np.float64))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--gpus", "2", "--dump-outputs", "x"]])
def test_bench_refuses_bad_arguments(argv):
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


@pytest.mark.gpu
@pytest.mark.parametrize("workload,log2n", [("satradix_u32", 16), ("satradix_pairs", 22)])
def test_bench_dumps_what_the_timed_steps_computed(tmp_path, workload, log2n):
    """`--steps K` times exactly K steps and the line says so; --dump-outputs writes the last one's result, which is
    numpy's (stable) sort of the seeded input — at every sampled position when the output exceeds the budget."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", workload,
                        "--log2n", str(log2n), "--seed", "5", "--no-cpu-baseline", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=600)
    d = _line(p)
    assert d["correct"] is True and d["steps"] == 3 and d["ms_per_step"] > 0
    host = bench.make_input(workload, 1 << log2n, 5)
    if workload == "satradix_pairs":
        want = host[np.argsort(host >> np.uint64(32), kind="stable")]
        idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(want.size, bench.DUMP_VALUES // 2, replace=False))
        assert d["dump_outputs"]["sample"]["positions"] == idx.size
        assert np.array_equal(np.load(tmp_path / "keys.npy"), (want[idx] >> np.uint64(32)).astype(np.float64))
        assert np.array_equal(np.load(tmp_path / "values.npy"), (want[idx] & np.uint64(0xFFFFFFFF)).astype(np.float64))
    else:
        assert d["dump_outputs"]["sample"] is None
        assert np.array_equal(np.load(tmp_path / "keys.npy"), np.sort(host).astype(np.float64))


def test_watchdog_ends_a_stuck_rank_with_a_nonzero_exit():
    """A leg that takes longer than --watchdog seconds (here: any leg, the limit is 50 ms) ends the rank with
    exit code 3 — a plain exit of a fresh child process — and the launcher reports failure instead of hanging."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "200", "--warmup", "1", "--dry-run", "--log2n", "15",
                        "--watchdog", "0.05"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode != 0
    assert "watchdog" in p.stderr
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]
