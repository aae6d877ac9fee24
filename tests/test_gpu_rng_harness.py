"""benchmarks/clo_hip_rng_bench (upstream's clo_rng_bench CLI) on the MI355X: its per-launch path compiles
clo_rng_get_source() + the bench kernel with hiprtc and makes one draw per state per launch; every output form
equals the numpy model (tests/rng_model.py), for every generator, with device GID seeds and host MT seeds."""
import os
import subprocess

import numpy as np
import pytest

import rng_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "benchmarks", "bin", "clo_hip_rng_bench")


def run(args, cwd=None):
    r = subprocess.run([BENCH] + args, capture_output=True, timeout=300, cwd=cwd)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout


def model(name, gws, runs, seed, hash, bits=32, maxint=0):
    st = M.dev_gid_states(name, gws, seed, hash) if hash else M.host_mt_states(name, gws, seed)
    return M.fill(name, st, gws * runs, bits, maxint)[0]


@pytest.mark.parametrize("name", M.NAMES)
@pytest.mark.parametrize("hash", ["KNUTH(x)", None])
def test_stdout_forms_match_the_model(name, hash):
    gws, runs, seed = 1000, 3, 17
    extra = ["-h", hash] if hash else []
    txt = run(["-r", name, "-o", "stdout-uint", "-g", str(gws), "-n", str(runs), "-s", str(seed)] + extra)
    got = np.array(txt.split(), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(got, model(name, gws, runs, seed, hash))
    raw = run(["-r", name, "-o", "stdout-bin", "-g", str(gws), "-n", str(runs), "-s", str(seed), "-b", "7"] + extra)
    assert np.array_equal(np.frombuffer(raw, dtype=np.uint32), model(name, gws, runs, seed, hash, bits=7))
    raw = run(["-r", name, "-o", "stdout-bin", "-g", str(gws), "-n", "2", "-s", str(seed), "-m", "6"] + extra)
    assert np.array_equal(np.frombuffer(raw, dtype=np.uint32), model(name, gws, 2, seed, hash, maxint=6))


def test_file_dh_header(tmp_path):
    run(["-r", "xorshift128", "-o", "file-dh", "-g", "512", "-n", "4", "-h", "XS1(x)", "-b", "16"], cwd=str(tmp_path))
    text = (tmp_path / "out_xorshift128_gid_XS1(x).dh.txt").read_text().split("\n")
    assert text[:3] == ["type: d", "count: 2048", "numbit: 16"]
    got = np.array(text[3:-1], dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(got, model("xorshift128", 512, 4, 0, "XS1(x)", bits=16))
    run(["-r", "lcg", "-o", "file-tsv", "-g", "100", "-n", "2"], cwd=str(tmp_path))
    rows = (tmp_path / "out_lcg_host_mt.tsv").read_text().rstrip("\n").split("\n")
    assert len(rows) == 2 and all(len(r.rstrip("\t").split("\t")) == 100 for r in rows)


def test_none_output_fill_against_launches():
    out = run(["-r", "parkmiller", "-o", "none", "-g", str(1 << 16), "-n", "16", "-h", "KNUTH(x)"]).decode()
    assert "states_match=1" in out and "fill_ms=" in out and "peak_share=" in out
