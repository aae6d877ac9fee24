"""The host layer the eight operation drivers share (cl_ops_amd/csrc/clo_internal.h, clo_op_host.c) on the CPU: the
stand-alone program tests/op_host/op_host_test.c checks range overlap and the order of the conflict helper, the key
kind of all eleven types, the name lookup, the object head and the staging of a host-data call (round trips, and the
failure on a context without a device with err and with err == NULL) over the host stubs of the thin C-ABI
(tests/hoststub/*stub*.c), under AddressSanitizer + UBSan, whose leak check covers what a failed call leaves behind.
The drivers must keep no copy of what the layer holds; nor may the sort and scan drivers that use the named stage and
the copy-out helper of clo_host_pipe.c."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cl_ops_amd", "csrc")
DRIVERS = ("clo_histogram.c", "clo_reduce_by_key.c", "clo_scan_by_key.c", "clo_merge.c", "clo_search.c", "clo_setop.c",
           "clo_select.c", "clo_topk.c")


def test_helpers_under_sanitizers(tmp_path):
    exe = str(tmp_path / "op_host")
    srcs = (sorted(glob.glob(os.path.join(CSRC, "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "op_host", "op_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("op host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def test_the_drivers_keep_no_copy_of_the_shared_layer():
    for name in DRIVERS:
        text = open(os.path.join(CSRC, name)).read()
        assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M), name
        for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
            assert word not in text, (name, word)
        assert "clo_op_head head;" in text and "clo_stage_close(" in text, name
    # the upstream-shaped sort and scan drivers: their host-data calls stand on the stage, their pipelines on the drain
    for name in ("clo_sort_abstract.c", "clo_scan_abstract.c", "clo_sort_satradix.c"):
        text = open(os.path.join(CSRC, name)).read()
        assert "pthread_" not in text, name
        if name != "clo_sort_satradix.c":
            for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new("):
                assert word not in text, (name, word)
            assert "clo_stage_close(" in text, name
