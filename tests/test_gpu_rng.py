"""CloRng on the MI355X against the numpy model (tests/rng_model.py): seeds of every generator and seed type, the
fill's values and final states over state counts, sizes, bits and maxint, continued streams, run-time compiled
hashes, EXT_DEV ownership, a fill past 2^32 numbers, a fill into a torch tensor, parkmiller's step over every int32
state, and a client kernel built with hiprtc from clo_rng_get_source()."""
import ctypes as C

import numpy as np
import pytest
import torch

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
import rng_model as M

pytestmark = pytest.mark.gpu

SEED_TYPES = ["dev_gid", "host_mt", "ext_dev", "ext_host"]


@pytest.fixture(scope="module")
def dev():
    ctx = clo.Context(0)
    q = clo.Queue(ctx)
    yield ctx, q
    q.close()
    ctx.close()


def ext_seeds(name, count, seed=7):
    """Seed bytes for the external seed types, with some zero and negative states among them."""
    raw = np.random.default_rng(seed).integers(0, 2 ** 32, count * M.SEED_SIZE[name] // 4, dtype=np.uint64).astype(np.uint32)
    raw[:M.SEED_SIZE[name] // 4] = 0
    return raw


def make(name, dev, seed_type, count, main_seed=0, hash=None):
    """(Rng, model states, the EXT_DEV buffer or None)."""
    ctx, q = dev
    buf = None
    if seed_type == "dev_gid":
        r = clo.Rng(name, ctx, q, "dev_gid", None, count, main_seed, hash)
        exp = M.dev_gid_states(name, count, main_seed, hash)
    elif seed_type == "host_mt":
        r = clo.Rng(name, ctx, q, "host_mt", None, count, main_seed)
        exp = M.host_mt_states(name, count, main_seed)
    else:
        raw = ext_seeds(name, count)
        exp = M.state_from_bytes(name, raw, count)
        if seed_type == "ext_host":
            r = clo.Rng(name, ctx, q, "ext_host", raw, count)
        else:
            buf = clo.Buffer(ctx, raw.nbytes)
            buf.write(q, raw)
            r = clo.Rng(name, ctx, q, "ext_dev", buf, count)
    return r, exp, buf


@pytest.mark.parametrize("seed_type", SEED_TYPES)
@pytest.mark.parametrize("name", M.NAMES)
def test_states_after_new(dev, name, seed_type):
    for hash in ([None, "KNUTH(x)", "XS1(x)"] if seed_type == "dev_gid" else [None]):
        r, exp, buf = make(name, dev, seed_type, 1000, main_seed=12345, hash=hash)
        assert r.size == 1000 * M.SEED_SIZE[name]
        assert r.source.startswith("#define CLO_RNG_")
        assert np.array_equal(r.states(dev[1]), exp), (name, seed_type, hash)
        r.close()
        if buf:
            buf.close()


def test_zero_state_stays_zero(dev):
    r, exp, _ = make("xorshift64", dev, "dev_gid", 4, 0)
    ctx, q = dev
    out = clo.Buffer(ctx, 4 * 40)
    r.fill(q, out, 40)
    got = out.read(q, np.uint32, 40)
    assert int(r.states(q)[0]) == 0 and not np.any(got[0::4])
    r.close()
    out.close()


def check_fill(dev, name, seed_type, S, numel, bits=32, maxint=0):
    ctx, q = dev
    r, st, buf = make(name, dev, seed_type, S, main_seed=99, hash="KNUTH(x)" if seed_type == "dev_gid" else None)
    out = clo.Buffer(ctx, max(4 * numel, 4))
    r.fill(q, out, numel, bits, maxint)
    got = out.read(q, np.uint32, numel)
    exp, fin = M.fill(name, st, numel, bits, maxint)
    assert np.array_equal(got, exp), (name, seed_type, S, numel, bits, maxint)
    assert np.array_equal(r.states(q), fin)
    r.close()
    out.close()
    if buf:
        buf.close()


@pytest.mark.parametrize("name", M.NAMES)
@pytest.mark.parametrize("S,numel", [(1, 1), (1, 777), (63, 10), (63, 63), (63, 4000), (1000, 999), (1000, 1000),
                                     (1000, 123457), (1 << 20, 1000), (1 << 20, 1 << 20), (1 << 20, (3 << 20) + 5)])
def test_fill_matches_model(dev, name, S, numel):
    check_fill(dev, name, "host_mt" if S % 2 else "dev_gid", S, numel)


@pytest.mark.parametrize("name", M.NAMES)
@pytest.mark.parametrize("bits,maxint", [(1, 0), (7, 0), (32, 1), (32, 6), (32, 2 ** 31 + 1), (7, 2 ** 32 - 1)])
def test_fill_bits_and_maxint(dev, name, bits, maxint):
    check_fill(dev, name, "ext_host", 1000, 4567, bits, maxint)
    check_fill(dev, name, "dev_gid", 1 << 12, (1 << 14) + 3, bits, maxint)


@pytest.mark.parametrize("name", ["lcg", "mwc64x", "parkmiller", "tauslcg"])
def test_fill_2_28(dev, name):
    check_fill(dev, name, "dev_gid", 1 << 20, 1 << 28)


@pytest.mark.parametrize("name", M.NAMES)
def test_two_fills_continue_the_streams(dev, name):
    ctx, q = dev
    r, st, _ = make(name, dev, "host_mt", 1001, main_seed=3)
    out = clo.Buffer(ctx, 4 * 5000)
    r.fill(q, out, 2500)
    a = out.read(q, np.uint32, 2500)
    r.fill(q, out, 5000, 7)
    b = out.read(q, np.uint32, 5000)
    ea, st = M.fill(name, st, 2500)
    eb, st = M.fill(name, st, 5000, 7)
    assert np.array_equal(a, ea) and np.array_equal(b, eb) and np.array_equal(r.states(q), st)
    r.close()
    out.close()


def test_custom_hashes(dev):
    ctx, q = dev
    for name in ("xorshift128", "parkmiller"):
        for hash in ("x = x << 2", "(x * 3 + 1)"):
            r = clo.Rng(name, ctx, q, "dev_gid", None, 3000, 11, hash)
            assert np.array_equal(r.states(q), M.dev_gid_states(name, 3000, 11, hash)), (name, hash)
            r.close()
        # "(x * 3 + 1)" is an expression statement: no hash at all
        assert np.array_equal(M.dev_gid_states(name, 10, 11, "(x * 3 + 1)"), M.dev_gid_states(name, 10, 11, None))
    with pytest.raises(clo.CloError) as e:
        clo.Rng("lcg", ctx, q, "dev_gid", None, 100, 0, "x = y +")
    assert e.value.code == CLO_ERROR_ARGS and "x = y +" in e.value.message and "error" in e.value.message


def test_fill_errors(dev):
    ctx, q = dev
    r = clo.Rng("lcg", ctx, q, "dev_gid", None, 16)
    out = clo.Buffer(ctx, 40)
    for numel, bits in ((10, 0), (10, 33), (11, 32)):
        with pytest.raises(clo.CloError) as e:
            r.fill(q, out, numel, bits)
        assert e.value.code == CLO_ERROR_ARGS
    small = clo.Buffer(ctx, 16 * 8 - 1)
    with pytest.raises(clo.CloError) as e:
        clo.Rng("lcg", ctx, q, "ext_dev", small, 16)
    assert e.value.code == CLO_ERROR_ARGS
    small.close()
    r.close()
    out.close()


def test_ext_dev_buffer_survives_destroy(dev):
    ctx, q = dev
    raw = ext_seeds("tauslcg", 500)
    buf = clo.Buffer(ctx, raw.nbytes)
    buf.write(q, raw)
    r = clo.Rng("tauslcg", ctx, q, "ext_dev", buf, 500)
    out = clo.Buffer(ctx, 4 * 1000)
    r.fill(q, out, 1000)
    _, fin = M.fill("tauslcg", M.state_from_bytes("tauslcg", raw, 500), 1000)
    r.close()
    after = buf.read(q, np.uint32, raw.size).reshape(500, 4)   # the client's buffer: still there, states advanced
    assert np.array_equal(after, fin)
    buf.close()
    out.close()


def test_fill_past_2_32_numbers(dev):
    ctx, q = dev
    S, numel = 1 << 20, (1 << 32) + (1 << 20) + 3
    r, st, _ = make("xorshift64", dev, "dev_gid", S, main_seed=5)
    t = torch.empty(numel, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.fill(q, t, numel)
    q.finish()
    keep = np.unique(np.concatenate([np.arange(8), np.arange(numel - 8, numel), (1 << 32) + np.arange(-4, 4),
                                     np.random.default_rng(0).integers(0, numel, 2000)])).astype(np.int64)
    got = t[torch.from_numpy(keep).cuda()].cpu().numpy().view(np.uint32)
    exp, fin = M.fill("xorshift64", st, numel, keep=keep)
    assert np.array_equal(got, exp)
    assert np.array_equal(r.states(q), fin)
    del t
    r.close()


def test_fill_into_a_torch_tensor(dev):
    ctx, q = dev
    r, st, _ = make("mwc64x", dev, "dev_gid", 4096, main_seed=1)
    t = torch.zeros(100003, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.fill(q, t, 100003, 16)
    q.finish()
    exp, _ = M.fill("mwc64x", st, 100003, 16)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), exp)
    r.close()


def test_parkmiller_over_every_int32_state(dev):
    """Every int32 state, loaded through EXT_DEV in chunks of 2^28: one draw each against torch.fmod in int64 (C's
    truncating remainder), states and outputs both."""
    ctx, q = dev
    chunk = 1 << 28
    out = torch.empty(chunk, dtype=torch.int32, device="cuda")
    for c in range(16):
        s = torch.arange(chunk, dtype=torch.int64, device="cuda") + (c * chunk - (1 << 31))
        states = s.to(torch.int32)
        torch.cuda.synchronize()
        buf = clo.Buffer(ctx, chunk * 4, device_ptr=states.data_ptr())
        r = clo.Rng("parkmiller", ctx, q, "ext_dev", buf, chunk)
        r.fill(q, out, chunk)
        q.finish()
        exp = torch.fmod(s * 16807, 2147483647).to(torch.int32)
        assert torch.equal(states, exp), c
        assert torch.equal(out, exp << 1), c
        r.close()
        buf.close()
        del s, states, exp


# ---- a client kernel compiled with hiprtc from clo_rng_get_source() ----
def _hiprtc_compile(src, name):
    rtc = C.CDLL("libhiprtc.so.7")   # the one the library links (already loaded)
    prog = C.c_void_p()
    assert rtc.hiprtcCreateProgram(C.byref(prog), src.encode(), b"user.hip", 0, None, None) == 0
    opts = (C.c_char_p * 2)(b"--offload-arch=gfx950", b"-O3")
    st = rtc.hiprtcCompileProgram(prog, 2, opts)
    if st != 0:
        n = C.c_size_t()
        rtc.hiprtcGetProgramLogSize(prog, C.byref(n))
        log = C.create_string_buffer(n.value + 1)
        rtc.hiprtcGetProgramLog(prog, log)
        raise AssertionError(log.value.decode())
    n = C.c_size_t()
    rtc.hiprtcGetCodeSize(prog, C.byref(n))
    code = C.create_string_buffer(n.value)
    rtc.hiprtcGetCode(prog, code)
    rtc.hiprtcDestroyProgram(C.byref(prog))
    return code


USER_KERNEL = r"""
extern "C" __global__ void user_next_int4(clo_statetype* states, unsigned int* out, unsigned int n) {
	const uint4 v = clo_rng_next_int4(states, n);
	const unsigned int g = GID1(), G = GLOBAL_SIZE();
	out[g] = v.x;
	out[G + g] = v.y;
	out[2 * G + g] = v.z;
	out[3 * G + g] = v.w;
}
"""


@pytest.mark.parametrize("name", M.NAMES)
def test_client_kernel_from_get_source(dev, name):
    ctx, q = dev
    G, n = 256 * 40, 1000003
    r, st, _ = make(name, dev, "dev_gid", 4 * G, main_seed=2, hash="XS1(x)")
    code = _hiprtc_compile(r.source + USER_KERNEL, name)
    hip = C.CDLL("libamdhip64.so.7")   # the runtime the library runs on
    mod, fn = C.c_void_p(), C.c_void_p()
    assert hip.hipModuleLoadData(C.byref(mod), code) == 0
    assert hip.hipModuleGetFunction(C.byref(fn), mod, b"user_next_int4") == 0
    out = torch.zeros(4 * G, dtype=torch.int32, device="cuda")
    sp = C.c_void_p(clo.api.lib.ccl_buffer_get_device_ptr(r.device_seeds))
    op, nn = C.c_void_p(out.data_ptr()), C.c_uint(n)
    args = (C.c_void_p * 3)(C.cast(C.byref(sp), C.c_void_p), C.cast(C.byref(op), C.c_void_p), C.cast(C.byref(nn), C.c_void_p))
    torch.cuda.synchronize()
    assert hip.hipModuleLaunchKernel(fn, G // 256, 1, 1, 256, 1, 1, 0, None, args, None) == 0
    assert hip.hipDeviceSynchronize() == 0
    # GID4: work-item g draws states g, G + g, 2G + g, 3G + g once each = one fill draw of all 4G states, % n
    exp, fin = M.fill(name, st, 4 * G, maxint=n)
    assert np.array_equal(out.cpu().numpy().view(np.uint32), exp)
    assert np.array_equal(r.states(q), fin)
    hip.hipModuleUnload(mod)
    r.close()
