"""Builds the executed reference: upstream's OpenCL C kernels, compiled for the host.

TEST INFRASTRUCTURE ONLY. Reads the kernel sources from the upstream cl_ops tree
(CLO_REFERENCE_DIR, default /root/reference), assembles every translation unit in
memory exactly as upstream's host code does, compiles it with the ROCm clang as
OpenCL C 1.2 for x86-64, and links it with oracle/clo_ref_rt.c (the work-item
built-ins and the launch loop) and a generated wrapper per kernel into
oracle/_ref/libclo_ref_<config>.so. Nothing of the reference is written to a
tracked file; oracle/_ref/ is ignored by git.

How each unit is put together (paths relative to the tree's src/):
  sorts     cl_ops/sort/clo_sort_abstract.c:144-168: four #define lines, then the source
  satradix  cl_ops/sort/clo_sort_satradix.c:425: "#define CLO_SORT_NUM_BITS n" before the source
  scan      cl_ops/scan/clo_scan_abstract.c:122-125: -DCLO_SCAN_ELEM_TYPE= -DCLO_SCAN_SUM_TYPE=
  rng       cl_ops/rng/clo_rng.c:371-372: workitem + generator + api, then
            benchmarks/clo_rng_bench.c:184-185: the bench kernel (167-168: -D CLO_RNG_BENCHMARK_MAXINT)
  rng init  cl_ops/rng/clo_rng.c:108-109: "#define CLO_RNG_HASH(x) hash", generator, init kernel

Usage: python oracle/ref_build.py [-j JOBS] [--list]
"""
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
RT = os.path.join(HERE, "clo_ref_rt.c")
CLANG = os.environ.get("CLO_REF_CLANG", "/opt/rocm/llvm/bin/clang")
CLFLAGS = ["-x", "cl", "-cl-std=CL1.2", "-Xclang", "-finclude-default-header",
           "-target", "x86_64-unknown-linux-gnu", "-O1", "-fPIC", "-w"]

INT_TYPES = ["uint", "ulong", "int", "long", "ushort", "uchar"]
KEY_TYPES = INT_TYPES + ["float", "double"]
# (elem, key, CLO_SORT_KEY_GET or None): whole-element keys, and a key in the high word of a ulong
PAIR_UINT = ("ulong", "uint", "(uint) ((x) >> 32)")
PAIR_FLOAT = ("ulong", "float", "as_float((uint) ((x) >> 32))")
COMPARES = {"asc": None, "desc": "((a) < (b))"}

SCAN_PAIRS = [
    # the integer pairs of the GPU parity and fuzz tests
    ("uint", "uint"), ("uint", "ulong"), ("uchar", "uint"), ("int", "long"), ("ushort", "ushort"), ("ulong", "ulong"),
    ("uchar", "ushort"), ("ushort", "ulong"),
    # narrower sums
    ("ulong", "uint"), ("uint", "uchar"), ("long", "short"), ("int", "ushort"), ("ulong", "int"),
    # floating-point elements into integer sums, integer elements into float sums, float sums
    ("float", "uint"), ("double", "long"), ("float", "int"), ("double", "uchar"), ("float", "ulong"),
    ("uint", "float"), ("float", "float"), ("double", "double"),
]
RNGS = ["lcg", "xorshift64", "xorshift128", "mwc64x", "parkmiller", "tauslcg"]
HASHES = {"nohash": None, "knuth": "KNUTH(x)", "xs1": "XS1(x)"}

C_TYPES = {"char": "signed char", "uchar": "unsigned char", "short": "short", "ushort": "unsigned short",
           "int": "int", "uint": "unsigned int", "long": "long", "ulong": "unsigned long",
           "float": "float", "double": "double", "size_t": "unsigned long"}


def reference_dir():
    return os.environ.get("CLO_REFERENCE_DIR", "/root/reference")


def have_reference():
    return os.path.isfile(os.path.join(reference_dir(), "src", "cl_ops", "scan", "clo_scan_blelloch.cl"))


def _read(rel):
    with open(os.path.join(reference_dir(), "src", rel)) as f:
        return f.read()


def sort_config_name(alg, elem, key, cmp_name):
    return "%s_%s%s_%s" % (alg, elem, "" if key == elem else "_k" + key, cmp_name)


def configs():
    """{config name: (translation unit text, extra compiler options, [source files it was read from])}"""
    out = {}
    f = "cl_ops/scan/clo_scan_blelloch.cl"
    for et, st in SCAN_PAIRS:
        out["scan_%s_%s" % (et, st)] = (lambda f=f: _read(f), ["-DCLO_SCAN_ELEM_TYPE=" + et, "-DCLO_SCAN_SUM_TYPE=" + st], [f])

    def sort_unit(f, elem, key, get_key, compare, prefix=""):
        macros = ("#define CLO_SORT_ELEM_TYPE %s\n#define CLO_SORT_KEY_TYPE %s\n#define CLO_SORT_COMPARE(a, b) %s\n"
                  "#define CLO_SORT_KEY_GET(x) %s\n" % (elem, key, compare or "((a) > (b))", get_key or "(x)"))
        return macros + prefix + _read(f)

    for alg in ("sbitonic", "abitonic", "gselect"):
        f = "cl_ops/sort/clo_sort_%s.cl" % alg
        for elem, key, gk in [(t, t, None) for t in KEY_TYPES] + [PAIR_UINT, PAIR_FLOAT]:
            for cn, cmp_ in COMPARES.items():
                out[sort_config_name(alg, elem, key, cn)] = (
                    lambda f=f, e=elem, k=key, g=gk, c=cmp_: sort_unit(f, e, k, g, c), [], [f])
    f = "cl_ops/sort/clo_sort_satradix.cl"
    for elem, key, gk in [(t, t, None) for t in INT_TYPES] + [PAIR_UINT]:
        for bits in range(1, 9):
            out["satradix%d_%s%s" % (bits, elem, "" if key == elem else "_k" + key)] = (
                lambda f=f, e=elem, k=key, g=gk, b=bits: sort_unit(f, e, k, g, None, "#define CLO_SORT_NUM_BITS %d\n" % b), [], [f])
    for r in RNGS:
        g = "cl_ops/rng/clo_rng_%s.cl" % r
        bench = ["cl_ops/rng/clo_rng_workitem.cl", g, "cl_ops/rng/clo_rng_api.cl", "benchmarks/clo_rng_bench.cl"]
        out["rng_%s_bits" % r] = (lambda b=bench: "".join(_read(x) for x in b), [], bench)
        out["rng_%s_maxint" % r] = (lambda b=bench: "".join(_read(x) for x in b), ["-D", "CLO_RNG_BENCHMARK_MAXINT"], bench)
        for hn, h in HASHES.items():
            init = [g, "cl_ops/rng/clo_rng_init.cl"]
            out["rng_%s_init_%s" % (r, hn)] = (
                lambda i=init, h=h: "#define CLO_RNG_HASH(x) %s\n" % (h or "x") + "".join(_read(x) for x in i), [], init)
    return out


def lib_path(config):
    return os.path.join(OUT, "libclo_ref_%s.so" % config)


_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)((?:.*\\\n)*.*)$", re.M)
_KERNEL = re.compile(r"__kernel\s+void\s+(\w+)\s*\(([^)]*)\)")


def kernels_of(text):
    """[(name, [C parameter types], reaches a barrier)] of a translation unit. A kernel needs fibers when its body
    names barrier() or a macro whose expansion does."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    yielding = {"barrier"}
    defs = _DEFINE.findall(text)
    grew = True
    while grew:
        grew = False
        for name, body in defs:
            if name not in yielding and any(re.search(r"\b%s\b" % y, body) for y in yielding):
                yielding.add(name)
                grew = True
    found = list(_KERNEL.finditer(text))
    out = []
    for i, m in enumerate(found):
        body = text[m.end():found[i + 1].start() if i + 1 < len(found) else len(text)]
        params = []
        for p in m.group(2).split(","):
            if "*" in p:
                params.append("void*")
            else:
                words = [w for w in p.split() if w not in ("const", "__private")]
                params.append(C_TYPES[words[0]])
        out.append((m.group(1), params, any(re.search(r"\b%s\b" % y, body) for y in yielding)))
    return out


def wrapper_source(kernels):
    """C text: for every kernel K, clo_ref_k_K(void** args) unpacks the argument list into K's signature, and
    clo_ref_k_K_fibers says whether K needs the fiber scheduler."""
    lines = ["/* generated by oracle/ref_build.py */"]
    for name, params, fibers in kernels:
        lines.append("void %s(%s);" % (name, ", ".join(params) or "void"))
        call = ", ".join("*(%s*) args[%d]" % (t, i) for i, t in enumerate(params))
        lines.append("void clo_ref_k_%s(void** args) { %s(%s); }" % (name, name, call))
        lines.append("const int clo_ref_k_%s_fibers = %d;" % (name, int(fibers)))
    lines.append("const char clo_ref_kernel_names[] = \"%s\";" % " ".join(k[0] for k in kernels))
    return "\n".join(lines) + "\n"


def build_one(config, unit, force=False):
    make_text, opts, sources = unit
    so = lib_path(config)
    deps = [os.path.join(reference_dir(), "src", s) for s in sources] + [RT, os.path.abspath(__file__)]
    if not force and os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(d) for d in deps):
        return config, False
    text = make_text()
    with tempfile.TemporaryDirectory(dir=OUT, prefix="tmp_" + config + "_") as tmp:
        obj, wrap = os.path.join(tmp, "k.o"), os.path.join(tmp, "w.c")
        p = subprocess.run([CLANG] + CLFLAGS + opts + ["-c", "-", "-o", obj], input=text.encode(),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if p.returncode != 0:
            raise RuntimeError("%s: OpenCL C compile failed:\n%s" % (config, p.stdout.decode()[-2000:]))
        with open(wrap, "w") as f:
            f.write(wrapper_source(kernels_of(text)))
        # no -march=native: the library travels to other machines; -Bsymbolic: every library binds to its own runtime;
        # --no-undefined: a built-in the runtime lacks fails here, not at load time
        subprocess.check_call([CLANG, "-O2", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-o", os.path.join(tmp, "lib.so"), obj, wrap, RT])
        os.replace(os.path.join(tmp, "lib.so"), so)
    return config, True


def build_all(jobs=None, force=False, quiet=False):
    """Builds every configuration that is missing or stale. Returns the number of libraries built."""
    if not have_reference():
        raise FileNotFoundError("no reference tree at %s (set CLO_REFERENCE_DIR)" % reference_dir())
    os.makedirs(OUT, exist_ok=True)
    jobs = min(8, jobs or os.cpu_count() or 1)
    cfg = configs()
    built = 0
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for config, did in ex.map(lambda kv: build_one(kv[0], kv[1], force), cfg.items()):
            built += did
    if not quiet:
        print("oracle/_ref: %d configurations, %d built, %d up to date" % (len(cfg), built, len(cfg) - built))
    return built


if __name__ == "__main__":
    if "--list" in sys.argv:
        print("\n".join(sorted(configs())))
        sys.exit(0)
    j = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else None
    build_all(j, force="--force" in sys.argv)
