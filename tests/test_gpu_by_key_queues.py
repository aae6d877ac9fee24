"""The by-key sort, CloReduceByKey, CloScanByKey, CloHistogram, CloMerge, CloSearch, CloSetOp, CloSelect, CloTopK, CloExpand,
CloSegReduce, CloSegSort and CloSegScan on the queue production uses (no profiling) and across queues. Every driver keeps its workspace behind a stream guard ("the workspace
belongs to one queue at a time"): one object is called six times on two live queues in turn, with no host
synchronisation between the calls and sizes that make it reuse and outgrow its workspace mid-sequence; then the queue of
its last call is destroyed and the object is used on a third one, through the host-data and the device form. Last, the
whole group-by pipeline (sort by key -> scan by key -> reduce by key -> histogram of the reduced keys -> merge of two
such outputs) runs on one non-profiling queue without a finish() until the end, and gives the bits of the same pipeline
on the session's profiling queue and of numpy. The results are compared, not the interleavings; everything is exact."""
import numpy as np
import pytest

from expand_model import expand
from hist_model import histogram
from merge_model import merge, order_key
from rbk_model import rbk
from sbk_model import sbk
from search_model import search
from segreduce_model import segreduce
from segscan_model import segscan
from segsort_model import segsort
from select_model import select
from setop_model import setop
from topk_model import topk
from test_gpu_reduce_by_key import structure, make_keys, make_values

pytestmark = pytest.mark.gpu

BIG = (1 << 22) + 3
SIZES = [4099, BIG, 3001, BIG, 5003, BIG + 8192]      # outgrown at the second call, reused small and large, outgrown again
LOWER, SHIFT, BINS = 1000, 2, 4096


class _SortByKey:
    """ushort keys, uint values carried along. Arrays: (keys, values) -> (keys_out, values_out)."""
    out_types = (np.uint16, np.uint32)

    def new(self, clo, ctx):
        return clo.Sorter("satradix", ctx, "ushort")

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        return rng.integers(0, 1 << 16, n, dtype=np.uint16), rng.integers(0, 1 << 32, n, dtype=np.uint32)

    def out_counts(self, ins):
        return ins[0].size, ins[0].size

    def call(self, obj, q, i, o, ins):
        return obj.by_key_with_device_data(q, i[0], i[1], o[0], o[1], ins[0].size)

    def want(self, ins):
        order = np.argsort(order_key(ins[0]), kind="stable")
        return ins[0][order], ins[1][order]

    def host(self, obj, q, ins):
        return obj.by_key_with_host_data(ins[0], ins[1], q_exec=q)


class _ReduceByKey:
    """uint keys in runs of 100 on average, uint values summed in ulong. -> (keys_out, aggr_out, the run count)."""
    out_types = (np.uint32, np.uint64, np.uint64)

    def new(self, clo, ctx):
        return clo.ReduceByKey(ctx, "uint", "uint", "ulong")

    def inputs(self, n, seed):
        return make_keys("uint", structure("geo100", n, 0, seed=seed), seed=seed % 7), make_values("uint", n, seed)

    def out_counts(self, ins):
        return ins[0].size, ins[0].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], o[0], o[1], o[2], ins[0].size)

    def want(self, ins):
        wk, wa, m = rbk(ins[0], ins[1], "sum", np.uint64)
        return wk, wa, np.array([m], np.uint64)

    def host(self, obj, q, ins):
        ko, ao = obj.with_host_data(ins[0], ins[1], q_exec=q)
        return ko, ao, np.array([ko.size], np.uint64)


class _ScanByKey(_ReduceByKey):
    """The same inputs; the exclusive running sum in uint (it wraps)."""
    out_types = (np.uint32,)

    def new(self, clo, ctx):
        return clo.ScanByKey(ctx, "uint", "uint", "uint")

    def out_counts(self, ins):
        return (ins[0].size,)

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], o[0], ins[0].size)

    def want(self, ins):
        return (sbk(ins[0], ins[1], "sum", np.uint32, False),)

    def host(self, obj, q, ins):
        return (obj.with_host_data(ins[0], ins[1], q_exec=q),)


class _Histogram:
    """uint keys, a tenth of them outside the range, uint values summed in ulong per bin."""
    out_types = (np.uint64,)

    def new(self, clo, ctx):
        return clo.Histogram(ctx, "uint", "uint", "ulong")

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        return (rng.integers(LOWER - 500, LOWER + (BINS << SHIFT) + 1200, n, dtype=np.int64).astype(np.uint32),
                rng.integers(0, 1 << 32, n, dtype=np.uint32))

    def out_counts(self, ins):
        return (BINS,)

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], o[0], ins[0].size, lower=LOWER, shift=SHIFT, num_bins=BINS)

    def want(self, ins):
        return (histogram(ins[0], ins[1], np.uint64, LOWER, SHIFT, BINS),)

    def host(self, obj, q, ins):
        return (obj.with_host_data(ins[0], ins[1], lower=LOWER, shift=SHIFT, num_bins=BINS, q_exec=q),)


class _Merge:
    """n ushort keys in A and a third as many in B, many ties inside and across; uint values = the source index."""
    out_types = (np.uint16, np.uint32)

    def new(self, clo, ctx):
        return clo.Merge(ctx, "ushort", 4)

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        na, nb = n - n // 3, n // 3
        v = np.arange(n, dtype=np.uint32)
        return np.sort(rng.integers(0, 5000, na).astype(np.uint16)), v[:na], np.sort(rng.integers(0, 5000, nb).astype(np.uint16)), v[na:]

    def out_counts(self, ins):
        return ins[0].size + ins[2].size, ins[0].size + ins[2].size

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], ins[0].size, i[2], i[3], ins[2].size, o[0], o[1])

    def want(self, ins):
        wk, p = merge(ins[0], ins[2])
        return wk, np.concatenate((ins[1], ins[3]))[p]

    def host(self, obj, q, ins):
        return obj.with_host_data(ins[0], ins[2], ins[1], ins[3], q_exec=q)


class _Search:
    """n ushort haystack keys with many ties and about n / 4 ascending needles under NEEDLES_SORTED, the form whose
    tiles' ranges live in the object's workspace. -> (pos_out,)."""
    out_types = (np.uint32,)

    def new(self, clo, ctx):
        return clo.Search(ctx, "ushort")

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        return np.sort(rng.integers(0, 5000, n).astype(np.uint16)), np.sort(rng.integers(0, 5100, max(1, n // 4)).astype(np.uint16))

    def out_counts(self, ins):
        return (ins[1].size,)

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], ins[0].size, i[1], ins[1].size, o[0], needles_sorted=True)

    def want(self, ins):
        return (search(ins[0], ins[1], False),)

    def host(self, obj, q, ins):
        return (obj.with_host_data(ins[0], ins[1], needles_sorted=True, q_exec=q),)


class _SetOp(_Merge):
    """The symmetric difference of _Merge's inputs. -> (the k keys, their values, k); the outputs hold the capacity."""
    out_types = (np.uint16, np.uint32, np.uint64)

    def new(self, clo, ctx):
        return clo.SetOp("symmetric_difference", ctx, "ushort", 4)

    def out_counts(self, ins):
        return ins[0].size + ins[2].size, ins[0].size + ins[2].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], ins[0].size, i[2], i[3], ins[2].size, o[0], o[1], o[2])

    def want(self, ins):
        wk, p = setop("symmetric_difference", ins[0], ins[2])
        return wk, np.concatenate((ins[1], ins[3]))[p], np.array([p.size], np.uint64)

    def host(self, obj, q, ins):
        ko, vo = obj.with_host_data(ins[0], ins[2], ins[1], ins[3], q_exec=q)
        return ko, vo, np.array([ko.size], np.uint64)


class _Select:
    """The partition of n uint keys by "lt" a threshold that lies in a one-element device buffer, uint values carried
    along. -> (all n rows of keys and of values, the k kept ones first, and k)."""
    out_types = (np.uint32, np.uint32, np.uint64)

    def new(self, clo, ctx):
        return clo.Select("partition", "lt", ctx, "uint", 4)

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        return (rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
                rng.integers(1 << 30, 3 << 30, 1, dtype=np.uint64).astype(np.uint32))

    def out_counts(self, ins):
        return ins[0].size, ins[0].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], i[2], o[0], o[1], o[2], ins[0].size)

    def want(self, ins):
        p, k = select("partition", "lt", ins[0], ins[2][0])
        return ins[0][p], ins[1][p], np.array([k], np.uint64)

    def host(self, obj, q, ins):
        ko, vo, k = obj.with_host_data(ins[0], ins[2][0], ins[1], q_exec=q)
        return ko, vo, np.array([k], np.uint64)


class _TopK:
    """The n // 3 + 1 largest of n uint keys with many ties (3000 values: the cut falls inside a tie run), in input
    order, uint values carried along. A call makes 2 * 4 + 3 dependent launches that talk through the object's
    workspace: the digit tables (cleared by a fill on the queue), the states and the tiles' counts.
    -> (keys_out, values_out, kth_out)."""
    out_types = (np.uint32, np.uint32, np.uint32)
    which, order = "largest", "input"

    def new(self, clo, ctx):
        return clo.TopK(self.which, self.order, ctx, "uint", 4)

    def k(self, n):
        return n // 3 + 1

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed)
        return rng.integers(0, 3000, n).astype(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def out_counts(self, ins):
        m = min(self.k(ins[0].size), ins[0].size)
        return m, m, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], i[1], o[0], o[1], o[2], ins[0].size, self.k(ins[0].size))

    def want(self, ins):
        p, kth = topk(self.which, self.order, ins[0], self.k(ins[0].size))
        return ins[0][p], ins[1][p], kth

    def host(self, obj, q, ins):
        ko, vo, kth = obj.with_host_data(ins[0], self.k(ins[0].size), ins[1], q_exec=q)
        return ko, vo, np.array([kth], np.uint32)


class _TopKSortedArg(_TopK):
    """The 1000 smallest of the same keys (below the cap of the sorted order) in the order of the sort, as indices with
    keys_out, kth_out not asked for: the sort kernel behind the apply sweep. -> (keys_out, the indices)."""
    out_types = (np.uint32, np.uint32)
    which, order = "smallest", "sorted"

    def k(self, n):
        return 1000

    def inputs(self, n, seed):
        return _TopK.inputs(self, n, seed)[:1]

    def out_counts(self, ins):
        return _TopK.out_counts(self, ins)[:2]

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], None, o[0], o[1], None, ins[0].size, self.k(ins[0].size))

    def want(self, ins):
        p, _ = topk(self.which, self.order, ins[0], self.k(ins[0].size))
        return ins[0][p], p

    def host(self, obj, q, ins):
        ko, vo, _ = obj.with_host_data(ins[0], self.k(ins[0].size), kth=False, q_exec=q)
        return ko, vo


def _segment_counts(n, seed):
    """uint counts whose sum is n: lengths geometric with mean 16, a tenth of the segments empty and, where n allows it,
    one segment of a fifth of the rows: at 2^22 rows it crosses hundreds of tiles of all three operations."""
    rng = np.random.default_rng(seed)
    c = rng.geometric(1 / 16, n // 12 + 8)
    while int(c.sum()) < 2 * n:
        c = np.concatenate((c, rng.geometric(1 / 16, n // 12 + 8)))
    c[rng.random(c.size) < 0.1] = 0
    if n > 100:
        c[c.size // 7] = n // 5
    c = c[:int(np.searchsorted(np.cumsum(c), n, "left")) + 1].copy()
    c[-1] -= int(c.sum()) - n
    assert int(c.sum()) == n and (c >= 0).all()
    return c.astype(np.uint32)


class _Expand:
    """n rows from uint counts: the segments' uint values, the segment ids and the ranks. -> (values_out, seg_out,
    rank_out, the total)."""
    out_types = (np.uint32, np.uint32, np.uint32, np.uint64)

    def new(self, clo, ctx):
        return clo.Expand("counts", ctx, "uint", "uint")

    def inputs(self, n, seed):
        counts = _segment_counts(n, seed)
        return counts, np.random.default_rng(seed + 1).integers(0, 1 << 32, counts.size, dtype=np.uint64).astype(np.uint32)

    def rows(self, ins):
        return int(ins[0].sum(dtype=np.uint64))

    def out_counts(self, ins):
        return self.rows(ins), self.rows(ins), self.rows(ins), 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], None, i[1], o[0], o[1], o[2], o[3], ins[0].size, self.rows(ins))

    def want(self, ins):
        seg, rank, total = expand("counts", ins[0], self.rows(ins))
        return ins[1][seg], seg, rank, np.array([total], np.uint64)

    def host(self, obj, q, ins):
        vo, so, ro, total = obj.with_host_data(ins[0], self.rows(ins), ins[1], seg=True, rank=True, q_exec=q)
        return vo, so, ro, np.array([total], np.uint64)


class _SegReduce(_Expand):
    """The same counts over n uint values summed in ulong: the ends' scan, the tiles' states, the carry scan and the
    fix-up talk through the object's workspace. -> (aggr_out, the total)."""
    out_types = (np.uint64, np.uint64)

    def new(self, clo, ctx):
        return clo.SegReduce("sum", "counts", ctx, "uint", "ulong", "uint")

    def inputs(self, n, seed):
        return _segment_counts(n, seed), np.random.default_rng(seed + 1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def out_counts(self, ins):
        return ins[0].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], None, i[1], o[0], o[1], ins[0].size, ins[1].size)

    def want(self, ins):
        aggr, total = segreduce("sum", "counts", ins[0], ins[1], "ulong")
        return aggr, np.array([total], np.uint64)

    def host(self, obj, q, ins):
        aggr, total = obj.with_host_data(ins[0], ins[1], q_exec=q)
        return aggr, np.array([total], np.uint64)


class _SegSort(_Expand):
    """The same counts over n uint keys with many ties (5000 values), uint values carried along: the rows ping-pong
    between the outputs and the copy in the object's workspace, up to eleven merge passes at 2^22 rows.
    -> (keys_out, values_out, the total)."""
    out_types = (np.uint32, np.uint32, np.uint64)

    def new(self, clo, ctx):
        return clo.SegSort("counts", ctx, "uint", 4, "uint")

    def inputs(self, n, seed):
        rng = np.random.default_rng(seed + 1)
        return _segment_counts(n, seed), rng.integers(0, 5000, n).astype(np.uint32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def out_counts(self, ins):
        return ins[1].size, ins[1].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], None, i[1], i[2], o[0], o[1], o[2], ins[0].size, ins[1].size)

    def want(self, ins):
        p, total = segsort("counts", ins[0], ins[1])
        return ins[1][p], ins[2][p], np.array([total], np.uint64)

    def host(self, obj, q, ins):
        ko, vo, total = obj.with_host_data(ins[0], ins[1], ins[2], q_exec=q)
        return ko, vo, np.array([total], np.uint64)


class _SegScan(_Expand):
    """The same counts over n uint values, the inclusive running sum in ulong: the ends' scan, the split, the tiles'
    states and the carry scan talk through the object's workspace. -> (data_out, the total)."""
    out_types = (np.uint64, np.uint64)

    def new(self, clo, ctx):
        return clo.SegScan("sum", "counts", ctx, "uint", "ulong", "uint", inclusive=True)

    def inputs(self, n, seed):
        return _segment_counts(n, seed), np.random.default_rng(seed + 1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)

    def out_counts(self, ins):
        return ins[1].size, 1

    def call(self, obj, q, i, o, ins):
        return obj.with_device_data(q, i[0], None, i[1], o[0], o[1], ins[0].size, ins[1].size)

    def want(self, ins):
        data, total = segscan("sum", "counts", ins[0], ins[1], "ulong", True)
        return data, np.array([total], np.uint64)

    def host(self, obj, q, ins):
        data, total = obj.with_host_data(ins[0], ins[1], q_exec=q)
        return data, np.array([total], np.uint64)


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype.itemsize == w.dtype.itemsize and np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), \
            "%s: output %d differs from the model" % (what, k)


@pytest.mark.parametrize("kind", [_SortByKey, _ReduceByKey, _ScanByKey, _Histogram, _Merge, _Search, _SetOp, _Select, _TopK, _TopKSortedArg, _Expand, _SegReduce,
                                  _SegSort, _SegScan], ids=lambda k: k.__name__.strip("_"))
def test_object_moves_between_queues(gpu, kind):
    import cl_ops_amd as clo
    ctx, _ = gpu
    k = kind()
    q1, q2 = clo.Queue(ctx), clo.Queue(ctx)               # no profiling: the queues production uses
    obj = k.new(clo, ctx)
    calls = []
    for c, n in enumerate(SIZES):                          # fresh inputs and outputs for every call, all there before the first
        ins = k.inputs(n, 100 + c)
        dev_in = [clo.Buffer(ctx, max(a.nbytes, 16)) for a in ins]
        for b, a in zip(dev_in, ins):
            b.write(q1, a)
        dev_out = [clo.Buffer(ctx, max(cnt * np.dtype(t).itemsize, 16)) for cnt, t in zip(k.out_counts(ins), k.out_types)]
        calls.append((ins, dev_in, dev_out))
    q1.finish()
    for c, (ins, dev_in, dev_out) in enumerate(calls):     # six calls back to back, the queues in turn
        assert k.call(obj, (q1, q2)[c % 2], dev_in, dev_out, ins)
    q1.finish()
    q2.finish()
    for c, (ins, dev_in, dev_out) in enumerate(calls):
        want = k.want(ins)
        got = [b.read(q1, t, w.size) for b, t, w in zip(dev_out, k.out_types, want)]
        _same(got, want, "call %d of %d elements on queue %d" % (c, SIZES[c], 1 + c % 2))
        same_in = [b.read(q1, a.dtype, a.size) for b, a in zip(dev_in, ins)]
        _same(same_in, ins, "call %d: the inputs" % c)
        for b in dev_in + dev_out:
            b.close()
    q2.close()                                             # the object's last call ran on q2: it remembers a queue that is gone
    q3 = clo.Queue(ctx)
    ins = k.inputs(BIG, 200)
    _same(k.host(obj, q3, ins), k.want(ins), "host data on a third queue")
    ins = k.inputs(70001, 201)
    dev_in = [clo.Buffer(ctx, a.nbytes) for a in ins]
    for b, a in zip(dev_in, ins):
        b.write(q3, a)
    want = k.want(ins)
    dev_out = [clo.Buffer(ctx, max(cnt * np.dtype(t).itemsize, 16)) for cnt, t in zip(k.out_counts(ins), k.out_types)]
    assert k.call(obj, q3, dev_in, dev_out, ins)
    q3.finish()
    _same([b.read(q3, t, w.size) for b, t, w in zip(dev_out, k.out_types, want)], want, "device data on a third queue")
    for x in dev_in + dev_out + [obj, q1, q3]:
        x.close()


N_PIPE, DISTINCT = (1 << 20) + 3, 700


def _pipeline_inputs(seed):
    """N_PIPE uint keys from DISTINCT values, every one of them present (so that the number of rows of the reduce by
    key is known to the host without a look at the device), and uint values."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(1 << 16, DISTINCT, replace=False)).astype(np.uint32)
    keys = pool[rng.integers(0, DISTINCT, N_PIPE)]
    keys[rng.permutation(N_PIPE)[:DISTINCT]] = pool
    return keys, rng.integers(0, 1 << 32, N_PIPE, dtype=np.uint32)


def _pipeline_model(keys, values):
    order = np.argsort(keys, kind="stable")
    sk, sv = keys[order], values[order]
    running = sbk(sk, sv, "sum", np.uint32, True)
    rk, ra, m = rbk(sk, sv, "sum", np.uint32)
    assert m == DISTINCT
    return [sk, sv, running, rk, ra, np.array([m], np.uint64), histogram(rk, None, np.uint32, 0, 8, 256)]


def _run_pipeline(clo, ctx, q, inputs):
    """Both inputs through sort by key -> scan by key -> reduce by key -> histogram, then the merge of the two reduced
    tables; nothing waits for the device before the last call is enqueued. Returns every intermediate array."""
    n = N_PIPE
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    s, sc = clo.Sorter("satradix", ctx, "uint"), clo.ScanByKey(ctx, "uint", "uint", "uint", inclusive=True)
    r, h, mg = clo.ReduceByKey(ctx, "uint", "uint", "uint"), clo.Histogram(ctx, "uint", None, "uint"), clo.Merge(ctx, "uint", 4)
    sides, bufs = [], []
    for keys, values in inputs:
        d = dict(kin=B(4 * n), vin=B(4 * n), sk=B(4 * n), sv=B(4 * n), run=B(4 * n), rk=B(4 * n), ra=B(4 * n), cnt=B(8), hist=B(4 * 256))
        d["kin"].write(q, keys)
        d["vin"].write(q, values)
        sides.append(d)
        bufs += list(d.values())
    mk, mv = B(4 * 2 * DISTINCT), B(4 * 2 * DISTINCT)
    q.finish()
    for d in sides:
        assert s.by_key_with_device_data(q, d["kin"], d["vin"], d["sk"], d["sv"], n)
        assert sc.with_device_data(q, d["sk"], d["sv"], d["run"], n)
        assert r.with_device_data(q, d["sk"], d["sv"], d["rk"], d["ra"], d["cnt"], n)
        assert h.with_device_data(q, d["rk"], None, d["hist"], DISTINCT, lower=0, shift=8, num_bins=256)
    a, b = sides
    assert mg.with_device_data(q, a["rk"], a["ra"], DISTINCT, b["rk"], b["ra"], DISTINCT, mk, mv)
    q.finish()
    got = []
    for d in sides:
        got.append([d["sk"].read(q, np.uint32, n), d["sv"].read(q, np.uint32, n), d["run"].read(q, np.uint32, n), d["rk"].read(q, np.uint32, DISTINCT),
                    d["ra"].read(q, np.uint32, DISTINCT), d["cnt"].read(q, np.uint64, 1), d["hist"].read(q, np.uint32, 256)])
    got.append([mk.read(q, np.uint32, 2 * DISTINCT), mv.read(q, np.uint32, 2 * DISTINCT)])
    for x in bufs + [mk, mv, s, sc, r, h, mg]:
        x.close()
    return got


def test_group_by_pipeline_on_a_non_profiling_queue(gpu):
    import cl_ops_amd as clo
    ctx, q_prof = gpu
    inputs = [_pipeline_inputs(31), _pipeline_inputs(32)]
    want = [_pipeline_model(*i) for i in inputs]
    wk, p = merge(want[0][3], want[1][3])
    want.append([wk, np.concatenate((want[0][4], want[1][4]))[p]])
    q = clo.Queue(ctx)
    plain = _run_pipeline(clo, ctx, q, inputs)
    q.close()
    prof = _run_pipeline(clo, ctx, q_prof, inputs)
    names = ["sorted keys", "sorted values", "running sums", "reduced keys", "sums per key", "run count", "histogram of the reduced keys"]
    for side, (g1, g2, w) in enumerate(zip(plain, prof, want)):
        for k, (x1, x2, y) in enumerate(zip(g1, g2, w)):
            what = "merge output %d" % k if side == 2 else "input %d, %s" % (side, names[k])
            assert x1.dtype == y.dtype and np.array_equal(x1, y), what + ": the non-profiling queue differs from numpy"
            assert np.array_equal(x1, x2), what + ": the two queues differ"
