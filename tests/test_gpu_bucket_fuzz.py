"""A seeded, stratified fuzz of CloBucket (include/clo_bucket.h) on the GPU: the strata of tests/bucket_strata.py, every
one against the numpy model of tests/bucket_model.py bit for bit, through the checked views of test_gpu_bucket.run_bucket
(guards, inputs unchanged). tests/test_bucket_cpu.py shows what the strata reach. A stratum may be skipped only where its
sizes are not built, and for key sizes 1, 2, 4 and 8 — all of which must be built — the share of skipped strata is
asserted to be 0."""
import numpy as np
import pytest

from bucket_strata import KEY_TYPES, NP, STRATA, VALUE_SIZE, strata
from test_gpu_bucket import run_bucket

pytestmark = pytest.mark.gpu

CHUNKS = 8


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def all_strata(dev):
    T = dev[0].bucket_tile(4, 0)
    assert T > 0
    return strata(T)


skipped = []


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_strata(dev, all_strata, chunk):
    clo = dev[0]
    for i in range(chunk, STRATA, CHUNKS):
        s = all_strata[i]
        ks = np.dtype(NP[s["key_type"]]).itemsize
        if clo.bucket_tile(ks, VALUE_SIZE[s["mode"]]) == 0:
            skipped.append(i)                                            # sizes that are not built
            continue
        run_bucket(dev, s["key_type"], s["keys"], s["mode"], s["num_bins"], s["lower"], s["shift"], s["count_type"],
                   "stratum %d (%s, %s)" % (i, s["dist"], s["size"]))


def test_nothing_was_skipped(dev, all_strata):
    """Key sizes 1, 2, 4 and 8 are all built: no stratum may have been skipped."""
    clo = dev[0]
    for kt in KEY_TYPES:
        for vs in (0, 4, 8):
            assert clo.bucket_tile(np.dtype(NP[kt]).itemsize, vs) > 0, (kt, vs)
    assert len(all_strata) == STRATA and not skipped, skipped
