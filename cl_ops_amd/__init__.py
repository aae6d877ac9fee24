"""cl_ops_amd — MI355X-native sort/scan/reduce-by-key/scan-by-key/histogram/merge/search/set-operation/join/selection/top-k/expansion/segmented-reduction/segmented-sort/segmented-scan/bucket-partition/segmented-arg-min-max/segmented-top-k/segmented-float-sum primitives and device RNGs behind the cl_ops C API.

The product is cl_ops_amd/lib/libcl_ops_hip.so (C-ABI, see include/): host
drivers in C (cl_ops_amd/csrc) + hand-written HIP kernels for gfx950
(cl_ops_amd/csrc/hip). This package is only the ctypes view of that library
used by the tests and bench.py; importing it fails loudly when the library has
not been built — there is no CPU or PyTorch fallback path.
"""
from . import _hip  # noqa: F401  (raises ImportError if the .so is missing)
from .api import (CloError, Context, Queue, Buffer, Sorter, Scanner, Profiler, HipEventTimer,  # noqa: F401
                  ShardTransport, ShardSort, CLO_TYPES, clo_type, wait_for_events)
from .rng import Rng, rng_names  # noqa: F401
from .reduce import ReduceByKey, reduce_by_key_tile  # noqa: F401
from .scan_by_key import ScanByKey, scan_by_key_tile  # noqa: F401
from .histogram import Histogram, histogram_tile, histogram_lds_bins  # noqa: F401
from .merge import Merge, merge_tile  # noqa: F401
from .search import Search, search_tile, search_lds_keys, search_pivots  # noqa: F401
from .setop import SetOp, setop_tile  # noqa: F401
from .join import Join, join_tile, join_out_tile, JOIN_KINDS, JOIN_NONE  # noqa: F401
from .select import Select, select_tile  # noqa: F401
from .expand import Expand, expand_tile, expand_lds_segments, EXPAND_FORMS  # noqa: F401
from .segreduce import SegReduce, segreduce_tile, SEGREDUCE_OPS, SEGREDUCE_FORMS  # noqa: F401
from .segsort import SegSort, segsort_tile, SEGSORT_FORMS  # noqa: F401
from .segscan import SegScan, segscan_tile, SEGSCAN_OPS, SEGSCAN_FORMS  # noqa: F401
from .bucket import Bucket, bucket_tile, BUCKET_MAX_BINS, BUCKET_SCAN_GROUP, BUCKET_SCAN_TRIP  # noqa: F401
from .segarg import SegArg, segarg_tile, segarg_carry_tiles, SEGARG_OPS, SEGARG_TIES, SEGARG_NONE  # noqa: F401
from .segtopk import SegTopK, segtopk_tile, segtopk_k_max, SEGTOPK_WHICH  # noqa: F401
from .segfsum import SegFSum, segfsum_tile, SEGFSUM_PAIRS  # noqa: F401
from .topk import TopK, topk_tile, topk_sweep_groups, topk_sorted_max, TOPK_WHICH, TOPK_ORDERS  # noqa: F401

__all__ = ["CloError", "Context", "Queue", "Buffer", "Sorter", "Scanner", "Profiler", "HipEventTimer",
           "ShardTransport", "ShardSort", "Rng", "rng_names", "ReduceByKey", "reduce_by_key_tile",
           "ScanByKey", "scan_by_key_tile", "Histogram", "histogram_tile", "histogram_lds_bins",
           "Merge", "merge_tile", "Search", "search_tile", "search_lds_keys", "search_pivots",
           "SetOp", "setop_tile", "Join", "join_tile", "join_out_tile", "JOIN_KINDS", "JOIN_NONE", "Select", "select_tile",
           "TopK", "topk_tile", "topk_sweep_groups", "topk_sorted_max", "TOPK_WHICH", "TOPK_ORDERS",
           "Expand", "expand_tile", "expand_lds_segments", "EXPAND_FORMS",
           "SegReduce", "segreduce_tile", "SEGREDUCE_OPS", "SEGREDUCE_FORMS",
           "SegSort", "segsort_tile", "SEGSORT_FORMS",
           "SegScan", "segscan_tile", "SEGSCAN_OPS", "SEGSCAN_FORMS",
           "Bucket", "bucket_tile", "BUCKET_MAX_BINS", "BUCKET_SCAN_GROUP", "BUCKET_SCAN_TRIP",
           "SegArg", "segarg_tile", "segarg_carry_tiles", "SEGARG_OPS", "SEGARG_TIES", "SEGARG_NONE",
           "SegTopK", "segtopk_tile", "segtopk_k_max", "SEGTOPK_WHICH",
           "SegFSum", "segfsum_tile", "SEGFSUM_PAIRS",
           "CLO_TYPES", "clo_type", "wait_for_events"]
