/*
 * cl_ops.h — aggregate public header (reference: src/cl_ops/cl_ops.h:33-48),
 * with the three modules of upstream: sort, scan and rng.
 */
#ifndef CL_OPS_H
#define CL_OPS_H

#include "clo_common.h"
#include "clo_ccl.h"
#include "clo_scan.h"
#include "clo_sort.h"
#include "clo_rng.h"
#include "clo_reduce.h"
#include "clo_scan_by_key.h"
#include "clo_histogram.h"
#include "clo_merge.h"
#include "clo_search.h"
#include "clo_setop.h"
#include "clo_select.h"
#include "clo_topk.h"
#include "clo_expand.h"
#include "clo_segreduce.h"
#include "clo_segsort.h"
#include "clo_segscan.h"
#include "clo_bucket.h"
#include "clo_segarg.h"
#include "clo_join.h"
#include "clo_segtopk.h"
#include "clo_segfsum.h"
#include "clo_hip.h"
#include "clo_shard.h"

#endif
