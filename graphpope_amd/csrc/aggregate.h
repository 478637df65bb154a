// SAGEConv(aggr='add' | 'max'): what aggregate.hip (the two kernels and their launches) and sage.hip (the layer around them) share.
// include/graphpope_hip.h, "Sum and max aggregation", is the contract.
#pragma once

#include "common.h"

namespace pope {

inline bool aggr_known(int aggr) { return aggr == POPE_AGGR_MEAN || aggr == POPE_AGGR_ADD || aggr == POPE_AGGR_MAX; }

// sage.hip: det_index.h's counting sort over a block -- for every source the destinations that list it (k_det_clear, k_det_index<false>,
// k_det_scan, k_det_index<true>; the last three only for a block with room for an edge).  start [n_src + 1], list [nnz].
void enqueue_det_block_index(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, int *start, int *list,
                             const int32_t *dims, hipStream_t stream);

// aggregate.hip: k_gather_reduce.  x [x_rows, c]: the block's sources, or (n_id) the feature matrix; `vec`: c % 4 == 0 and x, agg, arg and
// x_dst (those given) are 16-byte aligned.  aggr: POPE_AGGR_ADD or POPE_AGGR_MAX.
void enqueue_gather_reduce(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x,
                           int64_t x_rows, int32_t c, int aggr, float *agg, int32_t *arg, float *x_dst, bool vec, const int32_t *dims,
                           hipStream_t stream);

// aggregate.hip: k_scatter_ordered over the index enqueue_det_block_index built in start / list (sorted [nnz]: room for the long lists).
// `vec`: c % 4 == 0 and grad_agg, grad_x and arg (if given) are 16-byte aligned.
void enqueue_scatter_ordered(const int32_t *rowptr, int64_t n_src, int64_t n_dst, int64_t nnz, const int *start, const int *list, int *sorted,
                             const int32_t *arg, const float *grad_agg, int32_t c, int aggr, float *grad_x, bool vec, const int32_t *dims,
                             hipStream_t stream);

}  // namespace pope
