/*
 * graphpope_hip.h -- C ABI of libgraphpope_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for GraphPOPE's one hot path: what a binding of the
 * reference (/root/reference, 100 % Python) would load with ctypes.  INTEGRATION.md shows that stub.
 * Plain pointers and sizes only; every buffer is allocated by the caller.  Unless a parameter name ends in
 * `_host`, pointers are DEVICE pointers valid on the device that is current on the calling thread
 * (hipSetDevice / torch.cuda.set_device), and work is enqueued on `stream` (a hipStream_t passed as
 * void*, NULL = the default stream).  The library owns no device memory.  What it keeps between calls, all of it
 * host-side: the per-thread error string; per device, a mutex-guarded ring of small pinned host slots (a call's
 * anchor ids and its BFS verdict travel through a slot of its own, reused only after the event behind its last
 * device-side user has completed -- calls from several host threads or on several streams do not share staging);
 * and two process-global diagnostic facilities that are off by default and NOT thread-safe: the level-timing hook
 * (pope_profile_levels) and the A/B knobs (pope_debug_set).
 *
 * Every function returns 0 on success or a negative POPE_ERR_* code; pope_last_error() then holds
 * a message for the calling thread.
 *
 * Alignment.  A float32 data operand -- features, aggregates, weights, biases, gradients, optimiser state, embedding tables, the
 * output matrix -- needs the alignment of its element type only: 4 bytes.  A base that is also 16-byte aligned (with row lengths that
 * are multiples of 4 floats) selects the kernels that move 16 bytes per access, LDS-DMA loaders among them; any other base gets the
 * scalar form of the same kernel, template instance or plan, with the same results (bit for bit wherever the call documents exact
 * results).  Every call tests the pointers it was given; the *_kernel_name_at queries below print what a given set of misaligned
 * operands selects.  Integer operands need the alignment of their type; the CSR builds take edges in pairs when src and dst are
 * 16-byte aligned and E is even, one at a time otherwise.  Scratch buffers are not data operands: the requirement stated with a call
 * (4 or 8 bytes) holds, and a scratch buffer whose call states none (the SAGE layer and the pairwise calls) must be 16-byte aligned.
 *
 * Which reference interface each entry point replaces (file:line into /root/reference):
 *
 *   pope_csr_build           utils.py:121        G = to_networkx(data)           (graph build from edge_index)
 *   pope_geodesic_bfs        utils.py:64-81,     the per-(node, anchor) nx.shortest_path loop and its
 *                            utils.py:92-114     multiprocessing fan-out, as one batched multi-source BFS
 *   pope_geodesic_finalize   utils.py:73,125,    1/len(path), tensor conversion and torch.cat((x, emb), 1)
 *                            utils.py:129-135
 *   pope_geodesic_run        utils.py:144-145    get_geodesic_distance_vector + concat_into_features in one call
 *   pope_geodesic_column_stats  utils.py:50-54   the BFS sums behind nx.closeness_centrality (biased anchor selection)
 *   pope_pagerank_weights /  utils.py:26-30      nx.pagerank_scipy power iteration as SpMV over the device CSR
 *   pope_pagerank_step                           (biased anchor selection, README's best row)
 *   pope_clustering_counts   utils.py:56-60      nx.clustering(to_networkx(data)): the exact integers (M^3)_ii, total and
 *                                                reciprocal degree behind every coefficient (biased anchor selection)
 *   pope_betweenness_batch   utils.py:32-36      nx.betweenness_centrality(to_networkx(data)): Brandes' two passes per source with
 *                                                every float64 addition in NetworkX's order (biased anchor selection)
 *   pope_eigenvector_iterate utils.py:44-48      nx.eigenvector_centrality_numpy(to_networkx(data)): the dominant eigenvector of M^T by a
 *                                                shifted float64 power iteration, loop resident on the device (biased anchor selection)
 *   pope_degree_counts /     utils.py:38-42      nx.degree_centrality(to_networkx(data)), the ascending stable sort and the last-K slice: exact
 *   pope_topk_u64                                integer degrees, keys (degree << 32 | node) and a radix select of the K largest (biased
 *                                                anchor selection, the command line's default sampling_method)
 *   pope_topk_f64            utils.py:29-30      the ascending stable sort of a method's float64 scores and the last-K slice (and the
 *                                                same lines of the other four score methods): a radix select over (score, node)
 *   pope_geodesic_hops       (no counterpart)    the integer hop matrix the floats are made of; parity tests
 *   pope_kmeans_plusplus /   utils.py:168-170    KMeans(n_clusters=K).fit(X).cluster_centers_ (k-means++ seeding, Lloyd
 *   pope_kmeans_lloyd_step                       iterations with the MFMA tile as the assignment step)
 *   pope_pairwise_minmax     utils.py:158-176    sklearn cosine/euclidean pairwise + MinMaxScaler
 *   pope_pairwise_features   utils.py:158-177    the same + concat_into_features inside the tile kernel
 *   pope_concat              utils.py:129-135    torch.cat for the node2vec branch (device-resident callers)
 *   pope_host_copy_2d        utils.py:129-135    torch.cat's feature half on the host cores (host -> host callers)
 *   sage_conv_forward /      main.py:206 and     PyG SAGEConv((x_src, x_dst), adj_t): mean aggregation over the
 *   sage_conv_backward       PyG SAGEConv [3p]   sampled CSR + lin_l + lin_r, and its gradients
 *   sage_full_layer_forward  main.py:204-211     one pass of the layer loop over the whole graph, every neighbour taken (inference)
 *   pope_gcn_conv_forward    (PyG GCNConv)       out = D^-1/2 (A + f I) D^-1/2 (x W) + b over the whole graph; _backward: its gradients
 *   pope_gat_conv_forward    (PyG GATConv)       out = softmax-weighted sums of (x W^T) per head over the whole graph; _backward: its gradients
 *   pope_gatv2_conv_forward  (PyG GATv2Conv)     the same with the score att . leaky(W_l x_j + W_r x_i) of every edge; _backward: its gradients
 *   sage_bn_relu_dropout_forward / _backward   main.py:207-209
 *                                BatchNorm1d + relu_ + F.dropout of the hidden layers, forward and backward
 *   sage_l2_normalize_forward / _backward   PyG SAGEConv(normalize=True) [3p]
 *                                F.normalize(out, p=2., dim=-1) behind SAGEConv.forward and its gradient, one launch each
 *   sage_aggregate_* / sage_conv_*_aggr   PyG SAGEConv(aggr='add' | 'max') [3p]
 *                                matmul(adj_t, x, reduce='add' | 'max') in the mean's place, forward and backward
 *   sage_cross_entropy_*     main.py:216         F.cross_entropy(y_hat, y): loss and gradient in two launches
 *   sage_eval_metrics        main.py:216-217,    F.cross_entropy + Accuracy() of a training / validation / test step, summed over a
 *                            227-228, 238        pass in three device words: loss sum, correct count, row count (one launch per batch)
 *   sage_adam_step           main.py:244         torch.optim.Adam step, all parameter tensors in one launch
 *   sage_grad_sqnorm /       main.py:285-290     Trainer(gradient_clip_val=0.5) = clip_grad_norm_(parameters, 0.5): the squared
 *   sage_adam_step_clip                          norm of all gradients in one launch, the coefficient applied inside the Adam launch
 *   sage_grad_bucket_pack    main.py:285-290     Trainer(gpus=n, accelerator='ddp'): the gradients of a step, pre-scaled, in one flat buffer
 *   sage_sample_hop          main.py:100-116     NeighborSampler -> torch_sparse.sample_adj (one hop), relabelled block
 *   pope_n2v_walks /         generate_node2vec_embedding.py:23-25   PyG Node2Vec(p = 1, q = 1, sparse = True): pos_sample / neg_sample
 *   pope_n2v_windows /                           (torch_cluster.random_walk, torch.randint), the window matrices, Node2Vec.loss with its
 *   pope_n2v_loss_grad /                         gradient, and torch.optim.SparseAdam -- the generator of the table attach_node2vec
 *   pope_n2v_sparse_adam                         loads (utils.py:155); the reference's script itself saves the untrained table
 *   pope_n2v_walks_biased    (the p, q of the same constructor)   torch_cluster.random_walk with p != 1 or q != 1: second-order walks
 *   pope_logreg_loss_grad /  generate_node2vec_embedding.py:23-25   PyG Node2Vec.test of the model constructed there: the objective of
 *   pope_logreg_predict                          LogisticRegression(solver='lbfgs').fit(train_z, train_y) and the predictions behind
 *                                                .score(test_z, test_y) [3p: torch_geometric.nn.Node2Vec.test, scikit-learn]
 */
#ifndef GRAPHPOPE_HIP_H
#define GRAPHPOPE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POPE_OK                 0
#define POPE_ERR_INVALID       -1   /* bad argument (null pointer, negative size, K <= 0, ...)            */
#define POPE_ERR_HIP           -2   /* a HIP runtime call failed; message has hipGetErrorString           */
#define POPE_ERR_INDEX         -3   /* edge_index or anchor id outside [0, N)                             */
#define POPE_ERR_HOP_OVERFLOW  -4   /* a hop count does not fit the plane capacity / hop dtype given      */
#define POPE_ERR_WORKSPACE     -5   /* caller workspace too small                                         */
#define POPE_ERR_NO_DEVICE     -6   /* no gfx950 device visible                                           */
#define POPE_ERR_UNSORTED      -7   /* CSR was built with defer_check and edge_index is not sorted by source */

/* Message for the last error on the calling thread ("" if none).  Never NULL; valid until the next call. */
const char *pope_last_error(void);

/* Library / build identification, e.g. "graphpope_hip 0.2 gfx950". */
const char *pope_version(void);

/*
 * POPE_OK if a gfx950 device is visible to the calling process (and, if cu_count is not NULL, its number of compute
 * units); POPE_ERR_NO_DEVICE otherwise -- the product path has no CPU fallback (utils.Graphpope raises).
 */
int pope_require_device(int32_t *cu_count_host);

/*
 * Diagnostic knobs for A/B runs (tools/ab_*.py and the kernel-variant tests): process-global, not thread-safe, never
 * needed by a caller.  value < 0 restores the automatic choice where one exists.
 */
#define POPE_KNOB_LIVE_MODE         0   /* level kernel: -1 auto (by graph size), 1 live-bit table staged in LDS, 2 table read from global memory, 3 global table behind a summary in LDS */
#define POPE_KNOB_FINALIZE_VARIANT  1   /* 1 (default) the pipelined finalise kernels (every load of a row in flight, next row requested before this one is stored, rows dealt round-robin; wide rows through LDS tables); 7 the round 1-3 kernel (serial loops); 0 the generic kernel -- kept so that tests can compare their bits; 8 / 9 / 10: as 1, with wide rows on the table kernel k_finalize_lut only without features (8, the default), always (9: features by the copy kernel in front of it) or never (10: the shuffle kernel k_finalize_wide); 11 / 12: k_finalize_lut over several short-rowed shards takes a batch per (shard, block of rows) (11, the default) or the flat (row, half-word) order (12) */
#define POPE_KNOB_FINALIZE_BLOCKS   2   /* grid of the finalise kernel (default: one work item per wave for the pipelined kernels, 2048 blocks for the round 1-3 one) */
#define POPE_KNOB_PAIRWISE_KERNEL   4   /* node2vec embedding: 0 auto (anchor-resident persistent kernel for depths <= 128), 1 one tile per block, 2 / 3 persistent kernel with one / two consumer sets */
#define POPE_KNOB_COPY_BATCHES      5   /* node2vec embedding: 16-piece batches per wave of the feature-copy kernel beside the tile kernel (default 1) */
#define POPE_KNOB_FAIL_HOST_REGISTER 7  /* host -> host boundary, tests of the fallbacks, bit mask: 1 = every hipHostRegister is refused (edge_index then goes up through pinned staging), 2 = behave as if the pinned ring's hipHostMalloc had been refused (float columns through the bounce buffer), 4 = behave as if the 4 MB bounce buffer had been refused too (blocking copies by the runtime) */
#define POPE_KNOB_SAGE_FORWARD_OVERLAP 14 /* sage_conv_forward(_indexed): 1 (default) the gather runs beside the x_dst half of the projection in one launch, the agg half follows; 0 gather, then the whole projection */
#define POPE_KNOB_GEMM_TILE16_BUFFERS 18 /* whole-tile forward GEMM: 4 (default) or 3 LDS stage buffers (two or one stage times to hide a request; same bits) */
#define POPE_KNOB_PREPARE_MERGE     19  /* pope_geodesic_run: 1 (default) = the clear + seed of the BFS state and the speculative CSR build as two roles of ONE launch (k_prepare; at most 256 anchors per call); 0 = two launches */
#define POPE_KNOB_STREAMK_XCD       20  /* SAGE weight-gradient GEMM (stream-K): 0 units dealt to the blocks in block order; 1 (default) = XCD-aware: the blocks that work on the same depth range of the tiles sharing their B rows are neighbours in one XCD (csrc/gemm_streamk_tn.h) -- the partial sums of a tile are cut at other depths, so the last bits may differ; deterministic either way */
#define POPE_KNOB_FORWARD_WHOLE_TILES 21 /* sage_conv_forward(_indexed): 1 (default) the projection takes the whole tiles fitted to the chip (csrc/gemm_tile16.h, and the overlapped forward built on them) where they qualify; 0 = never: stream-K or the plain tile kernel, the references of the tests.  Nothing else changes (not the plain kernel's tile, not the backward pass) */
#define POPE_KNOB_LEVEL1_APPLY      22  /* pope_geodesic_run behind k_prepare (POPE_KNOB_PREPARE_MERGE on, at most 256 anchors) on graphs of up to 262 144 nodes: 1 (default) = the CSR role records the edges into anchors and a small launch (k_bfs_level1_apply) applies them as level 1; 0 = level 1 is a launch of the level kernel like every other level.  Same bits either way */
#define POPE_KNOB_LEVEL_COMPACT     23  /* level kernels with the live table in LDS and one tile per node (graphs of up to 262 144 nodes, at most 256 anchors): a 256-slot chunk with at most this many live slots (default 16, measured; at most 64, one per lane: larger values mean 64) compacts them across the wave and loads their rows in one round trip, in every launch but that of level 1; 0 = every chunk takes the general path.  A kernel argument.  Same bits either way */
/* (Knob numbers 6, 8-13, 16 and 17 belonged to experiments that were measured slower and removed in round 5 -- a copy role and block caps
 * in the level launches, the last levels inside the finalise launch, side streams in the SAGE backward pass, split-bf16 products, the
 * one-launch SAGE layer, the registered result mode; 3 and 15 forced tile shapes and stream-K variants of the SAGE GEMMs that were
 * measured and not kept: DESIGN.md keeps their figures.  pope_debug_set returns POPE_ERR_INVALID for a retired number.) */
int pope_debug_set(int32_t knob, int32_t value);

/* ------------------------------------------------------------------------------------------------
 * Graph: forward CSR (row = source node, columns = targets) in int32, built on the device into
 * caller-allocated arrays.  Distance is measured node -> anchor along edge direction (utils.py:73
 * nx.shortest_path(G, source=node, target=anchor) on a DiGraph), so the bottom-up BFS pulls over a
 * node's OUT-edges: this is the only adjacency the path needs.
 * ------------------------------------------------------------------------------------------------ */
size_t pope_csr_scratch_bytes(int64_t N, int64_t E);
size_t pope_csr_aux_elems(int64_t E);          /* int32 elements of `aux` below */

/*
 * edge_index: int64 [2, E] row-major on the device, PyG convention: edge e is
 * edge_index[e] -> edge_index[E + e].  Self-loops and repeated edges are allowed and kept.
 * Written (all caller-allocated, int32):
 *   rowptr [N + 1], col [E rounded up to a multiple of 4, >= 4], erow [same]: CSR slot p holds the edge erow[p] -> col[p], slots sorted
 *       by erow (erow is the row id of every slot: the edge-parallel BFS kernel streams erow/col instead of
 *       chasing rowptr).  Column order inside a row: the edge list's own order if edge_index is already sorted by source
 *       (PyG's coalesced order: preserved, no atomics); otherwise ascending by target (a row-wise sort follows the
 *       counting scatter, so the CSR is a pure function of the edge set: repeated builds are identical).
 *   aux [pope_csr_aux_elems(E)]: header (counts, status flags) + the rows that span several 256-slot chunks.
 * defer_check = 0: synchronises `stream` once; returns POPE_ERR_INDEX for an id outside [0, N) and falls back
 *   to a counting sort when edge_index is not sorted by source.
 * defer_check = 1: fully asynchronous; only the sorted fast path is attempted and its verdict stays in aux:
 *   pope_geodesic_bfs then returns POPE_ERR_INDEX / POPE_ERR_UNSORTED (rebuild with defer_check = 0).
 * Requires 0 <= N < 2^31 and 0 <= E < 2^31.
 */
int pope_csr_build(const int64_t *edge_index, int64_t E, int64_t N, int32_t *rowptr, int32_t *col, int32_t *erow,
                   int32_t *aux, void *scratch, size_t scratch_bytes, int32_t defer_check, void *stream);

/*
 * The same CSR in canonical form whatever the order of edge_index: rows by source, every row's targets ascending
 * (repeated edges adjacent).  Synchronises `stream` once (index check).  Used by the rankings below.
 */
int pope_csr_build_canonical(const int64_t *edge_index, int64_t E, int64_t N, int32_t *rowptr, int32_t *col, int32_t *erow,
                             int32_t *aux, void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Biased anchor selection: PageRank scores (utils.py:26-30 nx.pagerank_scipy(to_networkx(data)); NetworkX 3: nx.pagerank),
 * float64, reproduced bit for bit so that the ascending stable sort picks the reference's anchors.
 *   pope_pagerank_weights  w[j] = 1 / (distinct targets of j), 0 for dangling nodes, from the canonical CSR by source.
 *   pope_pagerank_step     x_out[i] = alpha * (sum over the in-neighbours j of i, ascending, of w[j] * x[j]
 *                                               + dangling_sum / N) + (1 - alpha) / N
 *                          over the canonical CSR of the REVERSED edge list (rows = targets, entries = sources).  One
 *                          power iteration; the host binding owns the loop (dangling_sum = sum of x over the dangling
 *                          nodes in index order, convergence on sum |x - xlast| < N * tol, as SciPy / NumPy evaluate them).
 * Asynchronous on `stream`.
 * ------------------------------------------------------------------------------------------------ */
int pope_pagerank_weights(const int32_t *rowptr, const int32_t *col, int64_t N, double *w, void *stream);
int pope_pagerank_step(const int32_t *rowptr_by_target, const int32_t *sources, int64_t N, const double *x, const double *w,
                       double dangling_sum, double alpha, double *x_out, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Biased anchor selection: clustering coefficients (utils.py:56-60 nx.clustering(to_networkx(data)), NetworkX 3.4.2's
 * directed, unweighted form).  With A the adjacency of the DiGraph without self-loops and M = A + A^T (entries 0, 1, 2):
 *   T[i]  = (M^3)_ii          (the directed triangles NetworkX counts at i)
 *   dt[i] = sum_k M_ik        (total degree)
 *   db[i] = #{k : M_ik = 2}   (reciprocal degree)
 * all int64 [N] on the device; the coefficient is 0 if T == 0 else T / ((dt (dt - 1) - 2 db) * 2), evaluated by the caller.
 * Inputs: the canonical CSR of edge_index (rowptr, col, erow: pope_csr_build_canonical) and the canonical CSR of the
 * flipped edge_index (rowptr_by_target, sources, erow_by_target); both hold the same E slots.  M has up to 2 E slots:
 * 2 E must fit int32 offsets (E <= 2^30 - 1), else POPE_ERR_INVALID.  Exact integer sums: the result does not depend on
 * the run order.  Asynchronous on `stream`.
 * scratch: pope_clustering_scratch_bytes(N, E): rocPRIM sizes its scan and sort temporaries for the current device, so the
 * answer is 0 when no device is visible, as for sizes pope_clustering_counts rejects (there: POPE_ERR_HIP / _INVALID).
 * ------------------------------------------------------------------------------------------------ */
size_t pope_clustering_scratch_bytes(int64_t N, int64_t E);                                   /* utils.py:56-60 */
int pope_clustering_counts(const int32_t *rowptr, const int32_t *col, const int32_t *erow, const int32_t *rowptr_by_target,
                           const int32_t *sources, const int32_t *erow_by_target, int64_t N, int64_t E, int64_t *T, int64_t *dt,
                           int64_t *db, void *scratch, size_t scratch_bytes, void *stream);  /* utils.py:56-60 nx.clustering */

/* ------------------------------------------------------------------------------------------------
 * Biased anchor selection: betweenness (utils.py:32-36 nx.betweenness_centrality(to_networkx(data)), NetworkX 3.4.2:
 * normalized, directed, every node a source, no endpoints), float64, reproduced bit for bit: every addition NetworkX
 * performs is performed in its order.  One call replays `num_sources` sources first_source .. first_source + num_sources - 1,
 * one wave64 each (FIFO BFS that accumulates sigma, then the dependencies delta from the end of the queue), and then adds
 * their dependencies to bc in ascending source order:  bc[w] = (...(bc[w] + delta_first[w]) + ...) + delta_last[w], the
 * source's own delta left out.  The caller zeroes bc, runs the batches in source order on one stream and applies NetworkX's
 * _rescale (one multiplication by 1 / ((N - 1)(N - 2)) if N > 2).
 * Inputs: the CSR by source in INSERTION order -- row v lists v's distinct successors in the order (v, w) first appears in
 * edge_index, one slot per distinct pair (E_by_source slots), the iteration order of the DiGraph's adjacency -- and a
 * de-duplicated CSR by target (row w lists w's distinct predecessors, any order, E_by_target slots).
 * Optional outputs (NULL = not wanted), row b = source first_source + b: sigma_out, delta_out float64 [num_sources, N],
 * dist_out int32 [num_sources, N] (-1 = not reached), queue_len_out int32 [num_sources] (the nodes the source reaches,
 * itself included).  Asynchronous on `stream`.
 * scratch: pope_betweenness_scratch_bytes(N, num_sources) = 36 bytes per (source, node) and change; answers without a GPU;
 * 0 for sizes pope_betweenness_batch rejects (N <= 0, N >= 2^31, batch <= 0, batch > N, more than 2^40 (source, node) pairs).
 * ------------------------------------------------------------------------------------------------ */
size_t pope_betweenness_scratch_bytes(int64_t N, int64_t batch);                              /* utils.py:32-36 */
int pope_betweenness_batch(const int32_t *rowptr, const int32_t *col, int64_t E_by_source, const int32_t *rowptr_by_target,
                           const int32_t *sources, int64_t E_by_target, int64_t N, int64_t first_source, int64_t num_sources,
                           double *bc, double *sigma_out, double *delta_out, int32_t *dist_out, int32_t *queue_len_out,
                           void *scratch, size_t scratch_bytes, void *stream);      /* utils.py:32-36 nx.betweenness_centrality */

/* ------------------------------------------------------------------------------------------------
 * Biased anchor selection: eigenvector centrality (utils.py:44-48 nx.eigenvector_centrality_numpy(to_networkx(data))), float64.
 * With M the adjacency of the DiGraph (one edge per distinct (u, v) pair, self-loops kept), the score vector is the eigenvector
 * of M^T for the eigenvalue of largest real part.  NetworkX asks ARPACK for it; here it is a shifted power iteration, so the
 * scores agree with NetworkX's to a measured tolerance, NOT bit for bit, and nodes with mathematically equal
 * scores are ordered deterministically where ARPACK's rounding noise orders them in NetworkX.  One iteration, in this order:
 *     ax = M^T x;  lambda = x . ax;  r = ||ax - lambda x||_2;  stop if r <= tol * lambda;  else x <- (ax + x) / ||ax + x||_2
 * pope_eigenvector_iterate enqueues `iterations` iterations (three launches each) on `stream` and returns at once.
 *   rowptr_by_target, sources: the canonical CSR of the flipped edge_index (pope_csr_build_canonical: rows = targets, sources
 *       ascending, repeated edges adjacent -- they count once).
 *   x [N]: in: the start vector, unit length (the caller's 1 / sqrt(N)); out: the iterate.
 *   control: 32 bytes {int64 iterations; double lambda; double r; int32 done; int32 pad}, zeroed by the caller before the first
 *       call.  Once the stop test passes `done` is set and every later kernel, of this call or the next, returns without
 *       writing: x is exactly the first vector that met the test however many iterations were queued behind it.  The caller
 *       copies the block back between calls and stops when `done` is set; the normalisation by sign(sum) * norm is the caller's.
 *   scratch: pope_eigenvector_scratch_bytes(N) (ax and the per-block partials of the three reductions); answers without a GPU,
 *       0 for an N the call rejects.  The same scratch must be passed to every call of one iteration sequence.
 * Deterministic: no floating-point atomics, every sum in a fixed order that depends on N alone.
 * POPE_ERR_INVALID for a null pointer, N <= 0, N >= 2^31 - 1, iterations <= 0 or tol <= 0 (or NaN); POPE_ERR_WORKSPACE for a
 * scratch that is too small; both before any HIP call.
 * ------------------------------------------------------------------------------------------------ */
size_t pope_eigenvector_scratch_bytes(int64_t N);                                              /* utils.py:44-48 */
int pope_eigenvector_iterate(const int32_t *rowptr_by_target, const int32_t *sources, int64_t N, double *x, void *scratch,
                             size_t scratch_bytes, int32_t iterations, double tol, void *control,
                             void *stream);                                /* utils.py:44-48 nx.eigenvector_centrality_numpy */

/* ------------------------------------------------------------------------------------------------
 * Biased anchor selection: degree centrality (utils.py:38-42 nx.degree_centrality(to_networkx(data)), ascending stable sort, the
 * last K kept), the default sampling_method.  Exact integers; the ranking is NetworkX's because its score deg * (1 / (n - 1)) is
 * strictly monotone in the integer degree.
 *   pope_degree_counts  degree[v] = in-degree + out-degree of v over the DISTINCT (u, v) pairs (a self-loop counts 2), int64 [N],
 *       from the canonical CSR by source (rowptr, col, erow: pope_csr_build_canonical).  The slots are [0, rowptr[N]), read on
 *       the device; col / erow may be padded beyond with anything.  An empty graph gives zeros.  If keys is not NULL,
 *       keys[v] = (uint64(degree[v]) << 32) | v: all distinct, and "the last K of the ascending stable sort by degree" is
 *       "the K largest keys, ascending", the node ids in the low words.  32-bit integer atomics (degree <= 2 N < 2^32): the
 *       result is exact and the same on every run.  Requires 0 < N < 2^31.  Asynchronous on `stream`.
 *   pope_topk_u64  out[0 .. K) = the K largest of keys[0 .. N) as a multiset, ascending; any keys, duplicates allowed, unsigned
 *       comparison (bit 63 is a value bit).  A radix select, eight digits from the most significant one, then a one-block sort
 *       of the K keys in LDS; the state lives in `scratch`, whose contents on entry do not matter, and never visits the host:
 *       asynchronous on `stream`.  Requires 0 < N < 2^31 and 1 <= K <= min(N, pope_topk_max_k()), else POPE_ERR_INVALID;
 *       POPE_ERR_WORKSPACE for a scratch below pope_topk_scratch_bytes(N, K); both before any HIP call.
 *   pope_topk_scratch_bytes  answers without a GPU; 0 for arguments pope_topk_u64 rejects.
 *   pope_topk_max_k  POPE_TOPK_MAX_K, what the one-block sort holds.
 *   pope_topk_f64  the select behind the other five biased methods (utils.py:26-30 pagerank, :32-36 betweenness, :44-48
 *       eigenvector, :50-54 closeness, :56-60 clustering: each sorts its float64 scores ascending and stably and keeps the last K,
 *       utils.py:29-30 and the same two lines of every method).  nodes_out[0 .. K) = the K largest of the N pairs (scores[v], v),
 *       ascending: element for element np.argsort(scores, kind="stable")[-K:].  Scores compare as NumPy sorts float64 (-0.0 ==
 *       +0.0; every NaN equal to every other NaN and above +inf), equal scores by node id.  scores_out, unless NULL, receives
 *       scores[nodes_out[i]] bit for bit.  The same radix select over a 96-bit key (the order-preserving 64-bit key of the score,
 *       then the node id: 12 digits, all keys distinct); the doubles are read in place, no array of N keys is written.  State in
 *       `scratch` (contents on entry do not matter), asynchronous on `stream`, nothing visits the host.  Requirements and error
 *       codes as pope_topk_u64, the scratch from pope_topk_f64_scratch_bytes(N, K) (answers without a GPU; 0 for refused sizes).
 *   pope_score_keys_host  keys[i] = that 64-bit key of scores[i], computed on the HOST by the function the kernels call: -0.0
 *       becomes +0.0, a NaN all ones, otherwise all bits flipped if the sign is set, else the sign bit set.  For tests.
 * ------------------------------------------------------------------------------------------------ */
#define POPE_TOPK_MAX_K 4096
int pope_degree_counts(const int32_t *rowptr, const int32_t *col, const int32_t *erow, int64_t N, int64_t *degree, uint64_t *keys,
                       void *stream);                                                          /* utils.py:38-42 */
size_t pope_topk_scratch_bytes(int64_t N, int64_t K);                                          /* utils.py:38-42 */
int pope_topk_u64(const uint64_t *keys, int64_t N, int64_t K, uint64_t *out, void *scratch, size_t scratch_bytes,
                  void *stream);                                                               /* utils.py:38-42 sorted(...)[-K:] */
int pope_topk_max_k(void);
size_t pope_topk_f64_scratch_bytes(int64_t N, int64_t K);                                      /* utils.py:29-30 */
int pope_topk_f64(const double *scores, int64_t N, int64_t K, int64_t *nodes_out, double *scores_out, void *scratch,
                  size_t scratch_bytes, void *stream);                                         /* utils.py:29-30 sorted(...)[-K:] */
int pope_score_keys_host(const double *scores, int64_t n, uint64_t *keys);

/* ------------------------------------------------------------------------------------------------
 * K-means anchors of the node2vec branch (utils.py:168-170  KMeans(n_clusters=K).fit(X).cluster_centers_, scikit-learn
 * defaults).  The host binding owns the control flow and the random numbers (the reference's KMeans draws from the global
 * NumPy stream: one choice() for the first seed, 2 + int(log K) uniforms per further seed); the device does the distances,
 * the reductions and the centre updates.  X is float32 [N, D], already centred by its column means (KMeans.fit does that).
 *   pope_column_moments     sum[c], sumsq[c] of every column in float64 (column means; the tolerance 1e-4 x mean variance)
 *   pope_shift_columns      out = X + sign * shift[c]
 *   pope_kmeans_plusplus    k-means++ seeding: chosen[K] (device int64) = the seeded rows, in order.  uniforms_host:
 *                           (K - 1) x n_trials doubles in [0, 1), step-major.  No host synchronisation after the upload.
 *   pope_kmeans_lloyd_step  one Lloyd iteration: labels (N x K products on the f32 MFMA tile + row argmin, first minimum
 *                           wins), new centres (mean of the members, float64 sums in index order; an empty cluster keeps
 *                           its centre), *changed (device int) = some label differs from labels_prev, *shift_total (device
 *                           double) = sum of squared centre shifts.  Deterministic.  Asynchronous on `stream`.
 * scratch: pope_kmeans_scratch_bytes(N, D, K) for the two kmeans calls; 4096 * D * 8 bytes for pope_column_moments.
 * ------------------------------------------------------------------------------------------------ */
size_t pope_kmeans_scratch_bytes(int64_t N, int32_t D, int32_t K);
int pope_column_moments(const float *X, int64_t N, int32_t D, double *sum, double *sumsq, void *scratch, size_t scratch_bytes,
                        void *stream);
int pope_shift_columns(const float *X, const float *shift, int64_t N, int32_t D, float sign, float *out, void *stream);
int pope_kmeans_plusplus(const float *X, int64_t N, int32_t D, int32_t K, int64_t first_id, const double *uniforms_host,
                         int32_t n_trials, int64_t *chosen, void *scratch, size_t scratch_bytes, void *stream);
int pope_kmeans_lloyd_step(const float *X, int64_t N, int32_t D, const float *centers, int32_t K, float *centers_new,
                           int32_t *labels, const int32_t *labels_prev, int32_t *changed, double *shift_total,
                           void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Geodesic embedding.
 *
 * Hop counts are kept BIT-SLICED ("hop planes"): anchors are packed 64 per uint64 word, W = pope_words(K)
 * words per node, and a plane is a uint64 [N, W] array.  planes[0] is the reachability plane (bit j of
 * node v set <=> a directed path v -> anchors[j] exists); planes[1 + b] holds bit b of the hop count.
 * This is also the shard exchange format for multi-GPU runs: a rank that owns anchors
 * [k0, k0 + K_local) produces planes for K_local and the shards are concatenated by an all-gather.
 * ------------------------------------------------------------------------------------------------ */

/* Words per node for K anchors: ceil(K / 64) rounded up to 1, 2 or a multiple of 4. */
int32_t pope_words(int32_t K);

/* Bytes of one plane, and of the scratch pope_geodesic_bfs needs (a control block, the anchors, three rotating frontier planes,
 * their three one-bit-per-node live tables and one summary of a live table). */
size_t pope_plane_bytes(int64_t N, int32_t K);
size_t pope_bfs_scratch_bytes(int64_t N, int64_t E, int32_t K);

/*
 * Multi-source BFS from all K anchors at once over the CSR of pope_csr_build.
 *   anchors_host   int64 [K] on the HOST (the reference samples them on the host: utils.py:22-24); duplicates kept.
 *   planes         uint64 [plane_capacity + 1, N, W]; need not be initialised.  On return planes
 *                  [0, 1 + *n_hop_bits) are valid, the rest untouched.
 *   scratch        pope_bfs_scratch_bytes(N, E, K) bytes.
 *   max_hop_host   (out, host) largest finite hop count found.
 *   n_hop_bits_host(out, host) number of hop-bit planes written = bits needed for *max_hop.
 * Returns POPE_ERR_HOP_OVERFLOW if a hop count would need more than plane_capacity bits.
 * Synchronises `stream` (the level loop polls a device flag every few levels).
 */
int pope_geodesic_bfs(const int32_t *rowptr, const int32_t *col, const int32_t *erow, const int32_t *aux,
                      int64_t N, int64_t E,
                      const int64_t *anchors_host, int32_t K, uint64_t *planes, int32_t plane_capacity, void *scratch, size_t scratch_bytes,
                      int32_t *max_hop_host, int32_t *n_hop_bits_host, void *stream);

/*
 * The same BFS in two halves (identical arguments): _begin enqueues the clears, the seed and the first 12 levels and
 * returns without waiting; _finish synchronises `stream`, reads the verdict and keeps going if the graph is deeper.
 * Work enqueued on `stream` in between (an all-gather of planes[0 .. 5), the finalise kernel) runs speculatively: it is
 * valid iff _finish reports *n_hop_bits <= 4 (planes 1..4 are cleared up front, so unused hop-bit planes read as zero).
 * The pinned anchor staging buffer is per device: do not begin a second BFS on the device before finishing the first.
 */
int pope_geodesic_bfs_begin(const int32_t *rowptr, const int32_t *col, const int32_t *erow, const int32_t *aux,
                            int64_t N, int64_t E, const int64_t *anchors_host, int32_t K, uint64_t *planes,
                            int32_t plane_capacity, void *scratch, size_t scratch_bytes, void *stream);
int pope_geodesic_bfs_finish(const int32_t *rowptr, const int32_t *col, const int32_t *erow, const int32_t *aux,
                             int64_t N, int64_t E, const int64_t *anchors_host, int32_t K, uint64_t *planes,
                             int32_t plane_capacity, void *scratch, size_t scratch_bytes, int32_t *max_hop_host,
                             int32_t *n_hop_bits_host, void *stream);

/*
 * out[v, 0:F] = x[v, :],  out[v, F + c0 + j] = 1.0f / (hops(v, anchor j) + 1), 0.0f if unreachable,
 * for the K_shard anchors of one shard.  out is float32 [N, out_cols] row-major with out_cols >= F + c0 + K_shard;
 * x may be NULL (then only the embedding columns are written: used for shards after the first).
 * Asynchronous on `stream`.
 */
int pope_geodesic_finalize(const uint64_t *planes, int32_t n_hop_bits, int64_t N, int32_t K_shard,
                           const float *x, int32_t F, float *out, int64_t out_cols, int32_t c0, void *stream);

/*
 * Multi-GPU form: `planes` holds n_shards all-gathered shards back to back, shard g at planes + g * shard_stride_words,
 * each [1 + n_hop_bits, N, W(K_shard)] for K_shard anchors; writes x and the columns of ALL shards
 * (out[v, F + g * K_shard + j]) in one pass over the output.  Asynchronous on `stream`.
 */
int pope_geodesic_finalize_shards(const uint64_t *planes, int32_t n_shards, int64_t shard_stride_words, int32_t n_hop_bits,
                                  int64_t N, int32_t K_shard, const float *x, int32_t F, float *out, int64_t out_cols,
                                  void *stream);

/* The name of the finalise kernel the three calls above and pope_geodesic_run launch for a shape, as a kernel trace shows it
 * ("k_finalize_pipe<2, 1>", "k_finalize_wide<0>", ...), written into name[0 .. cap): lets a measurement label itself with the
 * kernel that really ran (utils.py:129-135 is one torch.cat whatever the shape).  It is the launch's own plan (csrc/geodesic.hip:
 * finalize_plan) under the current pope_debug_set settings, fed with what this signature cannot know as assumptions: 16-byte-aligned
 * x and out, c0 = 0, out_cols = F + n_shards * K_shard, hop counts of at most four bits (graphs no deeper than 15 levels), a
 * side-stream slot on the device.  A call with an unaligned base or odd pitch, or on a deeper graph, launches the generic
 * k_finalize instead, which this query cannot tell.  Host logic: needs no device. */
int pope_finalize_kernel_name(int64_t N, int32_t K_shard, int32_t F, int32_t has_x, int32_t n_shards, char *name, size_t cap);
/* The same query with the alignment assumption lifted: bit 0 of `misaligned` says that x, bit 1 that out is NOT 16-byte aligned (other
 * bits: POPE_ERR_INVALID).  pope_finalize_kernel_name is this call with misaligned = 0. */
int pope_finalize_kernel_name_at(int64_t N, int32_t K_shard, int32_t F, int32_t has_x, int32_t n_shards, uint32_t misaligned, char *name,
                                 size_t cap);

/* The same for the level kernel of a BFS over N nodes from K anchors ("k_bfs_level<4, 1, 0>": words per tile, how the live-bit table is
 * read, how a node's tiles are walked -- csrc/geodesic.hip: level_plan, the function the launch follows, under the current
 * POPE_KNOB_LIVE_MODE).  The name follows N, K and the knob alone; the edge count and the device's CU count only size the grid.
 * Host logic: needs no device. */
int pope_level_kernel_name(int64_t N, int32_t K, char *name, size_t cap);

/*
 * The whole geodesic hot path in ONE call (what utils.py:137-147 does after sampling the anchors):
 * edge_index -> CSR -> multi-source BFS -> out[v, 0:F] = x[v, :], out[v, F + j] = 1 / (hops(v, anchor j) + 1).
 * Everything is enqueued speculatively (sorted-CSR fast path, 12 BFS levels, the finalise kernel reading the
 * depth from device memory).  The host then waits ONCE, for the BFS verdict only: the finalise kernel publishes it
 * in pinned host memory when it starts, and the call returns while `out` is still being written -- `out`, like the
 * result of any asynchronous call, is complete in `stream` order (synchronise `stream` before reading it from the
 * host or from another stream).  Unsorted edge lists and graphs deeper than 10 hops transparently take the general
 * path (stream synchronisations in between).
 * workspace: pope_geodesic_run_workspace_bytes(N, E, K, plane_capacity) bytes, device memory, no initialisation
 * needed; afterwards pope_geodesic_run_planes() locates the hop planes inside it (planes [0, 1 + *n_hop_bits) valid).
 * out may be NULL (BFS only).  Returns POPE_ERR_HOP_OVERFLOW if plane_capacity bits cannot hold the depth.
 */
size_t pope_geodesic_run_workspace_bytes(int64_t N, int64_t E, int32_t K, int32_t plane_capacity);
uint64_t *pope_geodesic_run_planes(void *workspace, int64_t N, int64_t E, int32_t K, int32_t plane_capacity);
int pope_geodesic_run(const int64_t *edge_index, int64_t E, int64_t N, const int64_t *anchors_host, int32_t K,
                      const float *x, int32_t F, float *out, int64_t out_cols, int32_t plane_capacity,
                      void *workspace, size_t workspace_bytes, int32_t *max_hop_host, int32_t *n_hop_bits_host,
                      void *stream);

/*
 * Measurement hook (bench.py): enable = 1: every BFS level launch is bracketed by HIP events on the launch stream and
 * pope_profile_read returns, per level launched since enabling, the level number and the elapsed milliseconds of its
 * kernel (waits for the events).  enable = 2: ONE event pair around each enqueued run of level launches (no events
 * between the kernels, so the pipeline is undisturbed); pope_profile_read then returns one entry per run with
 * levels[i] = -(number of launches in the run) and the elapsed milliseconds of the whole run.  0 disables.
 * Not thread-safe; off by default.
 */
void pope_profile_levels(int32_t enable);
int32_t pope_profile_read(int32_t *levels_host, float *level_ms_host, int32_t capacity);
/* How many of the level-1 launches enqueued since pope_profile_levels(1 or 2) were k_bfs_level1_apply (POPE_KNOB_LEVEL1_APPLY) and
 * not the level kernel; the entries pope_profile_read returns do not tell the two apart: level 1 is level 1. */
int32_t pope_profile_level1_applies(void);

/* Integer hop matrix: hops int32 [N, K] node-major, -1 = unreachable.  Asynchronous on `stream`. */
int pope_geodesic_hops(const uint64_t *planes, int32_t n_hop_bits, int64_t N, int32_t K,
                       int32_t *hops, void *stream);

/*
 * Column statistics of the hop matrix, straight from the planes: reach[j] = number of nodes with a path to anchor j
 * (the anchor included), hop_sum[j] = sum of their hop counts; both int64 [K] on the device.  What closeness
 * centrality needs (utils.py:50-54: nx.closeness_centrality uses inward distances on a DiGraph).  Asynchronous.
 */
size_t pope_column_stats_scratch_bytes(int32_t K);
int pope_geodesic_column_stats(const uint64_t *planes, int32_t n_hop_bits, int64_t N, int32_t K, int64_t *hop_sum,
                               int64_t *reach, void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * node2vec-space embedding: pairwise distance to the anchor rows + per-column min-max scaling.
 * ------------------------------------------------------------------------------------------------ */
#define POPE_METRIC_COSINE_DISTANCE   0   /* 'distance'   -> sklearn cosine_distances   */
#define POPE_METRIC_COSINE_SIMILARITY 1   /* 'similarity' -> sklearn cosine_similarity  */
#define POPE_METRIC_EUCLIDEAN         2   /* 'euclidean'  -> sklearn euclidean_distances */

size_t pope_pairwise_scratch_bytes(int64_t N, int32_t K, int32_t D);

/*
 * X float32 [N, D]; A float32 [K, D] (the anchor rows); writes the min-max scaled [N, K] block into
 * out[v, c0 + j] of a float32 [N, out_cols] matrix.  Scaling is per column over all N rows:
 * y = e * (1 / range) + (0 - min * (1 / range)), range < 10 * FLT_EPSILON treated as 1.
 * Asynchronous on `stream`.
 */
int pope_pairwise_minmax(const float *X, int64_t N, int32_t D, const float *A, int32_t K, int32_t metric,
                         float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                         void *stream);
/* utils.py:165-167 as written there -- embedding[anchor_nodes] and the distances in one call: anchor j is row anchor_ids[j]
 * (DEVICE int64, each in [0, N)) of X, read through the ids by the tile kernel (no gathered copy of the anchor rows, no gather
 * launch in front of the call).  x = NULL / F = 0: the embedding columns alone.  Scratch: pope_pairwise_by_id_scratch_bytes. */
size_t pope_pairwise_by_id_scratch_bytes(int64_t N, int32_t K, int32_t D);
int pope_pairwise_features_by_id(const float *x, int32_t F, const float *X, int64_t N, int32_t D, const int64_t *anchor_ids, int32_t K,
                                 int32_t metric, float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                                 void *stream);

/*
 * The same with the feature half of utils.py:177 concat_into_features fused in: out[v, 0:F] = x[v, :] (x float32 [N, F],
 * may be NULL) is streamed by the blocks of the tile kernel between their product and their epilogue, next to the embedding
 * columns out[v, c0 + j], c0 >= F: the copy's HBM time hides under the MFMA work.  Asynchronous on `stream`.
 */
int pope_pairwise_features(const float *x, int32_t F, const float *X, int64_t N, int32_t D, const float *A, int32_t K,
                           int32_t metric, float *out, int64_t out_cols, int32_t c0, void *scratch, size_t scratch_bytes,
                           void *stream);

/* What pope_pairwise_features (by_id = 0) or pope_pairwise_features_by_id (by_id = 1) launches for these sizes on a device of cu_count
 * compute units, in launch order, joined by '+', as a kernel trace shows them, written into name[0 .. cap) (POPE_ERR_INVALID for bad
 * arguments and if the names do not fit; 256 bytes always do).  has_x = 0 or F = 0: the embedding columns alone.  Depths up to 128 in
 * 16-byte pieces with out below 4 GB: "k_pairwise_persistent[sets=S]" (S consumer sets), "k_copy_features" behind it when the feature
 * copy runs on the side stream, "k_minmax_finish", then "k_minmax_apply4" (16-byte pieces) or "k_minmax_apply".  Everything else:
 * "k_gather_anchor_rows" (by_id only), "k_sqnorm<V>", "k_pairwise<L>" (L: operand layout, 1 depth-contiguous vectors with V = true,
 * 0 generic with V = false; "[copy]" behind it: the blocks carry the feature copy), "k_minmax_fold", "k_minmax_reduce" and the apply
 * kernel.  "pope_concat" in front: the feature copy as a pass of its own (F or F + K no multiple of 4, or more than 4096 feature
 * columns beside the persistent kernel).  It is the library's own choice (csrc/pairwise.hip: pairwise_plan) for 16-byte-aligned
 * bases, c0 = F, out_cols = F + K and a device with a side-stream slot, under the current POPE_KNOB_PAIRWISE_KERNEL.  Host logic:
 * needs no device. */
int pope_pairwise_kernel_name(int64_t N, int32_t D, int32_t K, int32_t F, int32_t has_x, int32_t by_id, int32_t cu_count, char *name,
                              size_t cap);
/* The same query with the alignment assumption lifted: bit i of `misaligned` says that operand i of {X, A, x, out, scratch} (the order of
 * csrc/pairwise.hip: PwAligned) is NOT 16-byte aligned (higher bits: POPE_ERR_INVALID).  A misaligned X or A refuses the persistent
 * kernel and the vector forms of k_sqnorm / k_pairwise, a misaligned x or out makes the feature copy a pope_concat in front, a misaligned
 * out or scratch turns k_minmax_apply4 into k_minmax_apply.  pope_pairwise_kernel_name is this call with misaligned = 0. */
int pope_pairwise_kernel_name_at(int64_t N, int32_t D, int32_t K, int32_t F, int32_t has_x, int32_t by_id, int32_t cu_count,
                                 uint32_t misaligned, char *name, size_t cap);

/* out[v, 0:F] = x[v, :] for a float32 [N, out_cols] matrix (the feature half of torch.cat). Asynchronous. */
int pope_concat(const float *x, int64_t N, int32_t F, float *out, int64_t out_cols, void *stream);

/*
 * HOST memory on both sides: copy `rows` rows of `row_bytes` bytes from src (row pitch src_pitch_bytes) to dst (row
 * pitch dst_pitch_bytes) with `threads` host threads (<= 0: all hardware threads) and streaming stores; returns when
 * the copy is complete.  The host half of torch.cat((data.x, embedding), 1) (utils.py:129-135) for the host -> host
 * Graphpope call: data.x never crosses PCIe -- it goes straight into the result tensor's first F columns on the
 * host cores while the GPU computes and ships only the K embedding columns.  No HIP call is made.
 */
int pope_host_copy_2d(const void *src_host, int64_t src_pitch_bytes, void *dst_host, int64_t dst_pitch_bytes,
                      int64_t row_bytes, int64_t rows, int32_t threads);

/*
 * The embedding half of the same torch.cat: `rows` rows of `row_bytes` bytes from DEVICE memory (pitch src_pitch_bytes)
 * into the last K columns of the host result (dst_host, row pitch dst_pitch_bytes; pinned memory makes it a true
 * asynchronous DMA on `stream`).  Only these K columns ever cross PCIe.  Asynchronous on `stream`.
 */
int pope_copy_2d_to_host(const void *src, int64_t src_pitch_bytes, void *dst_host, int64_t dst_pitch_bytes,
                         int64_t row_bytes, int64_t rows, void *stream);

/*
 * The whole torch.cat((data.x, embedding), 1) of the host -> host call (utils.py:129-135) into an ORDINARY PAGEABLE
 * result, as the reference returns one: out[:, :x_row_bytes] = x_host rows (host threads, streaming stores) and
 * out[:, x_row_bytes : x_row_bytes + emb_row_bytes] = emb rows (DEVICE memory, DMA on `stream`, behind whatever produced
 * emb there).  The feature columns are filled by `threads` host threads over `chunks` row chunks (<= 0: 8; first touch:
 * MADV_HUGEPAGE is applied first); the embedding rows come over in 8 MB chunks through three pinned slots that are allocated
 * once per process, and the worker threads copy each landed chunk out while the next one is on the bus -- no page of the
 * result is ever registered with the runtime.  If the pinned ring is refused (or a row is wider than a slot) the rows are staged
 * through a 4 MB pinned bounce buffer of the library's own and copied out by the calling thread (slower, same bytes; only if
 * that buffer is refused as well does a blocking copy by the runtime write the pageable rows).  `stream` is synchronised
 * before the call returns.  x_row_bytes or emb_row_bytes may be 0.
 */
int pope_assemble_host_result(const void *x_host, int64_t x_pitch_bytes, int64_t x_row_bytes, const void *emb,
                              int64_t emb_pitch_bytes, int64_t emb_row_bytes, void *out_host, int64_t out_pitch_bytes,
                              int64_t rows, int32_t threads, int32_t chunks, void *stream);

/*
 * The same in two halves, so that the page faults and the feature copy run UNDERNEATH the upload of edge_index and the GPU
 * work: pope_assemble_begin starts the host threads on out[:, :x_row_bytes] = x_host and returns a handle (NULL + an error
 * message on bad arguments); pope_assemble_finish brings the embedding columns down as pope_assemble_host_result does,
 * waits for everything and frees the handle (also when it fails).  pope_assemble_abort frees a handle that will not be finished.
 */
void *pope_assemble_begin(const void *x_host, int64_t x_pitch_bytes, int64_t x_row_bytes, void *out_host, int64_t out_pitch_bytes,
                          int64_t rows, int32_t threads, int32_t chunks);
int pope_assemble_finish(void *handle, const void *emb, int64_t emb_pitch_bytes, int64_t emb_row_bytes, void *stream);
void pope_assemble_abort(void *handle);
/* Optional, returns at once: the process's pinned ring (24 MB, 2 ms of hipHostMalloc) is allocated by a helper thread on
 * `device` (< 0: the thread's default), beside the caller's GPU work, instead of inside the first pope_assemble_finish. */
void pope_assemble_prepare(int32_t device);
/* 1 if pope_assemble_finish_codes can be used now (the pinned ring exists or could be allocated by this call), else 0 -- the
 * caller then brings float columns down with pope_assemble_finish, which stages them through the bounce buffer.  Waits for an
 * allocation that pope_assemble_prepare started. */
int32_t pope_assemble_ring_ready(void);

/*
 * The geodesic embedding in its transport form (utils.py:73 1 / len(path), one byte per element instead of four):
 * pope_geodesic_hop_codes writes codes[v * pitch + j] = 0 if node v has no path to anchor j, hops + 1 otherwise, and the
 * 256 floats the bytes stand for (lut[0] = 0, lut[c] = 1 / c, the finalise kernel's own arithmetic) -- hop counts above 254
 * are refused (POPE_ERR_INVALID; use pope_geodesic_finalize).  pope_assemble_finish_codes is pope_assemble_finish for that
 * form (it needs the pinned ring): K code bytes per row cross PCIe -- a quarter of the float columns -- and the worker threads write
 * out[:, x_row_bytes + 4 j] = lut[code] while they copy out of the ring; the host looks floats up, it computes none.
 */
int pope_geodesic_hop_codes(const uint64_t *planes, int32_t n_hop_bits, int32_t max_hop, int64_t N, int32_t K, uint8_t *codes,
                            int64_t codes_pitch_bytes, float *lut, void *stream);
int pope_assemble_finish_codes(void *handle, const uint8_t *codes, int64_t codes_pitch_bytes, int32_t K, const float *lut, void *stream);

/*
 * Caller-owned pageable HOST memory as a DMA endpoint for the length of one call: pope_host_pin registers the WHOLE PAGES
 * inside [host, host + bytes) with the HIP runtime -- never the partial pages at the two ends, which a heap allocation shares
 * with other objects (POPE_ERR_HIP if refused, or if fewer than 1 MB of whole pages lie inside: the caller then stages through
 * pinned memory instead); pope_copy_to_device enqueues the asynchronous host -> device copy on `stream` (for a pinned buffer:
 * the body by DMA from the registered pages, the two end fragments as plain copies); pope_host_unpin releases the pages (after
 * the copy has completed; POPE_ERR_INVALID for a pointer pope_host_pin did not pin).  Used for edge_index (utils.py:121):
 * 14.4 MB go up straight from the caller's tensor.
 */
int pope_host_pin(const void *host, size_t bytes);
int pope_host_unpin(const void *host);
int pope_copy_to_device(const void *src_host, void *dst, size_t bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * SAGEConv over a sampled bipartite block (CSR by destination; destinations are the first n_dst sources).
 *   out = lin_l(mean_{j in N(i)} x_src[j]) + lin_r(x_src[i]),  lin_l with bias, lin_r without.
 * ------------------------------------------------------------------------------------------------ */
/*
 * Device extents.  A mini-batch sampled on the device (sage_sample_batch_device) has data-dependent sizes; reading them
 * back costs a host synchronisation per step.  Every SAGE entry point below therefore takes `dims`: NULL (the int64 size
 * arguments ARE the sizes), or a DEVICE pointer to int32 [4] = {n_dst, n_src, nnz, 0} as the sampler wrote it.  The size
 * arguments are then CAPACITIES (buffer extents, grid sizing; true value <= capacity) and every kernel reads the true
 * sizes on the device: nothing is read back, and the same launches can be captured into a HIP graph and replayed on new
 * batches.  Rows beyond the true extents of an output are left untouched.
 */
size_t sage_conv_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out);   /* backward */
size_t sage_conv_forward_scratch_bytes(int64_t n_dst, int32_t c_in, int32_t c_out);                         /* forward  */

/*
 * rowptr int32 [n_dst + 1], col int32 [nnz] (indices into x_src), x_src f32 [n_src, c_in],
 * w_l / w_r f32 [c_out, c_in], b_l f32 [c_out] or NULL, out f32 [n_dst, c_out].
 * agg (f32 [n_dst, c_in]) receives the mean-aggregated features (kept for backward).
 * scratch: sage_conv_forward_scratch_bytes(n_dst, c_in, c_out) bytes (0 for small layers: scratch may be NULL then) --
 * the partial-tile slabs of the stream-K projection; with less, the projection falls back to whole-tile kernels.
 * Asynchronous.
 */
int sage_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                      const float *x_src, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                      int32_t c_out, float *agg, float *out, void *scratch, size_t scratch_bytes, const int32_t *dims,
                      void *stream);

/* The aggregation half on its own: agg[i, :] = mean_{p in row i} x_src[col[p], :] (zero for empty rows).  Asynchronous. */
int sage_gather_mean(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                     const float *x_src, int32_t c_in, float *agg, void *stream);

/*
 * Gradients.  grad_out f32 [n_dst, c_out].  grad_x f32 [n_src, c_in] (may be NULL), grad_w_l, grad_w_r
 * f32 [c_out, c_in], grad_b_l f32 [c_out] (may be NULL) are OVERWRITTEN.  Asynchronous.
 */
/*
 * sage_conv_forward on rows of a resident feature matrix: block-local source j is feats[n_id[j]] (feats: [n_rows, c_in],
 * n_id: int64 [n_src] on the device, its first n_dst entries are the destinations).  Replaces convert_batch's
 * x = data.x[n_id] (main.py:118-123) followed by the layer: the [n_src, c_in] gather is never materialised.
 * x_dst (out): [n_dst, c_in] = feats[n_id[:n_dst]], to be passed to sage_conv_backward as x_src (with n_src = n_dst and
 * grad_x = NULL: features have no gradient).
 */
int sage_conv_forward_indexed(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                              int64_t nnz, const float *feats, int64_t n_rows, int32_t c_in, const float *w_l, const float *b_l,
                              const float *w_r, int32_t c_out, float *agg, float *x_dst, float *out, void *scratch,
                              size_t scratch_bytes, const int32_t *dims, void *stream);
/*
 * The same two forward calls for a layer whose output goes into BatchNorm (main.py:206-207: x = convs[i](...); x = bns[i](x)): the
 * projection's epilogue also leaves the column sums of `out` and of its squares, per row tile, in bn_pa / bn_pb ([bn_parts_cap, c_out]
 * float64 each; bn_parts_cap >= ceil(n_dst / 16) always suffices) -- the first stage of the BatchNorm statistics, which otherwise is a
 * launch of its own that reads `out` back.  bn_info (HOST, 2 ints, out): [0] = row tiles written (0: this shape's kernels produce no
 * statistics -- call sage_bn_relu_dropout_forward as usual), [1] = rows per tile; pass both to sage_bn_relu_dropout_forward_stats.
 */
int sage_conv_forward_stats(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                            int32_t c_in, const float *w_l, const float *b_l, const float *w_r, int32_t c_out, float *agg, float *out,
                            void *scratch, size_t scratch_bytes, const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap,
                            int32_t *bn_info, void *stream);
int sage_conv_forward_indexed_stats(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                                    int64_t nnz, const float *feats, int64_t n_rows, int32_t c_in, const float *w_l, const float *b_l,
                                    const float *w_r, int32_t c_out, float *agg, float *x_dst, float *out, void *scratch,
                                    size_t scratch_bytes, const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap,
                                    int32_t *bn_info, void *stream);
/* The kernels the four forward calls above launch for the projection of a layer of this shape on a device of cu_count compute units,
 * as a kernel trace shows them, written into name[0 .. cap): "k_gather_beside_gemm<R>+k_gemm_tile16<R, B>" (the gather beside half of
 * the projection, then the other half), "k_gemm_tile16<R, B>", "k_gemm_streamk_ld<32>" or "k_gemm<TM, TN>" (layout parameters omitted).
 * It is the library's own choice (csrc/sage.hip: forward_plan) for 16-byte-aligned operands, host extents and the scratch the size
 * queries ask for, under the current pope_debug_set settings.  Host logic: needs no device. */
int sage_forward_kernel_name(int64_t n_dst, int32_t c_in, int32_t c_out, int32_t cu_count, char *name, size_t cap);
/* The same query with the alignment assumption lifted: bit i of `misaligned` says that operand i of {x, agg, own, x_dst_out, w_l, w_r} (the
 * order of csrc/sage.hip: FwdAligned) is NOT 16-byte aligned (higher bits: POPE_ERR_INVALID).  x: the matrix the rows are gathered from
 * (x_src, or feats); own: the matrix the one-pass projection reads the destination rows from (x_src itself, else x_dst, else the tail of
 * the scratch buffer: for a plain call set bits 0 and 2 together); x_dst_out: the x_dst an indexed call was given.  With a non-zero mask
 * the string also names the gather ("k_gather_mean<V>+" in front; the overlapped form carries its own) and prints the plain tile kernel
 * as "k_gemm<TM, TN, WM, WN, LA, LB>" (LA / LB as in sage_backward_kernel_name).  sage_forward_kernel_name is this call with
 * misaligned = 0. */
int sage_forward_kernel_name_at(int64_t n_dst, int32_t c_in, int32_t c_out, int32_t cu_count, uint32_t misaligned, char *name, size_t cap);
int sage_conv_backward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz,
                       const float *x_src, const float *agg, int32_t c_in, const float *w_l, const float *w_r,
                       int32_t c_out, const float *grad_out, float *grad_x, float *grad_w_l, float *grad_b_l,
                       float *grad_w_r, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream);
/* The kernels sage_conv_backward launches for a layer of these CAPACITIES on a device of cu_count compute units, in launch order, joined
 * by '+', as a kernel trace shows them, written into name[0 .. cap) (POPE_ERR_INVALID if they do not fit; 256 bytes always do).  The
 * weight gradients come first: "k_colsum_partial<V>+k_gemm_streamk_tn<32>+k_streamk_tn_fixup<32>" (stream-K; "[xcd]" behind the first
 * kernel marks the XCD-aware deal, the column sums are there only with a bias gradient), or "k_gemm_dual<64, 64, 2, 2>[splits=S]+
 * k_scatter_and_finals" (the whole small layer in two launches), or "k_gemm<TM, TN, WM, WN, LA, LB>[splits=S]+k_slab_reduce" (split-K twin;
 * LA / LB: operand layouts, 0 generic, 1 depth-contiguous vectors, 2 outer-contiguous vectors; one split: no marker, no reduction)
 * followed by "k_colsum_partial<V>+k_colsum_final"; then, with an input gradient, "k_zero_rows" (n_src > n_dst), the twin "k_gemm<...>"
 * of grad_x and k_scatter_mean.  It is the library's own choice (csrc/sage.hip: backward_plan) for 16-byte-aligned operands, at
 * least one edge and the scratch sage_conv_scratch_bytes asks for, under the current pope_debug_set settings; device extents change
 * nothing (the launches are sized by the capacities).  sage_conv_backward_indexed launches what need_grad_x = 0 names, with
 * k_gather_rows in front unless the weight gradients are stream-K.  Host logic: needs no device.
 * Deterministic mode (sage_set_deterministic(1), below) with an input gradient: no "k_zero_rows" and no "k_scatter_mean", the dual path
 * ends in "k_bwd_finals", and every chain closes with "k_det_clear+k_det_index<false>+k_det_scan+k_det_index<true>+k_scatter_sum_det<V>"
 * (the index build and the sum; V: 16-byte accesses, c_in % 4 == 0).  Without an input gradient the mode changes no name. */
int sage_backward_kernel_name(int64_t n_dst, int64_t n_src, int32_t c_in, int32_t c_out, int32_t need_grad_x, int32_t need_grad_b,
                              int32_t cu_count, char *name, size_t cap);
/* The same query with the alignment assumption lifted: bit i < 8 of `misaligned` says that operand i of {grad_out, agg, x, x_tmp, w_l,
 * w_r, grad_agg, grad_x} (the order of csrc/sage.hip: BwdAligned) is NOT 16-byte aligned.  x: x_src, or feats of the indexed call; x_tmp
 * and grad_agg lie in the scratch buffer.  Bit 8 says that the call is sage_conv_backward_indexed (need_grad_x must be 0): the string then
 * names "k_gather_rows" where it runs.  Higher bits: POPE_ERR_INVALID.  sage_backward_kernel_name is this call with misaligned = 0. */
int sage_backward_kernel_name_at(int64_t n_dst, int64_t n_src, int32_t c_in, int32_t c_out, int32_t need_grad_x, int32_t need_grad_b,
                                 int32_t cu_count, uint32_t misaligned, char *name, size_t cap);

/*
 * Deterministic mode.  sage_conv_backward adds the input gradient of a hidden layer with float atomics, in the order the waves
 * arrive: the one place where two runs of a training step on the same inputs may differ in their last bits.  sage_set_deterministic(1)
 * replaces that scatter by the sum below and makes sage_eval_metrics launch ONE block (one atomic add per launch: the adds of a pass
 * land in stream order); both are then pure functions of their inputs.  Off (0) is the default and changes nothing.  Process-wide host
 * state, like pope_debug_set; needs no device; returns the previous value.  The setting is read when a call is made: launches captured
 * into a HIP graph keep the mode they were captured under, and sage_conv_scratch_bytes includes the room of the index while it is on
 * (size and call must see the same setting).  sage_conv_backward_indexed has no input gradient and is unaffected.
 */
int32_t sage_set_deterministic(int32_t on);
int32_t sage_get_deterministic(void);
/*
 * The sum on its own.  rowptr / col: the block (CSR by destination), grad_agg f32 [n_dst, c], grad_x f32 [n_src, c], IN and OUT.
 * For every true source row j < n_src and every column ch:
 *     acc = (j < n_dst) ? grad_x[j][ch] as found on entry : +0.0f
 *     for every slot p with col[p] == j, in ASCENDING p:           (i = the destination row that holds slot p)
 *         acc = fadd_rn(acc, fmul_rn(grad_agg[i][ch], inv_i))      (inv_i = 1.0f / (float)(rowptr[i + 1] - rowptr[i]), correctly rounded)
 *     grad_x[j][ch] = acc
 * The product is rounded, then added: no fused multiply-add.  Rows at or beyond the true n_src are left untouched; rows in
 * [n_dst, n_src) are OVERWRITTEN, so nothing needs to zero them first.  Slots outside [0, nnz) and sources outside [0, n_src) are
 * skipped.  `dims` as under "Device extents": the sizes are then capacities and the true {n_dst, n_src} are read on the device (the
 * true nnz is rowptr[n_dst]).  scratch: sage_scatter_mean_det_scratch_bytes(n_src, n_dst, nnz) bytes (the capacities), 4-byte aligned,
 * rebuilt by every call: nothing an earlier call left there is read.  Asynchronous, no host synchronisation, no allocation; capturable.
 * POPE_ERR_INVALID before any HIP call: a null pointer, a negative size, n_dst > n_src, sizes >= 2^31 - 1, c <= 0, too little scratch.
 * n_src == 0 is an empty call.  With capacities n_src == n_dst and nnz == 0 there is nothing to add or overwrite: no launch.
 */
size_t sage_scatter_mean_det_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz);
int sage_scatter_mean_det(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *grad_agg,
                          int32_t c, float *grad_x, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream);

/*
 * Sum and max aggregation: SAGEConv(aggr='add' | 'max'), the two other aggregators PyG 1.7.0's SAGEConv accepts (believed, SURVEY.md:
 * kwargs.setdefault('aggr', 'mean'), then matmul(adj_t, x, reduce=aggr)).  The block is sage_conv_forward's: CSR by destination, the
 * destinations are the first n_dst sources, `dims` as under "Device extents".  Only the aggregation half differs from the mean's layer
 * (csrc/aggregate.hip); out = agg W_l^T + b_l + x_dst W_r^T runs on the projection kernels of sage_conv_forward.
 *
 * Forward, per destination i and column ch, over the slots p in [rowptr[i], rowptr[i + 1]):
 *   add   s = +0.0f, then s = s + x[col[p]][ch] for p ASCENDING, with ONE accumulator: the result equals a sequential float32 loop bit for
 *         bit.  An empty row gives +0.
 *   max   best = x[col[beg]][ch] and a = col[beg]; then, p ascending, v = x[col[p]][ch] replaces best (and a = col[p]) iff v > best, or v
 *         is NaN and best is not.  Ties stay with the first slot; if any neighbour value is NaN the result is NaN and a is the first NaN's
 *         source.  best never starts from 0: a column of negatives has a negative maximum.  An empty row gives +0 and a = -1.
 *         arg[i][ch] = a (int32 [n_dst, c]) is the BLOCK-LOCAL source id -- in indexed mode the position in n_id, not the feature row.
 *         arg may be NULL: nothing is recorded, for layers whose input takes no gradient (layer 0 behind a feature matrix always is one).
 * Backward: the gradient of agg goes to grad_x by an ORDERED sum under both aggregators and in both modes of sage_set_deterministic --
 * never with float atomics, so add and max are bit-reproducible and the mode changes nothing for them.  For every true source j < n_src
 * and every column ch:
 *     acc = (j < n_dst) ? grad_x[j][ch] as found on entry : +0.0f
 *     for every slot p with col[p] == j, in ASCENDING p:           (i = the destination row that holds slot p)
 *         add: acc = acc + grad_agg[i][ch]
 *         max: acc = acc + grad_agg[i][ch]   only if arg[i][ch] == j and p is the FIRST slot of row i that names j
 *     grad_x[j][ch] = acc
 * A destination that lists j twice contributes twice under add and once under max.  Rows [n_dst, n_src) are OVERWRITTEN; rows at or
 * beyond the true n_src are untouched; slots outside [0, nnz) and sources outside [0, n_src) are skipped, forward and backward.
 * Everything else (scratch rebuilt by every call, empty calls, what is refused) is the contract of sage_scatter_mean_det.
 *
 * All entry points are asynchronous and capturable: no host synchronisation, no allocation.  Before any HIP call: POPE_ERR_INVALID for an
 * unknown aggr, for POPE_AGGR_MAX with a grad_x but no arg, for a null pointer or a bad size; POPE_ERR_WORKSPACE for too little scratch,
 * the needed size in pope_last_error().
 *
 * sage_aggregate_forward / sage_aggregate_backward: the two halves on their own, as sage_gather_mean and sage_scatter_mean_det are for the
 * mean (aggr: POPE_AGGR_ADD or POPE_AGGR_MAX; POPE_AGGR_MEAN is refused: the mean has those two calls).  x f32 [x_rows, c]: the block's
 * sources (n_id NULL; x_rows >= n_src), or the resident feature matrix with source j in row n_id[j]; x_dst f32 [n_dst, c] or NULL (indexed
 * mode only) receives the destinations' own rows.  scratch: sage_aggregate_backward_scratch_size(n_src, n_dst, nnz), 4-byte aligned.
 * (Both size queries of this family answer in bytes and are named _scratch_size, as sage_full_layer_scratch_size is.)
 *
 * sage_conv_forward_aggr / sage_conv_forward_indexed_aggr: the arguments of sage_conv_forward_stats / sage_conv_forward_indexed_stats, then
 * aggr and arg.  bn_pa, bn_pb and bn_info may all be NULL (no statistics wanted: the plain forward call).  The gather is k_gather_reduce,
 * then the projection sage_conv_forward would choose for the shape -- except the form that overlaps the gather with half of the projection,
 * whose gather role is the mean's; the statistics hand-off is a property of the projection and stays.  aggr = POPE_AGGR_MEAN is FORWARDED:
 * the call then runs what the _stats (or plain) entry point runs, the overlapped form included, and ignores arg.
 * sage_conv_backward_aggr: the arguments of sage_conv_backward, then aggr and arg (const; NULL under add, or without a grad_x).  The
 * weight, bias and grad_x[:n_dst] / grad_agg products are sage_conv_backward's in the form deterministic mode takes (the scatter a step of
 * its own), with k_scatter_ordered at that step.  scratch: sage_conv_backward_aggr_scratch_size, which always holds the index.  A caller
 * behind sage_conv_forward_indexed_aggr passes the destination rows (x_dst) with n_src = n_dst and grad_x = NULL, as for the mean.
 * POPE_AGGR_MEAN is forwarded to sage_conv_backward (the size of this query is never less than sage_conv_scratch_bytes).
 */
#define POPE_AGGR_MEAN 0
#define POPE_AGGR_ADD  1
#define POPE_AGGR_MAX  2
int sage_aggregate_forward(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz,
                           const float *x, int64_t x_rows, int32_t c, int32_t aggr, float *agg, int32_t *arg, float *x_dst,
                           const int32_t *dims, void *stream);
size_t sage_aggregate_backward_scratch_size(int64_t n_src, int64_t n_dst, int64_t nnz);
int sage_aggregate_backward(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t *arg,
                            const float *grad_agg, int32_t c, int32_t aggr, float *grad_x, void *scratch, size_t scratch_bytes,
                            const int32_t *dims, void *stream);
int sage_conv_forward_aggr(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                           int32_t c_in, const float *w_l, const float *b_l, const float *w_r, int32_t c_out, float *agg, float *out,
                           void *scratch, size_t scratch_bytes, const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap,
                           int32_t *bn_info, int32_t aggr, int32_t *arg, void *stream);
int sage_conv_forward_indexed_aggr(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst, int64_t nnz,
                                   const float *feats, int64_t n_rows, int32_t c_in, const float *w_l, const float *b_l, const float *w_r,
                                   int32_t c_out, float *agg, float *x_dst, float *out, void *scratch, size_t scratch_bytes,
                                   const int32_t *dims, double *bn_pa, double *bn_pb, int32_t bn_parts_cap, int32_t *bn_info, int32_t aggr,
                                   int32_t *arg, void *stream);
size_t sage_conv_backward_aggr_scratch_size(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out);
int sage_conv_backward_aggr(const int32_t *rowptr, const int32_t *col, int64_t n_src, int64_t n_dst, int64_t nnz, const float *x_src,
                            const float *agg, int32_t c_in, const float *w_l, const float *w_r, int32_t c_out, const float *grad_out,
                            float *grad_x, float *grad_w_l, float *grad_b_l, float *grad_w_r, void *scratch, size_t scratch_bytes,
                            const int32_t *dims, int32_t aggr, const int32_t *arg, void *stream);
/* The indexed pair without a matrix of the destination rows.  sage_conv_forward_indexed accepts x_dst = NULL (scratch:
 * sage_conv_forward_indexed_scratch_bytes), and sage_conv_backward_indexed computes the same gradients as sage_conv_backward
 * reading x_dst[i] = feats[n_id[i]] through n_id (the weight-gradient kernel's loader follows the index; kernel paths that
 * cannot build the rows in the scratch tail).  The input features get no gradient.  main.py:118-123, 206. */
size_t sage_conv_forward_indexed_scratch_bytes(int64_t n_dst, int32_t c_in, int32_t c_out);
size_t sage_conv_backward_indexed_scratch_bytes(int64_t n_src, int64_t n_dst, int64_t nnz, int32_t c_in, int32_t c_out);
int sage_conv_backward_indexed(const int32_t *rowptr, const int32_t *col, const int64_t *n_id, int64_t n_src, int64_t n_dst,
                               int64_t nnz, const float *feats, int64_t n_rows, const float *agg, int32_t c_in, const float *w_l,
                               const float *w_r, int32_t c_out, const float *grad_out, float *grad_w_l, float *grad_b_l,
                               float *grad_w_r, void *scratch, size_t scratch_bytes, const int32_t *dims, void *stream);

/*
 * Exact full-graph layer for inference (main.py:204-211, one pass of the layer loop over ALL N nodes and ALL their neighbours: what the
 * trained model predicts for the graph itself, no sampling):
 *     out[v] = act( mean_{p in row v} x[col[p]] W_l^T + b_l + x[v] W_r^T )
 *   rowptr int32 [N + 1], col int32 [nnz]: the CSR by destination over all N nodes (pope_csr_build of the flipped edge list, adj_t in the
 *   reference).  Repeated edges count as often as they occur; an empty row aggregates to 0.  x f32 [N, c_in], w_l / w_r f32 [c_out, c_in],
 *   b_l f32 [c_out] or NULL, out f32 [N, c_out].
 *   bn_gamma / bn_beta / bn_mean / bn_var f32 [c_out]: all four given, act = eval-mode BatchNorm (running statistics) followed by ReLU;
 *   all four NULL, act is the identity.  Some of them: POPE_ERR_INVALID.
 * The mean is linear, so the layer projects first -- PR [N, 2 c_out] = x [W_l ; W_r]^T + [0 ; b_l], ONE product that reads x once, by
 * the projection kernels of sage_conv_forward -- and gathers the projected rows P[j] = PR[j, :c_out], R[v] = PR[v, c_out:]: about
 * c_in + 14 c_out floats per node at nnz = 10 N instead of 13 c_in + 3 c_out for aggregate-first.  This order is used for EVERY shape;
 * for c_out > c_in it moves more bytes than aggregate-first would (no shape of the command line reaches that case).
 * Summation order (the tests pin it; CHUNK = 512):
 *   a row of deg <= CHUNK slots:  s = +0, then s = s + P[col[p]] for p ascending;
 *   a longer row (a hub):         part_k = +0, then part_k = part_k + P[col[p]] over its k-th run of CHUNK slots, p ascending (the last run
 *                                 may be shorter); s = +0, then s = s + part_k for k ascending;
 *   then, each operation rounded to float32 on its own:  t = s * inv + R[v] as a product and a sum, inv = 1 / (float)deg (0 for an empty
 *   row); with BatchNorm  t = ((t - mean) * rstd) * gamma + beta, rstd = (float)(1 / sqrt((double)var + eps)), and t = 0 where t < 0.
 * No float atomics: out is a pure function of the inputs, bit for bit.  Hub rows go through an integer counter onto a list in scratch
 * and are summed by two further launches sized by capacity (the counts stay on the device: no read-back, no block waits for another).
 * N and nnz must be < INT32_MAX, c_out <= INT32_MAX / 2; a shape that does not fit is POPE_ERR_INVALID (size query: 0), never wrapped.
 * scratch: sage_full_layer_scratch_size(N, nnz, c_in, c_out) bytes (the size query of this call), 4-byte aligned; with less: POPE_ERR_WORKSPACE, the needed size in
 * pope_last_error, nothing launched.  No byte beyond that size is touched.  x / out / scratch that are not 16-byte aligned, or
 * c_out % 4 != 0, take scalar accesses and give the same values.  Asynchronous.
 */
size_t sage_full_layer_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out);
int sage_full_layer_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                            const float *w_l, const float *b_l, const float *w_r, int32_t c_out, const float *bn_gamma,
                            const float *bn_beta, const float *bn_mean, const float *bn_var, float bn_eps, float *out, void *scratch,
                            size_t scratch_bytes, void *stream);
/* The launches of sage_full_layer_forward (main.py:204-211) for this shape on a device of cu_count compute units, in launch order, joined
 * by '+', as a kernel trace shows them: "k_full_prepare+k_gemm_tile16<R, B>" or "...+k_gemm<TM, TN, WM, WN, LA, LB>", then
 * "+k_full_aggregate<V, BN>" and, where a row can be longer than CHUNK (nnz > CHUNK), "+k_full_hub_partial<V>+k_full_hub_finish<V, BN>".
 * Bit i of `misaligned`: operand i of {x, out, scratch} is NOT 16-byte aligned (higher bits: POPE_ERR_INVALID; the weights are copied by
 * scalar accesses, their alignment changes nothing).  Host logic: needs no device. */
int sage_full_layer_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int32_t has_bn, int32_t cu_count,
                                uint32_t misaligned, char *name, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * GCNConv on the whole graph (csrc/gcn.h): project, then the normalised propagate, forward and backward.
 *
 *     out = A^ (x W) + b,     A^ = D^-1/2 (A + f I) D^-1/2
 * PyG 1.7.0 GCNConv(improved, cached, add_self_loops, normalize, bias), its adj_t path [3p: PyG is not installed, parity unpinned].
 *   rowptr int32 [N + 1], col int32 [nnz]: the CSR by destination (row i lists the sources j that i sums over; pope_csr_build_canonical of
 *   the flipped edge list).  Repeated edges count as often as they appear.  x f32 [N, c_in], weight f32 [c_in, c_out] (PyG 1.7.0's
 *   layout), bias f32 [c_out] or NULL, out f32 [N, c_out].
 *   self_weight f (a float in [0, 1e6]): f > 0 is add_self_loops (1, or 2 with improved): slots with col[p] == row are skipped and every
 *   row gets ONE self term of weight f (fill_diag: the diagonal is replaced, not added to).  f = 0: no self term, self-loop slots are
 *   ordinary edges.
 *   dinv f32 [N] from pope_gcn_degree_norm, or NULL (normalize=False: a plain sum, every weight 1).
 * pope_gcn_degree_norm:  deg_i = the slots of row i that are counted (all of them; with f > 0 all but those with col[p] == i) + f, and
 *   dinv_i = deg_i > 0 ? (float)(1.0 / sqrt((double)deg_i)) : 0.  Call it with the f the propagate is given.
 *
 * The summation contract (the tests pin it bit for bit; CHUNK = 512 as for sage_full_layer_forward).  For row i and column c, all
 * float32, every product and every sum rounded on its own (no fused multiply-add):
 *   1. term(p) = dinv[j] * h[j, c] with j = col[p]; without dinv there is no multiply (the kernels multiply by 1.0f: the same bits).
 *   2. a slot whose j is outside [0, N) contributes nothing; with f > 0 neither does a slot with j == i.
 *   3. a row of at most CHUNK slots:  s = +0, then s = s + term(p) for p ascending.
 *   4. a longer row is cut into runs of CHUNK slot POSITIONS (skipped slots still occupy theirs): part_k = +0, then part_k = part_k +
 *      term(p) over run k, p ascending; s = +0, then s = s + part_k for k ascending.
 *   5. the finish, in this order:  with f > 0  s = s + (dinv[i] * f) * h[i, c]  (f * h[i, c] without dinv);
 *                                  with dinv   s = dinv[i] * s;
 *                                  with bias   s = s + b[c].
 * The backward pass is the same kernel over the CSR BY SOURCE (the transpose) with the SAME dinv vector, A^T_ji = dinv_j dinv_i:
 *   t = A^T grad_out,  grad_weight = x^T t,  grad_x = t W^T (only when asked for),  grad_bias = the column sums of grad_out.
 * No float atomics anywhere: every result is a pure function of the inputs, bit for bit, in either mode of sage_set_deterministic.
 * Hub rows (more than CHUNK slots) go through an integer counter onto a list in scratch and are summed by two further launches sized by
 * capacity (no read-back, no block waits for another).  Every index read from the CSR is range-checked: an invalid CSR gives wrong
 * numbers, never a fault.
 *
 * pope_gcn_propagate          out [N, C] = A^ h (+ bias) for h f32 [N, C]; out must not alias h.
 * pope_gcn_conv_forward       P = x W in scratch (whole tiles of gemm_tile16.h on a transposed copy of W where the shape and the alignment
 *                             qualify, else the plain tile kernel on W where it lies), then the propagate with the bias.
 * pope_gcn_conv_backward      rowptr_t / col_t: the CSR by source.  grad_out f32 [N, c_out]; grad_x f32 [N, c_in] or NULL; grad_weight f32
 *                             [c_in, c_out]; grad_bias f32 [c_out] or NULL.  Everything is overwritten, nothing accumulated.
 * N in (0, INT32_MAX), nnz in [0, INT32_MAX), widths > 0: anything else is POPE_ERR_INVALID (size queries: 0).  scratch: the call's own
 * _scratch_size query, 4-byte aligned; with less: POPE_ERR_WORKSPACE, the needed size in pope_last_error, nothing launched.  No byte
 * beyond that size is touched; the layout is a function of the sizes alone.  Operands that are not 16-byte aligned, or widths that are
 * not multiples of 4, take scalar accesses and give the same values (the propagate: the same bits).  Asynchronous.
 * ------------------------------------------------------------------------------------------------ */
int pope_gcn_degree_norm(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, float self_weight, float *dinv, void *stream);
size_t pope_gcn_propagate_scratch_size(int64_t N, int64_t nnz, int32_t C);
int pope_gcn_propagate(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                       const float *h, int32_t C, const float *bias, float *out, void *scratch, size_t scratch_bytes, void *stream);
size_t pope_gcn_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out);
int pope_gcn_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                          const float *x, int32_t c_in, const float *weight, const float *bias, int32_t c_out, float *out, void *scratch,
                          size_t scratch_bytes, void *stream);
size_t pope_gcn_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out);
int pope_gcn_conv_backward(const int32_t *rowptr_t, const int32_t *col_t, int64_t N, int64_t nnz, const float *dinv, float self_weight,
                           const float *x, int32_t c_in, const float *weight, int32_t c_out, const float *grad_out, float *grad_x,
                           float *grad_weight, float *grad_bias, void *scratch, size_t scratch_bytes, void *stream);
/* The launches of pope_gcn_conv_forward (backward = 0) or pope_gcn_conv_backward (backward != 0; with a bias gradient) for this shape on a
 * device of cu_count compute units, in launch order, joined by '+', as a kernel trace shows them.  Forward: "k_gcn_transpose+
 * k_gemm_tile16<R, B>" or "k_gemm<TM, TN, WM, WN, LA, LB>", then "k_gcn_propagate<V, N>" (V: 16-byte accesses; N: the narrow form of
 * c_out <= 64, one column per lane and 32 rows in flight), which where a row can be longer than CHUNK (nnz > CHUNK) stands between
 * "k_gcn_clear" and "k_gcn_hub_partial<V, N>+k_gcn_hub_finish<V, N>".  Backward: the propagate, the weight
 * gradient's "k_gemm<...>[splits=S]+k_slab_reduce", with need_grad_x a second "k_gemm<...>", then "k_colsum_partial<V>+k_colsum_final".
 * Bit i of `misaligned`: operand i of {x, weight, out or grad_out, grad_x, scratch} is NOT 16-byte aligned (higher bits:
 * POPE_ERR_INVALID).  Host logic: needs no device. */
int pope_gcn_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t c_out, int32_t backward, int32_t need_grad_x, int32_t cu_count,
                         uint32_t misaligned, char *name, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * GATConv on the whole graph (csrc/gat.h): project, score, edge softmax, attention propagate, forward and backward.
 *
 * PyG 1.7.0 GATConv(in, out, heads, concat, negative_slope, dropout, add_self_loops, bias) on a single x [3p: PyG is not installed, parity
 * unpinned]; attention dropout is not part of it.  With H heads of C channels, rowptr / col the CSR by destination as for pope_gcn_*:
 *   h [N, H, C] = x weight^T, weight f32 [H C, c_in] (lin_l.weight; lin_r is the same module), att_l and att_r f32 [H, C];
 *   a_src[j, k] = sum_c h[j, k, c] att_l[k, c],  a_dst[i, k] likewise with att_r;
 *   for the slot p = (j -> i):  e = a_src[j, k] + a_dst[i, k],  e' = e > 0 ? e : negative_slope * e;
 *   alpha[p, k] = exp(e' - m[i, k]) / s[i, k] over the TERMS of row i, m their largest e', s the sum of their exp(e' - m);
 *   agg[i, k, :] = sum over the terms of alpha * h[j, k, :];
 *   concat: out [N, H C] = agg + bias [H C];  else out [N, C] = (sum_k agg[:, k, :]) / H + bias [C].
 * The terms of row i.  add_self_loops: the slots whose id is in [0, N) and is not i, plus ONE self term i -> i (the diagonal is replaced,
 * as in pope_gcn_*); without: every slot with an id in [0, N), self-loop slots being ordinary edges.  Repeated edges are separate terms.
 * A slot that is no term has alpha 0.  A row without terms has agg = 0 and nothing is divided.  s >= 1 for a row with terms, so PyG's
 * "+ 1e-16" changes no float32 bit and is left out.
 *
 * The summation contract.  All float32, every product, sum and quotient rounded on its own (no fused multiply-add):
 *   scores      a = +0, then a = a + h[i, k, c] * att[k, c] for c ascending.
 *   attention   m is exact.  exp is expf.  For s, lane l of the row's wave adds exp(e' - m) of the terms among the slots beg + l, beg + l
 *               + 64, ... ascending from +0; the 64 lane sums are folded by the butterfly s_l = s_l + s_(l xor d), d = 32, 16, .. 1; then
 *               s = s + exp(e'_self - m) with self loops.  (Rows longer than CHUNK take the same order: the wave walks the whole row.)
 *               alpha = exp(e' - m) / s.  alpha f32 [nnz, H] in the slot order of the CSR by destination, alpha_self f32 [N, H] (0
 *               without self loops).  The tests hold alpha to the rule of tests/gat_cases.py, not to bits.
 *   propagate   GIVEN alpha, pinned bit for bit (CHUNK = 512): term(p) = alpha[p, k] * h[j, k, c]; a slot that is no term contributes
 *               nothing; a row of at most CHUNK slots: s = +0, s = s + term(p) for p ascending; a longer row by runs of CHUNK slot
 *               POSITIONS, part_r = +0 + its terms ascending, then s = +0 + part_r for r ascending; then with a self term
 *               s = s + alpha_self[i, k] * h[i, k, c]; then concat: s = s + bias[k C + c]; else, in a launch of its own,
 *               o = +0, o = o + s[i, k, c] for k ascending, o = o / (float)H, o = o + bias[c].
 *   backward    with g the gradient of agg (grad_out, or grad_out / (float)H for every head):
 *               dalpha_p = +0 + g[i, k, c] * h[j, k, c] for c ascending;  t[i, k] = sum alpha_p * dalpha_p in the order of s above (the
 *               self term last);  de_p = (alpha_p * (dalpha_p - t)) * (e > 0 ? 1 : negative_slope), e the float32 sum of the forward pass;
 *               grad_a_dst[i, k] = sum de_p in the order of s, + de_self;  grad_a_src[j, k] = the same over the CSR by source, de read
 *               through the slot map, + de_self[j, k];  GH[j, k, c] = the propagate above over the CSR by source (alpha through the slot
 *               map, rows g, the self term alpha_self[j, k] * g[j, k, c]), then + grad_a_src[j, k] * att_l[k, c], then + grad_a_dst[j, k]
 *               * att_r[k, c];  grad_att_l[k, c] = sum_j grad_a_src[j, k] * h[j, k, c] by COLSUM row slices (rows ascending within a
 *               slice, slices by k_colsum_final), grad_att_r likewise;  grad_weight [H C, c_in] = GH^T x (split depth + k_slab_reduce);
 *               grad_x = GH weight, only when asked for;  grad_bias = the column sums of grad_out.
 * No float atomics anywhere: every result is a pure function of the inputs, bit for bit, in either mode of sage_set_deterministic.  Hub
 * rows go through gcn.h's integer-counter list and two capacity-sized launches.  Every index read from a CSR or the slot map is
 * range-checked: an invalid CSR gives wrong numbers, never a fault.
 *
 * pope_gat_slot_map         slot_map int32 [nnz]: for slot q = (j -> i) of the CSR by source (rowptr_t / col_t) the slot of the CSR by
 *                           destination that holds the same edge: the first j in row i (binary search; both CSRs have ascending rows, as
 *                           pope_csr_build_canonical builds them) plus q's rank among the equal ids of its row; -1 where they do not match.
 * pope_gat_attention        the scores and the attention alone: writes a_src, a_dst [N, H], alpha, alpha_self.  It needs no scratch.
 * pope_gat_propagate        the propagate alone behind a given alpha: alpha_self NULL = no self term and self-loop slots are ordinary;
 *                           out [N, H C] (concat) or [N, C]; out must not alias h.
 * pope_gat_conv_forward     projection (whole tiles of gemm_tile16.h where shape and alignment qualify, else the plain tile kernel), scores,
 *                           attention, propagate.  h [N, H C], a_src, a_dst, alpha, alpha_self are the CALLER's: the backward pass takes
 *                           them back.
 * pope_gat_conv_backward    grad_x f32 [N, c_in] or NULL; grad_weight [H C, c_in]; grad_att_l, grad_att_r [H, C]; grad_bias [H C] / [C] or
 *                           NULL.  Everything is overwritten, nothing accumulated.
 * N in (0, INT32_MAX), nnz in [0, INT32_MAX), c_in, H, C > 0, H C <= INT32_MAX / 2, negative_slope in [0, 1]: anything else is
 * POPE_ERR_INVALID (size queries: 0).  scratch: the call's own _scratch_size query; with less: POPE_ERR_WORKSPACE, the needed size in
 * pope_last_error, nothing launched.  No byte beyond that size is touched.  Operands that are not 16-byte aligned, or widths that are not
 * multiples of 4, take scalar accesses and give the same values (the propagate: the same bits).  Asynchronous.
 * ------------------------------------------------------------------------------------------------ */
int pope_gat_slot_map(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, int64_t N, int64_t nnz,
                      int32_t *slot_map, void *stream);
int pope_gat_attention(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *h, int32_t H, int32_t C,
                       const float *att_l, const float *att_r, float negative_slope, int32_t add_self_loops, float *a_src, float *a_dst,
                       float *alpha, float *alpha_self, void *stream);
size_t pope_gat_propagate_scratch_size(int64_t N, int64_t nnz, int32_t H, int32_t C, int32_t concat);
int pope_gat_propagate(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *alpha, const float *alpha_self,
                       const float *h, int32_t H, int32_t C, int32_t concat, const float *bias, float *out, void *scratch,
                       size_t scratch_bytes, void *stream);
size_t pope_gat_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat);
int pope_gat_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                          const float *weight, const float *att_l, const float *att_r, const float *bias, int32_t H, int32_t C,
                          int32_t concat, float negative_slope, int32_t add_self_loops, float *h, float *a_src, float *a_dst, float *alpha,
                          float *alpha_self, float *out, void *scratch, size_t scratch_bytes, void *stream);
size_t pope_gat_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat);
int pope_gat_conv_backward(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                           int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight, const float *att_l,
                           const float *att_r, int32_t H, int32_t C, int32_t concat, float negative_slope, int32_t add_self_loops,
                           const float *h, const float *a_src, const float *a_dst, const float *alpha, const float *alpha_self,
                           const float *grad_out, float *grad_x, float *grad_weight, float *grad_att_l, float *grad_att_r,
                           float *grad_bias, void *scratch, size_t scratch_bytes, void *stream);
/* The launches of pope_gat_conv_forward (backward = 0) or pope_gat_conv_backward (backward != 0; with a bias gradient) for this shape on a
 * device of cu_count compute units, in launch order, joined by '+'.  Forward: "k_gemm_tile16<R, B>" or "k_gemm<...>", "k_gat_scores+
 * k_gat_attention", "k_gat_propagate<V, N>" (between "k_gcn_clear" and "k_gat_hub_partial<V, N>+k_gat_hub_finish<V, N>" where nnz >
 * CHUNK), and without concat "k_gat_head_mean".  Backward: without concat "k_gat_spread_grad", then "k_gat_edge_grad+k_gat_src_grad", the
 * propagate, "k_gat_att_partial+k_colsum_final+k_colsum_final", the weight gradient's "k_gemm<...>[splits=S]+k_slab_reduce", with
 * need_grad_x a second "k_gemm<...>", then "k_colsum_partial<V>+k_colsum_final".  Bit i of `misaligned`: operand i of {x, weight, h, out
 * or grad_out, grad_x, scratch} is NOT 16-byte aligned (higher bits: POPE_ERR_INVALID).  Host logic: needs no device. */
int pope_gat_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat, int32_t backward, int32_t need_grad_x,
                         int32_t cu_count, uint32_t misaligned, char *name, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * GATv2Conv on the whole graph (csrc/gatv2.h): two projections, per-edge dynamic attention, edge softmax, gat.h's propagate, forward and
 * backward.
 *
 * PyG GATv2Conv(in, out, heads, concat, negative_slope, dropout, add_self_loops, bias, share_weights) on a single x [3p: PyG is not
 * installed, parity unpinned]; attention dropout, bipartite inputs and edge features are not part of it.  With H heads of C channels and
 * rowptr / col the CSR by destination as for pope_gat_*:
 *   hl [N, H, C] = x weight_l^T + bias_l,  hr = x weight_r^T + bias_r  (weights f32 [H C, c_in], linear biases f32 [H C] or NULL;
 *   weight_r NULL = shared weights: hr IS hl), att f32 [H, C];
 *   for the slot p = (j -> i):  z[k, c] = hl[j, k, c] + hr[i, k, c],  e[p, k] = sum_c att[k, c] * (z > 0 ? z : negative_slope * z);
 *   alpha, agg and out from e exactly as pope_gat_* form them from e', the rows summed being hl[j]; the terms of a row are pope_gat_*'s.
 * The derivative of the LeakyReLU at 0 is negative_slope.
 *
 * The summation contract.  All float32, every product, sum and quotient rounded on its own (no fused multiply-add):
 *   e           t[c] = att[c] * leaky(hl[j, c] + hr[i, c]) over the H C columns, cut into slabs of 256; in a slab, lane l (0 .. 63) holds the
 *               columns c0 + 4 l + q, q = 0 .. 3.  C % 4 == 0: u[l] = ((t0 + t1) + t2) + t3, then for d = 1, 2, 4, 8, 16, 32, all lanes at
 *               once, u[l] = u[l] + u[l + d] where l + d < 64 and column c0 + 4 (l + d) exists and lies in the head of lane l; the head's
 *               part P of the slab is u of its first lane in the slab.  Otherwise four planes, plane q holding t[c0 + 4 l + q] in lane l
 *               (its head: that column's), each folded by the same rule; P = ((P0 + P1) + P2) + P3 with Pq the folded value of the head's
 *               first lane in plane q and +0 for a plane without a column of the head.  e = P of the head's first slab, then e = e + P
 *               over its further slabs ascending.  The same bits for every row, hub or not, and for 16-byte and 4-byte loads; the tests
 *               hold e to a NumPy restatement of this paragraph bit for bit.  A slot that is no term has e = 0; e_self = 0 without self
 *               loops.
 *   attention   pope_gat_*'s over the given e (m exact, expf, lane sums ascending, the butterfly, then the self term).
 *   propagate   pope_gat_propagate over hl, unchanged.
 *   backward    g as for pope_gat_*.  dalpha_p[k] = sum_c g[i, k, c] * hl[j, k, c] in the order of e (the term is the product);
 *               t[i, k] = sum alpha_p dalpha_p and de_p = alpha_p * (dalpha_p - t) in the order of s, the self term last;
 *               by destination, acc = +0 and per term in slot order (rows longer than CHUNK: runs of CHUNK slot positions from +0, added
 *               in run order), the self term last:  grad_hr[i, k, c] += (de_p * att[k, c]) * (z > 0 ? 1 : negative_slope),
 *               att_rows[i, k, c] += de_p * leaky(z);  grad_att = the column sums of att_rows by COLSUM row slices;
 *               by source through the slot map, the same walk:  grad_hl[j, k, c] += (de_p * att[k, c]) * leaky'(z), then
 *               += alpha_p * g[i, k, c];  shared weights: grad_hl = grad_hl + grad_hr element by element, then one of each of the following;
 *               grad_weight_l = grad_hl^T x,  grad_weight_r = grad_hr^T x (split depth + k_slab_reduce);  grad_bias_l, grad_bias_r = the
 *               column sums of grad_hl, grad_hr;  grad_x = grad_hl weight_l + grad_hr weight_r in ONE launch (the second product into the
 *               accumulators of the first);  grad_bias = the column sums of grad_out.
 * No float atomics anywhere; hub rows as for pope_gat_*.  Every index read from a CSR or the slot map is range-checked, every loop is
 * bounded by rowptr clamped to nnz: an invalid CSR gives wrong numbers, never a fault.
 *
 * pope_gatv2_scores         e [nnz, H] and e_self [N, H] alone, from given hl, hr [N, H C] (which may be the same) and att.  No scratch.
 * pope_gatv2_attention      the same, then alpha [nnz, H] and alpha_self [N, H] (alpha may be e, alpha_self may be e_self).
 * pope_gatv2_conv_forward   the projections (pope_gat_conv_forward's kernel choice, the linear bias in the epilogue), scores, softmax,
 *                           propagate.  hl, hr [N, H C] (hr unused with shared weights), alpha, alpha_self are the CALLER's: the backward
 *                           pass takes them back.
 * pope_gatv2_conv_backward  grad_x f32 [N, c_in] or NULL; grad_weight_l, grad_weight_r [H C, c_in] (grad_weight_r unused with shared
 *                           weights); grad_bias_l, grad_bias_r [H C] or NULL; grad_att [H, C]; grad_bias [H C] / [C] or NULL.  Everything
 *                           is overwritten, nothing accumulated.
 * N in (0, INT32_MAX), nnz in [0, INT32_MAX), c_in, H, C > 0, H C <= INT32_MAX / 4, negative_slope in [0, 1]: anything else is
 * POPE_ERR_INVALID (size queries: 0).  scratch: the call's own _scratch_size query; with less: POPE_ERR_WORKSPACE, the needed size in
 * pope_last_error, nothing launched.  No byte beyond that size is touched.  Asynchronous.
 * ------------------------------------------------------------------------------------------------ */
int pope_gatv2_scores(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *hl, const float *hr, int32_t H, int32_t C,
                      const float *att, float negative_slope, int32_t add_self_loops, float *e, float *e_self, void *stream);
int pope_gatv2_attention(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *hl, const float *hr, int32_t H,
                         int32_t C, const float *att, float negative_slope, int32_t add_self_loops, float *e, float *e_self, float *alpha,
                         float *alpha_self, void *stream);
size_t pope_gatv2_conv_forward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat);
int pope_gatv2_conv_forward(const int32_t *rowptr, const int32_t *col, int64_t N, int64_t nnz, const float *x, int32_t c_in,
                            const float *weight_l, const float *bias_l, const float *weight_r, const float *bias_r, const float *att,
                            const float *bias, int32_t H, int32_t C, int32_t concat, float negative_slope, int32_t add_self_loops, float *hl,
                            float *hr, float *alpha, float *alpha_self, float *out, void *scratch, size_t scratch_bytes, void *stream);
size_t pope_gatv2_conv_backward_scratch_size(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat);
int pope_gatv2_conv_backward(const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t, const int32_t *col_t, const int32_t *slot_map,
                             int64_t N, int64_t nnz, const float *x, int32_t c_in, const float *weight_l, const float *weight_r,
                             const float *att, int32_t H, int32_t C, int32_t concat, float negative_slope, int32_t add_self_loops,
                             const float *hl, const float *hr, const float *alpha, const float *alpha_self, const float *grad_out,
                             float *grad_x, float *grad_weight_l, float *grad_bias_l, float *grad_weight_r, float *grad_bias_r,
                             float *grad_att, float *grad_bias, void *scratch, size_t scratch_bytes, void *stream);
/* The launches of pope_gatv2_conv_forward (backward = 0) or pope_gatv2_conv_backward (backward != 0; with every bias gradient) in launch
 * order, joined by '+', as pope_gat_kernel_name gives pope_gat_*'s.  Forward: one projection per weight, "k_gatv2_scores<V, O, false, S>+
 * k_gatv2_softmax" (V: 16-byte loads, O: C % 4 == 0, S: H C <= 256), then pope_gat_*'s propagate names.  Backward: without concat "k_gat_spread_grad",
 * "k_gatv2_scores<V, O, true, S>+k_gatv2_edge_grad", "k_gatv2_rowsum<V, false>" and "k_gatv2_rowsum<V, true>" (each between "k_gcn_clear" and
 * its "k_gatv2_hub_partial<..>+k_gatv2_hub_finish<..>" where nnz > CHUNK), grad_att's "k_colsum_partial<V>+k_colsum_final", with shared
 * weights "k_gatv2_add", per weight "k_gemm<...>[splits=S]+k_slab_reduce+k_colsum_partial<V>+k_colsum_final", with need_grad_x one
 * "k_gemm<...>", then "k_colsum_partial<V>+k_colsum_final".  Bit i of `misaligned`: operand i of {x, weight_l, weight_r, hl, hr, att, out
 * or grad_out, grad_x, scratch} is NOT 16-byte aligned (higher bits: POPE_ERR_INVALID).  Host logic: needs no device. */
int pope_gatv2_kernel_name(int64_t N, int64_t nnz, int32_t c_in, int32_t H, int32_t C, int32_t concat, int32_t share_weights,
                           int32_t backward, int32_t need_grad_x, int32_t cu_count, uint32_t misaligned, char *name, size_t cap);

/* ------------------------------------------------------------------------------------------------
 * Fan-out neighbour sampling on the device (one hop of PyG NeighborSampler / torch_sparse.sample_adj, main.py:100-116).
 *   rowptr / col    int32 CSR of the whole graph by TARGET node (row v lists the nodes whose features v aggregates;
 *                   adj_t in the reference).  For the symmetric Flickr / PubMed graphs this is pope_csr_build's CSR.
 *   targets         int64 [n_targets] distinct node ids on the device.
 *   fanout          > 0: rows with more neighbours keep `fanout` distinct ones, chosen by a keyed pseudo-random
 *                   permutation that is a pure function of (seed, hop, node); < 0: keep all neighbours.
 *   out_rowptr      int32 [n_targets + 1], out_col int32 [nnz_capacity]: the sampled block, LOCAL ids.
 *   out_n_id        int64 [n_targets + nnz_capacity]: targets (same order) followed by the newly met nodes in order
 *                   of first appearance; out_col indexes into it.
 *   nnz_host / n_src_host   (out, host) edges kept and length of out_n_id.
 * nnz_capacity >= n_targets * fanout (fanout > 0) or the sum of the targets' degrees (fanout < 0).
 * Synchronises `stream` once (the two counts come back to the host).
 * ------------------------------------------------------------------------------------------------ */
size_t sage_sample_scratch_bytes(int64_t N, int64_t n_targets, int64_t nnz_capacity);
int sage_sample_hop(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *targets, int64_t n_targets,
                    int32_t fanout, uint64_t seed, int32_t hop, int32_t *out_rowptr, int32_t *out_col, int64_t nnz_capacity,
                    int64_t *out_n_id, int64_t *nnz_host, int64_t *n_src_host, void *scratch, size_t scratch_bytes,
                    void *stream);

/*
 * Every hop of a mini-batch in one call: hop h samples `fanouts_host[h]` neighbours around hop h-1's node list (hop 0:
 * `seeds`), exactly as n_hops successive sage_sample_hop calls with hop = h would.  out_rowptr / out_col / out_n_id:
 * HOST arrays of n_hops device pointers sized by capacity -- with t_cap[0] = n_seeds and
 * t_cap[h] = t_cap[h-1] * (1 + fanouts[h-1]):  out_rowptr[h] t_cap[h] + 1 ints, out_col[h] t_cap[h] * fanouts[h] ints,
 * out_n_id[h] t_cap[h] * (1 + fanouts[h]) int64.  nnz_host / n_src_host: (out, host) [n_hops].
 * scratch: sage_sample_scratch_bytes(N, t_cap[last], t_cap[last] * fanouts[last]) -- the capacities, whatever the batch turns out to
 * hold; less is POPE_ERR_WORKSPACE before the first hop is enqueued.  Synchronises `stream` once per hop.
 */
int sage_sample_batch(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *seeds, int64_t n_seeds,
                      const int32_t *fanouts_host, int32_t n_hops, uint64_t seed, int32_t *const *out_rowptr,
                      int32_t *const *out_col, int64_t *const *out_n_id, int64_t *nnz_host, int64_t *n_src_host, void *scratch,
                      size_t scratch_bytes, void *stream);

/*
 * sage_sample_batch WITHOUT any host synchronisation (the device-extent form): every hop runs over its capacity and reads
 * the true target count of the hop before it on the device.  dims (out, device): int32 [n_hops][4], dims[h] =
 * {n_dst, n_src, nnz, 0} of hop h -- what the SAGE entry points take as `dims`; out_rowptr[h] rows past n_dst are empty,
 * out_col[h] / out_n_id[h] entries past nnz / n_src are unspecified.  seed_dev (device uint64, or NULL) is ADDED to `seed`
 * on the device: a captured launch follows that word (sage_advance_counters).  Buffers and scratch as sage_sample_batch.
 */
int sage_sample_batch_device(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *seeds, int64_t n_seeds,
                             const int32_t *fanouts_host, int32_t n_hops, uint64_t seed, const uint64_t *seed_dev,
                             int32_t *const *out_rowptr, int32_t *const *out_col, int64_t *const *out_n_id, int32_t *dims,
                             void *scratch, size_t scratch_bytes, void *stream);
/* The next batch of an epoch without a loader (main.py:100-123): seeds = order[*first_dev .. + n_seeds) with `order` the epoch's
 * (shuffled) node list and `first_dev` a device word the caller advances by n_seeds per step; with `labels` (and y_out)
 * y_out[i] = labels[seed i] (main.py:122).  Everything else as sage_sample_batch_device. */
int sage_sample_epoch_batch_device(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *order, const int64_t *first_dev,
                                   int64_t n_seeds, const int64_t *labels, int64_t *y_out, const int32_t *fanouts_host, int32_t n_hops,
                                   uint64_t seed, const uint64_t *seed_dev, int32_t *const *out_rowptr, int32_t *const *out_col,
                                   int64_t *const *out_n_id, int32_t *dims, void *scratch, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Hidden-layer epilogue: BatchNorm1d + ReLU + dropout as one op  (main.py:207-209)
 *
 * Replaces   x = self.bns[i](x); x = x.relu_(); x = F.dropout(x, p=self.dropout, training=self.training)
 * and its autograd.  x, y and the grad_x / grad_y matrices are [M, C] float32 row-major on the device; gamma, beta, the running and
 * the saved statistics and grad_gamma / grad_beta are [C].
 *   training != 0: batch statistics (biased variance), running_mean / running_var updated in place with `momentum`
 *                  (unbiased variance), as torch.nn.BatchNorm1d; both running pointers may be NULL (track_running_stats=False).
 *                  Dropout keeps an element with probability 1 - p and scales it by 1 / (1 - p); the mask is a pure
 *                  function of (seed, element index), recomputed in backward: no mask tensor.
 *   training == 0: running statistics, no dropout.
 * Conditioning: the batch variance is E[x^2] - E[x]^2 over float64 sums of the float32 inputs, so its relative error grows as
 * (mean^2 / var) * M * 2^-52 where torch's Welford pass stays at float32 rounding; the tests pin it up to a column offset of 1000
 * times the column's spread (there 1e6 * M * 2^-52, below float32 rounding for every M the model sees).
 * save_mean / save_rstd (out) feed the backward call.  grad_gamma / grad_beta may be NULL.  Asynchronous.
 * rows_dev (device int32, or NULL): the true row count, M then being the capacity ("Device extents" above).
 * seed_dev (device uint64, or NULL): added to `seed` on the device (a replayed HIP graph draws a new mask per replay).
 * scratch: sage_bn_scratch_bytes(C) bytes.
 * ------------------------------------------------------------------------------------------------ */
size_t sage_bn_scratch_bytes(int32_t C);
int sage_bn_relu_dropout_forward(const float *x, int64_t M, int32_t C, const float *gamma, const float *beta,
                                 float *running_mean, float *running_var, int64_t *num_batches_tracked, float momentum, float eps, int32_t training,
                                 float p, uint64_t seed, float *y, float *save_mean, float *save_rstd, void *scratch,
                                 size_t scratch_bytes, const int32_t *rows_dev, const uint64_t *seed_dev, void *stream);
/* The forward pass with the first stage of the statistics taken from the kernel that wrote x (sage_conv_forward_stats: pa / pb
 * [parts, C] float64, one part per rows_per_part rows; with rows_dev only the parts in front of the true row count are read): two
 * launches instead of three.  Same arithmetic otherwise (float64 sums; the order of the additions differs from the three-launch form). */
int sage_bn_relu_dropout_forward_stats(const float *x, int64_t M, int32_t C, const float *gamma, const float *beta,
                                       float *running_mean, float *running_var, int64_t *num_batches_tracked, float momentum, float eps,
                                       int32_t training, float p, uint64_t seed, float *y, float *save_mean, float *save_rstd, void *scratch,
                                       size_t scratch_bytes, const int32_t *rows_dev, const uint64_t *seed_dev, const double *pa,
                                       const double *pb, int32_t parts, int32_t rows_per_part, void *stream);
int sage_bn_relu_dropout_backward(const float *x, const float *grad_y, int64_t M, int32_t C, const float *gamma,
                                  const float *beta, const float *save_mean, const float *save_rstd, int32_t training,
                                  float p, uint64_t seed, float *grad_x, float *grad_gamma, float *grad_beta, void *scratch,
                                  size_t scratch_bytes, const int32_t *rows_dev, const uint64_t *seed_dev, void *stream);
/* The backward pass, and out of its float64 sums the column sums of grad_x (grad_x_colsum, float32 [C]): the bias gradient of the layer
 * that produced x (main.py:206-207), which sage_conv_backward otherwise computes by reading grad_x back (pass it grad_b_l = NULL). */
int sage_bn_relu_dropout_backward_bias(const float *x, const float *grad_y, int64_t M, int32_t C, const float *gamma,
                                       const float *beta, const float *save_mean, const float *save_rstd, int32_t training,
                                       float p, uint64_t seed, float *grad_x, float *grad_gamma, float *grad_beta, void *scratch,
                                       size_t scratch_bytes, const int32_t *rows_dev, const uint64_t *seed_dev, float *grad_x_colsum,
                                       void *stream);

/* ------------------------------------------------------------------------------------------------
 * L2 normalisation of a SAGEConv output  (PyG 1.7.0 SAGEConv(normalize=True): out = F.normalize(out, p=2., dim=-1))
 *
 * Replaces   torch.nn.functional.normalize(x, p=2, dim=-1, eps=1e-12)   behind PyG's SAGEConv.forward, and its autograd.  x, y, grad_y and
 * grad_x are [M, C] float32 row-major on the device, inv_norm is float32 [M].  One launch per direction, one wave per row.
 *   forward    inv_norm[i] = 1 / max(sqrt(sum_c x[i, c]^2), eps),   y[i, :] = x[i, :] * inv_norm[i].   y may be x.
 *   backward   where the norm exceeded eps:   grad_x[i, :] = inv_norm[i] * (grad_y[i, :] - y[i, :] * (y[i, :] . grad_y[i, :]))
 *              where it was clamped:          grad_x[i, :] = grad_y[i, :] / eps    (torch's gradient through clamp_min; an all-zero row too)
 *              grad_x may be grad_y; y must be neither.  The branch is read off inv_norm, no flag is saved: the forward pass clamps by
 *              `norm < eps ? eps : norm`, so a clamped row holds exactly the float32 1 / eps, and the backward pass tests inv_norm[i] for
 *              that value.  A row whose float32 norm is eps or one rounding above it has the same reciprocal and takes the clamped form
 *              (torch: the projected one from norm == eps on); the two differ by less than the rounding of the norm itself.
 * Arithmetic: the sum of squares and the dot product are accumulated in FLOAT32, as the norm kernels of torch's CUDA / HIP backend do
 * (a row of 1e20 overflows to inf there and here, and comes out as zeros).  Column c belongs to lane (c / 4) % 64; a lane adds its columns
 * in ascending order by fused multiply-adds onto +0, the 64 partials are folded by the xor butterfly 32, 16, ... 1.  The order is fixed:
 * no float atomics, no scratch, the same bits on every call and in every mode of the library, and -- the vector and the scalar form of
 * the kernels share the order -- at every alignment.  Square root, reciprocal and division are correctly rounded; y * d, the difference
 * and the scaling of the backward pass are rounded one by one.  A NaN in a row makes y, inv_norm and grad_x of that row NaN and touches
 * no other row.
 * x / y / grad_y / grad_x that are not 16-byte aligned, or C % 4 != 0, take 4-byte accesses (sage_l2_normalize_kernel_name_at).
 * rows_dev (device int32, or NULL): the true row count, M then being the capacity ("Device extents" above; read as the `rows_dev` of
 * sage_bn_relu_dropout_forward is): rows at or beyond it are neither read nor written, in y, inv_norm and grad_x alike.
 * M == 0: POPE_OK, nothing launched.  M < 0, M >= INT32_MAX, C <= 0, eps <= 0 or a null matrix: POPE_ERR_INVALID, nothing launched.
 * Asynchronous.
 * ------------------------------------------------------------------------------------------------ */
int sage_l2_normalize_forward(const float *x, int64_t M, int32_t C, float eps, float *y, float *inv_norm, const int32_t *rows_dev,
                              void *stream);
int sage_l2_normalize_backward(const float *y, const float *inv_norm, const float *grad_y, int64_t M, int32_t C, float eps, float *grad_x,
                               const int32_t *rows_dev, void *stream);
/* The two launches for this shape as a kernel trace shows them: "k_l2_normalize<V>+k_l2_normalize_backward<V>", V = true (16-byte
 * accesses) or false.  Bit i of `misaligned`: operand i of {x, y, grad_y, grad_x} is NOT 16-byte aligned (the forward call looks at x and
 * y, the backward call at y, grad_y and grad_x; higher bits: POPE_ERR_INVALID).  Host logic: needs no device. */
int sage_l2_normalize_kernel_name_at(int64_t M, int32_t C, uint32_t misaligned, char *name, size_t cap);

/*
 * One Adam step over every parameter tensor in a single launch  (main.py:244: torch.optim.Adam(self.parameters(), lr)).
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers (float32, contiguous, numel[t] elements).
 * Update rule of torch.optim.Adam (amsgrad off): decoupled nothing, weight_decay added to the gradient, bias
 * corrections from `step` (1-based, the step being taken).  Hyper-parameters are doubles: 1 - beta, lr / (1 - beta1^t)
 * and sqrt(1 - beta2^t) are formed in double and rounded to float once, as torch does.  Asynchronous.
 * step_dev (device int64, or NULL): the step count read on the device instead of `step` (replayed HIP graphs).
 */
int sage_adam_step(int32_t n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                   float *const *exp_avg_sq, const int64_t *numel, double lr, double beta1, double beta2, double eps,
                   double weight_decay, int64_t step, const int64_t *step_dev, void *stream);
/* The same step with the LAST STAGE OF THIS STEP'S CROSS-ENTROPY as one more block of the same launch (main.py:216 + 244: the loss is a
 * number the host logs after the step, it need not hold up the backward pass): xent_rows = the row_scratch that
 * sage_cross_entropy_forward(fused = 2) filled, xent_n its row count; loss_out[0] = the mean loss, loss_out[1] = 1 / count. */
int sage_adam_step_loss(int32_t n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                        float *const *exp_avg_sq, const int64_t *numel, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int64_t step, const int64_t *step_dev, const float *xent_rows, int64_t xent_n,
                        float *loss_out, void *stream);

/*
 * Gradient-norm clipping inside the optimiser step  (main.py:285-290: both Trainer(...) calls pass gradient_clip_val=0.5, i.e.
 * torch.nn.utils.clip_grad_norm_(parameters, 0.5) with norm_type 2 between backward and the Adam step).  Two launches replace
 * torch's chain of small ones, with no host synchronisation, no atomics and nothing that depends on the order blocks run in:
 *
 *   sage_grad_sqnorm      partials[b] = float64 sum of squares of the 4096-element chunks b, b + P, b + 2 P, ... of ALL gradient
 *                         tensors of the step, P = sage_grad_norm_partials(n_tensors, numel) = clamp(sum of ceil(numel / 4096), 1, 256).
 *                         grads / numel are HOST arrays.  One launch per 128 tensors; a later launch adds onto the earlier ones.
 *   sage_adam_step_clip   sage_adam_step, or sage_adam_step_loss when xent_rows is not NULL, with every block first adding
 *                         partials[0 .. n_partials) in one fixed order: total = (float)sqrt(sum), coef = max_norm / (total + 1e-6f)
 *                         clamped to at most 1 (a NaN stays a NaN, as in torch.clamp), and each gradient element multiplied by coef in
 *                         float32 before the weight-decay term and the moments.  The gradients in memory are NOT modified (torch scales
 *                         them in place).  norm_out (device float32 [2], or NULL) receives (total, coef).
 *
 * n_partials is the count sage_grad_sqnorm wrote: the size query over the list IT ran over, which may hold more tensors than one
 * sage_adam_step_clip call (several parameter groups share one global norm).  POPE_ERR_INVALID without any HIP call: max_norm
 * negative or NaN, partials NULL, fewer partials than the size query gives for the call's own tensors, more than 256.
 * sage_grad_norm_partials needs no GPU; it returns 0 for a bad list.
 */
size_t sage_grad_norm_partials(int32_t n_tensors, const int64_t *numel);
int sage_grad_sqnorm(int32_t n_tensors, const float *const *grads, const int64_t *numel, double *partials, size_t partials_len,
                     void *stream);
int sage_adam_step_clip(int32_t n_tensors, float *const *params, const float *const *grads, float *const *exp_avg,
                        float *const *exp_avg_sq, const int64_t *numel, double lr, double beta1, double beta2, double eps,
                        double weight_decay, int64_t step, const int64_t *step_dev, double max_norm, const double *partials,
                        size_t n_partials, float *norm_out, const float *xent_rows, int64_t xent_n, float *loss_out, void *stream);

/*
 * Plumbing of a training step replayed as a HIP graph (main.py:213-222 training_step + Lightning's backward / optimizer
 * step, with no host in the loop).  sage_advance_counters: counters[i] += increments_host[i] for i < n <= 8, one launch
 * (the dropout / sampling seeds and Adam's step count live in device words).  sage_copy_segments: n device-to-device
 * copies in ONE launch (a batch of a pre-sampled pool into the step's fixed buffers); dst / src / bytes are HOST arrays.
 */
int sage_advance_counters(int64_t *counters, const int64_t *increments_host, int32_t n, void *stream);
int sage_copy_segments(int32_t n, void *const *dst, const void *const *src, const int64_t *bytes, void *stream);

/*
 * Gradient bucket of data-parallel training  (main.py:285-290: Trainer(gpus=args.n_gpus, accelerator='ddp')): the gradients of a step
 * in ONE flat float32 buffer, pre-scaled by 1 / world, so that the ranks average them with one all-reduce and sage_grad_sqnorm /
 * sage_adam_step* read them from addresses that do not change from step to step.  numel / grads / offsets are HOST arrays.
 *
 *   sage_grad_bucket_layout   offsets[t] (may be NULL) = start of tensor t in float elements = sum over s < t of numel[s] rounded up to a
 *                             multiple of 4: list order, no overlap, every start 16-byte aligned.  Returns the total length (a multiple
 *                             of 4), or -1 for a negative size or a null list.  Needs no GPU.
 *   sage_grad_bucket_pack     flat[offsets[t] + j] = grads[t][j] * scale (one float32 rounding), the padding behind each tensor +0.0f,
 *                             nothing outside [flat, flat + total) written.  One launch per sage_grad_bucket_table() tensors, a block per
 *                             sage_grad_bucket_chunk() elements of a tensor; 16-byte loads where grads[t] is 16-byte aligned, scalar loads
 *                             otherwise.  No atomics, no scratch, no host synchronisation: capturable.  POPE_ERR_INVALID with nothing
 *                             launched: flat NULL or not 16-byte aligned, flat_len below the layout's total, a bad list, grads[t] NULL
 *                             with numel[t] > 0.
 */
int64_t sage_grad_bucket_layout(int32_t n, const int64_t *numel, int64_t *offsets);
int32_t sage_grad_bucket_chunk(void);
int32_t sage_grad_bucket_table(void);
int sage_grad_bucket_pack(int32_t n, const float *const *grads, const int64_t *numel, float scale, float *flat, int64_t flat_len,
                          void *stream);

/*
 * Cross-entropy with integer labels, mean over the rows whose label is not ignore_index  (main.py:216, 224, 233:
 * F.cross_entropy(y_hat, y)).  Forward writes the scalar loss, 1 / (number of counted rows) and the UNSCALED gradient
 * softmax(logits) - onehot(target) [N, C] (zero rows for ignored labels); backward multiplies it by the upstream scalar
 * gradient and by 1 / count, both read on the device.  row_scratch: N floats.  *bad_label (device int, zeroed by the
 * caller) is set when a label lies outside [0, C) and is not ignore_index.  Asynchronous.
 * Counted rows are those whose label is neither ignore_index nor outside [0, C), whatever their logits hold: 1 / count is formed from
 * that count in every form, the fused gradient is scaled by the same count, and a NaN in a counted row makes the mean loss NaN (so
 * do a +inf logit and a row of all -inf; -inf at the label column alone gives +inf), as F.cross_entropy does.  The loss is NaN and
 * 1 / count is 0 when no row is counted.
 * fused != 0: ONE launch for the whole forward pass, and grad_unscaled then holds the gradient ALREADY SCALED by 1 / count,
 * i.e. the gradient of the mean loss for an upstream gradient of 1 -- a training step that seeds its backward pass with 1
 * (loss.backward()) needs no backward launch at all; sage_cross_entropy_backward must not be applied to it.
 * fused == 2: as fused == 1, but the scalar loss and 1 / count are NOT written: the caller hands row_scratch to sage_adam_step_loss,
 * whose launch finishes them (one launch less per training step).
 */
int sage_cross_entropy_forward(const float *logits, const int64_t *target, int64_t N, int32_t C, int64_t ignore_index,
                               float *loss, float *grad_unscaled, float *inv_count, float *row_scratch, int32_t *bad_label,
                               int32_t fused, void *stream);
int sage_cross_entropy_backward(const float *grad_unscaled, int64_t N, int32_t C, const float *grad_loss, const float *inv_count,
                                float *grad_logits, void *stream);

/*
 * Loss and accuracy of a pass, accumulated on the device  (main.py:216-217, 227-228, 238: every training / validation / test step
 * logs F.cross_entropy(y_hat, y) and Accuracy()(y_hat.softmax(-1), y), and Lightning averages them over the pass).  One launch ADDS
 * the batch's share into acc -- 24 bytes on the device: double loss_sum; int64 correct; int64 rows -- and never resets it: the
 * caller zeroes acc before a pass and reads it once behind it (mean loss = loss_sum / rows, accuracy = correct / rows).
 *   loss_sum += sum over the counted rows of logsumexp(row) - row[target], each term formed in float32 exactly as
 *               sage_cross_entropy_forward forms it, the terms added in float64.  Blocks add with an atomic: the last bits may
 *               depend on the order they arrive in (not under sage_set_deterministic(1): one block, one add per launch).  A NaN in a counted row makes the sum NaN.
 *   correct  += rows whose argmax equals target, the argmax being numpy.argmax's: the first index of the maximum; a NaN is
 *               maximal and the first NaN wins.  Exact.
 *   rows     += counted rows: those whose label is neither ignore_index nor outside [0, C).  A label outside [0, C) that is not
 *               ignore_index also sets *bad_label (device int, zeroed by the caller), as in sage_cross_entropy_forward.  Exact.
 * POPE_ERR_INVALID without any HIP call: a null pointer, M <= 0, M >= 2^31 - 1, C <= 0.  Asynchronous; capturable.
 */
int sage_eval_metrics(const float *logits, const int64_t *target, int64_t M, int32_t C, int64_t ignore_index, void *acc,
                      int32_t *bad_label, void *stream);

/*
 * node2vec  (generate_node2vec_embedding.py:23-25: torch_geometric.nn.Node2Vec(edge_index, embedding_dim=128, walk_length=20,
 * context_size=10, walks_per_node=10, num_negative_samples=1, p=1, q=1, sparse=True); PyG's pos_sample / neg_sample / loss and
 * torch.optim.SparseAdam [3p]).  pope_n2v_walks draws first-order walks (p = q = 1), pope_n2v_walks_biased second-order (p, q)
 * walks.  All calls are asynchronous on `stream` and validate their sizes and pointers before any HIP call.
 *
 * pope_n2v_walks: rowptr [N + 1] / col: the forward CSR (pope_csr_build or pope_csr_build_canonical).  starts int64 [B].
 *   pos int64 [B, walk_length + 1]: row i starts at starts[i]; every step goes to a uniformly drawn out-neighbour SLOT (a repeated
 *   edge counts once per slot, a self-loop is a neighbour); a node without out-neighbours stays where it is (torch_cluster's rule).
 *   neg int64 [B_neg, walk_length + 1], B_neg <= B (NULL with B_neg = 0): row i = starts[i] followed by walk_length nodes uniform
 *   on [0, N) (PyG neg_sample).  pos == NULL: only the negative rows are made.
 *   The 32 random bits used at (row, step) are a counter hash of (seed, first_row + i, step, positive-or-negative) and of nothing
 *   else: a row does not depend on B, on the launch geometry or on the other rows of the call, and the steps of one row are
 *   independent draws.  Walks and negatives are bitwise reproducible.
 * pope_n2v_walks_biased: node2vec's second-order walks: pos int64 [B, walk_length + 1] only (negative rows keep coming from
 *   pope_n2v_walks with pos == NULL).  PRECONDITION: every CSR row's targets are ascending (pope_csr_build_canonical); repeated
 *   edges are allowed and count with their multiplicity as candidates.  On an unsorted row a candidate may be classified wrongly,
 *   but nothing is read outside the row.  p, q: finite doubles > 0; inv_p = 1 / p, inv_q = 1 / q, w_max = max(inv_p, 1, inv_q), in
 *   double on the host.  With t the previous node, v the current one and x a candidate slot of v's row, the weight is inv_p if
 *   x == t, else 1 if x is in t's OUT-row (binary search), else inv_q.  torch_cluster tests the edge in the other direction (x -> t);
 *   on symmetric graphs (Flickr, PubMed) the two agree.  With G = 0x9E3779B97F4A7C15, D = 0xD1B54A32D192ED03, row = first_row + i:
 *       step_key(row, s)   = mix64(seed + G (2 row + 1)) ^ (D (s + 1))            (mix64: the splitmix64 finaliser)
 *       draw(s, j, which)  = mix64(step_key + G (2 j + which)) >> 32             (which 0: candidate, 1: acceptance)
 *       below(u, n)        = (u * n) >> 32
 *   draw(s, 0, 0) is pope_n2v_walks' draw at (row, s).  Step 0 has no previous node: col[lo + below(draw(0, 0, 0), deg)].  A node
 *   without out-neighbours keeps the walker, and t does not change.  Step s >= 1: try j = 0 .. 15 proposes
 *   x = col[lo + below(draw(s, j, 0), deg)] and accepts it iff (double)draw(s, j, 1) * w_max < w * 4294967296.0 -- a candidate of
 *   weight w_max is always accepted, so p = q = 1 gives pope_n2v_walks' positive rows bit for bit on the same CSR.  After 16
 *   rejections an exact pass: W = the slots' weights summed in slot order (double), target = (double)draw(s, 16, 0) * 2^-32 * W, the
 *   first slot whose running prefix sum is > target (the last slot if none is).  The mixture is exactly the node2vec distribution.
 *   Every loop is bounded whatever p, q and the graph: 16 tries, deg slots, at most 31 halvings per search.  A row depends on
 *   (seed, first_row + i) and the graph alone; bitwise reproducible.  POPE_ERR_INVALID without any HIP call: N < 1 or N >= 2^31,
 *   walk_length < 1, B < 0, first_row < 0, p or q not finite or <= 0, a null pointer with B > 0.  B == 0: POPE_OK, nothing launched.
 * pope_n2v_windows: rows int64 [R, len] -> windows int64 [(len + 1 - context) * R, context], windows[j * R + r] = rows[r, j : j + context]:
 *   the matrices PyG's pos_sample / neg_sample return (torch.cat over j).
 * pope_n2v_loss_grad: emb float32 [N, D]; rows int64 [R, len]; 2 <= context <= len.  Row r contributes its len + 1 - context windows
 *   rows[r, j : j + context] (len == context: one window per row, PyG's window-matrix form; len == walk_length + 1: the walk itself,
 *   the windows are never materialised).  Per window, start = w[0], out_k = <emb[start], emb[w[k]]>, k = 1 .. context - 1; the term is
 *   -log(sigmoid(out) + 1e-15) (negative == 0) or -log(1 - sigmoid(out) + 1e-15) (negative != 0), evaluated literally in that form, in
 *   float64.  *loss_acc (device float64) += scale * (sum of the call's terms).  grad (float32 [N, D], or NULL: loss only) += scale * the
 *   gradient, touched[v] (uint8 [N]) = 1 for every row v added to.  With scale = 1 / (number of terms) two calls leave
 *   pos.mean() + neg.mean().  A row with a node id outside [0, N) contributes nothing.
 *   D: a multiple of 32 from 32 to 256 (128 is the tuned case); a row's embedding rows are staged in LDS, so
 *   (len (D + 1) + (len + 1 - context)(context - 1) + 16 D) * 4 + 4 (len + 16) <= 65536.  Anything else: POPE_ERR_INVALID.
 *   The gradient is accumulated with float atomic adds, at most one row of adds per walk position (a wave first sums in LDS what its 8
 *   walks add to the same node): its last bits depend on the order the
 *   adds arrive in and may differ between two runs, and so may the last bits of the float64 loss.
 * pope_n2v_sparse_adam: torch.optim.SparseAdam over emb [N, D] in one launch.  A row with touched[v] == 0 is left alone, moments
 *   included (they do not decay).  A touched row gets m += (g - m)(1 - beta1), v += (g g - v)(1 - beta2),
 *   p += -step_size * (m / (sqrt(v) + eps)), step_size = lr sqrt(1 - beta2^step) / (1 - beta1^step), with the 1-based `step` (host
 *   value, step >= 1); its grad row and its flag are cleared in the same launch.  Every operation written there -- each subtraction,
 *   multiplication, addition, the root and the division -- is one float32 operation rounded once to nearest, in that order (nothing
 *   is contracted into an FMA; the root and the quotient are the correctly rounded ones); -step_size, 1 - beta1, 1 - beta2 and eps
 *   are formed in double on the host and rounded to float32 once.  The result is a pure function of the inputs, bit for bit the
 *   NumPy float32 restatement in tests/node2vec_loss_cases.py; torch.optim.SparseAdam's CPU kernel gives the same moments bit for bit
 *   and parameters within one ulp of it.
 *
 * Deterministic mode (sage_set_deterministic(1); graphpope_amd.node2vec.loss_grad then makes the two calls below in place of
 * pope_n2v_loss_grad, so that a seed fixes a training run to the bit -- same binary, same device).  Both validate before any HIP
 * call, run asynchronously on `stream`, allocate nothing and take an empty call (R = 0 / M = 0) with null pointers.
 * pope_n2v_position_grads: the arithmetic of pope_n2v_loss_grad (embedding rows staged in LDS, products and the literal
 *   -log(sigmoid + 1e-15) forms in float64, the float coefficient scale * d term / d out, one gradient row per walk POSITION summed
 *   in registers) without merging and without atomics.  Position i of row r stores its row to contrib[(r * len + i) * D ..] (float32
 *   [R * len, D]) with plain stores and ids[r * len + i] = rows[r, i] (int32 [R * len]).  row_loss[r] (float64 [R]) = the UNSCALED sum
 *   of the row's terms, reduced over the wave in a fixed pattern.  A row holding any id outside [0, N): all len of its ids are -1,
 *   its row_loss is 0, its contrib rows are unspecified.  The output is a pure function of (emb, the row, the scalars): it does not
 *   depend on R or on the launch geometry.  D as above; LDS: (len (D + 1) + (len + 1 - context)(context - 1)) * 4 + 4 (len + 16) <= 65536.
 * pope_n2v_accumulate_det: for every node v with at least one entry e, ids[e] == v, and every column d:
 *       acc = 0.0                                                   (float64)
 *       for e ASCENDING with ids[e] == v:  acc = acc + (double)contrib[e][d]
 *       grad[v][d] = (float)((double)grad[v][d] + acc)              (one rounding to float32)
 *       touched[v] = 1
 *   ids int32 [M], contrib float32 [M, D], grad float32 [N, D] IN and OUT, touched uint8 [N].  Entries with ids[e] < 0 or >= N are
 *   skipped; nodes without entries are neither read nor written.  Then *loss_acc += scale * S, S = the float64 sum of
 *   row_loss[0 .. R) in an order that is a function of R alone: ONE add per call, landing in stream order (row_loss == NULL or
 *   R == 0: no loss part).  scratch: pope_n2v_accumulate_det_scratch_bytes(M, N) bytes (4 (N + 1) + 8 M: the inverted index of ids;
 *   0 for M = 0 and for sizes the call refuses; needs no device), 4-byte aligned, rebuilt from zero by every call: nothing an
 *   earlier call left there is read.  Seven short launches (clear, count, scan, fill, rank, sum, loss).  A list of up to 64 entries
 *   is sorted by the wave that sums it; a longer one is ranked by one thread per entry, each against its whole list (quadratic: a hub
 *   with 26 880 of 53 760 entries costs 16.6 ms), and summed by ONE wave, since the order above allows no partial
 *   sums.  Every index read from ids or from the scratch is range-checked:
 *   a bad call skips entries and never writes out of bounds.  POPE_ERR_INVALID: a null pointer, a negative size, N >= 2^31,
 *   M >= 2^31 - 1, a bad D.  POPE_ERR_WORKSPACE: too little scratch.
 */
int pope_n2v_walks(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *starts, int64_t B, int64_t B_neg,
                   int32_t walk_length, uint64_t seed, int64_t first_row, int64_t *pos, int64_t *neg, void *stream);
int pope_n2v_walks_biased(const int32_t *rowptr, const int32_t *col, int64_t N, const int64_t *starts, int64_t B, int32_t walk_length,
                          uint64_t seed, int64_t first_row, double p, double q, int64_t *pos, void *stream);
int pope_n2v_windows(const int64_t *rows, int64_t R, int32_t len, int32_t context, int64_t *windows, void *stream);
int pope_n2v_loss_grad(const float *emb, int64_t N, int32_t D, const int64_t *rows, int64_t R, int32_t len, int32_t context,
                       int32_t negative, double scale, double *loss_acc, float *grad, uint8_t *touched, void *stream);
int pope_n2v_sparse_adam(float *emb, float *grad, uint8_t *touched, float *exp_avg, float *exp_avg_sq, int64_t N, int32_t D,
                         double lr, double beta1, double beta2, double eps, int64_t step, void *stream);
int pope_n2v_position_grads(const float *emb, int64_t N, int32_t D, const int64_t *rows, int64_t R, int32_t len, int32_t context,
                            int32_t negative, double scale, int32_t *ids, float *contrib, double *row_loss, void *stream);
size_t pope_n2v_accumulate_det_scratch_bytes(int64_t M, int64_t N);
int pope_n2v_accumulate_det(const int32_t *ids, int64_t M, const float *contrib, int32_t D, int64_t N, float *grad, uint8_t *touched,
                            const double *row_loss, int64_t R, double scale, double *loss_acc, void *scratch, size_t scratch_bytes,
                            void *stream);

/* ---- Logistic regression on embedding rows (csrc/logreg.hip): PyG's Node2Vec.test for the model of
 * generate_node2vec_embedding.py:23-25 -- scikit-learn's LogisticRegression(solver='lbfgs') fitted on the embedding rows of the
 * training nodes and scored on those of the test nodes.  The optimiser (scipy's L-BFGS-B, as scikit-learn drives it) stays on the host
 * in graphpope_amd/logreg.py; these are the objective it evaluates and the predictions.  All validate before any HIP call (a message
 * behind pope_last_error(), no GPU needed), run asynchronously on `stream`, allocate nothing, and take m == 0 as an empty call that
 * launches nothing (null pointers allowed).
 *
 * Shared layout.  z float32 [N, d] with row stride ldz >= d (elements).  ids int64 [m] selects rows of z, repeats and any order
 *   allowed; ids == NULL: rows 0 .. m - 1.  A row outside [0, N) is never read: its raw values are NaN.  classes in
 *   [2, pope_logreg_max_classes() = 64]; R = 1 if classes == 2, else classes.  w float64 [R (d + fit_intercept)]: element (class c,
 *   column j) at j * R + c, the intercept at j = d -- scikit-learn's w0.ravel(order="F"), so scipy's vector goes in and out
 *   unpermuted.  raw = z W^T + b: z is widened to float64 on load, every product, exponential and sum is float64.
 * pope_logreg_loss_grad: scikit-learn's LinearModelLoss.loss_gradient, unweighted.  y int32 [m] encoded to 0 .. classes - 1 (a value
 *   outside matches no class).  classes > 2 (HalfMultinomialLoss): loss = (1/m) sum_i (logsumexp(raw_i) - raw_i[y_i]) + l2/2 |W|^2,
 *   grad_W = (1/m) (P - Y)^T z + l2 W, grad_b = (1/m) sum_i (P - Y)_i, P = softmax(raw) around the row maximum.  classes == 2
 *   (HalfBinomialLoss, one weight row): loss_i = log(1 + exp(raw_i)) - y_i raw_i and the residual sigmoid(raw_i) - y_i, in the four
 *   branches of scikit-learn's closs_grad_half_binomial, which overflow nowhere.  The intercept is not penalised; l2 is the caller's
 *   1 / (C m).  *loss (float64) and grad (float64, w's layout) are overwritten.  A NaN in a row of z makes the loss NaN (the row
 *   maximum keeps a NaN).  No float atomics: every sum has a fixed order, so the same inputs give the same bits on every call, and
 *   rows selected through ids give the bits of the same rows materialised.  scratch: pope_logreg_scratch_bytes(m, d, classes)
 *   bytes, 8-byte aligned (residual [m, R rounded up to 1, 4, 8, 16, 32 or 64] | row loss [m] | partial [slices, R (d + 1)] | loss sum [slices], float64; 0 for extents
 *   the call refuses); nothing an earlier call left there is read.  Three launches: rows (one wave per row), the gradient's and the
 *   loss's partial sums over slices of pope_logreg_slice_rows() = 256 rows (8 waves x 32 rows in row order, the 8 in wave order),
 *   the final sums in slice order.
 * pope_logreg_predict: pred int32 [m]: classes > 2 the FIRST index of the row maximum (np.argmax's rule, a NaN counting as a
 *   maximum), classes == 2 raw > 0.  y (optional, int32 [m], encoded, -1 for a label no training row had): *correct (int64,
 *   optional, needs y) = the number of rows with pred == y, zeroed by the call and counted with integer atomics.
 * POPE_ERR_INVALID: a null pointer, classes outside [2, 64], d < 1, ldz < d, m < 0 or >= 2^38, N < 1 with m > 0, too little or
 *   misaligned scratch.
 */
int32_t pope_logreg_max_classes(void);
int32_t pope_logreg_slice_rows(void);
size_t pope_logreg_scratch_bytes(int64_t m, int32_t d, int32_t classes);
int pope_logreg_loss_grad(const float *z, int64_t ldz, int64_t N, const int64_t *ids, int64_t m, int32_t d, const int32_t *y,
                          int32_t classes, int32_t fit_intercept, const double *w, double l2, double *loss, double *grad, void *scratch,
                          size_t scratch_bytes, void *stream);
int pope_logreg_predict(const float *z, int64_t ldz, int64_t N, const int64_t *ids, int64_t m, int32_t d, int32_t classes,
                        int32_t fit_intercept, const double *w, const int32_t *y, int32_t *pred, int64_t *correct, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHPOPE_HIP_H */
