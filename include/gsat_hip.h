/*
 * gsat_hip.h -- C ABI of libgsat_hip.so, the MI355X (gfx950) implementation of GSAT's
 * edge-attention -> stochastic mask -> masked message passing hot path.
 *
 * The reference (mihikamd/DP-GSAT) has no FFI: its boundary is a Python nn.Module protocol whose
 * arithmetic runs inside torch-geometric / torch-scatter / torch-sparse kernels.  Each entry point
 * below replaces the chain of third-party launches behind one reference call site, cited as
 * "replaces: <file:line>" (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success or a negative GSAT_ERR_* code; no exception crosses the
 *     ABI; gsat_last_error() returns a thread-local message for the last failure on this thread.
 *   - all tensor pointers are DEVICE pointers, contiguous row-major, fp32 unless typed otherwise;
 *     edge_index / batch keep the reference's int64 API type, everything the library produces for
 *     its own kernels (CSR arrays, permutations, segment pointers) is int32.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never allocates,
 *     frees or retains device memory, never synchronises the host, and only enqueues work on the
 *     `stream` argument (a hipStream_t passed as void*), so calls are graph-capturable and
 *     re-entrant (forward on the Python thread, backward on autograd's worker thread).
 *   - "nullable" pointers may be NULL to switch the corresponding term off.
 */
#ifndef GSAT_HIP_H
#define GSAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSAT_ABI_VERSION 4

#define GSAT_OK 0
#define GSAT_ERR_HIP (-1)        /* a HIP runtime call failed */
#define GSAT_ERR_ARG (-2)        /* bad argument (null pointer, negative extent, unsupported width) */
#define GSAT_ERR_WORKSPACE (-3)  /* workspace too small */
#define GSAT_ERR_UNSUPPORTED (-4)
#define GSAT_ERR_BLAS (-5)         /* reserved: no entry point returns it since the library GEMMs were replaced (round 1) */

int gsat_abi_version(void);

/* Device-resident seed stream for captured steps: state[0] = base seed (written once by the host), state[1] = counter; every call bumps
 * the counter and writes splitmix64(base, counter) (63 bits) to out[0], which the dropout / sampler kernels read through their seed_dev
 * argument.  One launch; deterministic given the base seed and the number of calls. */
int gsat_seed_next(uint64_t* state, uint64_t* out, void* stream);
const char* gsat_last_error(void);

/* =============================== integer edge bookkeeping ==================================== */

/* Workspace (bytes) needed by gsat_build_csr / gsat_reverse_edge_perm for E edges. */
size_t gsat_csr_workspace_bytes(int64_t num_edges, int64_t num_rows);
size_t gsat_rev_workspace_bytes(int64_t num_edges);

/*
 * Group the E edge slots by `rows` (stable): perm = edge ids sorted by (rows[e], e),
 * rowptr[r]..rowptr[r+1] = slots of row r, other_sorted[k] = (int32) other[perm[k]].
 * replaces: the scatter index handling inside MessagePassing.propagate
 *           (src/models/conv_layers.py:21,44,163) -- done once per batch instead of per launch.
 * rows/other: int64[E]; rowptr: int32[num_rows+1]; other_sorted, perm: int32[E].
 * err_flag (int32[1], device, caller-zeroed): incremented for every out-of-range row id.
 */
int gsat_build_csr(const int64_t* rows, const int64_t* other, int64_t num_edges, int64_t num_rows,
                   int32_t* rowptr, int32_t* other_sorted, int32_t* perm, int32_t* err_flag,
                   void* workspace, size_t workspace_bytes, void* stream);

/*
 * Both CSRs of one collated batch from ONE stable sort of 2E (row, edge id) keys -- by destination (forward aggregation) and by
 * source (every backward) -- plus what the host side derives from them: the hub-row chunk lists of both (gsat_row_chunks), the
 * by-source-slot -> by-destination-slot map used by the PNA backward, and int32 copies of the two edge_index rows.  Results are
 * identical to two gsat_build_csr calls (same stable order); the point is half the dependent launches per fresh batch.
 * edge_index [2,E] int64 (row 0 = source, row 1 = target).  replaces: the scatter index of MessagePassing.propagate
 * (src/models/conv_layers.py:21,44,163) for a whole batch.  workspace: gsat_csr_pair_workspace_bytes(E, N).
 * err_flag: int32[4], zeroed BY THE CALL (its first launch): [0] = number of out-of-range node ids, [1] / [2] = number of hub chunks of the
 * by-destination / by-source CSR (chunk_ptr_*[N]), so one small device->host read answers every host-side question.
 */
size_t gsat_csr_pair_workspace_bytes(int64_t E, int64_t num_nodes);
int gsat_build_csr_pair(const int64_t* edge_index, int64_t E, int64_t num_nodes, int32_t* rowptr_dst, int32_t* src_by_dst,
                        int32_t* eid_by_dst, int32_t* rowptr_src, int32_t* dst_by_src, int32_t* eid_by_src,
                        int32_t* slot_dst_of_srcslot, int32_t* chunk_ptr_dst, int32_t* chunk_ptr_src, int32_t* src32,
                        int32_t* dst32, int32_t* err_flag, void* workspace, size_t workspace_bytes, void* stream);

/*
 * rev[k] = id of the edge (dst_k, src_k); flags[0] = 1 iff the edge multiset equals its transpose
 * (is_undirected), flags[1] = number of sorted positions where edge and transposed keys differ.
 * Pairing rule for duplicate edges: stable (key, edge id) order on both sides.
 * replaces: is_undirected + torch_sparse.transpose + reorder_like
 *           (example/gsat.py:80-83, src/run_gsat.py:231-247, src/utils/utils.py:19-25).
 * edge_index: int64[2,E]; rev: int32[E]; flags: int32[2].
 */
int gsat_reverse_edge_perm(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes,
                           int32_t* rev, int32_t* flags, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * The same permutation and flags from the two CSRs of gsat_build_csr_pair (its clamped src32 / dst32 included), without a sort:
 * the k-th copy (by edge id) of (s,d) pairs with the k-th copy of (d,s); an edge without a partner keeps rev[k] = k and counts
 * in flags[1] (so flags[1] = number of unpaired edges here, 0 iff undirected -- the only property the callers use).
 * Each edge walks the shorter of the two rows that hold its copies, so hub-leaf edges cost the leaf's degree.
 */
int gsat_reverse_edge_perm_csr(const int32_t* src32, const int32_t* dst32, const int32_t* rowptr_dst, const int32_t* src_by_dst,
                               const int32_t* eid_by_dst, const int32_t* rowptr_src, const int32_t* dst_by_src,
                               const int32_t* eid_by_src, int64_t num_edges, int64_t num_nodes, int32_t* rev, int32_t* flags,
                               void* stream);

/*
 * Segment pointer of a non-decreasing id vector (PyG `batch`): ptr[g]..ptr[g+1] = rows of
 * segment g.  flags[0] counts order violations / out-of-range ids (0 = valid input).
 * replaces: the per-call `degree(batch)` + scatter index of InstanceNorm and global pools
 *           (src/utils/get_model.py:50-51, src/models/gin.py:34, src/models/pna.py:47).
 */
int gsat_segment_ptr(const int64_t* seg_ids, int64_t num_rows, int64_t num_segments, int32_t* ptr,
                     int32_t* flags, void* stream);
/* same in ONE launch, plus the int32 copy seg_ids32[n] of the ids; *flags is only incremented: the caller zeroes it */
int gsat_segment_ptr32(const int64_t* seg_ids, int64_t n, int64_t num_segments, int32_t* ptr, int32_t* seg_ids32,
                       int32_t* flags, void* stream);

/*
 * Which build the CSR entry points take (host only, no device work).  Up to out[2] keys they count (count / scan / place / order),
 * above that, or with GSAT_CSR_COUNTING=0 in the environment, they sort with rocPRIM; both give the same arrays.
 * gsat_csr_counting_limits: out[0] = longest row ordered one thread per entry, out[1] = entries per LDS chunk of a longer row,
 * out[2] = the key limit.  gsat_csr_counts(keys): 1 if a build of that many keys counts, 0 if it sorts; gsat_build_csr has
 * num_edges keys, gsat_build_csr_pair 2 * E.
 */
void gsat_csr_counting_limits(int64_t out[3]);
int gsat_csr_counts(int64_t keys);

/* out[e] = batch[index[e]]  (edge -> graph id, `batch[col]` of example/gsat.py:136). int64 out; index values outside
 * [0, table_len) are clamped into the table (they are counted as range errors by the CSR builders). */
int gsat_gather_i64(const int64_t* table, int64_t table_len, const int64_t* index, int64_t n, int64_t* out, void* stream);

/* ============================ masked message passing: sum (GIN / GINE) ====================== */

/*
 * Rows with more than GSAT_LONG_ROW_EDGES entries (power-law hubs) are split into chunks of that many
 * consecutive CSR slots: chunk sums go to a partial workspace and are added per row in chunk order, so the
 * result stays atomics-free and bitwise reproducible.  chunk_ptr[r]..chunk_ptr[r+1] = chunk ids of row r
 * (empty for short rows); built once per CSR by gsat_row_chunks.  Pass chunk_ptr = NULL to process every
 * row whole.
 */
#define GSAT_LONG_ROW_EDGES 256
size_t gsat_row_chunks_workspace_bytes(int64_t num_rows);
int gsat_row_chunks(const int32_t* rowptr, int64_t num_rows, int32_t* chunk_ptr /* [num_rows+1] */,
                    void* workspace, size_t workspace_bytes, void* stream);
/* floats needed for the partial-sum workspace of a CSR with num_edges entries and row width H */
size_t gsat_long_row_partial_floats(int64_t num_edges, int64_t H);

/*
 * out[i,:] = self_coef * self_rows[i,:] + sum_{k in row i} w_k * msg_k
 *   msg_k = x[col[k],:]                                   (edge_emb == NULL : GINConv)
 *         = relu(x[col[k],:] + edge_emb[eid[k],:])         (edge_emb != NULL : GINEConv)
 *   w_k   = att[eid[k]]  (att == NULL -> 1)
 * replaces: GINConv.forward/message and GINEConv.forward/message up to `self.nn`
 *           (src/models/conv_layers.py:14-34, 37-66): index_select + mul + scatter_sum + add.
 * x: [*,H]; self_rows: [N,H] (NULL -> x; not read when self_coef == 0); att: [E] nullable;
 * edge_emb: [E,H] nullable; rowptr int32[N+1]; col, eid: int32[E]; out: [N,H].  H % 4 == 0, H <= 2048.
 * chunk_ptr / partial: long-row support (both nullable together), see above.
 */
int gsat_aggr_sum_fwd(const float* x, const float* self_rows, const float* att, const float* edge_emb,
                      const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                      int64_t num_rows, int64_t num_edges, int64_t H, float self_coef, float* out,
                      const int32_t* chunk_ptr, float* partial, void* stream);

/*
 * Backward of gsat_aggr_sum_fwd over the TRANSPOSED structure (edges grouped by source node j):
 *   dx[j,:]   = self_coef * dout[j,:] + sum_{k in srcrow j} att_k * dout[dst[k],:] (* [pre_k > 0])
 *   datt[eid[k]]        = < msg_k , dout[dst[k],:] >
 *   dedge_emb[eid[k],:] = att_k * dout[dst[k],:] * [pre_k > 0]        (GINE only)
 * replaces: autograd backward of the above (example/trainer.py:34, src/run_gsat.py:634).
 * rowptr_src int32[N+1]; dst_sorted, eid_src int32[E]; datt nullable; dedge_emb nullable;
 * chunk_ptr / partial: long-row support for the by-source CSR.
 */
int gsat_aggr_sum_bwd(const float* x, const float* att, const float* edge_emb, const float* dout,
                      const int32_t* rowptr_src, const int32_t* dst_sorted, const int32_t* eid_src,
                      int64_t num_rows, int64_t num_edges, int64_t H, float self_coef, float* dx, float* datt,
                      float* dedge_emb, const int32_t* chunk_ptr, float* partial, void* stream);

/* ============================ masked message passing: PNA multi-aggregation ================== */

/* aggregator codes (order of `aggregators` = order of the YAML list, src/configs/PNA-*.yml) */
#define GSAT_AGG_SUM 0
#define GSAT_AGG_MEAN 1
#define GSAT_AGG_MIN 2
#define GSAT_AGG_MAX 3
#define GSAT_AGG_VAR 4
#define GSAT_AGG_STD 5
/* scaler codes (src/models/conv_layers.py:229-259) */
#define GSAT_SCALE_IDENTITY 0
#define GSAT_SCALE_AMPLIFICATION 1
#define GSAT_SCALE_ATTENUATION 2
#define GSAT_SCALE_LINEAR 3
#define GSAT_SCALE_INVERSE_LINEAR 4

/*
 * out[i, ((s*A + a)*F + p*H) : +H] = scaler_s(deg_i) * aggr_a over in-edges k of row i of
 *   m_k = att_k * [ x[i,:] || x[col[k],:] (|| edge_emb[eid[k],:]) ],   F = 2H (3H with edge_emb)
 * mean: count clamped >= 1; min/max: 0 for empty rows; var = mean(m^2) - mean(m)^2;
 * std = sqrt(relu(var) + 1e-5) (so sqrt(1e-5) for empty rows); deg_i = unweighted in-degree.
 * replaces: PNAConvSimple.message + aggregate up to `post_nn`
 *           (src/models/conv_layers.py:160-185, aggregators :193-226, scalers :229-259).
 * aggregators / scalers are HOST int32 arrays (1..8 entries).  H % 4 == 0, H <= 512 (widths above 256 run as one launch per
 * 256-channel chunk; the tiled backward below covers 64 <= H <= 256).
 */
int gsat_pna_fwd(const float* x, const float* att, const float* edge_emb, const int32_t* rowptr,
                 const int32_t* col, const int32_t* eid, int64_t num_rows, int64_t H,
                 const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                 float avg_deg_lin, float avg_deg_log, float* out, void* stream);

/*
 * Backward, destination-row pass.  For every in-edge slot k (CSR-by-destination order):
 *   dmsg[k,:]           = gradient w.r.t. the gathered row x[col[k],:]      ([E,H], slot order)
 *   datt[eid[k]]        = gradient w.r.t. att of that edge                    (nullable)
 *   dedge_emb[eid[k],:] = gradient w.r.t. edge_emb                            (nullable)
 *   dx_self[i,:]        = gradient w.r.t. x[i,:] through the x_i third of the message
 * min/max route to the FIRST slot attaining the extremum (torch-scatter CPU rule); std's relu has
 * zero slope at var <= 0.  The caller finishes dx[j,:] = dx_self[j,:] + sum_{slots of source j}
 * dmsg[slot,:] with gsat_aggr_sum_fwd over the by-source CSR (col = slot map, att = NULL).
 * replaces: autograd backward of the PNA scatter passes (example/trainer.py:34).
 */
int gsat_pna_bwd(const float* x, const float* att, const float* edge_emb, const float* dout,
                 const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t num_rows, int64_t H,
                 const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                 float avg_deg_lin, float avg_deg_log, float* dx_self, float* dmsg, float* datt,
                 float* dedge_emb, void* stream);

/*
 * The same two passes for batches with long (hub) rows: chunk_ptr = the by-destination hub-chunk list of gsat_build_csr_pair /
 * gsat_row_chunks (rows of more than GSAT_LONG_ROW_EDGES in-edges split into chunks of that many), workspace =
 * gsat_pna_long_row_floats(E, H, edge_emb != NULL) floats.  A long row is no longer walked by one lane group: its chunks are
 * reduced in parallel (statistics + first min/max slots per chunk), folded in chunk order by the row's group, and -- backward --
 * its per-edge gradients are written chunk-parallel from the row's routing record.  Bitwise reproducible; short rows unchanged.
 * chunk_ptr == NULL behaves exactly like gsat_pna_fwd / gsat_pna_bwd.
 */
size_t gsat_pna_long_row_floats(int64_t num_edges, int64_t H, int has_edge_emb);
int gsat_pna_fwd_long(const float* x, const float* att, const float* edge_emb, const int32_t* rowptr,
                      const int32_t* col, const int32_t* eid, int64_t num_rows, int64_t num_edges, int64_t H,
                      const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                      float avg_deg_lin, float avg_deg_log, float* out, const int32_t* chunk_ptr, float* workspace, void* stream);
int gsat_pna_bwd_long(const float* x, const float* att, const float* edge_emb, const float* dout,
                      const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t num_rows, int64_t num_edges, int64_t H,
                      const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                      float avg_deg_lin, float avg_deg_log, float* dx_self, float* dmsg, float* datt,
                      float* dedge_emb, const int32_t* chunk_ptr, float* workspace, void* stream);

/*
 * Tiled backward for the reference's aggregator lists (mean,min,max,std[,sum]; identity scaler; no edge_attr third): one
 * launch writes dx directly.  A workgroup owns a window ("tile") of consecutive destination rows and their in-edges; the
 * per-edge gradient rows stay in LDS and are summed per source there, so dmsg [E,H] is only touched by edges whose source lies
 * outside the window ("spilled"); a second small launch adds those.  Summation
 * order per source: dx_self, in-window rows in by-source slot order, spilled rows in by-source slot order (bitwise reproducible).
 *   gsat_pna_tile_plan:   window geometry for width H and an LDS budget per workgroup (0 -> 80 KiB): windows span
 *                         rows_nominal .. rows_nominal + rows_slack rows and hold edges_cap in-edges in LDS.
 *   gsat_pna_build_tiles: tile_desc int32[T+1][4] (16-byte aligned) = (first row, rowptr[row], rowptr_src[row], 0) of every window,
 *                         T = ceil(N / rows_nominal); window t starts at max(start of the graph containing row
 *                         t*rows_nominal, t*rows_nominal - rows_slack) when node_ptr [G+1] / node_seg [N] (gsat_segment_ptr32) are
 *                         given -- block-diagonal batches then lose almost no edge to a window boundary -- else at t*rows_nominal.
 *                         Also lists, once per batch, the sources that have a spilled edge (spill_rows[0 .. *spill_count), any order).
 *   gsat_pna_bwd_tiled:   rows_cap >= the longest window (rows_nominal + rows_slack <= 2 rows_nominal); dmsg [E,H] is scratch.
 * replaces: autograd backward of PNAConvSimple.message/aggregate (src/models/conv_layers.py:166-185).
 */
int gsat_pna_tile_plan(int64_t H, int64_t lds_budget_bytes, int32_t* rows_nominal, int32_t* rows_slack, int32_t* edges_cap);
int gsat_pna_build_tiles(const int32_t* node_ptr, const int32_t* node_seg, const int32_t* rowptr, const int32_t* rowptr_src,
                         const int32_t* slot_dst_of_srcslot, int64_t num_rows, int rows_nominal, int rows_slack, int edges_cap,
                         int32_t* tile_desc, int32_t* spill_rows /* [num_rows] */, int32_t* spill_count /* [1] */, void* stream);
int gsat_pna_bwd_tiled(const float* x, const float* att, const float* dout, const int32_t* rowptr, const int32_t* col,
                       const int32_t* eid, const int32_t* tile_desc, int64_t num_tiles, int rows_nominal, int rows_cap, int edges_cap,
                       const int32_t* rowptr_src, const int32_t* slot_dst_of_srcslot, int64_t num_rows, int64_t num_edges, int64_t H,
                       const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                       const int32_t* spill_rows, const int32_t* spill_count, float* dx, float* dmsg, float* datt,
                       const float* dx_add /* [N,H] or NULL: added to dx (a gradient reaching x by another path, e.g. the layer's residual) */,
                       void* stream);

/*
 * Node attention without the lift (example/gsat.py:112-117 `edge_att = node_att[src] * node_att[dst]`, then PNAConvSimple.message): the
 * aggregation kernels form the edge weight node_att[row] * node_att[source] at the load -- the same product, bit for bit, as
 * gsat_lift_fwd followed by gsat_pna_fwd -- so there is no [E] attention tensor, no edge-id indirection and no lift kernel either way.
 *   gsat_pna_fwd_node_att:        as gsat_pna_fwd without edge_emb / hub chunks; node_att [N].
 *   gsat_pna_bwd_tiled_node_att:  as gsat_pna_bwd_tiled; dnode_att [N] (may be NULL) = sum over the edges of a node, as destination and as
 *                                 source, of d w_e * node_att[other end], summed in CSR order inside the two passes of the tile kernel
 *                                 (bitwise reproducible); dw [E] is scratch for the spilled edges' shares (needed when dnode_att != NULL).
 * replaces: GSAT.lift_node_att_to_edge_att + its autograd backward fused into PNAConvSimple's aggregation (src/models/pna.py:57-59).
 */
/*
 * PNAConvSimple without the x_i half of the aggregate (src/models/conv_layers.py:148-153 post_nn(aggregate(message))).  The x_i part of
 * the message is the same vector for every in-edge of a row, so its aggregates are a closed form of x_i and four statistics of the row's
 * edge weights; the [N, A*2*H] aggregate is therefore never written: the forward emits the x_j parts and the four scalars, and the post_nn
 * GEMMs rebuild the x_i columns in their operand loader (the arithmetic of gsat_pna_fwd up to the order of two multiplications).
 *   gsat_pna_fwd_compact:  aggj [N, A*H] (aggregator-major), scal [N,8] = (sum a / n, sum a^2 / n, min a, max a, sum a, 0, 0, 0) of the row's
 *                          edge weights, n = max(in-degree, 1), min / max stored as 0 for a row without in-edges.  att NULL: unit weights;
 *                          att [E] with eid; att = node attention [N] with eid NULL (as gsat_pna_fwd_node_att).  Aggregators
 *                          (mean,min,max,std[,sum]), identity scaler, no edge features.
 *   gsat_pna_post_fwd:     out [N, Ho] = Agg W^T + bias, W [Ho, A*2*H] row-major (nn.Linear), split-bf16 x 3 MFMA.  H % 32 == 0.
 *   gsat_pna_post_dw:      dW [Ho, A*2*H] = dout^T Agg, reduced over the rows in ordered slabs (workspace: *_workspace_floats).  H % 64 == 0.
 * The backward's dAgg = dout W stays a plain GEMM into [N, A*2*H] (gsat_gemm_bf16x3) and feeds gsat_pna_bwd_tiled[_node_att].
 */
int gsat_pna_fwd_compact(const float* x, const float* att, const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t num_rows,
                         int64_t H, const int32_t* aggregators, int num_aggregators, float* aggj, float* scal, void* stream);
int gsat_pna_post_fwd(const float* x, const float* aggj, const float* scal, int64_t num_rows, int64_t H,
                      int num_aggregators, const float* W, int64_t ldw, const float* bias, int64_t Ho, float* out, void* stream);
size_t gsat_pna_post_dw_workspace_floats(int64_t num_rows, int64_t H, int num_aggregators, int64_t Ho);
int gsat_pna_post_dw(const float* x, const float* aggj, const float* scal, int64_t num_rows, int64_t H,
                     int num_aggregators, const float* dout, int64_t Ho, float* dW, float* workspace, size_t workspace_floats, void* stream);

int gsat_pna_fwd_node_att(const float* x, const float* node_att, const int32_t* rowptr, const int32_t* col, int64_t num_rows, int64_t H,
                          const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers, float avg_deg_lin,
                          float avg_deg_log, float* out, void* stream);
int gsat_pna_bwd_tiled_node_att(const float* x, const float* node_att, const float* dout, const int32_t* rowptr, const int32_t* col,
                                const int32_t* tile_desc, int64_t num_tiles, int rows_nominal, int rows_cap, int edges_cap,
                                const int32_t* rowptr_src, const int32_t* slot_dst_of_srcslot, int64_t num_rows, int64_t num_edges, int64_t H,
                                const int32_t* aggregators, int num_aggregators, const int32_t* scalers, int num_scalers,
                                const int32_t* spill_rows, const int32_t* spill_count, float* dx, float* dmsg, float* dnode_att, float* dw,
                                const float* dx_add, int accumulate_dnode_att /* 1: dnode_att += (the layers of a model share one attention) */,
                                void* stream);

/* ================================ BatchNorm1d over node rows ================================= */

/*
 * y = [relu]( (x - mean) * rstd * gamma + beta ), per channel over the N rows.  training: batch statistics
 * (two-pass mean / biased variance), running_mean / running_var updated in place with `momentum` (running_var
 * takes the unbiased variance, as torch); eval: running statistics.  save_mean / save_rstd [C] feed the backward.
 * replaces: nn.BatchNorm1d in GIN.MLP (src/models/gin.py:55-62) and PyG BatchNorm + F.relu in PNA
 *           (src/models/pna.py:45,57).  workspace: gsat_bn_workspace_floats() floats.  C % 4 == 0.
 */
size_t gsat_bn_workspace_floats(int64_t N, int64_t C);
int gsat_bn_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                int64_t N, int64_t C, int training, float momentum, float eps, int relu, float* y,
                float* save_mean, float* save_rstd, float* workspace, void* stream);
int gsat_bn_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* save_mean,
                const float* save_rstd, int64_t N, int64_t C, int training, int relu, float* dx, float* dgamma,
                float* dbeta, float* workspace, void* stream);

/*
 * The tail of a PNA layer in the same passes:  y = dropout_p( [relu](BN(x)) + residual )
 * replaces: `h = F.relu(batch_norm(conv(...))); x = h + x; x = F.dropout(x, p, training)` (src/models/pna.py:57-59).
 * residual may be NULL; dropout_p = 0 disables dropout (eval).  The keep mask is Philox stream 3, i.e.
 * gsat_philox_keep_mask(seed, 3, N, C, p) -- by value, or read from *seed_dev when that is not NULL (hipGraph replays) --
 * and is recomputed in the backward, which also returns dresidual = dy * keep / (1 - p) (NULL to skip).
 */
int gsat_bn_act_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    int64_t N, int64_t C, int training, float momentum, float eps, int relu, const float* residual,
                    float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* y, float* save_mean,
                    float* save_rstd, float* workspace, void* stream);
int gsat_bn_act_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* save_mean,
                    const float* save_rstd, int64_t N, int64_t C, int training, int relu, float dropout_p,
                    uint64_t seed, const uint64_t* seed_dev, float* dx, float* dresidual, float* dgamma,
                    float* dbeta, float* workspace, void* stream);

/*
 * The same two calls for a fixed-capacity batch whose rows >= *n_valid_dev (one int32 on the device, clamped to [0, N]) are padding:
 * training mean / biased variance / running statistics (unbiased factor n / max(n - 1, 1)) over the first n = *n_valid_dev rows on
 * both statistics paths; y is written for every row with the same formula.  Backward: sum dy and sum dy xhat, dgamma and dbeta from the
 * counted rows, dx with 1 / max(n, 1); rows >= n of dx and dresidual are exact zeros.  Eval mode ignores the count.  The dropout
 * mask is keyed by row, so a counted row draws what it draws in the unpadded batch.
 */
int gsat_bn_act_fwd_valid(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                          int64_t N, int64_t C, int training, float momentum, float eps, int relu, const float* residual,
                          float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* y, float* save_mean,
                          float* save_rstd, float* workspace, const int32_t* n_valid_dev, void* stream);
int gsat_bn_act_bwd_valid(const float* x, const float* dy, const float* gamma, const float* beta, const float* save_mean,
                          const float* save_rstd, int64_t N, int64_t C, int training, int relu, float dropout_p,
                          uint64_t seed, const uint64_t* seed_dev, float* dx, float* dresidual, float* dgamma,
                          float* dbeta, float* workspace, const int32_t* n_valid_dev, void* stream);

/*
 * BatchNorm over a batch that is sharded across ranks: the same kernels in separate steps, with the two tiny cross-rank
 * reductions left to the caller (torch.distributed all-reduce of [C] vectors), so a sharded run reproduces the single-process
 * statistics at the same global batch:
 *   forward:  S = all_reduce(gsat_bn_local_sum(x, NULL)); mean = S / N_global;
 *             Q = all_reduce(gsat_bn_local_sum(x, mean)); rstd = 1/sqrt(Q / N_global + eps); gsat_bn_apply_fwd(...)
 *   backward: (s1, s2) = all_reduce(gsat_bn_local_bwd_sums(...)); gsat_bn_apply_bwd(..., s1, s2, N_global, ...);
 *             the parameter gradients dbeta / dgamma are the LOCAL s1 / s2 (they are averaged with all other gradients).
 * workspace: gsat_bn_workspace_floats(N, C) floats.  replaces: what torch.nn.SyncBatchNorm would do for src/models/gin.py:58, pna.py:45.
 */
int gsat_bn_local_sum(const float* x, const float* centre, int64_t N, int64_t C, float* out, float* workspace, void* stream);
int gsat_bn_apply_fwd(const float* x, const float* gamma, const float* beta, const float* mean, const float* rstd, int64_t N, int64_t C,
                      int relu, const float* residual, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* y, void* stream);
int gsat_bn_local_bwd_sums(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                           int64_t N, int64_t C, int relu, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* sum_dy,
                           float* sum_dy_xhat, float* workspace, void* stream);
int gsat_bn_apply_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean, const float* rstd,
                      const float* sum_dy, const float* sum_dy_xhat, int64_t global_rows, const float* global_rows_dev /* nullable: device
                      float overriding global_rows, so the count reduced across ranks never visits the host */, int64_t N, int64_t C,
                      int relu, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* dx, float* dresidual, void* stream);

/*
 * out[c] = sum_r x[r,c], two-stage fixed-order reduction (bitwise reproducible).  Bias gradients of the Linear layers
 * (replaces the autograd `sum(0)` of nn.Linear in src/models/gin.py:55-62, src/models/conv_layers.py:153-155).
 * workspace: gsat_colsum_workspace_floats(C) floats.
 */
size_t gsat_colsum_workspace_floats(int64_t C);
int gsat_colsum(const float* x, int64_t R, int64_t C, float* out, float* workspace, void* stream);

/* =============================== categorical encoders (ogb) ================================= */

/*
 * out[n,:] = sum_col W[offset(col) + x[n,col], :],  offset(col) = dims[0] + ... + dims[col-1]
 * replaces: ogb AtomEncoder / BondEncoder forward (src/models/gin.py:22-25,45-47; src/models/pna.py:19-22,53-55).
 * x: int64 [N,ncol]; dims: HOST int32[ncol] table sizes; W: the ncol tables concatenated [sum(dims), H].
 * Out-of-range categories are clamped into their table.
 */
int gsat_embsum_fwd(const int64_t* x, const int32_t* dims, int ncol, const float* W, int64_t N, int64_t H,
                    float* out, void* stream);
/*
 * One-hot matrix O [N, R_padded] (R_padded >= sum(dims), multiple of 4): O[n, offset(col)+x[n,col]] = 1.
 * The encoder backward is dW = O^T dout (gsat_gemm_f32 with a_t = 1) instead of a sorted scatter-add.
 */
int gsat_onehot_rows(const int64_t* x, const int32_t* dims, int ncol, int64_t N, int64_t R_padded, float* O,
                     void* stream);

/* ================================ dense fp32 MFMA GEMM ======================================== */

/*
 * C[M,N] = (accumulate ? C : 0) + op(A) op(B) + bias,   exact fp32 (v_mfma_f32_32x32x2_f32).
 *   a_t == 0: A is [M,K] row-major;  a_t != 0: A is [K,M] row-major (reduction over rows, split-K slabs)
 *   b_t != 0: B is [N,K] row-major (nn.Linear weight);  b_t == 0: B is [K,N] row-major
 * replaces: the `addmm` launches of nn.Linear inside the attention MLP (src/utils/get_model.py:61).
 * Contiguous extents and leading dimensions must be multiples of 4; workspace (floats) from
 * gsat_gemm_workspace_floats() is only needed when a_t != 0; bias (nullable, [N]) only when a_t == 0.
 */
size_t gsat_gemm_workspace_floats(int a_t, int64_t M, int64_t N, int64_t K);
/* what gsat_gemm_f32 (allow_split == 0) or gsat_gemm_bf16x3 (allow_split != 0) will launch for these arguments (host-side, no launch, no
   HIP call; the dispatcher itself runs on the same function).  plan is HOST int32[8]:
     [0] kernel family: 0 = tile fp32, 1 = tile split-bf16, 2 = weight-stationary fp32, 3 = weight-stationary split-bf16
     [1] TM, [2] TN: the block tile is (64 TM) x (64 TN); 0 for the weight-stationary kernels
     [3] K splits (1 = none; > 1 needs the workspace)
     [4] ordered slab sum of a split product: 0 = none, 1 = scalar, 4 | 8 | 16 = lanes per 16-byte output quad (the dispatcher takes the
         scalar sum instead when the workspace is not 16-byte aligned)
     [5] NB, [6] KR (fp32) or KSTEPS (split-bf16), [7] NQ of the weight-stationary kernels; 0 for the tile kernels
   The environment's tuning overrides (GSAT_GEMM_TILE, GSAT_GEMM_PRECISION, ...) apply as in the dispatcher.  For tests and logs. */
int gsat_gemm_plan(int allow_split, int a_t, int b_t, int64_t M, int64_t N, int64_t K, int has_bias, int accumulate,
                   int64_t ldb, int32_t* plan);
int gsat_gemm_f32(int a_t, int b_t, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                  const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int accumulate,
                  float* workspace, size_t workspace_floats, void* stream);
/*
 * Same contract, but products of >= 2 GFLOP run as split-bf16: every fp32 operand x = hi + lo (two bf16), the product is
 * lo*lo + lo*hi + hi*lo + hi*hi accumulated in fp32 on v_mfma_f32_32x32x16_bf16 (componentwise error <= 2^-16 of |A||B| plus the fp32
 * accumulation; 2-5x faster).
 * For callers whose outputs are not re-normalised by a small per-graph sigma (the backbone's Linear layers).
 */
int gsat_gemm_bf16x3(int a_t, int b_t, int64_t M, int64_t N, int64_t K, const float* A, int64_t lda,
                     const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias, int accumulate,
                     float* workspace, size_t workspace_floats, void* stream);
/*
 * Weight gradient C[Mo,No] = (accumulate ? C : 0) + A^T B with A [K,Mo] and B [K,No] row-major (K = rows of the batch), split-bf16 as
 * above.  Large products on whole 128 x 128 tiles run on a streaming kernel: about one workgroup per CU, each holding one output tile
 * over a contiguous range of rows, partial tiles summed in range order (bitwise reproducible; the last bits differ from
 * gsat_gemm_bf16x3(a_t = 1), whose split points lie elsewhere).  Every other product runs as gsat_gemm_bf16x3(a_t = 1, b_t = 0).
 * gsat_gemm_wgrad_plan (host arithmetic, no launch) writes HOST int32[4]:
 *   [0] 1 = streaming kernel, 0 = the gsat_gemm_bf16x3 path    [1] S, the number of row ranges (K splits)
 *   [2] rows per range (a multiple of 32; the last range holds the rest)
 *   [3] workspace floats the call needs (streaming kernel: S * Mo * No)
 * The workspace must be 16-byte aligned, like A, B and C; lda, ldb, ldc multiples of 4.
 */
int gsat_gemm_wgrad_plan(int64_t Mo, int64_t No, int64_t K, int32_t* plan);
int gsat_gemm_wgrad_x3(int64_t Mo, int64_t No, int64_t K, const float* A, int64_t lda, const float* B, int64_t ldb,
                       float* C, int64_t ldc, int accumulate, float* workspace, size_t workspace_floats, void* stream);
/*
 * The two backward products of a Linear layer that read the same output gradient G [R,Cg] (R = rows of the batch), split-bf16 as above:
 *   OUT[R,Co] = G W  (W [Cg,Co] row-major)          DW[Cg,Cy] = (accumulate ? DW : 0) + G^T Y  (Y [R,Cy] row-major)
 * Where gsat_gemm_bf16x3(a_t = 0, b_t = 0) would take its weight-stationary kernel and gsat_gemm_wgrad_x3 its streaming kernel, and two
 * workgroups' LDS fits a CU (Cg <= 256), both run in ONE launch: every workgroup runs one of the two kernels' bodies unchanged, the two kinds interleaved so that a CU holds one of each.
 * OUT and DW have the bits of the two separate calls, which is what runs for every other shape and under GSAT_GEMM_PAIR=0.
 * gsat_gemm_pair_plan (host arithmetic, no launch) writes HOST int32[4]:
 *   [0] 1 = one launch, 0 = the two separate calls    [1] weight-gradient workgroups    [2] backward-data workgroups
 *   [3] dynamic LDS bytes of a workgroup              ([1]..[3] are 0 when [0] is 0)
 * The workspace is that of gsat_gemm_wgrad_x3(Cg, Cy, R) (gsat_gemm_wgrad_plan [3]), 16-byte aligned like G, W, OUT, Y and DW; every
 * leading dimension a multiple of 4.
 */
int gsat_gemm_pair_plan(int64_t R, int64_t Cg, int64_t Co, int64_t Cy, int32_t* plan);
int gsat_gemm_pair_x3(int64_t R, int64_t Cg, int64_t Co, int64_t Cy, const float* G, int64_t ldg, const float* W, int64_t ldw,
                      float* OUT, int64_t ldo, const float* Y, int64_t ldy, float* DW, int64_t lddw, int accumulate,
                      float* workspace, size_t workspace_floats, void* stream);

/* =============================== attention extractor MLP ===================================== */

/*
 * ExtractorMLP + concrete sampler:
 *   edge mode:  z_e = MLP([emb[src_e] || emb[dst_e]], segment = batch[src_e])   (M = E rows)
 *   node mode:  z_n = MLP(emb[n], segment = batch[n])                            (M = N rows)
 *   MLP = Linear(C0,C1) -> InstanceNorm(per graph) -> ReLU -> Dropout(p)
 *      -> Linear(C1,C2) -> InstanceNorm -> ReLU -> Dropout(p) -> Linear(C2,1)
 *   InstanceNorm: per-graph, per-channel mean, biased variance of the centred values, eps 1e-5,
 *   no affine, batch statistics in train and eval.
 *   att = sigmoid(z + log u - log(1-u)) when `training` and `u` given, else sigmoid(z).
 * replaces: ExtractorMLP.forward (example/gsat.py:131-139; src/run_gsat.py:909-927), MLP /
 *   BatchSequential / InstanceNorm / ReLU / Dropout (src/utils/get_model.py:47-68) and
 *   GSAT.sampling / concrete_sample (example/gsat.py:94-103; src/run_gsat.py:877-885).
 * In edge mode layer 1 is evaluated on NODES (P = emb W1[:, :H]^T, Q = emb W1[:, H:]^T, then
 * h1_e = P[src_e] + Q[dst_e] + b1), so the [E, 2H] concat and the E-row first GEMM never exist.
 * Dropout keep-masks: `mask1/mask2` (float 0/1) if given, else Philox4x32-10 of (seed, layer, row, col).
 */
typedef struct gsat_attn_args {
    int64_t M, N, G;
    int32_t H, C1, C2;
    int32_t edge_mode;
    int32_t training;
    float p_drop;
    uint64_t seed;
    const int32_t* src;        /* [E] int32 edge_index[0]   (edge mode) */
    const int32_t* dst;        /* [E] int32 edge_index[1]   (edge mode) */
    const int32_t* seg_ptr;    /* [G+1] MLP rows grouped by graph */
    const int32_t* seg_order;  /* [M] row ids in grouped order, NULL = identity */
    const int32_t* row_seg;    /* [M] graph id of every row */
    const float *W1, *b1, *W2, *b2, *W3, *b3;   /* nn.Linear layout [out, in] */
    const float* emb;          /* [N,H] */
    const float* mask1;        /* nullable [M,C1] */
    const float* mask2;        /* nullable [M,C2] */
    const float* u;            /* nullable [M] */
    float* P;                  /* [N,C1] saved: edge P ; node h1 (no bias) */
    float* Q;                  /* [N,C1] saved: edge Q ; node: NULL */
    float* a1;                 /* [M,C1] saved: dropout(relu(norm(h1))) */
    float* h2;                 /* [M,C2] saved: a1 W2^T (no bias) */
    float* stats;              /* [G*(2*C1+2*C2)] saved: mean1 | rstd1 | mean2 | rstd2 */
    float* logits;             /* [M] out */
    float* att;                /* [M] out, nullable */
    void* fwd_workspace;       /* gsat_attn_fwd_workspace_bytes() bytes (0 for batches of small graphs) */
    size_t fwd_workspace_bytes;
    const uint64_t* seed_dev;  /* nullable DEVICE word overriding `seed` (hipGraph replays: new dropout mask per replay) */
    int32_t noise_philox;      /* != 0 with `training` and u == NULL: draw the concrete sampler's u in the kernel (Philox stream 4 of
                                  `seed`, row-keyed) instead of reading a tensor -- the reference's uniform_ launch (example/gsat.py:96) */
    int32_t fused;             /* one-launch forward (whole graphs per workgroup, attn_fused.hip): 1 = whenever the shapes allow it, -1 = never,
                                  0 = automatic (GSAT_ATTN_FUSED=1 / 0 overrides): node mode, H % 16 == 0, M >= 32768 rows; its layer products
                                  are split-bf16 x 6 on the bf16 matrix pipe (fp32-level accuracy; GSAT_ATTN_FUSED_X6=0: exact fp32 MFMA) */
    const int32_t* node_ptr;   /* [G+1] node segments of the batch; edge mode needs it for the fused forward (NULL: staged pipeline) */
} gsat_attn_args;

typedef struct gsat_attn_grads {
    const float* dlogits;      /* nullable [M] gradient w.r.t. logits */
    const float* datt;         /* nullable [M] gradient w.r.t. att (needs args->att) */
    const int32_t* rowptr_src; /* edge mode: by-source CSR + edge ids */
    const int32_t* eid_by_src;
    const int32_t* rowptr_dst; /* edge mode: by-destination CSR + edge ids */
    const int32_t* eid_by_dst;
    const int32_t* chunk_ptr_src; /* nullable: long-row chunks of the two CSRs (gsat_row_chunks) */
    const int32_t* chunk_ptr_dst;
    float *demb, *dW1, *db1, *dW2, *db2, *dW3, *db3;
    void* workspace;
    size_t workspace_bytes;
} gsat_attn_grads;

size_t gsat_attn_fwd_workspace_bytes(const gsat_attn_args* args);
/* which forward gsat_attn_fwd will run for these arguments (host-side, no launch): 0 = staged pipeline (layer products exact fp32 MFMA),
   1 = one-launch forward with exact fp32 MFMA, 2 = one-launch forward with split-bf16 x 6 products.  For logs and benchmark lines. */
int gsat_attn_fwd_kind(const gsat_attn_args* args);
/*
 * Every kernel choice gsat_attn_fwd and gsat_attn_bwd would make for these arguments under the current environment (host-side, no launch,
 * pointers of `args` are only tested for NULL): writes HOST int32[GSAT_ATTN_PATHS_N], `n` = the slots `out` holds (>= GSAT_ATTN_PATHS_N).
 * The two entry points branch on the same evaluation of the predicates, so the report cannot drift from the dispatch.  For tests and logs.
 *   forward:   FWD_KIND as gsat_attn_fwd_kind; for the one-launch forward also FWD_PQG (edge mode: 1 = P | Q of a tile's nodes through
 *              global memory, 0 = in the tile), FWD_NRB (64-row blocks per row wave: tiles of 64 * NRB rows) and FWD_NCBW (32-column
 *              blocks of layer 2 per column wave); these three are 0 for the staged pipeline.
 *   both:      SLICES = row slices per graph of the segmented statistics (1 for batches of small graphs).
 *   backward:  BWD_FUSED 1 = the one-launch backward down to dh1 (GSAT_ATTN_BWD_FUSED=1 where eligible) with BWD_NCHT layer-1 chunks in
 *              its template, 0 = staged kernels; BWD_DUAL_L2 / BWD_PAIR_L2 = da1 | dW2 through the dual tile kernel (GSAT_DUAL_GEMM=1) /
 *              as one gsat_gemm_pair_x3 launch, both 0 = two GEMM calls (also 0 under BWD_FUSED, which forms them itself);
 *              BWD_DUAL_L1 / BWD_PAIR_L1 = demb | dW1 likewise; BWD_SPLIT 1 = split-bf16 products, 0 = exact fp32 MFMA
 *              (GSAT_ATTN_BWD_SPLIT=0); BWD_MERGED 1 = dW3 / db3 finished in one launch from the head kernel's partials, 0 = two two-stage
 *              column sums (GSAT_ATTN_BWD_MERGED=0, sliced segments, or BWD_FUSED).
 */
#define GSAT_ATTN_PATH_FWD_KIND 0
#define GSAT_ATTN_PATH_FWD_PQG 1
#define GSAT_ATTN_PATH_FWD_NRB 2
#define GSAT_ATTN_PATH_FWD_NCBW 3
#define GSAT_ATTN_PATH_SLICES 4
#define GSAT_ATTN_PATH_BWD_FUSED 5
#define GSAT_ATTN_PATH_BWD_NCHT 6
#define GSAT_ATTN_PATH_BWD_DUAL_L2 7
#define GSAT_ATTN_PATH_BWD_DUAL_L1 8
#define GSAT_ATTN_PATH_BWD_PAIR_L2 9
#define GSAT_ATTN_PATH_BWD_PAIR_L1 10
#define GSAT_ATTN_PATH_BWD_SPLIT 11
#define GSAT_ATTN_PATH_BWD_MERGED 12
#define GSAT_ATTN_PATHS_N 13
int gsat_attn_paths(const gsat_attn_args* args, int32_t* out, int n);
size_t gsat_attn_bwd_workspace_bytes(const gsat_attn_args* args);
int gsat_attn_fwd(const gsat_attn_args* args, void* stream);
int gsat_attn_bwd(const gsat_attn_args* args, const gsat_attn_grads* grads, void* stream);

/* ---- memory-bounded edge-mode extractor: a1 and da1 streamed by groups of whole graphs ------------------------------------------------
 * gsat_attn_fwd saves a1 [M, C1] and gsat_attn_bwd takes a second [M, C1] buffer (da1 -> dh1) from its workspace: with M = E and
 * C1 = 4H these two are most of the memory of a step on large graphs.  The per-graph InstanceNorm makes graphs independent everywhere
 * but in the weight-gradient sums, so the entry points below run the junction of layer 1 and layer 2 one GROUP of consecutive graphs at
 * a time through a scratch of `scratch_rows` rows.  Saved between forward and backward: P, Q, h2, stats, att -- no [M, C1] tensor; the
 * backward computes a group's a1 again from P, Q, b1, the saved statistics and the keep decisions (Philox draws and explicit masks are
 * keyed by the GLOBAL row, so a streamed step uses the keep decisions and the noise of the unstreamed one).  Edge mode only
 * (GSAT_ERR_UNSUPPORTED otherwise); no float atomics, groups run in order: two runs with one plan are bitwise equal.
 *
 * gsat_attn_stream_plan: HOST code, no launch.  seg_ptr [G+1] (HOST: edge rows per graph), budget >= 1 rows.  Greedy in graph order: a
 *   group is the longest run of consecutive graphs whose rows sum to <= budget; a graph with more rows is a group of its own; graphs
 *   without rows never open a group (they join the group before them, or the first one).  Writes group_ptr [n_groups+1] (graph ids;
 *   room for G+1 entries), n_groups and scratch_rows = the largest row count of a group, at least 1.
 * gsat_attn_stream_check: ONE launch; stores into the DEVICE word `verdict` the OR of GSAT_ATTN_STREAM_BAD_ORDER (some row m lies
 *   outside [seg_ptr[row_seg[m]], seg_ptr[row_seg[m]+1]): rows are not grouped by graph in row order) and GSAT_ATTN_STREAM_BAD_CROSS
 *   (node_seg[src[m]] != node_seg[dst[m]], or != row_seg[m]: an edge joins two graphs); 0 = the batch can be streamed.  Streaming rests
 *   on both: a group's rows are one contiguous range, and the CSR rows of a group's nodes hold edge ids of that range only.
 * gsat_attn_stream_fwd / _bwd: `args` / `grads` as for gsat_attn_fwd / gsat_attn_bwd with args->a1 == NULL (not read) and
 *   args->seg_order == NULL (required); args->fwd_workspace holds gsat_attn_stream_fwd_workspace_bytes() bytes and grads->workspace
 *   gsat_attn_stream_bwd_workspace_bytes() bytes.  group_ptr / n_groups / scratch_rows: a plan as gsat_attn_stream_plan writes it (any
 *   partition of [0, G) into runs of at most scratch_rows rows is accepted); seg_ptr_host / node_ptr_host: HOST copies of args->seg_ptr
 *   and args->node_ptr.  The plan is validated on the host before the first launch.  db1 = db2 = 0 exactly, as in gsat_attn_bwd.
 */
#define GSAT_ATTN_STREAM_BAD_ORDER 1
#define GSAT_ATTN_STREAM_BAD_CROSS 2
int gsat_attn_stream_plan(const int32_t* seg_ptr, int64_t G, int64_t budget, int32_t* group_ptr, int64_t* n_groups, int64_t* scratch_rows);
int gsat_attn_stream_check(const int32_t* src, const int32_t* dst, const int32_t* node_seg, const int32_t* seg_ptr, const int32_t* row_seg,
                           int64_t M, int64_t N, int64_t G, int32_t* verdict, void* stream);
size_t gsat_attn_stream_fwd_workspace_bytes(const gsat_attn_args* args, int64_t scratch_rows);
int gsat_attn_stream_fwd(const gsat_attn_args* args, const int32_t* group_ptr, int64_t n_groups, const int32_t* seg_ptr_host,
                         const int32_t* node_ptr_host, int64_t scratch_rows, void* stream);
size_t gsat_attn_stream_bwd_workspace_bytes(const gsat_attn_args* args, const int32_t* group_ptr, int64_t n_groups,
                                            const int32_t* seg_ptr_host, int64_t scratch_rows);
int gsat_attn_stream_bwd(const gsat_attn_args* args, const gsat_attn_grads* grads, const int32_t* group_ptr, int64_t n_groups,
                         const int32_t* seg_ptr_host, const int32_t* node_ptr_host, int64_t scratch_rows, void* stream);

/* Standalone per-graph InstanceNorm (src/utils/get_model.py:50-51,64) for BatchSequential users.
 * y = (x - mean_g) * rstd_g ; stats [G*2*C] = mean | rstd (saved for backward). */
int gsat_instance_norm_fwd(const float* x, const int32_t* seg_ptr, const int32_t* seg_order,
                           const int32_t* row_seg, int64_t M, int64_t G, int64_t C, float* y,
                           float* stats, void* stream);
int gsat_instance_norm_bwd(const float* y, const float* dy, const float* stats, const int32_t* seg_ptr,
                           const int32_t* seg_order, const int32_t* row_seg, int64_t M, int64_t G,
                           int64_t C, float* dx, float* workspace /* [G*2*C] */, void* stream);

/* u[m]: the concrete sampler's noise gsat_attn_fwd draws for row m when noise_philox is set (parity tests pass it back explicitly) */
int gsat_philox_noise(uint64_t seed, int64_t M, float* u, void* stream);

/* keep[m,c] in {0,1}: the Philox dropout mask gsat_attn_* uses for (seed, layer, row m, column c). */
int gsat_philox_keep_mask(uint64_t seed, int32_t layer, int64_t M, int64_t C, float p_drop, float* keep,
                          void* stream);

/* GIN layer tail (src/models/gin.py:49-52: x = F.dropout(relu(conv(x)), p)): y = relu(x) * keep / (1 - p), keep drawn from the Philox
 * stream 5 of `seed` keyed by (row, column) -- or from the device word `seed_dev` (captured steps).  The backward needs y alone:
 * dx = dy / (1 - p) where y > 0, else 0.  C % 4 == 0. */
int gsat_relu_dropout_fwd(const float* x, int64_t N, int64_t C, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* y,
                          void* stream);
int gsat_relu_dropout_bwd(const float* y, const float* dy, int64_t N, int64_t C, float dropout_p, float* dx, void* stream);

/* ============================ samplers, lift, symmetrise, info loss ========================== */

/*
 * att = sigmoid((logits + noise_term) / temp);  mode 0: no noise (eval);
 * mode 1 (concrete): noise_term = log(u) - log(1-u), u = noise[m]   (example/gsat.py:94-103)
 * mode 2 (gumbel):   noise_term = -log(-log(U + eps) + eps)          (src/run_gsat.py:182-187)
 * backward: dlogits = datt * att * (1 - att) / temp.
 */
int gsat_sample_fwd(const float* logits, const float* noise, int mode, float temp, float eps, int64_t M,
                    float* att, void* stream);
int gsat_sample_bwd(const float* att, const float* datt, float temp, int64_t M, float* dlogits, void* stream);

/*
 * Gumbel-sigmoid (mode 2 above) whose uniform is drawn inside the kernel: U[m] = word m & 3 (x, y, z, w) of
 * philox4x32(seed, m >> 2, 0, 5, 0x5A17) -- Philox stream 5 -- as (float)(word >> 8) * 2^-24, in [0, 1) like torch.rand; one draw
 * serves four consecutive rows.  The seed is *seed_dev when seed_dev != NULL (a captured hipGraph draws new noise on every replay
 * once gsat_seed_next rewrites that word), else `seed`.  att is bitwise gsat_sample_fwd(mode 2) on the U that
 * gsat_philox_gumbel_noise reports for the same seed; the backward is gsat_sample_bwd.  16-byte loads and stores when logits and att
 * are 16-byte aligned, scalar ones otherwise.  M == 0: no launch; M >= 2^31 or tau <= 0: GSAT_ERR_ARG.
 */
int gsat_gumbel_sigmoid_philox(const float* logits, int64_t M, float tau, float eps, uint64_t seed, const uint64_t* seed_dev,
                               float* att, void* stream);
int gsat_philox_gumbel_noise(uint64_t seed, int64_t M, float* U, void* stream);

/*
 * edge_att[e] = node_att[src_e] * node_att[dst_e]
 * replaces: lift_node_att_to_edge_att (example/gsat.py:112-117, src/run_gsat.py:870-875).
 * backward walks both CSRs (no atomics): dnode[n] = sum_out d_e a[dst_e] + sum_in d_e a[src_e].
 */
int gsat_lift_fwd(const float* node_att, const int32_t* src, const int32_t* dst, int64_t num_edges,
                  float* edge_att, void* stream);
int gsat_lift_bwd(const float* node_att, const float* dedge_att, const int32_t* rowptr_src,
                  const int32_t* dst_by_src, const int32_t* eid_by_src, const int32_t* rowptr_dst,
                  const int32_t* src_by_dst, const int32_t* eid_by_dst, int64_t num_nodes,
                  float* dnode_att, void* stream);

/*
 * out[k] = (att[k] + att[rev[k]]) / 2 ; rev from gsat_reverse_edge_perm (an involution, so the same
 * call maps d(out) to d(att)).  replaces: example/gsat.py:81-83, src/run_gsat.py:233-235,243-245.
 */
int gsat_symmetrise(const float* att, const int32_t* rev, const int32_t* undirected_flag /* nullable device int32: 0 -> out = att */,
                    int64_t num_edges, float* out, void* stream);

/*
 * out[0] = mean_m [ a log(a/r + 1e-6) + (1-a) log((1-a)/(1-r+1e-6) + 1e-6) ], r = r_vec[m] if r_vec
 * else r_scalar.  replaces: example/gsat.py:31; src/run_gsat.py:127,132 (tensor prior).
 * partial: scratch float[1024].  backward: datt[m] = gout[0]/M * d term / d a (r is detached).
 */
int gsat_info_loss_fwd(const float* att, const float* r_vec, float r_scalar, int64_t M, float* partial,
                       float* out, void* stream);
int gsat_info_loss_bwd(const float* att, const float* r_vec, float r_scalar, const float* gout, int64_t M,
                       float* datt, void* stream);

/*
 * The info loss of a fixed-capacity batch: the mean runs over the first m = *m_valid_dev entries (int32 on the device, clamped to
 * [0, M]; the divisor is max(m, 1)), datt[k] = 0 exactly for k >= m.  r_dev (one float on the device, may be NULL) overrides r_scalar,
 * so the get_r(epoch) schedule can change between replays of a captured step.
 */
int gsat_info_loss_valid_fwd(const float* att, const float* r_vec, float r_scalar, const float* r_dev, int64_t M,
                             const int32_t* m_valid_dev, float* partial, float* out, void* stream);
int gsat_info_loss_valid_bwd(const float* att, const float* r_vec, float r_scalar, const float* r_dev, const float* gout,
                             int64_t M, const int32_t* m_valid_dev, float* datt, void* stream);

/*
 * Soft-F1 sparsity loss over the first m entries: loss[0] = (1 - f1) + sum|p| / max(m, 1) with TP = sum p*y, P = sum p, G = sum y,
 * precision = TP / (P + 1e-6), recall = TP / (G + 1e-6), f1 = 2 precision recall / (precision + recall + 1e-6).
 * replaces: src/run_gsat.py:151-180.  m = *m_valid_dev (int32 on the device, clamped to [0, M]) or M when m_valid_dev is NULL; entries at
 * or beyond m are not read.  partial: scratch float[1024], 16-byte aligned.  stats float[8] = (TP, P, G, sum|p|, dloss/dTP, dloss/dP,
 * 1 / max(m, 1), 0) feeds the backward: dp[k] = gout[0] * (stats[4] y[k] + stats[5] + sign(p[k]) stats[6]) for k < m and exactly 0
 * beyond (y is a label: no gradient).  Two-stage sums in a fixed order, no atomics: equal inputs give equal bits.  One block of the
 * first stage covers gsat_f1_sparsity_block_entries() entries until gsat_f1_sparsity_max_blocks() blocks are in use.
 */
int gsat_f1_sparsity_fwd(const float* p, const float* y, int64_t M, const int32_t* m_valid_dev, float* partial, float* loss,
                         float* stats, void* stream);
int gsat_f1_sparsity_bwd(const float* p, const float* y, const float* stats, const float* gout, int64_t M,
                         const int32_t* m_valid_dev, float* dp, void* stream);
int64_t gsat_f1_sparsity_block_entries(void);
int64_t gsat_f1_sparsity_max_blocks(void);

/*
 * The classification criterion (src/utils/get_model.py:19-34) over the first b rows of logits [G, C]: b = *g_valid_dev (int32 on the
 * device, clamped to [0, G]) or G when g_valid_dev is NULL; rows at or beyond b are not read.
 *   mode 0 (binary):      mean over the b C entries of max(z, 0) - z y + log1p(exp(-|z|)); target float[G, C].
 *   mode 1 (cross entropy): mean over the b rows of logsumexp(z_row) - z_row[y] (max-subtracted); target float[G] holds the class index.
 *                         An index outside [0, C) (or NaN) makes the loss NaN and is never used as an offset.
 *   mode 2 (multi-label): mode 0's term over the entries whose target is not NaN, divided by their number in the rows < b.
 * The divisor is clamped to at least 1: an empty selection gives the loss 0 and zero gradients (torch gives NaN), as in
 * gsat_info_loss_valid_*.  partial: scratch float[512] (sums, then the counts as uint32 bits).  stats float[4] = (sum, divisor,
 * 1 / divisor, 0) feeds the backward: dlogits = gout[0] (sigmoid(z) - y) / divisor (modes 0, 2; 0 on unlabelled entries) or
 * gout[0] (softmax(z_row) - onehot(y)) / divisor (mode 1; NaN over a row whose label is no class), and exactly 0 in every row >= b
 * whatever it holds (the target is a label: no gradient).  Two-stage sums in a fixed order, no atomics: equal inputs give equal bits.
 * Kernels only (no memset / memcpy), nothing is read back: capturable.  One first-stage block covers gsat_criterion_block_items(C, mode)
 * entries (modes 0, 2) or rows (mode 1; 4 lanes per row for C <= 16, else 64) until gsat_criterion_max_blocks() blocks are in use.
 * 1 <= G <= 2^20 and 1 <= C <= 1024 (GSAT_ERR_UNSUPPORTED beyond, never a truncation).
 */
int gsat_criterion_fwd(const float* logits, const float* target, int64_t G, int64_t C, int mode, const int32_t* g_valid_dev,
                       float* partial, float* loss, float* stats, void* stream);
int gsat_criterion_bwd(const float* logits, const float* target, const float* stats, const float* gout, int64_t G, int64_t C, int mode,
                       const int32_t* g_valid_dev, float* dlogits, void* stream);
int64_t gsat_criterion_block_items(int64_t C, int mode);
int64_t gsat_criterion_max_blocks(void);

/* out[i] = (int32) in[i] */
int gsat_narrow_i64(const int64_t* in, int64_t n, int32_t* out, void* stream);

/* ================================ device-side batch assembly ================================= */

/*
 * Collate the graphs `graph_ids` of a packed dataset into one batch, on the device.
 * Packed dataset: nodes / edges of all graphs concatenated; node_ptr_all / edge_ptr_all int64[G_all+1];
 * edge_local_all int64[2, num_edges_all] with node ids LOCAL to their graph.
 * out_node_ptr / out_edge_ptr int64[num_graphs+1] = exclusive scans of the selected graphs' node / edge counts.
 * Outputs: batch[N] (graph id per node), node_src_row[N] (row of x_all to copy), edge_index[2,E] (offset to batch ids),
 * edge_src_slot[E] (slot of edge_attr_all / edge_label_all to copy).
 * replaces: PyG DataLoader collation / Batch.from_data_list (src/utils/get_data_loaders.py:130-145) [3P]: node offset of
 * edge_index by the cumulative node count, batch[n] = graph id, graph order = order of graph_ids.
 */
int gsat_collate(const int64_t* graph_ids, int64_t num_graphs, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                 const int64_t* edge_local_all, int64_t num_edges_all, const int64_t* out_node_ptr,
                 const int64_t* out_edge_ptr, int64_t N, int64_t E, int64_t* batch, int64_t* node_src_row,
                 int64_t* edge_index, int64_t* edge_src_slot, void* stream);

/*
 * gsat_collate into tensors of fixed capacity (batch / node_src_row [N_cap], edge_index [2, E_cap], edge_src_slot [E_cap]): one launch.
 * Rows < N_real and slots < E_real (the last entries of out_node_ptr / out_edge_ptr, read on the device) are what gsat_collate writes.
 * Padding nodes get graph id num_graphs and source row -1.  Padding slot E_real + j (source slot -1) joins the padding nodes
 * a = N_real + q % n_pad and b = N_real + (q + 1) % n_pad, q = j / 2: a -> b for even j, b -> a for odd j, and the self loop a -> a in
 * the last slot of an odd count -- a symmetric set that touches no real node.  valid (int32[4]) = (N_real, E_real, num_graphs, overflow).
 * N_real + 2 > N_cap or E_real > E_cap: overflow = 1 and an all-padding batch (N_real = E_real = 0); nothing is written out of bounds.
 */
int gsat_collate_padded(const int64_t* graph_ids, int64_t num_graphs, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                        const int64_t* edge_local_all, int64_t num_edges_all, const int64_t* out_node_ptr,
                        const int64_t* out_edge_ptr, int64_t N_cap, int64_t E_cap, int64_t* batch, int64_t* node_src_row,
                        int64_t* edge_index, int64_t* edge_src_slot, int32_t* valid, void* stream);

/*
 * The two scans of a ragged batch in one launch (one block).  graph_ids int64[num_slots]: a graph id, or a negative value for an EMPTY
 * slot.  out_node_ptr / out_edge_ptr int64[num_slots + 1] = exclusive scans of the slots' node / edge counts, an empty slot counting 0;
 * safe_ids int64[num_slots] = the ids with 0 in the empty slots; empty uint8[num_slots] = 1 for an empty slot; state int64[2] =
 * (number of filled slots, spoiled).  spoiled = 1 when a filled slot follows an empty one (empty slots must be trailing) or an id is
 * not below num_graphs_all; such an id counts nothing and is never used as an offset.  Integer sums: bitwise repeatable; capturable.
 */
int gsat_ragged_scan(const int64_t* graph_ids, int64_t num_slots, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                     int64_t num_graphs_all, int64_t* out_node_ptr, int64_t* out_edge_ptr, int64_t* state, int64_t* safe_ids,
                     uint8_t* empty, void* stream);

/*
 * gsat_ragged_scan for a primal / dual pair (a dataset and its line-graph dataset), one launch of one block: a third exclusive scan,
 * out_dual_edge_ptr int64[num_slots + 1], of the slots' dual edge counts (dual_edge_ptr_all: the dual dataset's edge_ptr_all), and
 * the JOINT verdict.  spoiled = 1 when a filled slot follows an empty one, an id is not below num_graphs_all, or the totals break
 * N + 2 <= N_cap, E <= E_cap or E_dual <= E_dual_cap (totals in int64; every capacity below 2^31, E_cap below 2^31 - 2 because the
 * dual node capacity is E_cap + 2).  The dual side's node scan is out_edge_ptr; both sides share safe_ids, empty and state, so that
 * gsat_collate_padded_ragged(..., state, ...) on either side overflows exactly when the other does.  Integer sums; capturable.
 */
int gsat_ragged_pair_scan(const int64_t* graph_ids, int64_t num_slots, const int64_t* node_ptr_all, const int64_t* edge_ptr_all,
                          const int64_t* dual_edge_ptr_all, int64_t num_graphs_all, int64_t N_cap, int64_t E_cap, int64_t E_dual_cap,
                          int64_t* out_node_ptr, int64_t* out_edge_ptr, int64_t* out_dual_edge_ptr, int64_t* state, int64_t* safe_ids,
                          uint8_t* empty, void* stream);

/*
 * gsat_collate_padded with a graph count read on the device: ragged_state int64[2] = (filled slots, spoiled) and the scans are
 * gsat_ragged_scan's, so the empty slots own no node and no edge and their graph_ids entries are never dereferenced.  valid[2] = the
 * number of filled slots; a spoiled batch is an overflow like one that does not fit, and an overflow batch has valid == (0, 0, 0, 1).
 * Padding nodes still get graph id num_graphs.
 */
int gsat_collate_padded_ragged(const int64_t* graph_ids, int64_t num_graphs, const int64_t* ragged_state, const int64_t* node_ptr_all,
                               const int64_t* edge_ptr_all, const int64_t* edge_local_all, int64_t num_edges_all,
                               const int64_t* out_node_ptr, const int64_t* out_edge_ptr, int64_t N_cap, int64_t E_cap, int64_t* batch,
                               int64_t* node_src_row, int64_t* edge_index, int64_t* edge_src_slot, int32_t* valid, void* stream);

/*
 * Line ("dual") graph: dual node k = primal directed edge k; dual edges join, in both directions, every two primal
 * edges that leave the same node.  counts[n] = d_n (d_n - 1) / 2; pair_ptr = exclusive scan of counts (int64[N+1]);
 * dual_edge_index int64[2, 2*num_pairs], ordered: source node ascending, pairs (i<j) in edge-id order, (e_i,e_j),(e_j,e_i).
 * replaces: the pure-Python pair loops of src/datasets/mutag_dual.py:345-377 (`group_by_first`).
 */
int gsat_line_graph_pair_counts(const int32_t* rowptr_src, int64_t num_nodes, int64_t* counts, void* stream);
int gsat_line_graph(const int32_t* rowptr_src, const int32_t* eid_by_src, const int64_t* pair_ptr, int64_t num_nodes,
                    int64_t num_pairs, int64_t* dual_edge_index, void* stream);

/*
 * Line graph with one dual node per UNDIRECTED primal edge (the ba_2motifs dual dataset of the fork).
 * Undirected edges are numbered in row-major order of (smaller endpoint, larger endpoint); dual nodes i != j are adjacent
 * when their primal edges share an endpoint; dual_edge_index is in (i, j) row-major order (dense_to_sparse order).
 * replaces: the dense-matrix Python loops of src/datasets/ba_2motifs_dual.py:35-62.
 * Step 1, gsat_und_edges: sorted_keys uint64[E] (src*N+dst ascending), rowptr int32[N+1] over that list, und_of_slot int32[E]
 *   (undirected id of every sorted slot, -1 for self loops), und_of_edge int32[E] (same by ORIGINAL edge id: maps primal edge
 *   attention onto dual nodes), und_src/und_dst int32[>= E/2 + 1, pass E] endpoints a < b of every undirected edge,
 *   status int32[4]: [0] = M (number of undirected edges), [1] = directed edges whose reverse is missing (must be 0: the rule is
 *   defined on symmetric edge sets), [2] = out-of-range ids (clamped).
 * Step 2, gsat_und_line_graph_counts: counts[i] = dual degree of dual node i (the caller scans them into dual_ptr int64[M+1]).
 * Step 3, gsat_und_line_graph: fills dual_edge_index int64[2, total], total = dual_ptr[M].
 */
size_t gsat_und_edges_workspace_bytes(int64_t num_edges);
int gsat_und_edges(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, uint64_t* sorted_keys, int32_t* rowptr,
                   int32_t* und_of_slot, int32_t* und_of_edge, int32_t* und_src, int32_t* und_dst, int32_t* status,
                   void* workspace, size_t workspace_bytes, void* stream);
int gsat_und_line_graph_counts(const int32_t* rowptr, const int32_t* und_of_slot, const int32_t* und_src, const int32_t* und_dst,
                               int64_t num_und, int64_t* counts, void* stream);
int gsat_und_line_graph(const int32_t* rowptr, const int32_t* und_of_slot, const int32_t* und_src, const int32_t* und_dst,
                        const int64_t* dual_ptr, int64_t num_und, int64_t total, int64_t* dual_edge_index, void* stream);

/* ================================ global pools / segment ops ================================ */

/*
 * out[g,:] = sum (mean != 0: mean, count clamped >= 1) of x[ptr[g]..ptr[g+1],:].
 * replaces: global_add_pool / global_mean_pool (src/models/gin.py:34,53; src/models/pna.py:47,62).
 */
int gsat_segment_pool_fwd(const float* x, const int32_t* ptr, int64_t num_segments, int64_t H,
                          int mean, float* out, void* stream);
int gsat_segment_pool_bwd(const float* dout, const int32_t* ptr, int64_t num_segments, int64_t H,
                          int mean, float* dx, void* stream);

/* ================================== explanation metrics ===================================== */

/*
 * Per-graph ranking of the edges by attention.  replaces: the per-graph host loop of get_precision_at_k
 * (src/run_gsat.py:783-791: two boolean masks over all E edges, a host argsort and an .item() per graph).
 * TOTAL ORDER (both paths): higher attention first; equal attention -> lower edge id first; -0.0 counts as +0.0.  NaN attention is
 * unsupported (its position is unspecified).  The reference's np.argsort(-att)[:k] is unstable, i.e. ambiguous under ties.
 * att fp32[E]; edge_ptr int32[G+1] / edge_order int32[E]: the edges grouped by graph (a permutation of [0, E));
 * label uint8[E] nullable (nonzero = explanation edge; required when hits is asked for); k >= 0.
 * Outputs, each nullable: order int32[E] (edge ids, graph by graph, best first: order[edge_ptr[g] + r] is the rank-r edge of graph g),
 * rank int32[E] (position of edge e inside its graph), topk uint8[E] (1 iff rank < k), hits int32[G] (labelled edges among the
 * first min(k, E_g) of graph g).
 * max_seg_edges: an upper bound of the edges of one graph, -1 = unknown.  path: 0 = auto (fused iff 0 <= max_seg_edges <=
 * gsat_rank_edges_lds_cap(), else general), 1 = fused (GSAT_ERR_ARG when the bound is unknown or above the cap: never a truncation),
 * 2 = general.  Fused: ONE launch, no workspace; graphs of <= 64 edges are sorted by one wavefront in registers, larger ones by one
 * workgroup in LDS; a graph that exceeds a wrong max_seg_edges (or whose
 * edge_ptr range is invalid) is skipped whole and gets hits = -1.  General: a stable radix sort of
 * (graph id, attention) keys plus two small launches, any graph size; workspace gsat_rank_edges_workspace_bytes(E).
 */
int64_t gsat_rank_edges_lds_cap(void);
size_t gsat_rank_edges_workspace_bytes(int64_t num_edges);
int gsat_rank_edges(const float* att, const int32_t* edge_ptr, const int32_t* edge_order, const uint8_t* label, int64_t num_edges,
                    int64_t num_graphs, int64_t k, int64_t max_seg_edges, int path, int32_t* order, int32_t* rank, uint8_t* topk,
                    int32_t* hits, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Exact, tie-aware ROC-AUC of att fp32[E] against label uint8[E] (0 / 1), as three integers: out uint64[3] = (U2, P, Nn) with
 * P / Nn the positive / negative counts and U2 = sum over positives of (2 * #negatives below + #negatives equal);
 * AUROC = U2 / (2 * P * Nn), undefined (the caller reports 0) when P * Nn == 0.  Integer sums: bitwise repeatable.
 * replaces: roc_auc_score(exp_labels, att) on host copies (src/run_gsat.py:761-763).
 */
size_t gsat_auroc_workspace_bytes(int64_t num_edges);
int gsat_auroc(const float* att, const uint8_t* label, int64_t num_edges, uint64_t* out, void* workspace, size_t workspace_bytes,
               void* stream);

/*
 * out fp32[3] = (delta_kl, mean attention of labelled edges, mean attention of unlabelled edges); a mean over no edge is 0.
 * delta_kl = sum_e p log(a / r) + (1 - p) log((1 - a) / (1 - r)), a = clamp(att, eps, 1 - eps), p = clamp(label, eps, 1 - eps),
 * r = clamp(mean(a), eps, 1 - eps); evaluated in fp64 with a fixed combine order (no float atomics: bitwise repeatable).
 * replaces: get_delta_kl and avg_signal / avg_bkg_att_weights (src/run_gsat.py:793-800, 773-774).
 */
size_t gsat_delta_kl_workspace_bytes(int64_t num_edges);
int gsat_delta_kl(const float* att, const uint8_t* label, int64_t num_edges, double eps, float* out, void* workspace,
                  size_t workspace_bytes, void* stream);

/* ==================================== evaluation scores ===================================== */

/*
 * Exact, tie-aware ROC-AUC of every column (task) of score fp32[R,T] against label fp32[R,T], both row-major.  Labels: NaN
 * (label != label) = unlabelled, skipped; 0 = negative; anything else = positive.  out uint64[T,3] = (U2, P, Nn) per task with
 * exactly the meaning gsat_auroc gives them, over the labelled rows of that task; a task without a labelled row gets (0, 0, 0).
 * Integers only: bitwise repeatable.  -0.0 == +0.0; NaN scores are unsupported (their position is unspecified; memory-safe).
 * One stable radix sort of (task | score bits) keys over 32 + bits(T) bits with the unlabelled entries under a sentinel task, one
 * scan of the negatives, the tasks' segment bounds and one integer pass (64-bit integer atomics: order independent).  Kernels only,
 * capturable; workspace gsat_auroc_tasks_workspace_bytes(R, T).  Any R, T >= 0 with R * T < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).
 * replaces: the ogb Evaluator's rocauc on host copies (src/run_gsat.py:756-759, src/pretrain_clf.py:104), which is the mean of
 * U2 / (2 P Nn) over the tasks with P > 0 and Nn > 0.
 */
size_t gsat_auroc_tasks_workspace_bytes(int64_t num_rows, int64_t num_tasks);
int gsat_auroc_tasks(const float* score, const float* label, int64_t num_rows, int64_t num_tasks, uint64_t* out, void* workspace,
                     size_t workspace_bytes, void* stream);

/*
 * Two-class histogram of att fp32[E]: hist uint64[2,bins] (row 0 = label 0 / background, row 1 = label nonzero / signal) and
 * outside uint64[2] are ADDED TO, never overwritten: the caller zeroes them once and accumulates batch after batch.
 * label uint8[E], nullable: then every entry is class 0.  1 <= bins <= 4096, lo < hi (GSAT_ERR_ARG otherwise).
 * The bin is part of the contract (fp64, no contraction): t = ((double)a - lo) * ((double)bins / (hi - lo)),
 * bin = min((int)floor(t), bins - 1) -- a == hi lands in the closed last bin, like numpy's; a < lo, a > hi or NaN is not binned
 * and adds 1 to outside[class].  -0.0 is 0.
 * Per-workgroup uint32 counters in LDS (<= 32 KiB), lanes of a wavefront with equal counters combined before the LDS atomic, non-zero
 * counters flushed with 64-bit global integer atomics: no float atomics, the result does not depend on any order.  One launch, no
 * workspace, capturable.  E < 2^40 (GSAT_ERR_UNSUPPORTED otherwise).
 * replaces: the host arrays behind add_histogram(bkg / signal_att_weights) and add_pr_curve (src/run_gsat.py:764-776).
 */
int gsat_att_histogram(const float* att, const uint8_t* label, int64_t num_edges, int64_t bins, double lo, double hi, uint64_t* hist,
                       uint64_t* outside, void* stream);

/* ================================== explanation subgraphs =================================== */

/*
 * Order-preserving extraction of a subgraph of a collated batch, with node relabelling.  replaces: the host-side
 * subgraph(node_subset.cpu(), data.edge_index.cpu(), ...) of example/trainer.py:140-170.
 * Inputs: edge_index int64[2,E]; N nodes; batch int64[N] (nullable: then no new_batch); node_ptr int32[G+1] (nullable: then no
 * new_node_ptr); keep uint8 (nonzero = keep) and mode:
 *   mode 0 (edge mode): keep has E entries.  drop_isolated != 0: the kept nodes are the endpoints of the kept edges;
 *                       drop_isolated == 0: every node is kept.
 *   mode 1 (node mode): keep has N entries; an edge is kept iff both endpoints are kept (PyG subgraph(..., relabel_nodes=True)).
 * Kept items stay in their original relative order, so every output is unique:
 *   node_id int64[cap_nodes]          old ids of the kept nodes, ascending
 *   edge_id int64[cap_edges]          old ids of the kept edges, ascending
 *   new_edge_index int64[2,cap_edges] endpoints relabelled by the rank of the node among the kept nodes (row stride cap_edges)
 *   new_batch int64[cap_nodes]        batch[node_id]
 *   new_node_ptr int32[G+1]           the exclusive scan of the kept nodes read at the old node_ptr: a graph that lost every node
 *                                     becomes an empty segment, G does not change
 *   edge_mask uint8[E]                required when E > 0: 0 / 1 per old edge, 1 iff the edge is kept (edge mode: the normalised
 *                                     input); also the flag array the output phase reads
 *   counts int64[4]                   (N', E', overflow flag, bad-id flag)
 * Capacities (<= N / E): nothing is ever written at or beyond cap_nodes / cap_edges entries; entries between a smaller true count and
 * the capacity are filled with id 0 (valid ids, never uninitialised memory, for the gathers that follow).  exact != 0: the overflow flag is set when
 * N' != cap_nodes or E' != cap_edges; exact == 0: when N' > cap_nodes or E' > cap_edges.  An edge with a node id outside [0, N) sets the
 * bad-id flag, is dropped (edge_mask 0) and its ids are never dereferenced.
 * phases: 1 = count only (flags, edge_mask and counts; capacities may be -1 = not declared), 2 = outputs only, from the flags a
 * phase-1 call left in the SAME workspace and edge_mask, 3 = both.  A caller that reads counts between 1 and 2 can size its outputs
 * exactly; a caller that knows the sizes passes 3 with exact = 1 and never reads anything back (capturable).
 * Launches: 4 (6 in edge mode with drop_isolated: the endpoint marks need a cleared array and a pass of their own), independent of
 * G, N, E; kernels only, no memset / memcpy nodes.  Two-level scan over workgroups of gsat_subgraph_block_items() items, no
 * inter-workgroup waiting; the endpoint marks are byte stores of 1 that race only with identical values.  N, E, G < 2^31
 * (GSAT_ERR_UNSUPPORTED otherwise).  workspace: gsat_subgraph_workspace_bytes(N, E).
 */
int64_t gsat_subgraph_block_items(void);
size_t gsat_subgraph_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int gsat_subgraph_index(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, const int64_t* batch, const int32_t* node_ptr,
                        int64_t num_graphs, const uint8_t* keep, int mode, int drop_isolated, int phases, int64_t cap_nodes,
                        int64_t cap_edges, int exact, int64_t* node_id, int64_t* edge_id, int64_t* new_edge_index, int64_t* new_batch,
                        int32_t* new_node_ptr, uint8_t* edge_mask, int64_t* counts, void* workspace, size_t workspace_bytes,
                        void* stream);

/*
 * gsat_subgraph_index into outputs of a fixed CAPACITY (cap_nodes, cap_edges), independent of the input's shape: the result is a
 * padded batch in the layout of gsat_collate_padded and no size is ever needed on the host.  mode / drop_isolated / keep, the order,
 * the relabelling and the bad-id rule are those of gsat_subgraph_index.
 * valid_in int32[4] (nullable): the valid word (N_real, E_real, graphs, overflow) of a padded input.  Node rows >= valid_in[0] and
 * edge slots >= valid_in[1] are never kept, in every mode (drop_isolated == 0 keeps every REAL node), and keep is not read there; an
 * edge slot below valid_in[1] with an endpoint outside [0, valid_in[0]) is a bad id.  pad_graph: the graph id of the padding nodes --
 * num_graphs - 1 of a padded input, G for an unpadded input of G graphs (the result then has G + 1 graphs).
 * Outputs: node_id int64[cap_nodes], edge_id int64[cap_edges], new_edge_index int64[2, cap_edges], new_batch int64[cap_nodes]
 * (nullable together with batch), edge_mask uint8[E] (0 in the slots that are not counted), valid_out int32[4].
 *   rows < N', slots < E'   what gsat_subgraph_index writes
 *   rows >= N'              padding nodes: new_batch = pad_graph, node_id = -1
 *   slots >= E'             padding edges, edge_id = -1, by the rule of gsat_collate_padded with N = N', E = E', n_pad = cap_nodes - N',
 *                           e_pad = cap_edges - E' (one __device__ function serves both kernels)
 *   valid_out               (N', E', g, 0) with g = valid_in[2], or G without valid_in
 * Overflow -- N' + 2 > cap_nodes, E' > cap_edges, valid_in[3] != 0 or a bad id: valid_out = (0, 0, 0, 1) and every row and slot is
 * padding.  Nothing is ever written out of bounds.
 * Launches: 5 (7 in edge mode with drop_isolated), independent of G, N, E; kernels only, no memset / memcpy nodes, nothing read back
 * (capturable).  N, E, G, the capacities < 2^31 (GSAT_ERR_UNSUPPORTED otherwise); cap_nodes >= 2.
 * workspace: gsat_subgraph_workspace_bytes(N, E).
 */
int gsat_subgraph_padded(const int64_t* edge_index, int64_t num_edges, int64_t num_nodes, const int64_t* batch, int64_t num_graphs,
                         const uint8_t* keep, int mode, int drop_isolated, const int32_t* valid_in, int64_t pad_graph, int64_t cap_nodes,
                         int64_t cap_edges, int64_t* node_id, int64_t* edge_id, int64_t* new_edge_index, int64_t* new_batch,
                         uint8_t* edge_mask, int32_t* valid_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * out[i,:] = table[index[i],:] for n rows of row_bytes >= 1 bytes each, any dtype (both row-major, contiguous).  16-byte lanes when
 * row_bytes, table and out are all 16-byte aligned, otherwise 8-, 4- or 1-byte lanes from the actual alignment.  The indices are
 * trusted (they come from gsat_subgraph_index).
 */
int gsat_gather_rows(const void* table, const int64_t* index, int64_t n, int64_t row_bytes, void* out, void* stream);

/* ================================= evaluation epoch log ===================================== */

/*
 * Appends one batch to a device-resident log of an evaluation epoch, at the offsets held in log_state int64[4] = (edges logged,
 * graphs logged, batches logged, flags) ON THE DEVICE; nothing is read back and the launch geometry depends on the capacities only
 * (capturable, kernels only).
 * The batch: att fp32[edge_cap] and label uint8[edge_cap] by edge id; edge_ptr int32[graph_cap + 1] / edge_order int32[edge_cap], the
 * edges grouped by graph with ascending edge ids inside a graph (gsat_build_csr over the edges' graph ids); logits
 * fp32[graph_cap, logit_cols] and y fp32[graph_cap, y_cols] (NaN = unlabelled, kept); valid int32[4] = (N_real, E_real, B, overflow)
 * of gsat_collate_padded, nullable: without it all graph_cap graphs are logged, with it the first B; losses fp32[3], nullable.
 * With G graphs and E = edge_ptr[G] edges to log and (e0, g0, b0) the counts in log_state:
 *   log_att[e0 + i], log_label[e0 + i] (0 / 1)   = att / label of edge edge_order[i], i < E
 *   log_graph_edge_ptr[g0 + g]                   = e0 + edge_ptr[g], 0 <= g <= G (entry g0 is only written when g0 == 0)
 *   log_logits / log_y rows g0 .. g0 + G - 1     = the first G rows
 *   log_batch_edge_ptr[b0 + 1] = e0 + E          (entry 0 = 0 is written by the first append)
 *   log_loss_sums double[3]                      += losses, or turn NaN when losses is null
 * and then log_state = (e0 + E, g0 + G, b0 + 1, flags) by a second launch that the stream orders after the copies, so entries below
 * the counts never change again.  A batch whose valid[3] is set appends nothing and sets flag bit 0; a batch that would exceed max_edges,
 * max_graphs or max_batches (or whose counts are not within its own capacities) appends nothing and sets flag bit 1.  Nothing is ever
 * written beyond the max_* entries.  Destination offsets are arbitrary: every store has element width.  max_edges < 2^31
 * (GSAT_ERR_UNSUPPORTED otherwise).
 * replaces: the host lists all_exp_labels / all_att / all_clf_labels / all_clf_logits of dual_run_one_epoch (src/run_gsat.py:646-668).
 */
int gsat_eval_log_append(const float* att, const uint8_t* label, const int32_t* edge_ptr, const int32_t* edge_order, const float* logits,
                         const float* y, const int32_t* valid, const float* losses, int64_t edge_cap, int64_t graph_cap,
                         int64_t logit_cols, int64_t y_cols, float* log_att, uint8_t* log_label, int32_t* log_graph_edge_ptr,
                         float* log_logits, float* log_y, int64_t* log_batch_edge_ptr, double* log_loss_sums, int64_t* log_state,
                         int64_t max_edges, int64_t max_graphs, int64_t max_batches, void* stream);

/*
 * out fp32[S,3]: row s is the gsat_delta_kl triple of att[seg_ptr[s] : seg_ptr[s+1]] (seg_ptr int64[S+1], non-decreasing, inside
 * [0, num_edges]); every segment has its own r = clamp(mean(clamp(a))).  An empty segment gives (0, 0, 0) like gsat_delta_kl for E = 0.
 * max_seg_len bounds the longest segment (num_edges always does); a segment above it, or bounds that are out of order, give a NaN
 * row -- never a partial evaluation.  A segment is cut into chunks of gsat_delta_kl_segments_chunk() entries, one workgroup per chunk of
 * one segment (grid: chunks of max_seg_len x S); chunk sums are added in index order, in fp64, without float atomics: bitwise
 * repeatable, and within summation-order rounding of gsat_delta_kl on the segment alone.  S = 0 is a no-op.  S <= 65535.
 * workspace: gsat_delta_kl_segments_workspace_bytes(S, max_seg_len).  Kernels only, capturable.
 * replaces: the per-batch get_delta_kl of dual_run_one_epoch (src/run_gsat.py:664), for all batches of an epoch at once.
 */
int64_t gsat_delta_kl_segments_chunk(void);
size_t gsat_delta_kl_segments_workspace_bytes(int64_t num_segments, int64_t max_seg_len);
int gsat_delta_kl_segments(const float* att, const uint8_t* label, const int64_t* seg_ptr, int64_t num_segments, int64_t num_edges,
                           int64_t max_seg_len, double eps, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ================================= classifier epoch log ===================================== */

/*
 * Appends one batch to a device-resident log of a classifier epoch, at the offsets held in log_state int64[4] = (graphs logged,
 * batches logged, flags, 0) ON THE DEVICE; two launches (the copies, then one thread that commits), nothing read back, no memset,
 * launch geometry from graph_cap only (capturable, kernels only).
 * The batch: logits fp32[graph_cap, logit_cols] and y fp32[graph_cap, y_cols] (NaN = unlabelled, kept); valid int32[4] = (N_real,
 * E_real, B, overflow) of gsat_collate_padded, nullable: without it all graph_cap rows are logged, with it the first B = valid[2];
 * rows at or beyond the count are never loaded; loss fp32[1], nullable.  With (g0, b0) the counts in log_state:
 *   log_logits / log_y rows g0 .. g0 + B - 1 = the first B rows
 *   log_loss_sum double[1]                   += loss[0], or turns NaN when loss is null
 * and then log_state = (g0 + B, b0 + 1, flags, 0).  B = 0 is a legal append: a batch with no rows.  A batch whose valid[3] is set
 * appends nothing and sets flag bit 0; a count outside [0, graph_cap], or an append that would exceed max_graphs or max_batches,
 * appends nothing and sets flag bit 1.  A flagged append writes nothing but its flag.  max_graphs < 2^31 (GSAT_ERR_UNSUPPORTED).
 * replaces: the host lists all_clf_labels / all_clf_logits / all_loss of run_one_epoch (src/pretrain_clf.py:75-91).
 */
int gsat_clf_log_append(const float* logits, const float* y, const int32_t* valid, const float* loss, int64_t graph_cap,
                        int64_t logit_cols, int64_t y_cols, float* log_logits, float* log_y, double* log_loss_sum, int64_t* log_state,
                        int64_t max_graphs, int64_t max_batches, void* stream);

/*
 * out int64[gsat_clf_log_counts_words(logit_cols, y_cols, mode)]: integer counts over the first clamp(log_state[0], 0, max_graphs)
 * logged rows, read in the kernel; the grid is sized from max_graphs.  The call zeroes out itself (a launch ahead of the counting
 * one).  Comparisons only, 64-bit integer atomics: order independent, bitwise repeatable.  mode as in gsat_criterion_fwd:
 *   0 binary, logit_cols == y_cols == 1: the predicted class is z > 0;
 *   1 multi-class, C = logit_cols in [2, 32], y_cols == 1: the predicted class is the argmax, the LOWEST index on ties;
 *   2 multi-label, T = logit_cols == y_cols in [1, 256]: the prediction of every (row, task) entry is z > 0 (a NaN logit predicts 0).
 * modes 0 and 1: out = confusion[C][C] (C = 2 in mode 0; row = label, column = prediction), then one counter `bad`: the rows whose
 * label is not an integer in [0, C) or whose logits hold a NaN; they match nothing, as in torch's preds == labels.
 * mode 2: out = [T][5]: per task (tn, fp, fn, tp) over its labelled entries (label 0 = negative, anything else positive) and the
 * number of its unlabelled (NaN) entries.
 * More classes or tasks: GSAT_ERR_UNSUPPORTED (and gsat_clf_log_counts_words gives -1, as for columns a mode does not take).
 * z > 0 differs from get_preds's sigmoid(z) > 0.5 only where the fp32 sigmoid rounds to exactly 0.5 for z > 0: z below about 1e-7.
 * replaces: get_preds and the accuracy of eval_one_batch / get_eval_score (src/pretrain_clf.py:93-100).
 */
int64_t gsat_clf_log_counts_words(int64_t logit_cols, int64_t y_cols, int mode);
int gsat_clf_log_counts(const float* log_logits, const float* log_y, const int64_t* log_state, int64_t max_graphs, int64_t logit_cols,
                        int64_t y_cols, int mode, int64_t* out, void* stream);

/* ================================= explanation fidelity log ================================= */

/*
 * Appends one batch to a device-resident log of explanation fidelity, at the offset held in log_state int64[4] = (graphs logged,
 * batches logged, flags, 0) ON THE DEVICE; two launches (the rows, then one thread that advances log_state), nothing read back, launch
 * geometry from graph_rows only (capturable, kernels only).
 * logits_full / logits_keep / logits_drop fp32[graph_rows, classes], classes >= 1: the backbone on the full graph, on the explanation
 * alone and on the graph without the explanation.  valid int32[4] (nullable) = (N_real, E_real, B, overflow) of a padded batch: with it
 * g = clamp(valid[2], 0, graph_rows) rows are logged, without it all graph_rows; rows >= g are never loaded.
 * Per graph i < g, at slot g0 + i:
 *   log_cls int32[max_graphs, 3]   the classes predicted from the three blocks
 *   log_p  double[max_graphs, 3]   the probability, under each block, of the class predicted from logits_full
 * classes == 1: class = (z >= 0), p = sigmoid(+z) for class 1 and sigmoid(-z) for class 0.  classes > 1: argmax with the lowest index on
 * ties, softmax with the row maximum subtracted, evaluated in fp64 from the fp32 logits.  NaN logits are unsupported.
 * A batch whose valid[3] is set appends nothing and sets flag bit 0; a batch that would exceed max_graphs appends nothing and sets flag
 * bit 1.  max_graphs, graph_rows < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).
 * replaces: nothing in the reference -- the host loop of example/trainer.py:140-170 stops at the extracted subgraph.
 */
int gsat_fidelity_append(const float* logits_full, const float* logits_keep, const float* logits_drop, int64_t graph_rows, int64_t classes,
                         const int32_t* valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs, void* stream);

/*
 * One launch of one workgroup: out int64[10] = (graphs, batches, flags, #(cls_drop != cls_full), #(cls_keep != cls_full)) and the bit
 * patterns of five doubles -- the sums over the logged graphs of p_full - p_drop, p_full - p_keep, p_full, p_keep, p_drop.  fp64 sums in
 * a fixed order, no float atomics: bitwise repeatable.  The caller reads out once and divides by the count.
 */
int gsat_fidelity_reduce(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t* out,
                         void* stream);

/* log_state = (0, 0, 0, 0), by a kernel (no memset node). */
int gsat_fidelity_reset(int64_t* log_state, void* stream);

/* ================================= fidelity curves: the stacked batch ======================== */

/*
 * The sparsity levels of a fidelity curve from ONE ranking.  rank int32[E] (gsat_rank_edges: position of an edge inside its graph),
 * edge_ptr int32[G + 1] and edge_graph int32[E] (the graph of every edge) on the device; ks int64[levels] OR ratios double[levels] in
 * HOST memory, exactly one of them, strictly increasing, ks >= 1, ratios in (0, 1], 1 <= levels <= 16 (GSAT_ERR_ARG otherwise).
 * Level s keeps, per graph of E_g edges, the edges with rank < min(k_s, E_g), or rank < ceil((double)E_g * ratio_s) evaluated in fp64
 * without contraction.  level uint8[E] = the smallest s that keeps the edge, `levels` when none does -- so `level <= s` is the top-k_s
 * (top-ratio_s) mask, bit for bit.  An edge whose graph id is outside [0, G) -- the padding graph of a padded batch when G counts the
 * ranked graphs -- gets `levels`, and its rank is not read.  One launch, capturable.  E, G < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).
 */
int gsat_fidelity_levels(const int32_t* rank, const int32_t* edge_ptr, const int32_t* edge_graph, int64_t E, int64_t G, const int64_t* ks,
                         const double* ratios, int64_t levels, uint8_t* level, void* stream);

/*
 * The V = 2 * levels + 1 padded extractions of a fidelity curve, side by side in one batch: variant 0 is the batch itself, variant
 * 1 + s keeps the edges with level <= s, variant 1 + levels + s keeps those with level > s; every node is kept in every variant.
 * Input: edge_index int64[2, E], batch int64[N], valid_in int32[4] (nullable; N_real, E_real, graphs, overflow of a padded batch --
 * rows and slots at or beyond its counts are never read), level uint8[E] (values above `levels` count as `levels`), G the number of
 * real graphs of an input without valid_in.
 * Variant v owns the node rows [v * cap_nodes, (v + 1) * cap_nodes), cap_nodes >= max(N, 2), the graph ids [v * graphs_per_variant,
 * (v + 1) * graphs_per_variant) with the padding graph last, and the edge slots [segment_offsets[v], segment_offsets[v + 1]);
 * segment_offsets int64[V + 1] in HOST memory, starting at 0, non-decreasing; E_stack = segment_offsets[V].  Inside its segment a
 * variant holds what gsat_subgraph_padded (edge mode, every node kept) gives for its mask at the capacity (cap_nodes, segment length),
 * with node ids moved by v * cap_nodes:
 *   out_edge_index int64[2, E_stack], out_edge_id int64[E_stack]   kept edges in their order and their slots in the input, then the
 *                                                                   slack as padding edges among the variant's padding nodes, id -1
 *   out_batch int64[V * cap_nodes]   v * graphs_per_variant + batch[i] for the variant's real rows -- every row when valid_in is given
 *                                    and cap_nodes == N, where gsat_subgraph_padded's caller shares the input's rows --, the variant's
 *                                    padding graph for the rest
 *   valid_out int32[V, 4]            (N_real, kept edges, graphs, 0)
 * A variant that does not fit (N_real + 2 > cap_nodes, more kept edges than its segment), an input whose valid_in[3] is set or an edge
 * with a node id outside [0, N_real) -- then every variant -- is all padding with (0, 0, 0, 1).  Nothing is written out of bounds.
 * 4 launches whatever `levels` is (per-workgroup counts per level bin; one workgroup scans them; scatter; fill), kernels only, no
 * atomics, nothing read back: capturable and bitwise repeatable.  Each workgroup owns gsat_fidelity_stack_block_items() edge slots.
 * workspace: gsat_fidelity_stack_workspace_bytes(E, levels).  Every extent, V * cap_nodes and V * graphs_per_variant < 2^31
 * (GSAT_ERR_UNSUPPORTED otherwise).
 * replaces: 2 * levels calls of gsat_subgraph_padded (5 launches each) and as many backbone forwards by one stacked forward.
 */
int64_t gsat_fidelity_stack_block_items(void);
size_t gsat_fidelity_stack_workspace_bytes(int64_t E, int64_t levels);
int gsat_fidelity_stack(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                        const uint8_t* level, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes, const int64_t* segment_offsets,
                        int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_batch, int32_t* valid_out, void* workspace,
                        size_t workspace_bytes, void* stream);

/*
 * gsat_fidelity_append with a level axis.  logits fp32[V * graphs_per_variant, classes], V = 2 * levels + 1: the backbone on a stacked
 * batch, block v being variant v.  valid int32[4] (nullable): the input batch's word; stack_valid int32[V, 4]: the stack's.  The graph
 * count g is clamp(valid[2], 0, graphs_per_variant), without valid the full variant's stack_valid[0][2].  log_state int64[20] =
 * (graphs, batches, flags, real edges, kept edges of level 0 .. 15).  Two launches: the rows, then one thread that advances log_state.
 * Per graph i < g at slot g0 + i, with c = the class of row i of block 0:
 *   log_cls int32[max_graphs, V]   the class predicted from every block
 *   log_p  double[max_graphs, V]   the probability of c under every block
 * by the class and probability rules of gsat_fidelity_append.  The commit adds stack_valid[0][1] to the real edges and
 * stack_valid[1 + s][1] to the kept edges of level s.  A batch whose valid[3] or any stack_valid[v][3] is set appends nothing and sets
 * flag bit 0; one that would exceed max_graphs appends nothing and sets flag bit 1.
 */
int gsat_fidelity_curve_append(const float* logits, int64_t graphs_per_variant, int64_t classes, int64_t levels, const int32_t* valid,
                               const int32_t* stack_valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs,
                               void* stream);

/*
 * One launch of one workgroup: out int64[5 + 7 * levels] = (graphs, batches, flags, real edges), kept edges [levels], #(cls_drop_s !=
 * cls_full) [levels], #(cls_keep_s != cls_full) [levels], then the bit patterns of doubles: the sum of p_full, and [levels] each of the
 * sums of p_keep_s, p_drop_s, p_full - p_drop_s, p_full - p_keep_s.  fp64 sums in a fixed order: bitwise repeatable.
 */
int gsat_fidelity_curve_reduce(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t levels,
                               int64_t* out, void* stream);

/* log_state int64[20] = 0, by a kernel (no memset node). */
int gsat_fidelity_curve_reset(int64_t* log_state, void* stream);

/*
 * gsat_fidelity_curve_append for a multi-label head: logits fp32[V * graphs_per_variant, tasks], and every (graph, task) is a binary
 * decision of its own -- class z >= 0, probability sigmoid(+-z), the one-logit rules of gsat_fidelity_append.  valid, stack_valid, the
 * graph count g, log_state int64[20] (log_state[0] counts GRAPHS), the two-launch shape, the commit and the flag rules are those of
 * gsat_fidelity_curve_append.  Per graph i < g at slot g0 + i and task t, with c = the class of logits[i][t] in block 0:
 *   log_cls int32[max_graphs, tasks, V]   the class of entry t predicted from every block
 *   log_p  double[max_graphs, tasks, V]   the probability of c under every block
 * One thread per (graph, task), the task running fastest; rows at or beyond g are never loaded.  With tasks = 1 the log is, bit for bit,
 * that of gsat_fidelity_curve_append with classes = 1.  1 <= tasks <= 1024 (the criterion's limit) and levels <= 16;
 * graphs_per_variant * tasks * V or max_graphs * tasks * V at or above 2^31: GSAT_ERR_UNSUPPORTED.
 */
int gsat_fidelity_curve_append_tasks(const float* logits, int64_t graphs_per_variant, int64_t tasks, int64_t levels, const int32_t* valid,
                                     const int32_t* stack_valid, int32_t* log_cls, double* log_p, int64_t* log_state, int64_t max_graphs,
                                     void* stream);

/*
 * One launch of `tasks` workgroups of 256 threads, workgroup t for task t: thread k adds graphs k, k + 256, ... in that order in fp64,
 * then a fixed-order sum over the workgroup.  No atomics: bitwise repeatable, and with tasks = 1 the sums of gsat_fidelity_curve_reduce
 * bit for bit.  With S = levels, T = tasks, A = 4 + S and D = A + 2 T S, out int64[4 + S + T (1 + 6 S)] is
 *   out[0 .. 3]                    graphs, batches, flags, real edges
 *   out[4 + s]                     kept edges of level s
 *   out[A + (0 T + t) S + s]       #(cls_drop_s != cls_full) of task t
 *   out[A + (1 T + t) S + s]       #(cls_keep_s != cls_full) of task t
 *   out[D + t]                     the bit pattern of a double: the sum of p_full of task t
 *   out[D + T + (k T + t) S + s]   bit patterns, k = 0 .. 3: the sums of p_keep_s, p_drop_s, p_full - p_drop_s, p_full - p_keep_s of task t
 */
int gsat_fidelity_curve_reduce_tasks(const int32_t* log_cls, const double* log_p, const int64_t* log_state, int64_t max_graphs, int64_t levels,
                                     int64_t tasks, int64_t* out, void* stream);

/*
 * gsat_fidelity_stack for `rankings` explanations of the same edges around ONE full variant: level uint8[rankings, E], row r being what
 * gsat_fidelity_levels writes for ranking r with the same `levels`.  rankings, levels >= 1 and rankings * levels <= 16 (GSAT_ERR_ARG
 * otherwise).  With R = rankings and S = levels there are V = 1 + 2 R S variants:
 *   v = 0                      the batch itself
 *   v = 1 + r S + s            the edges with level[r][e] <= s
 *   v = 1 + R S + r S + s      the edges with level[r][e] > s
 * so gsat_fidelity_curve_append / _reduce called with levels = R S hold ranking r, level s at their flat level r S + s.  Every other
 * argument, the guards, the overflow rule and the outputs are gsat_fidelity_stack's with this V: segment_offsets int64[V + 1] in HOST
 * memory, valid_out int32[V, 4], out_batch int64[V * cap_nodes].  The segment of a variant of ranking r holds, bit for bit, what
 * gsat_fidelity_stack writes for level row r alone at the same segment length and cap_nodes; only the node-id and graph-id offsets
 * follow the new variant index.  An overflowing variant is all padding alone; valid_in[3] or a node id out of range makes every variant
 * all padding.  4 launches whatever R and S are (per-workgroup counts over the R (S + 1) bins, one scan workgroup, scatter, fill), no
 * atomics, nothing read back: capturable and bitwise repeatable.  A thread loads the endpoints of its edge slots once and each of
 * their R level bytes once.  workspace: gsat_fidelity_stack_multi_workspace_bytes(E, rankings, levels) (0 for arguments out of range).
 * replaces: R calls of gsat_fidelity_stack and R stacked backbone forwards (each with its own copy of the batch) by one.
 */
size_t gsat_fidelity_stack_multi_workspace_bytes(int64_t E, int64_t rankings, int64_t levels);
int gsat_fidelity_stack_multi(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                              const uint8_t* level, int64_t rankings, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes,
                              const int64_t* segment_offsets, int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_batch,
                              int32_t* valid_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Agreement of two rankings of the same edges, level by level.  level_a, level_b uint8[E] (gsat_fidelity_levels with the same
 * `levels`, 1 .. 16); valid int32[4] (nullable): the first clamp(valid[1], 0, E) entries count -- none when valid[3] is set -- and the
 * others are never loaded; without it all E.  ADDS into acc int64[levels, 3], per level s:
 *   acc[s][0] += #(a <= s and b <= s)    acc[s][1] += #(a <= s)    acc[s][2] += #(b <= s)
 * An entry whose level is `levels` or above (in no level: the padding graph, or below every cut) is in none of the counts.  One
 * launch: per-workgroup LDS counts, then one int64 atomicAdd per bin and workgroup -- integer sums, so the result does not depend on
 * the order and is repeatable.  Capturable.  Jaccard of level s = acc[s][0] / (acc[s][1] + acc[s][2] - acc[s][0]), overlap
 * coefficient = acc[s][0] / min(acc[s][1], acc[s][2]).  E < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).
 */
int gsat_level_overlap(const uint8_t* level_a, const uint8_t* level_b, int64_t E, int64_t levels, const int32_t* valid, int64_t* acc,
                       void* stream);

/* acc int64[levels, 3] = 0, by a kernel (no memset node). */
int gsat_level_overlap_reset(int64_t* acc, int64_t levels, void* stream);

/*
 * gsat_fidelity_stack over NODES: the V = 2 * levels + 1 padded node-induced extractions of a fidelity curve side by side.  node_level
 * uint8[N] is what gsat_fidelity_levels writes for a ranking of the nodes inside their graphs (values above `levels` count as
 * `levels`).  Variant 0 keeps every real node, variant 1 + s the real nodes with level <= s, variant 1 + levels + s those with level > s.
 * A row at or beyond valid_in[0] is never kept and its level byte is never read; an edge slot at or beyond valid_in[1] is never read.
 * Variant v owns the node rows [v * cap_nodes, (v + 1) * cap_nodes), the graph ids [v * graphs_per_variant, (v + 1) *
 * graphs_per_variant) with the padding graph last, and the edge slots [segment_offsets[v], segment_offsets[v + 1]); segment_offsets
 * int64[V + 1] in HOST memory, starting at 0, non-decreasing; E_stack = segment_offsets[V].  Inside them it holds, bit for bit, what
 * gsat_subgraph_padded writes with mode = 1, drop_isolated = 0, the variant's keep mask, the same valid_in, pad_graph =
 * graphs_per_variant - 1 and the capacity (cap_nodes, segment length) -- the node ids of out_edge_index moved by v * cap_nodes and
 * out_batch by v * graphs_per_variant:
 *   out_node_id int64[V * cap_nodes]  kept nodes in ascending old order, -1 for padding rows
 *   out_batch int64[V * cap_nodes]    the graph of every kept node, the variant's padding graph for the rest
 *   out_edge_index int64[2, E_stack], out_edge_id int64[E_stack]   the edges with BOTH ends kept, in their order, relabelled, and their
 *                                     slots in the input; then the slack as padding edges among the variant's padding nodes, id -1
 *   valid_out int32[V, 4]             (N'_v, E'_v, graphs, 0)
 * An isolated kept node stays; a graph that lost every node is an empty segment.  Overflow is PER VARIANT (N'_v differs): a variant with
 * N'_v + 2 > cap_nodes or more kept edges than its segment is all padding with (0, 0, 0, 1) and the others stand; valid_in[3] != 0 or
 * a counted edge with an endpoint outside [0, N_real) makes every variant all padding.  Nothing is written out of bounds.
 * 5 launches whatever `levels` is (per-workgroup counts of the nodes' bins and of the edges' max / min endpoint bins; one workgroup
 * scans them; node scatter with a per-node prefix table int32[N, levels + 1] in the workspace; edge scatter; fill), kernels only, no
 * atomics, nothing read back: capturable and bitwise repeatable.  Each workgroup owns gsat_fidelity_stack_block_items() node rows or
 * edge slots.  1 <= levels <= 16 and cap_nodes >= 2 (GSAT_ERR_ARG otherwise); every extent, V * cap_nodes and V * graphs_per_variant
 * < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).  workspace: gsat_fidelity_stack_nodes_workspace_bytes(N, E, levels) (0 for arguments out of
 * range).
 * replaces: 2 * levels calls of gsat_subgraph_padded in node mode (5 launches each) and as many backbone forwards by one stacked forward.
 */
size_t gsat_fidelity_stack_nodes_workspace_bytes(int64_t N, int64_t E, int64_t levels);
int gsat_fidelity_stack_nodes(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* batch, int64_t G, const int32_t* valid_in,
                              const uint8_t* node_level, int64_t levels, int64_t graphs_per_variant, int64_t cap_nodes,
                              const int64_t* segment_offsets, int64_t* out_edge_index, int64_t* out_edge_id, int64_t* out_node_id,
                              int64_t* out_batch, int32_t* valid_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Connectivity of explanations: the connected components of every graph's kept edges at every level of a fidelity curve.
 * edge_index int64[2, E]; node_ptr / edge_ptr int32[G' + 1] and edge_order int32[E] the nodes and the edge slots grouped by graph (the
 * batch index's, G' >= G); level uint8[E] what gsat_fidelity_levels writes with 1 <= levels <= 16: level s keeps the slots with
 * level[e] <= s, a byte of `levels` or above is in no level.  G: the graphs to look at, the first ones -- for a padded batch num_graphs - 1,
 * so that the padding graph is never touched.  valid int32[4] (nullable, a padded batch's word): only the graphs below
 * clamp(valid[2], 0, G) are looked at, none when valid[3] is set; an edge slot at or beyond clamp(valid[1], 0, E) is never loaded (neither
 * its endpoints nor its level byte) and is kept at no level.
 * Connectivity ignores direction; a self-loop joins nothing (its node is touched and its slot counts where its node's component
 * counts); duplicate and one-directional edges are fine.  The nodes touched at level s are the endpoints of its kept slots.
 *   per_graph int32[G, levels, 5] (nullable)  per graph g and level s: components among the touched nodes, kept slots, the most kept
 *                                     slots inside one component, touched nodes, the most nodes inside one component (two independent
 *                                     maxima); (0, 0, 0, 0, 0) with nothing kept
 *   acc int64[levels, 8] (nullable)   ADDED to, per looked-at graph that is not skipped: acc[s] += (1, components, kept, big_edges,
 *                                     touched, big_nodes, components == 1, 0); acc[0][7] counts the skipped graphs
 *   node_comp int32[N] (nullable)     of the LAST level: the smallest node id (batch-global) of the node's component, -1 for an
 *                                     untouched node
 *   edge_big uint8[E] (nullable)      of the LAST level: 1 iff the slot is kept and lies in its graph's component with the most kept
 *                                     slots, ties going to the component with the smaller label; 0 for every other loaded slot
 * Rows and slots of graphs that are not looked at are not written; neither are node_comp / edge_big of a skipped graph, nor edge_big of
 * a slot at or beyond valid[1].
 * max_seg_nodes: the caller's bound on the nodes of one graph.  -1 (unknown) or above gsat_level_components_lds_cap(): GSAT_ERR_ARG,
 * never a truncation.  A graph is SKIPPED WHOLE -- its per_graph rows are -1 and it adds 1 to acc[0][7] only -- when it has more nodes
 * than max_seg_nodes, when its node or slot range is not inside [0, N] / [0, E], when one of its slots names an edge outside [0, E), or
 * when a loaded slot has an endpoint outside the graph's node range; the checks run before anything is indexed with its ids.
 * ONE launch, caller-owned outputs, no workspace, nothing read back: capturable.  A wavefront takes a graph of at most
 * gsat_level_components_wave_nodes() = 64 nodes in an LDS slice of its own (no workgroup barrier in that tier), the workgroup a larger
 * one up to the cap of 4096 nodes: 13 bytes of labels, counters and marks per node plus four packed edge words per node, 116 KiB of the
 * 160 KiB LDS at the cap (slots beyond the kept words are re-read from global memory).  Labels start as the node's own id and are
 * carried from level to level (the kept sets are nested); per level, min-label hooking by LDS atomicMin along the NEW slots and pointer
 * jumping, rounds bounded by the node count; the counts are taken from LDS counters indexed by root after each level converges.  The
 * fixed point is unique, so the result is integer, exact and bitwise repeatable whatever the order of the atomics.
 * E, N, G >= 2^31: GSAT_ERR_UNSUPPORTED.
 * replaces: the attention's copy to the host and a networkx / scipy connected-components loop over graphs and levels.
 */
int64_t gsat_level_components_lds_cap(void);
int64_t gsat_level_components_wave_nodes(void);
int gsat_level_components(const int64_t* edge_index, int64_t E, int64_t N, const int32_t* node_ptr, const int32_t* edge_ptr,
                          const int32_t* edge_order, int64_t G, const uint8_t* level, int64_t levels, int64_t max_seg_nodes,
                          const int32_t* valid, int32_t* per_graph, int64_t* acc, int32_t* node_comp, uint8_t* edge_big, void* stream);

/* acc int64[levels, 8] = 0, by a kernel (no memset node). */
int gsat_level_components_reset(int64_t* acc, int64_t levels, void* stream);

/*
 * Post-hoc edge-mask explainer (PyG's GNNExplainer with edge_reduction = 'sum' for the size term and a mean for the entropy) around the
 * mask-weighted message passing.  One mask logit m per edge slot, a = sigmoid(m) is what the backbone takes as edge_atten.  The
 * objective of a batch is the sum over its real graphs of a per-graph objective, so a graph's mask does not depend on its batch:
 *   L = sum_g crit_g(z_g, t_g) + sum_e [ size_coef a_e + ent_coef H(a_e) / E_g(e) ],   H(a) = -a ln(a + 1e-15) - (1 - a) ln(1 - a + 1e-15)
 * with E_g(e) the edge count of the graph of e's source node.
 *
 * gsat_mask_init -- ONE launch over all E slots (the capacity of a padded batch), so that a captured body needs no memset:
 *   m <- init[e] (init float32[E], nullable) or init_value;  mu = nu = 0;  a = sigmoid(m);
 *   inv_eg[e] = 1 / E_g(e) from src32 int32[E], node_seg32 int32[N] (graph of every node) and edge_ptr int32[G + 1] (edge slots grouped
 *   by graph); 1 for a slot whose ids are out of range;
 *   state float32[4] = (steps taken t = 0, 1 / (1 - b1^(t + 1)), 1 / sqrt(1 - b2^(t + 1)), 0) -- the bias corrections of the NEXT step,
 *   evaluated in fp64 from the fp64 betas as torch's Adam evaluates them on the host (1 - b2^t of a b2 rounded to fp32 would be off
 *   by 1e-5 of itself in the first steps; the moments use 1 - beta rounded once from fp64).  E = 0 writes the state alone.
 *
 * gsat_mask_step -- one elementwise launch, then one single-thread launch that advances `state` (the elementwise launch only READS
 * it, so no workgroup can see a counter another one has moved: a captured step can be replayed T times).  valid int32[4] (nullable): a
 * padded batch's word (N_real, E_real, graphs, overflow); m_valid = clamp(valid[1], 0, E), b = clamp(valid[2], 0, G); without it m_valid
 * = E and b = G.  g_a float32[E] is the gradient of the project's MEAN criterion over the b graphs with respect to a; the factor b, read
 * on the device, turns it into the gradient of the per-graph sum.  For e < m_valid:
 *   G_e = a (1 - a) (b g_a[e] + size_coef + ent_coef dH/da inv_eg[e])
 *   dH/da = -ln(a + 1e-15) - a / (a + 1e-15) + ln(1 - a + 1e-15) + (1 - a) / (1 - a + 1e-15)
 *   mu = b1 mu + (1 - b1) G;  nu = b2 nu + (1 - b2) G^2;  m -= lr state[1] mu / (sqrt(nu) state[2] + eps);  a = sigmoid(m)
 * which is torch.optim.Adam without weight decay and amsgrad.  Entries at or beyond m_valid are neither loaded nor written; a batch
 * whose valid[3] is set changes nothing, the state included; E = 0 is a no-op.  A saturated logit (a = 0 or 1 in fp32) has G = 0 and
 * every term stays finite.  Four entries per thread, 16-byte accesses when the six arrays are 16-byte aligned.  No atomics: bitwise
 * repeatable.  lr > 0, betas in [0, 1), eps, size_coef, ent_coef >= 0 (GSAT_ERR_ARG otherwise).
 * replaces: sigmoid, the two regularisers and their autograd, the chain through the sigmoid and the optimiser's launches per step.
 *
 * gsat_mask_objective -- out float32[G, 2] = per graph (sum of a, mean of H(a)) over the graph's slots edge_order[edge_ptr[g] ..
 * edge_ptr[g + 1]); one wavefront per graph, lanes stride the slots, fixed-order sums; any graph size.  Graphs at or beyond b, and
 * every graph of an overflowing batch, get (0, 0); slots at or beyond m_valid are not loaded.
 *
 * gsat_segment_minmax_norm -- out[e] = (att[e]^power - min_g) / (max_g - min_g + eps) with the minimum and maximum of att^power over
 * the slots of e's graph, through edge_order (not assumed to be the identity).  power = 10, eps = 1e-6 is the rule of the
 * reference's visualize_a_graph(norm=True); power = 1 is plain min-max (no pow is evaluated).  A graph with one edge and a constant
 * graph give 0; slots of graphs at or beyond b or at or beyond m_valid get 0 without a load.  One wavefront per graph, two passes.
 * Every extent < 2^31 (GSAT_ERR_UNSUPPORTED otherwise).
 */
int gsat_mask_init(const float* init, float init_value, const int32_t* src32, const int32_t* node_seg32, const int32_t* edge_ptr, int64_t N,
                   int64_t G, int64_t E, double b1, double b2, float* m, float* mu, float* nu, float* a, float* inv_eg, float* state,
                   void* stream);
int gsat_mask_step(float* m, float* mu, float* nu, float* a, const float* g_a, const float* inv_eg, int64_t E, int64_t G,
                   const int32_t* valid, float* state, float lr, double b1, double b2, float eps, float size_coef, float ent_coef,
                   void* stream);
int gsat_mask_objective(const float* a, const int32_t* edge_ptr, const int32_t* edge_order, int64_t E, int64_t G, const int32_t* valid,
                        float* out, void* stream);
int gsat_segment_minmax_norm(const float* att, const int32_t* edge_ptr, const int32_t* edge_order, int64_t E, int64_t G, float power,
                             float eps, const int32_t* valid, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GSAT_HIP_H */
