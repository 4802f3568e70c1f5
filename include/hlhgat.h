/*
 * hlhgat.h — C-ABI of the MI355X-native (gfx950) Hodge-Laplacian
 * message-passing hot path of HL-HGAT.
 *
 * Every entry point takes plain device pointers, sizes and a HIP stream
 * (passed as void*), launches asynchronously on that stream and returns
 * HLHGAT_OK (0) or an error code; hlhgat_last_error() returns a
 * thread-local message for the last failure.  No entry point allocates
 * device memory or synchronises the stream (graph-capture safe); scratch
 * space is supplied by the caller (see the *_workspace_bytes queries).
 *
 * Layout conventions (DESIGN.md "Data layout in HBM"):
 *  - features are fp32, row-major [rows][ld] with ld >= width;
 *  - a sparse operator A (L0, L1, |B1|) is CSR with int32 rowptr[n+1],
 *    int32 col[nnz], fp32 val[nnz] (val == NULL means all ones);
 *  - a polynomial basis slab is k-major: block k is [n][F] contiguous.
 *
 * Reference interfaces replaced (paths relative to deepika090/HL-HGAT):
 *  - PyG MessagePassing.propagate + message(x_j, norm) = norm*x_j, aggr='add'
 *      lib/Hodge_Cheb_Conv.py:412,416,424,430,494,502,442-443,518-519
 *      -> hlhgat_csr_*, hlhgat_spmm, hlhgat_poly_step
 *  - HodgeLaguerreConv.forward recurrence   lib/Hodge_Cheb_Conv.py:480-515
 *  - HodgeChebConv.forward recurrence       lib/Hodge_Cheb_Conv.py:394-439
 *      -> hlhgat_poly_basis_fwd / hlhgat_poly_basis_bwd
 *  - torch_geometric Linear / nn.Linear projections (lins[k], WV_*, WQ/WK)
 *      lib/Hodge_Cheb_Conv.py:462-465,497,509,270-289,276-289
 *      -> hlhgat_proj_fwd / hlhgat_proj_bwd_data / hlhgat_proj_bwd_weight
 *  - adj2par1 + torch.sparse.mm(|B1|, .) and (|B1|^T, .)
 *      lib/Hodge_Dataset.py:169-191, lib/Hodge_Cheb_Conv.py:294-295,100-101
 *      -> hlhgat_incidence_csr, hlhgat_edge_gather2 (+ hlhgat_poly_step as
 *         the node-side segment mean)
 *  - NodeEdgeInt/MSI only_att score     lib/Hodge_Cheb_Conv.py:297-305,103-111
 *      -> hlhgat_att_score_fwd / hlhgat_att_score_bwd
 *  - torch_scatter.scatter_mean / global_mean_pool (cluster pooling, readout)
 *      lib/Hodge_Cheb_Conv.py:50-53, lib/Hodge_ST_Model.py:636
 *      -> hlhgat_segment_mean_fwd / hlhgat_segment_mean_bwd
 */
#ifndef HLHGAT_H_
#define HLHGAT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HLHGAT_OK 0
#define HLHGAT_EINVAL 1 /* bad argument (shape, alignment, null pointer) */
#define HLHGAT_EHIP 2   /* HIP runtime error */

#define HLHGAT_POLY_LAGUERRE 0 /* HodgeLaguerreConv recurrence */
#define HLHGAT_POLY_CHEB 1     /* HodgeChebConv recurrence */
/* HL-HGAT-DEMO HodgeLaguerreFastConv as published: its k >= 2 terms
 * propagate the layer input x instead of Tx_1
 * (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:561); needed to reproduce outputs of
 * models trained with it (HL-HGAT-DEMO/weights/HL_HGAT_Brain.pt). */
#define HLHGAT_POLY_LAGUERRE_DEMO 2

#define HLHGAT_SIGMA_SIGMOID 0 /* nn.Sigmoid (NodeEdgeInt default) */
#define HLHGAT_SIGMA_RELU 1    /* nn.ReLU (attpool heads) */

/* ---- library ---------------------------------------------------------- */
int hlhgat_version(void);
const char* hlhgat_last_error(void);

/* ---- CSR construction ------------------------------------------------- */
/* Scratch bytes needed by hlhgat_csr_from_coo for nnz entries. */
size_t hlhgat_csr_workspace_bytes(int64_t nnz);

/* COO (row[e], col[e], w[e]) -> CSR keyed by row.  Entries are ordered by
 * (row, col) exactly as torch.sparse coalesce orders them, duplicates kept
 * (propagate sums duplicates, so does the SpMM).  w may be NULL (val NULL).
 * Rows/cols are int64 (PyG edge_index); both must lie in [0,n_rows) and
 * [0,n_cols).  `perm` (optional, int32[nnz]) receives the source entry of
 * each CSR slot.  Replaces the gather/scatter set-up of PyG propagate
 * (lib/Hodge_Cheb_Conv.py:494,502) and the coalesce inside torch.sparse.mm
 * (lib/Hodge_Cheb_Conv.py:294-295). */
int hlhgat_csr_from_coo(const int64_t* row, const int64_t* col, const float* w,
                        int64_t nnz, int64_t n_rows, int64_t n_cols,
                        int32_t* rowptr, int32_t* col_out, float* val_out,
                        int32_t* perm, void* workspace, size_t workspace_bytes,
                        void* stream);

/* Fast path for COO already sorted by (row, col) — e.g. dense_to_sparse output
 * of the Hodge builder (lib/Hodge_Dataset.py:467-468) shifted by PairData
 * batching (lib/Hodge_Dataset.py:40-48).  Caller guarantees sortedness;
 * hlhgat_coo_check_sorted can verify it on device. */
int hlhgat_csr_from_sorted_coo(const int64_t* row, const int64_t* col,
                               const float* w, int64_t nnz, int64_t n_rows,
                               int32_t* rowptr, int32_t* col_out,
                               float* val_out, void* stream);

/* Writes 1 to *flag_dev if (row,col) is non-decreasing lexicographically and
 * every index is in range, else 0. */
int hlhgat_coo_check_sorted(const int64_t* row, const int64_t* col, int64_t nnz,
                            int64_t n_rows, int64_t n_cols, int32_t* flag_dev,
                            void* stream);

/* Incidence CSR of |B1| (adj2par1, lib/Hodge_Dataset.py:169-191): for each
 * node v, the edges e with edge_index[0][e]==v or edge_index[1][e]==v, in
 * increasing e.  edge_index is int64 [2][n_edges] (row 0 = i, row 1 = j).
 * Needs hlhgat_csr_workspace_bytes(2*n_edges) of scratch. */
int hlhgat_incidence_csr(const int64_t* edge_index, int64_t n_edges,
                         int64_t n_nodes, int32_t* rowptr, int32_t* edge_ids,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- halo tiles (LDS-staged SpMM for large Laplacians) ----------------- */
/* A tiling of a CSR operator's rows for the LDS-staged SpMM: tile t owns the
 * schedule positions [tile_ptr[t], tile_ptr[t+1]) (rows order[p], order = the
 * operator's row schedule, NULL = natural) and the distinct columns those
 * rows reference, halo[halo_ptr[t] .. halo_ptr[t+1]) (ascending).  The
 * entries are re-laid in SCHEDULE order: position p's entries are
 * [srp[p], srp[p+1]) of lcol (tile-local column = index into the tile's
 * halo) and sval (the CSR values permuted the same way; NULL = all ones).
 * One workgroup stages a tile's entries and the halo rows of X in LDS with
 * bulk coalesced loads, then every row is summed from LDS: each X row is read
 * from L2 once per tile instead of once per entry (TSP-scale L1: ~20 entries
 * per row, ~5 uses per staged row).  Per-row summation order is the CSR
 * order, so results are bitwise those of the plain SpMM.  Built on the HOST
 * by hlhgat_halo_tiles; sval on device by hlhgat_gather_f32(val, eperm). */
typedef struct hlhgat_halo {
  const int32_t* hdr;       /* [n_tiles][8] {p0, rows, halo0, n_halo, e0, n_entries, 0, 0} */
  const int32_t* tile_ptr;  /* [n_tiles+1] schedule positions */
  const int32_t* halo_ptr;  /* [n_tiles+1] offsets into halo */
  const int32_t* halo;      /* distinct columns of each tile, ascending */
  const int32_t* srp;       /* [n_rows+1] entry offsets in schedule order */
  const uint16_t* lcol;     /* [nnz] tile-local column, schedule order */
  const float* sval;        /* [nnz] values, schedule order (NULL = ones) */
  int64_t n_tiles;
  int32_t max_halo;         /* bounds of any tile (size the LDS image) */
  int32_t max_rows;
  int32_t max_nnz;
} hlhgat_halo_t;

/* HOST function (host pointers, no stream): pack consecutive rows of the
 * schedule greedily into tiles of <= max_rows rows, <= max_nnz entries and
 * <= max_halo distinct columns.  Outputs (capacities): tile_ptr, halo_ptr and
 * srp n_rows+1; halo, lcol and eperm nnz (eperm[i] = CSR entry of
 * schedule-ordered entry i); hdr 8*n_rows (per-tile header, see
 * hlhgat_halo_t).  Returns HLHGAT_EINVAL if one row alone exceeds
 * max_halo columns or max_nnz entries (use the plain SpMM then). */
int hlhgat_halo_tiles(const int32_t* rowptr, const int32_t* col, int64_t n_rows,
                      int64_t n_cols, const int32_t* order, int32_t max_rows,
                      int32_t max_nnz, int32_t max_halo, int32_t* tile_ptr,
                      int32_t* halo_ptr, int32_t* halo, int32_t* srp, uint16_t* lcol,
                      int32_t* eperm, int32_t* hdr, int64_t* n_tiles, int64_t* n_halo);

/* ---- multi-level graph coarsening (HOST functions, host pointers) --------
 * hlhgat_graclus replaces the torch_cluster 1.6.0 graclus_cluster call of
 * MLGC / MLGC_weighted (lib/Hodge_Dataset.py:252-253, :311): greedy matching
 * over edge_index [2, n_edges] (row-major: rows then cols; self-loops
 * ignored; weight NULL = all ones) visiting nodes in perm order (the
 * reference draws torch.randperm; the caller passes its permutation), each
 * unmatched node paired with the last of its unmatched neighbours (ascending
 * column order) whose weight is >= the best so far, starting from 0 (the
 * weighted branch of torch_cluster's graclus_cpu: ties to the last, zero
 * weights match); both get id min(u, v), an unpaired node keeps id u.
 * cluster: [n_nodes] out. */
int hlhgat_graclus(const int64_t* edge_index, const double* weight, int64_t n_edges,
                   int64_t n_nodes, const int64_t* perm, int64_t* cluster);
/* hlhgat_mlgc_map replaces the per-edge loop of MLGC (lib/Hodge_Dataset.py:
 * 254-275, same at :312-333): c_node[u] = rank of cluster[u] among the
 * distinct ids; c_edge[i] = +inf if edge i's ends share a coarse node, else
 * the index of coarse edge (min, max) numbered in first-seen order, written
 * to coarse_edges [2, n_edges capacity] (row 0 = min at [0..), row 1 = max
 * at [n_edges..)).  Unlike the reference's float key imax + 1e-4 * imin,
 * pairs never collide (the reference's key does once a level has > 10^4
 * coarse nodes). */
int hlhgat_mlgc_map(const int64_t* cluster, int64_t n_nodes, const int64_t* edge_index,
                    int64_t n_edges, int64_t* c_node, float* c_edge, int64_t* coarse_edges,
                    int64_t* n_coarse_nodes, int64_t* n_coarse_edges);
/* One MLGC level for a batch of graphs, the per-sample work of the
 * reference's CIFAR10SP get() (main_cifar10SP_HL_HGCNN_dense_int3_attpool.py:
 * 94-103: MLGC on every sample): per graph g, hlhgat_graclus over its i<j
 * edge list taken both ways (unit weights, node order perm) then
 * hlhgat_mlgc_map over the i<j list, the graphs spread over n_threads host
 * threads.  Indices are local to each graph: its nodes are [node_ptr[g],
 * node_ptr[g+1]) of perm / c_node, its edges [edge_ptr[g], edge_ptr[g+1]) of
 * edges ([2][E], E = edge_ptr[n_graphs]) / c_edge; its coarse edges go to
 * columns [edge_ptr[g], edge_ptr[g] + coarse_e[g]) of coarse_edges ([2][E]);
 * coarse_n[g] = its coarse node count. */
int hlhgat_mlgc_batch(int64_t n_graphs, const int64_t* node_ptr, const int64_t* edge_ptr,
                      const int64_t* edges, const int64_t* perm, int n_threads, int64_t* c_node,
                      float* c_edge, int64_t* coarse_edges, int64_t* coarse_n,
                      int64_t* coarse_e);

/* Flags of hlhgat_mlgc_prune / hlhgat_mlgc_device. */
/* the matching sees each edge from its first end only (MLGC_Weight passes
 * graclus the i<j list one way, HL-HGAT-DEMO/lib/Hodge_Dataset.py:193-194);
 * without it, both ways (MLGC / MLGC_weighted, lib/Hodge_Dataset.py:252, :311) */
#define HLHGAT_MLGC_ONE_WAY 1u
/* remove the coarse edges that exactly one fine edge supports
 * (HL-HGAT-DEMO/lib/Hodge_Dataset.py:222-230) */
#define HLHGAT_MLGC_PRUNE_SINGLE 2u
/* then remove the coarse nodes no remaining coarse edge touches
 * (HL-HGAT-DEMO/lib/Hodge_Dataset.py:234-241) */
#define HLHGAT_MLGC_DROP_ISOLATED 4u

/* HOST function.  The two pruning passes of the DEMO's MLGC_Weight
 * (HL-HGAT-DEMO/lib/Hodge_Dataset.py:222-241) on hlhgat_mlgc_map's outputs:
 * c_node_in [n_nodes] (int64 ranks), c_edge [n_edges] and coarse_edges
 * [2][n_edges capacity] in place, *n_coarse_nodes / *n_coarse_edges in and
 * out; c_node [n_nodes] out as float32 (the reference's dtype; ids stay
 * exact: n_nodes, n_edges < 2^24 is an argument check).
 * HLHGAT_MLGC_PRUNE_SINGLE: a coarse edge that exactly one fine edge maps to
 * is removed and that fine edge's c_edge becomes +inf; the remaining coarse
 * edges keep their first-seen order and are renumbered from 0, every finite
 * c_edge with them.  HLHGAT_MLGC_DROP_ISOLATED (after the pruning): a coarse
 * node that ends no remaining coarse edge is removed, the fine nodes mapped to
 * it get c_node = +inf, the other ids drop by the number of removed ids below
 * them and the coarse edges are relabelled (PyG remove_isolated_nodes).  No
 * flag: c_node = (float)c_node_in, nothing else changes.
 * The reference keys a coarse edge by the float imax + 0.0001 * imin (:207);
 * the integer pair keys used here are equivalent while a level has fewer than
 * 10^4 coarse nodes (beyond that the reference's keys collide, these do not). */
int hlhgat_mlgc_prune(int64_t n_nodes, int64_t n_edges, unsigned flags, const int64_t* c_node_in,
                      float* c_node, float* c_edge, int64_t* coarse_edges,
                      int64_t* n_coarse_nodes, int64_t* n_coarse_edges);

/* ---- multi-level graph coarsening on the device --------------------------
 * One MLGC level for a batch of graphs in ONE launch, one workgroup per
 * graph: the graclus visit loop (torch_cluster graclus_cluster as MLGC calls
 * it, lib/Hodge_Dataset.py:252-253, :311; HL-HGAT-DEMO/lib/Hodge_Dataset.py:
 * 193-194), the fine -> coarse maps (lib/Hodge_Dataset.py:254-275;
 * HL-HGAT-DEMO :195-216) and MLGC_Weight's pruning passes (HL-HGAT-DEMO
 * :222-241) -- hlhgat_mlgc_batch (+ hlhgat_mlgc_prune per graph) on device
 * pointers, bit for bit.
 * edge_index: int64 [2][n_edges], the batch's i<j list with PairData offsets
 * (global node ids); graph g's edges are [edge_ptr[g], edge_ptr[g+1]), its
 * nodes [node_ptr[g], node_ptr[g+1]).  inc_rowptr / inc_edge: the batch's
 * incidence CSR (hlhgat_incidence_csr over n_nodes) -- the neighbour lists.
 * weight: [n_edges] per edge or NULL (ones).  perm: [n_nodes], graph g's visit
 * order as LOCAL ids in its node slot.  flags: HLHGAT_MLGC_*.
 * Outputs are local to each graph, in hlhgat_mlgc_batch's layout: c_node
 * [n_nodes] and c_edge [n_edges] as float32 (+inf: a contracted or pruned
 * edge, a dropped node), graph g's coarse edges (local coarse ids) at the
 * head of its edge slot of coarse_edges [2][n_edges] (the rest of the slot is
 * unspecified), coarse_n[g] / coarse_e[g] its coarse counts.
 * Matching: nodes in perm order; an unmatched node u takes, among its
 * unmatched neighbours with weight >= 0, the largest weight and among equals
 * the largest id (with unique pairs, the host's "last neighbour in ascending
 * column order with w >= best so far"; NaN never matches); both get id
 * min(u, v); with no candidate u keeps id u.
 * Preconditions: unique edge pairs, i < j, per graph n, m < 2^24.  An edge
 * with an end outside its graph's node range (or listed in the incidence of a
 * node of another graph) is treated as absent (c_edge +inf where it lies in
 * the graph's own slot), a perm entry outside [0, n) is skipped, a graph whose
 * offsets leave the arrays or the workspace is left with zero counts; each
 * raises HLHGAT_DEVERR_MLGC_RANGE and nothing is written out of bounds.
 * Per-graph state lives in LDS when it fits (64 KiB), else in the graph's
 * slice of workspace; the results are the same bits either way. */
size_t hlhgat_mlgc_device_workspace_bytes(int64_t n_nodes, int64_t n_edges, int64_t n_graphs);
int hlhgat_mlgc_device(int64_t n_graphs, const int64_t* node_ptr, const int64_t* edge_ptr,
                       const int32_t* inc_rowptr, const int32_t* inc_edge,
                       const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                       const double* weight, const int64_t* perm, unsigned flags, float* c_node,
                       float* c_edge, int64_t* coarse_edges, int64_t* coarse_n,
                       int64_t* coarse_e, void* workspace, size_t workspace_bytes, void* stream);

/* ---- native data loader (HOST functions, host pointers) -----------------
 * Replaces the reference's per-step DataLoader collation of PairData
 * (lib/Hodge_Dataset.py:40-48; main_zinc_HL_HGCNN_dense_int3_pyr.py:223-225)
 * plus the batch tables the device step reads.  A packed dataset holds every
 * graph's arrays back to back (InMemoryDataset-style slices, graph-local
 * indices): */
typedef struct {
  int64_t n_graphs;
  const int64_t* node_ptr; /* [G+1] x_t rows (nodes) per graph, cumulative */
  const int64_t* edge_ptr; /* [G+1] x_s rows (edges) */
  const int64_t* lt_ptr;   /* [G+1] L0 COO entries */
  const int64_t* ls_ptr;   /* [G+1] L1 COO entries */
  const float* x_t;        /* [N][f_t] */
  int64_t f_t;
  const float* x_s;        /* [E][f_s] */
  int64_t f_s;
  const int32_t* lt_row;   /* L0 COO, graph-local node ids, row-sorted */
  const int32_t* lt_col;
  const float* lt_w;
  const int32_t* ls_row;   /* L1 COO, graph-local edge ids, row-sorted */
  const int32_t* ls_col;
  const float* ls_w;
  const int32_t* b1_src;   /* [E] B1 edge list (edge_index), graph-local */
  const int32_t* b1_dst;
  const float* y;          /* [G][y_dim] (y_dim 0: none) */
  int64_t y_dim;
} hlhgat_packed_graphs_t;
/* The collated batch: capacities in (rows_t, rows_s, nnz_t, nnz_s equal to
 * the batch's sizes = no padding; rows above them = hodge_dataset.pad_batch's
 * padding), caller-allocated outputs (the table pointers may be NULL to skip
 * a table); n_t / n_s out = the real rows. */
typedef struct {
  int64_t rows_t, rows_s, nnz_t, nnz_s;
  float* x_t;               /* [rows_t][f_t] */
  float* x_s;               /* [rows_s][f_s] */
  int64_t* edge_index_t;    /* [2][nnz_t] */
  float* edge_weight_t;     /* [nnz_t] */
  int64_t* edge_index_s;    /* [2][nnz_s] */
  float* edge_weight_s;     /* [nnz_s] */
  int64_t* edge_index;      /* [2][rows_s] */
  float* y;                 /* [B][y_dim] */
  int64_t* num_node1;       /* [B] */
  int64_t* num_edge1;       /* [B] */
  int32_t* csr_rowptr_t;    /* [rows_t+1] */
  int32_t* csr_col_t;       /* [nnz_t] */
  int32_t* csr_rowptr_s;    /* [rows_s+1] */
  int32_t* csr_col_s;       /* [nnz_s] */
  int32_t* inc_rowptr;      /* [rows_t+1] incidence CSR of |B1| */
  int32_t* inc_eids;        /* [2 rows_s] */
  float* deg_t;             /* [rows_t] degree (padding rows: 1) */
  float* inv_deg_t;         /* [rows_t] fp32 1 / degree */
  int32_t* seg_ptr_t;       /* [B+1] */
  int32_t* seg_ptr_s;       /* [B+1] */
  uint8_t* valid_mask_t;    /* [rows_t] row < n_t */
  int64_t n_t, n_s;         /* out */
} hlhgat_collated_t;
/* sizes[4] = (nodes, edges, L0 entries, L1 entries) of the graphs idx[0..n). */
int hlhgat_collate_sizes(const hlhgat_packed_graphs_t* d, const int64_t* idx, int64_t n_idx,
                         int64_t* sizes);
/* Collate graphs idx[0..B) (in that order) into *out: bitwise the arrays of
 * hodge_dataset.collate followed by pad_batch. */
int hlhgat_collate(const hlhgat_packed_graphs_t* d, const int64_t* idx, int64_t B,
                   hlhgat_collated_t* out);

/* dst[i] = src[idx[i]] for i < n (device; e.g. halo sval = val[eperm]). */
int hlhgat_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst,
                      void* stream);

/* ---- SpMM and fused polynomial step ----------------------------------- */
/* `halo` (optional, below) selects the LDS-staged kernel: see hlhgat_halo_t.
 * It must describe this operator with this row_order; NULL = plain kernel. */
/* Y = A·X (PyG propagate with aggr='add', source_to_target, when A is the
 * CSR keyed by edge_index[1]).  X,Y [n][d] with row strides ldx, ldy.
 * row_order (optional, int32[n_rows], a permutation) is the order in which
 * rows are SCHEDULED (e.g. hlhgat_locality_order): results are identical for
 * any order (each row's entries are still summed in CSR order); only which
 * rows share an XCD's L2 at a time changes.  NULL = natural order. */
int hlhgat_spmm(const int32_t* rowptr, const int32_t* col, const float* val,
                int64_t n_rows, int64_t nnz, const int32_t* row_order,
                const hlhgat_halo_t* halo, const float* X, int64_t ldx,
                int64_t d, float* Y, int64_t ldy, void* stream);

/* Generic fused step (one launch):
 *   Y = (alpha * rs[r] * (A·X)[r] + beta*X[r] + gamma*Z[r]) / div
 *       + p*P[r] + q*Q[r]
 * Z, P, Q, rs (row scale) may be NULL (term dropped).  Y may alias P (each
 * row is read then written by the same lanes).  A is n_rows x n_rows when
 * beta != 0; otherwise X may have any row count >= max(col)+1. */
int hlhgat_poly_step(const int32_t* rowptr, const int32_t* col,
                     const float* val, const float* rs, int64_t n_rows,
                     int64_t nnz, const int32_t* row_order,
                     const hlhgat_halo_t* halo, const float* X,
                     int64_t ldx, int64_t d,
                     const float* Z, int64_t ldz, const float* P, int64_t ldp,
                     const float* Q, int64_t ldq, float alpha, float beta,
                     float gamma, float div, float p, float q, float* Y,
                     int64_t ldy, void* stream);

/* hlhgat_poly_step over a rectangular incidence operator (rows: n_rows nodes;
 * columns: the n_src edges, each referenced by exactly two rows): the same
 * kernel, timed as HLHGAT_PROF_INCIDENCE with the gathered operand counted as
 * n_src rows (what it reads), not n_rows.  Y = alpha rs (A X) + gamma Z.  Replaces the torch.sparse.mm(|B1|, .) of
 * lib/Hodge_Cheb_Conv.py:294 (and the node-side adjoint of :295). */
int hlhgat_incidence_step(const int32_t* rowptr, const int32_t* col, const float* val,
                          const float* rs, int64_t n_rows, int64_t nnz, int64_t n_src,
                          const float* X, int64_t ldx, int64_t d, const float* Z, int64_t ldz,
                          float alpha, float gamma, float* Y, int64_t ldy, void* stream);

/* Polynomial basis T_1..T_{K-1} of X over A (K >= 1; K==1 is a no-op).
 * kind = HLHGAT_POLY_LAGUERRE: T_1 = X - A X,
 *        T_{k+1} = (-A T_k + (2k+1) T_k - k T_{k-1}) / (k+1)
 *        (lib/Hodge_Cheb_Conv.py:494,507)
 * kind = HLHGAT_POLY_CHEB:     T_1 = A X, T_{k+1} = 2 A T_k - T_{k-1}
 *        (lib/Hodge_Cheb_Conv.py:416,430-432)
 * kind = HLHGAT_POLY_LAGUERRE_DEMO: T_1 = X - A X,
 *        T_{k+1} = (-A X + (2k+1) T_k - k T_{k-1}) / (k+1)
 *        (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:554,561,566; K <= 16)
 * X: [n][F] row stride ldx.  T: (K-1) contiguous blocks of [n][F]. */
int hlhgat_poly_basis_fwd(int kind, const int32_t* rowptr, const int32_t* col,
                          const float* val, int64_t n, int64_t nnz,
                          const int32_t* row_order, const hlhgat_halo_t* halo,
                          const float* X, int64_t ldx, int64_t F, int K, float* T,
                          void* stream);

/* Adjoint of hlhgat_poly_basis_fwd.  On entry G holds K contiguous blocks
 * [n][F]: G_k = dLoss/dT_k from the consumers of each T_k (block 0 = the
 * direct gradient of X).  On exit block 0 holds dLoss/dX.  Blocks 1..K-1 are
 * used as scratch.  The CSR passed must be A^T (== A for the symmetric Hodge
 * Laplacians). */
int hlhgat_poly_basis_bwd(int kind, const int32_t* rowptr_t,
                          const int32_t* col_t, const float* val_t, int64_t n,
                          int64_t nnz, const int32_t* row_order,
                          const hlhgat_halo_t* halo, int64_t F,
                          int K, float* G, void* stream);

/* ---- Hodge-factored L1 (large, high-degree edge Laplacians) ------------ */
/* Every L1 the reference builds is 2 B1^T B1 / lmax in fp32
 * (lib/Hodge_Dataset.py:451-456, :780-799; MLGC :283-287): its entries are
 * fl(2 v / lmax) with v in {2, +-1}, so L1 = alpha_e * B1^T B1 EXACTLY, with
 * alpha_e = L1[e,e] / 2 (constant per graph).  Then
 *     L1 X = alpha * B1^T (B1 X):   Z = B1 X   (node rows: signed sum of the
 *                                              node's incident edge rows)
 *                                   Y[e] = alpha_e (Z[j] - Z[i])
 * which gathers ~4 feature rows per edge instead of nnz(L1)/E (~20 at
 * BASELINE config 5, ~18 at config 3).  Same real-arithmetic result as the
 * CSR SpMM; fp32 rounding differs (measured <= 3e-7 relative at config 5),
 * so this path is NOT bitwise equal to propagate; the CSR path is.  The
 * caller (hlhgat.ops.set_hodge_factor, checked on the host by
 * hodge_dataset.hodge_factor_ok) guarantees the identity. */
typedef struct hlhgat_hodge_factor {
  const int32_t* node_rowptr; /* [n_nodes+1] incidence CSR of B1 (node rows) */
  const int32_t* node_edge;   /* [2 n_edges] incident edge ids, ascending */
  const float* node_sign;     /* [2 n_edges] -1 (node = edge_index[0][e]) / +1 */
  const int32_t* node_order;  /* optional row schedule of the node rows */
  int64_t n_nodes;
  const int32_t* ends;        /* [n_edges][2] (edge_index[0][e], edge_index[1][e]) */
  const float* alpha;         /* [n_edges] L1[e,e] / 2 */
  const int32_t* edge_order;  /* optional row schedule of the edge rows */
  int64_t n_edges;
} hlhgat_hodge_factor_t;

/* Floats of scratch (Z = B1 X) the factored entry points need for width F. */
int64_t hlhgat_hodge_factor_work_floats(int64_t n_nodes, int64_t F);

/* Y = L1 X through the factorisation (two launches).  X, Y [n_edges][d]. */
int hlhgat_hodge_spmm(const hlhgat_hodge_factor_t* f, const float* X, int64_t ldx,
                      int64_t d, float* Y, int64_t ldy, float* work, void* stream);

/* hlhgat_poly_step with A = L1 factored: Y = (alpha (L1 X)[r] + beta X[r] +
 * gamma Z[r]) / div + p P[r] + q Q[r]  (two launches; no row scale). */
int hlhgat_hodge_poly_step(const hlhgat_hodge_factor_t* f, const float* X, int64_t ldx,
                           int64_t d, const float* Z, int64_t ldz, const float* P, int64_t ldp,
                           const float* Q, int64_t ldq, float alpha, float beta, float gamma,
                           float div, float p, float q, float* Y, int64_t ldy, float* work,
                           void* stream);

/* hlhgat_poly_basis_fwd / _bwd with every L1 application factored (each
 * step = one incidence launch + one fused edge-step launch whose epilogue is
 * the recurrence's).  L1 is symmetric, so the adjoint uses the same factor.
 * Replaces the same reference lines as hlhgat_poly_basis_fwd / _bwd. */
int hlhgat_poly_basis_fwd_factored(int kind, const hlhgat_hodge_factor_t* f,
                                   const float* X, int64_t ldx, int64_t F, int K, float* T,
                                   float* work, void* stream);
int hlhgat_poly_basis_bwd_factored(int kind, const hlhgat_hodge_factor_t* f, int64_t F,
                                   int K, float* G, float* work, void* stream);

/* ---- on-device Hodge Laplacian builder -------------- */
/* Replaces the per-graph dense construction of the reference
 * (lib/Hodge_Dataset.py:451-468, :780-799; DEMO notebook cells 11, 19):
 * par1 = adj2par1(...).to_dense(); L0 = par1 par1^T; lmax = eigh(L0).max();
 * L0 = 2 par1 par1^T / lmax; L1 = 2 par1^T par1 / lmax; dense_to_sparse.
 * Input: a block-diagonal batch's edge list (int64 [2][E], i < j per edge,
 * PairData offsets) and its incidence CSR (hlhgat_incidence_csr).
 *
 * hlhgat_hodge_lmax: lmax of every graph's L0 = B1 B1^T (graph g = nodes
 * [node_ptr[g], node_ptr[g+1])), one wave per graph (vectors and the local
 * adjacency in LDS when they fit in 48 KB), fp64 Lanczos by the three-term
 * recurrence with local re-orthogonalisation (min(n, steps) iterations,
 * 1 <= steps <= 1024; the largest Ritz value converges first and loss of
 * orthogonality only adds ghost copies) and Sturm bisection of the
 * tridiagonal matrix.  Workspace: 3 n_nodes doubles (the vectors of graphs
 * that miss the LDS).
 * Accuracy against a dense fp64 eigh (tests/test_hodge_lmax.py):
 * the result is a Ritz value, so it never exceeds lmax; a graph with
 * n <= steps nodes is exact to fp64 rounding.  At steps = 64 the workloads'
 * kNN graphs (k = 8 .. 25, any size, with edge dropout) and grids up to
 * 20 x 20 agree to ~1e-14 relative, chain-like trees of up to ~450 nodes
 * to 1e-7 or better -- inside the reference's own float32 eigh rounding (~1e-7), so
 * entries built from this lmax differ from the reference's by an ulp at most.
 * Slowly mixing graphs do NOT converge in 64 steps: a path of 100 .. 1000
 * nodes or a ring of 444 .. 1000 is off by ~1e-4, a 30 x 30 grid by 2e-6.  Such
 * graphs (path-like, large lattices) need steps ~ n; steps = min(n, 1024)
 * gives 1e-7 or better on them. */
int64_t hlhgat_hodge_lmax_workspace_bytes(int64_t n_nodes, int steps);
int hlhgat_hodge_lmax(const int32_t* inc_rowptr, const int32_t* inc_edge,
                      const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                      const int64_t* node_ptr, int64_t n_graphs, int steps, double* lmax,
                      void* workspace, int64_t workspace_bytes, void* stream);
/* hlhgat_eig_pe: the eigenvector positional encodings of every graph of the
 * batch and its lambda_max in ONE launch, replacing the reference's per-sample
 * dense eighs (eig_pe, lib/Hodge_Dataset.py:97-112, called at
 * main_cifar10SP_HL_HGCNN_dense_int3_attpool.py:86-91 on L0 = 2 B1 B1^T / lmax,
 * and torch.linalg.eigh(L0).max(), lib/Hodge_Dataset.py:782).  Per graph, one
 * workgroup, fp64: Lanczos with full re-orthogonalisation (restarted when an
 * invariant subspace closes), eigenvalues of the tridiagonal matrix by Sturm
 * multisection, its eigenvectors by inverse iteration, pe = Q y.  Output:
 * pe[v][0 .. k-2] (float32, row stride ldpe) = eigenvectors 1 .. k-1 of the
 * unscaled L0 = B1 B1^T (ascending eigenvalues; the same vectors as the
 * scaled L0's), zero columns where the graph has fewer than k nodes;
 * lmax[g] = the largest eigenvalue of the unscaled L0 (fp64).  Eigenvectors
 * are defined up to sign (and rotation within equal eigenvalues).
 * max_nodes >= every graph's node count (sizes the workspace slice a graph
 * too large for the LDS uses: one slice per workgroup, min(n_graphs, CUs)
 * workgroups, so the size depends on the current device); 2 <= k <= 64.
 * A graph with more than max_nodes nodes is not computed: its pe rows are
 * zero, its lmax is 0 and HLHGAT_DEVERR_EIGPE_SIZE is raised. */
int64_t hlhgat_eig_pe_workspace_bytes(int64_t n_graphs, int64_t max_nodes, int k);
int hlhgat_eig_pe(const int32_t* inc_rowptr, const int32_t* inc_edge, const int64_t* edge_index,
                  int64_t n_edges, int64_t n_nodes, const int64_t* node_ptr, int64_t n_graphs,
                  int64_t max_nodes, int k, float* pe, int64_t ldpe, double* lmax,
                  void* workspace, int64_t workspace_bytes, void* stream);
/* hlhgat_eig_pe_edges: the EDGE-side eigenvector PE of every graph of the
 * batch in one launch -- the molecular datasets' eig_pe(L1)
 * (lib/Hodge_Dataset.py:458, :587, with eig_pe at :97-112): pe[e][0 .. k-2]
 * (float32, row stride ldpe, at the graph's edge rows) = eigenvectors
 * 1 .. k-1, ascending, of the unscaled L1 = B1^T B1 (the same vectors as the
 * reference's scaled L1; column 0 dropped as its [:, 1:k] does).  The same
 * solver as hlhgat_eig_pe over the operator y = B1^T (B1 x).  The batch's
 * edges are grouped by graph: edge_ptr [n_graphs + 1] beside node_ptr, i < j
 * per edge, PairData offsets.  L1's kernel is the cycle space (dimension
 * E - n + c): an exactly degenerate cluster at 0 whose basis is arbitrary
 * (the reference's is LAPACK's); the nonzero spectrum is L0's; a tree's L1 is
 * nonsingular.  2 <= k <= 64; columns >= E_g - 1 of a graph with E_g < k
 * edges are zero; E_g = 0 writes nothing; a graph with more than max_edges
 * edges (which size the workspace slice) gets zero rows and
 * HLHGAT_DEVERR_EIGPE_SIZE, nothing else is touched.  Deterministic: a second
 * launch is bitwise equal.  Vectors are defined up to sign, and up to rotation
 * inside a cluster of equal eigenvalues. */
int64_t hlhgat_eig_pe_edges_workspace_bytes(int64_t n_graphs, int64_t max_edges, int k);
int hlhgat_eig_pe_edges(const int32_t* inc_rowptr, const int32_t* inc_edge,
                        const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                        const int64_t* node_ptr, const int64_t* edge_ptr, int64_t n_graphs,
                        int64_t max_edges, int k, float* pe, int64_t ldpe, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Row sizes of L0 (deg(v) + 1, 0 for an isolated node) and L1 (deg(i) +
 * deg(j) - 1); exclusive-scan them into the row pointers. */
int hlhgat_hodge_row_sizes(const int32_t* inc_rowptr, const int64_t* edge_index,
                           int64_t n_edges, int64_t n_nodes, int32_t* sizes_l0,
                           int32_t* sizes_l1, void* stream);
/* L0 / L1 in CSR, columns ascending, entries fl(fl(2 v) / lam_node[row's
 * graph]) -- the reference's float32 arithmetic -- with v the integer entry
 * of B1 B1^T (deg, -1) / B1^T B1 (2, +1 same-end, -1 tail-to-head).
 * cap_l0 / cap_l1 = the entries col_l* / val_l* hold: a row that would end
 * past them (row pointers sized for a simple graph given a multigraph)
 * writes nothing and raises HLHGAT_DEVERR_HODGE_SIZE. */
int hlhgat_hodge_build(const int32_t* inc_rowptr, const int32_t* inc_edge,
                       const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                       const float* lam_node, const int32_t* rowptr_l0, int32_t* col_l0,
                       float* val_l0, int64_t cap_l0, const int32_t* rowptr_l1,
                       int32_t* col_l1, float* val_l1, int64_t cap_l1, void* stream);

/* ---- dense per-simplex projections (fp32 MFMA) ------------------------ */
#define HLHGAT_MAX_BLOCKS 16

/* Forward:  C[m][n] = beta_acc*C[m][n] + sum_b sum_k A_b[m][k]*W_b[n][k]
 *                     + bias[n]
 * A_b: [M][kb[b]] row stride lda[b]; W_b: [N][kb[b]] row stride ldw[b]
 * (nn.Linear weight layout).  accumulate != 0 adds into C.  bias may be NULL.
 * Replaces out = sum_k lins[k](T_k) + bias (lib/Hodge_Cheb_Conv.py:487,497,
 * 509,512-513) and Linear(cat[a,b]) (lib/Hodge_Cheb_Conv.py:307-308). */
int hlhgat_proj_fwd(int nblocks, const float* const* A, const int64_t* lda,
                    const float* const* W, const int64_t* ldw,
                    const int64_t* kb, int64_t M, int64_t N, const float* bias,
                    float* C, int64_t ldc, int accumulate, void* stream);

/* Data gradient:  dA_b[m][k] (+)= sum_n dC[m][n] * W_b[n][k]. */
int hlhgat_proj_bwd_data(int nblocks, const float* dC, int64_t lddc,
                         const float* const* W, const int64_t* ldw,
                         const int64_t* kb, int64_t M, int64_t N,
                         float* const* dA, const int64_t* ldda,
                         int accumulate, void* stream);

/* Scratch floats needed by hlhgat_proj_bwd_weight. */
int64_t hlhgat_proj_bwd_weight_workspace_floats(int nblocks, const int64_t* kb,
                                                int64_t M, int64_t N,
                                                int with_bias);

/* Weight / bias gradient (deterministic split-M reduction, no atomics):
 *   dW_b[n][k] (+)= sum_m dC[m][n] * A_b[m][k];   dbias[n] (+)= sum_m dC[m][n]
 * dbias may be NULL. */
int hlhgat_proj_bwd_weight(int nblocks, const float* dC, int64_t lddc,
                           const float* const* A, const int64_t* lda,
                           const int64_t* kb, int64_t M, int64_t N,
                           float* const* dW, const int64_t* lddw, float* dbias,
                           int accumulate, float* workspace,
                           int64_t workspace_floats, void* stream);

/* The Linear backward (torch.nn.Linear / the HodgeLaguerreConv projections,
 * lib/Hodge_Cheb_Conv.py:63-66 backward) in two launches when the operands are
 * 16-B aligned: the weight / bias gradient's split partials of
 * hlhgat_proj_bwd_weight (nb_w blocks; `workspace` sized by
 * hlhgat_proj_bwd_weight_workspace_floats) together with the data gradient of
 * hlhgat_proj_bwd_data (nb_d blocks) in one, then the split reduction;
 * bit-identical to those two calls; either side may be empty (nb = 0).
 * Unaligned operands fall back to the two calls.  The weight gradient is
 * written (accumulate = 0); accumulate_d != 0 adds the data gradient into
 * dA (e.g. straight into the gradient slab of the dense concatenation,
 * hlhgat.ops.DenseConcat). */
int hlhgat_proj_bwd(int64_t M, int64_t N, const float* dC, int64_t lddc,
                    int nb_w, const float* const* A, const int64_t* lda,
                    const int64_t* kb_w, float* const* dW, const int64_t* lddw,
                    float* dbias, int nb_d, const float* const* W,
                    const int64_t* ldw, const int64_t* kb_d, float* const* dA,
                    const int64_t* ldda, int accumulate_d, float* workspace,
                    int64_t workspace_floats, void* stream);

/* Deferred split reduction.  hlhgat_proj_bwd_defer is hlhgat_proj_bwd whose
 * weight-gradient split reduction may be handed back instead of launched:
 *   - defer_out != NULL and the one-launch path is taken: the reduction is
 *     NOT launched; its descriptor goes to *defer_out and *deferred = 1.  The
 *     caller must keep `workspace` alive and run the descriptor (merge it into
 *     a later call on the same stream, or hlhgat_reduce_run) before anything
 *     reads dW / dbias;
 *   - merge != NULL: a descriptor deferred earlier ON THE SAME STREAM; its
 *     reduction runs as extra workgroups of this call's launch (or as its own
 *     launch first when this call cannot take the one-launch path).
 * The reduction itself is unchanged, so dW / dbias are bitwise those of
 * hlhgat_proj_bwd; what goes away is one dependent launch per Linear
 * backward on the stream's chain. */
typedef struct {
  int64_t words[160];
} hlhgat_reduce_desc_t;
int hlhgat_proj_bwd_defer(int64_t M, int64_t N, const float* dC, int64_t lddc, int nb_w,
                          const float* const* A, const int64_t* lda, const int64_t* kb_w,
                          float* const* dW, const int64_t* lddw, float* dbias, int nb_d,
                          const float* const* W, const int64_t* ldw, const int64_t* kb_d,
                          float* const* dA, const int64_t* ldda, int accumulate_d,
                          float* workspace, int64_t workspace_floats,
                          const hlhgat_reduce_desc_t* merge, hlhgat_reduce_desc_t* defer_out,
                          int* deferred, void* stream);
int hlhgat_reduce_run(const hlhgat_reduce_desc_t* desc, void* stream);

/* ---- boundary-operator interaction ------------------------------------ */
/* out[e] = ca*sa[i]*x[i] + cb*sb[j]*x[j] (+ z[e]) (+ out[e] if accumulate)
 * with (i,j) = edge_index[:,e] (sa/sb per-node scale vectors, z a per-edge
 * addend [n_edges][ldz]; each may be NULL).  With ca=cb=0.5 and no scales
 * this is x_t2s = (|B1|^T x_t)/2 (lib/Hodge_Cheb_Conv.py:295). */
int hlhgat_edge_gather2(const int64_t* edge_index, int64_t n_edges,
                        const float* x, int64_t ldx, int64_t d, const float* sa,
                        const float* sb, float ca, float cb, const float* z,
                        int64_t ldz, float* out, int64_t ldo, int accumulate,
                        void* stream);

/* The TSP edge readout x_t2s = |B1^T x_t| / 2 (lib/Hodge_ST_Model.py:846-848)
 * with g == NULL: out[e] = |x[j] - x[i]| / 2 for edge e = (i, j)
 * (edge_index [2][n_edges]); with g: its backward's edge factor
 * out[e] = (g[e] / 2) * sgn(x[j] - x[i]) (then B1 out, hlhgat_poly_step on
 * the signed incidence CSR, gives dx).  Bitwise the unfused
 * sparse.mm / abs / div and their backwards. */
int hlhgat_edge_absdiff(const int64_t* edge_index, int64_t n_edges, const float* x,
                        int64_t ldx, int64_t d, const float* g, int64_t ldg, float* out,
                        int64_t ldo, void* stream);

/* ---- attention score (NodeEdgeInt only_att) ---------------------------- */
/* a[r] = sigma((w_cross*<Qc[r],Kr[r]> + w_self*<Qs[r],Kr[r]>) / sqrt_dk)
 * with w_cross = (1-lambda), w_self = lambda (lib/Hodge_Cheb_Conv.py:299-304).
 * Qc, Qs, Kr: [n][dk] with row strides. */
int hlhgat_att_score_fwd(int64_t n, int64_t dk, const float* Qc, int64_t ldqc,
                         const float* Qs, int64_t ldqs, const float* Kr,
                         int64_t ldk, float w_cross, float w_self,
                         float sqrt_dk, int sigma, float* a, void* stream);

/* Backward of hlhgat_att_score_fwd given a (the forward output) and da. */
int hlhgat_att_score_bwd(int64_t n, int64_t dk, const float* Qc, int64_t ldqc,
                         const float* Qs, int64_t ldqs, const float* Kr,
                         int64_t ldk, float w_cross, float w_self,
                         float sqrt_dk, int sigma, const float* a,
                         const float* da, float* dQc, float* dQs, float* dK,
                         int64_t ldg, void* stream);

/* The NEAtt product x0 * att of the attention-pooling heads
 * (main_pepfunc_HL_HGCNN_dense_int3_attpool.py:134-136, lib/Hodge_ST_Model.py:
 * 276-280): y[r][:] = x[r][:] * a[r] over n rows of d features (y may be a
 * column block of a wider slab, ldy). */
int hlhgat_row_scale_fwd(int64_t n, int64_t d, const float* x, int64_t ldx,
                         const float* a, float* y, int64_t ldy, void* stream);
/* Its backward in one pass: dx[r][:] = dy[r][:] * a[r] and
 * da[r] = sum_j dy[r][j] * x[r][j]. */
int hlhgat_row_scale_bwd(int64_t n, int64_t d, const float* x, int64_t ldx,
                         const float* a, const float* dy, int64_t lddy, float* dx,
                         int64_t lddx, float* da, void* stream);

/* ---- segment mean (scatter_mean / global_mean_pool) -------------------- */
/* out[s] = mean over rows r of CSR segment s of x[r] (rows listed in
 * seg_rows, or contiguous when seg_rows == NULL); empty segments give 0. */
int hlhgat_segment_mean_fwd(const int32_t* seg_ptr, const int32_t* seg_rows,
                            int64_t n_seg, const float* x, int64_t ldx,
                            int64_t d, float* out, int64_t ldo, void* stream);
/* dx[r] = dout[seg(r)] / |seg| for every row r of a segment.  Contiguous
 * segments (seg_rows NULL): rows [0, seg_ptr[0]) and [seg_ptr[n_seg], n_rows)
 * of dx get exact zeros (global_mean_pool's adjoint, lib/Hodge_ST_Model.py:636),
 * so every one of the n_rows rows is written.  Listed members (scatter_mean):
 * n_rows is ignored and rows in no segment are left untouched (caller
 * zero-fills). */
int hlhgat_segment_mean_bwd(const int32_t* seg_ptr, const int32_t* seg_rows,
                            int64_t n_seg, const float* dout, int64_t ldo,
                            int64_t d, float* dx, int64_t ldx, int64_t n_rows,
                            void* stream);

/* Backward of the MLGC cluster pooling (scatter_mean over pos_ts / pos_ss,
 * lib/Hodge_ST_Model.py:1066-1069) from the pool tables
 * (hlhgat.hodge_dataset.pool_tables): seg_ptr has n_seg + 2 entries and its
 * extra segment n_seg lists the rows in no cluster (inf cluster id: padding
 * rows, edges between clusters), so seg_rows[0 .. seg_ptr[n_seg+1]) is a
 * permutation of the n_rows rows.  dx[r] = dout[s] / |s| for a member of
 * cluster s, exact zeros for the extra segment's rows: every row of dx is
 * written (no caller zero fill). */
int hlhgat_pool_mean_bwd(const int32_t* seg_ptr, const int32_t* seg_rows,
                         int64_t n_seg, const float* dout, int64_t ldo,
                         int64_t d, float* dx, int64_t ldx, int64_t n_rows,
                         void* stream);

/* ---- BatchNorm1d (training) + optional fused ReLU ---------------------- */
/* gnn.BatchNorm / nn.BatchNorm1d in training mode over x [n][C] (batch
 * statistics, biased variance for normalisation, unbiased for the running
 * update, momentum as torch), followed by ReLU when relu != 0 — the
 * conv -> BatchNorm -> ReLU tail of every HL block (lib/Hodge_ST_Model.py:
 * 556-566) and of NodeEdgeInt's WV_* MLPs (lib/Hodge_Cheb_Conv.py:276-289).
 * weight/bias may be NULL (affine=False); running stats may be NULL.
 * The workspace must be zero-filled before its first use and must not be
 * shared by launches that run concurrently; the kernels leave it reusable. */
int64_t hlhgat_bn_workspace_bytes(int64_t n, int64_t C);
/* n_valid (optional, device int32 scalar): rows >= *n_valid are capacity
 * padding of a static-shape batch: excluded from the statistics, their
 * outputs (and, backward, input gradients) written as 0.  NULL = all n. */
/* Eval-mode BatchNorm1d (+ ReLU) from the running statistics, one launch:
 * y = relu?((x - running_mean) * (w / sqrt(running_var + eps)) + b).  Replaces
 * torch's eval-mode batch_norm (+ relu) in the reference's test() loops
 * (lib/Hodge_ST_Model.py:556-566 under model.eval(); main_zinc...:165-177).
 * weight / bias may be NULL (1 / 0). */
int hlhgat_bn_apply_running(const float* x, int64_t ldx, int64_t n, int64_t C,
                            const float* weight, const float* bias, const float* running_mean,
                            const float* running_var, float eps, int relu, float* y,
                            int64_t ldy, void* stream);
int hlhgat_bn_fwd_train(const float* x, int64_t ldx, int64_t n,
                        const int32_t* n_valid, int64_t C,
                        const float* weight, const float* bias,
                        float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float momentum, float eps,
                        int relu, float* y, int64_t ldy, float* save_mean,
                        float* save_invstd, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* Backward; y (the forward output) supplies the ReLU mask, NULL if no ReLU.
 * dweight/dbias may be NULL. */
/* The two halves of hlhgat_bn_fwd_train: statistics only (save_mean /
 * save_invstd, running stats, num_batches_tracked) and apply only
 * (y = relu?(x * s + t) with s = weight * invstd, t = bias - mean * s; rows
 * >= *n_valid written as 0). */
int hlhgat_bn_stats_train(const float* x, int64_t ldx, int64_t n, const int32_t* n_valid,
                          int64_t C, float* running_mean, float* running_var,
                          int64_t* num_batches_tracked, float momentum, float eps,
                          float* save_mean, float* save_invstd, void* workspace,
                          int64_t workspace_bytes, void* stream);
int hlhgat_bn_apply(const float* x, int64_t ldx, int64_t n, const int32_t* n_valid, int64_t C,
                    const float* weight, const float* bias, const float* save_mean,
                    const float* save_invstd, int relu, float* y, int64_t ldy, void* stream);

/* BatchNorm forward statistics and normalisation in one launch
 * (k_bn_fwd_grid: rows held in registers while the finalising workgroup --
 * the last to arrive -- publishes the statistics) or as two; default 1 (env
 * HLHGAT_BN_ONE_LAUNCH=0 turns it off).  Both give bitwise the same results.
 * The one launch is taken when its grid (<= 256 workgroups) is at most half
 * of the device's resident-workgroup capacity for it.  It assumes nothing
 * about residency: a workgroup waits for the statistics at most
 * hlhgat_set_bn_wait_us microseconds, then hands its rows to the finaliser
 * and exits (the finaliser normalises them from x with the same operations),
 * so the launch completes with the same bits beside any other kernels. */
/* Projection + BatchNorm1d (+ ReLU) forward, training mode: the
 * hlhgat_proj_fwd GEMM x = sum_b A_b W_b^T + bias (stored to x: the backward
 * reads it), then hlhgat_bn_fwd_train on x into y -- in ONE launch
 * (k_proj_bn_fwd: the projection's workgroups finish the BatchNorm from
 * their registers after a bounded grid-wide reduction) when N % 64 == 0, the
 * operands are 16-B aligned with ld % 4 == 0, ceil(M / 64) <= 512 and the
 * grid fits half of the chip's resident capacity; otherwise the two calls.
 * Its wait is bounded like k_bn_fwd_grid's: a workgroup that gives up leaves
 * its tile to the finaliser, which normalises it from the stored x.
 * Replaces Linear -> BatchNorm1d -> ReLU and HodgeLaguerreConv -> BatchNorm
 * -> ReLU (lib/Hodge_Cheb_Conv.py:276-289, lib/Hodge_ST_Model.py:556-566).
 * Statistics equal the two-call path's to fp64 summation order (not
 * bitwise).  Workspace: hlhgat_bn_workspace_bytes(M, N). */
int hlhgat_proj_bn_fwd(int nblocks, const float* const* A, const int64_t* lda,
                       const float* const* W, const int64_t* ldw, const int64_t* kb, int64_t M,
                       int64_t N, const float* bias, float* x, int64_t ldx,
                       const int32_t* n_valid, const float* bn_weight, const float* bn_bias,
                       float* running_mean, float* running_var, int64_t* num_batches_tracked,
                       float momentum, float eps, int relu, float* y, int64_t ldy,
                       float* save_mean, float* save_invstd, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* Large-tile projection kernels (128 x 128 workgroup tiles, 2 x 2 32x32x2
 * MFMA accumulators per wave; the config 3-5 shapes): mode 0 = never (the
 * default: slower inside the measured two-chain steps),
 * -1 = by shape (per-operation rules from the config-5 census; min_m rows at
 * least, default 32769, env HLHGAT_GEMM_BIG_MIN_M), 1 = every 16-B aligned
 * shape.  Env HLHGAT_GEMM_BIG sets the initial mode.  min_m <= 0 keeps the
 * current threshold. */
int hlhgat_set_gemm_big(int mode, int64_t min_m);
/* Matmul precision of the projections, process-wide like hlhgat_set_gemm_big.
 * HLHGAT_GEMM_FP32 (the default): the fp32 MFMA kernels, bit for bit as
 * without this switch.  HLHGAT_GEMM_BF16: hlhgat_proj_fwd, hlhgat_proj_bwd_data
 * and hlhgat_proj_bwd_weight run kernels that round their two operands to bf16
 * (round to nearest even) on load and accumulate the exact products in fp32
 * (v_mfma_f32_16x16x32_bf16): forward rounds A and W, the data gradient dC and
 * W, the weight gradient dC and A.  Storage, bias, accumulate adds, the bias
 * gradient (summed from the unrounded dC) and the deterministic split
 * reduction stay fp32; the summation order is unspecified but fixed: two runs
 * are bitwise equal.  The mode is read when a GEMM is launched (forward and
 * backward alike), so a captured graph keeps the mode it was captured in.
 * In bf16 mode an eligible hlhgat_proj_bn_fwd runs the bf16 projection and
 * then the fp32 BatchNorm kernels, and hlhgat_proj_bwd / hlhgat_proj_bwd_defer
 * with an eligible side run the two separate calls (a merge descriptor is
 * reduced first, nothing is deferred: *deferred = 0).  The temporal
 * convolution front end (hlhgat_tconv_*) is fp32 in either mode. */
#define HLHGAT_GEMM_FP32 0
#define HLHGAT_GEMM_BF16 1
int hlhgat_set_gemm_precision(int mode);
int hlhgat_get_gemm_precision(void);
/* 1 if a GEMM call with these reduction widths takes the bf16 kernels in bf16
 * mode, else 0 (it runs the fp32 kernels, e.g. the 18-wide input projection or
 * an N = 1 head).  The rule: 1 <= nblocks <= HLHGAT_MAX_BLOCKS; every
 * kb[b] > 0 and kb[b] % 8 == 0; every row stride ld[b] >= kb[b] and
 * ld[b] % 4 == 0 (ld may be NULL: not checked); N > 0 and N % 4 == 0;
 * aligned16 != 0, i.e. every operand pointer of the call (the blocks and,
 * for the gradients, dC) is 16-byte aligned.  The gradients also need
 * lddc % 4 == 0.  The outputs need no alignment. */
int hlhgat_gemm_bf16_eligible(int nblocks, const int64_t* kb, const int64_t* ld, int64_t N,
                              int aligned16);
/* Host-side counters of GEMM calls made in bf16 mode: out[0] = calls sent to
 * the bf16 kernels, out[1] = calls that fell back to the fp32 kernels
 * (ineligible).  reset != 0 zeroes them after reading. */
int hlhgat_gemm_precision_stats(int64_t out[2], int reset);
/* 0: the fused Linear backward (hlhgat_proj_bwd / _defer) uses one
 * data-gradient workgroup per (row block, 64-column tile) instead of one per
 * row block covering every column tile (N <= 64); bitwise the same (tests). */
int hlhgat_set_proj_bwd_rows(int on);
/* 0: hlhgat_proj_bn_fwd always takes the two-call path (tests). */
int hlhgat_set_proj_bn_fused(int on);
/* 1: hlhgat_proj_bn_fwd's fused path as two launches -- the projection with
 * the statistics in its epilogue (its last workgroup finalises them; no
 * workgroup waits), then the BatchNorm apply over x -- bitwise the same y. */
int hlhgat_set_proj_bn_split(int on);
/* Diagnostics: k_proj_bn_fwd stamps s_memrealtime (100 MHz) into buf, 8
 * words per workgroup (blockIdx.y * gridDim.x + blockIdx.x): start, main loop
 * done, partials written, group level done, statistics known (finaliser:
 * generation bumped; others: poll returned), y stored, flags (1: last of its
 * group, 2: finaliser); launches whose grid needs more than `words` words
 * stamp nothing.  buf = NULL, words = 0: off (default). */
int hlhgat_set_proj_bn_stamps(void* buf, int64_t words);
/* Workgroups k_proj_bn_fwd may use (half of the resident capacity). */
int hlhgat_proj_bn_fused_capacity(int64_t* out);
int hlhgat_set_bn_one_launch(int on);
int hlhgat_get_bn_one_launch(void);
/* BatchNorm backward (hlhgat_bn_bwd_train) in one launch (k_bn_bwd_grid: the
 * reduction's grid keeps each row's masked gradient and x - mean in
 * registers, the last arriver of the reduction tree publishes dx's
 * coefficients and every workgroup stores dx of its own rows; the bounded
 * wait and hand-over of the forward kernels) instead of the reduction and the
 * apply launch; default 1.  Taken when hlhgat_set_bn_one_launch is on too
 * (0 there turns off both directions), a thread's rows fit the registers
 * (<= 32) and the grid is at most 256 workgroups and at most the kernel's
 * share of the resident capacity.  0: the two launches; both give bitwise
 * the same dx, dweight and dbias. */
int hlhgat_set_bn_bwd_one_launch(int on);
int hlhgat_get_bn_bwd_one_launch(void);
/* Microseconds a one-launch BatchNorm workgroup waits for its tile's
 * statistics before it hands its rows to the finaliser (default 1000; 0 =
 * hand over at once unless already final: a test hook that forces the
 * hand-over path, bitwise the same results). */
int hlhgat_set_bn_wait_us(unsigned wait_us);

/* Times a one-launch BatchNorm workgroup gave up waiting for its tile's
 * statistics (and handed its rows over): reads the device counter
 * (synchronising). */
int hlhgat_bn_wait_timeouts(unsigned* out);
/* The first HLHGAT_BN_LOG_MAX give-ups since the last reset, as recorded by
 * the workgroup that gave up: *logged = give-ups recorded in all (may exceed
 * what is copied); out[0 .. min(*logged, max, HLHGAT_BN_LOG_MAX)). */
#define HLHGAT_BN_LOG_MAX 64
typedef struct {
  uint32_t kernel;    /* 1 = k_bn_fwd_grid, 2 = k_proj_bn_fwd, 3 = k_bn_bwd_grid */
  uint32_t tile;      /* column tile (blockIdx.y) */
  uint32_t block;     /* row partition / row block (blockIdx.x) */
  uint32_t total;     /* arrivals the finaliser needs (workgroups; groups for k_proj_bn_fwd
                         and for k_bn_bwd_grid above its flat limit) */
  uint32_t arrivals;  /* arrivals counted when the wait ran out */
  uint32_t gen0;      /* the tile's generation when the workgroup arrived */
  uint32_t gen_seen;  /* the generation read after giving up */
  uint32_t wait_us;   /* the wait bound in force */
  uint32_t outcome;   /* 1 = reclaimed its rows (final by then), 2 = handed to the finaliser */
} hlhgat_bn_giveup_t;
int hlhgat_bn_giveup_log(hlhgat_bn_giveup_t* out, int max, int* logged);
/* Zero the give-up counter and log (synchronises the device). */
int hlhgat_bn_giveup_reset(void);

/* The reduction half of hlhgat_bn_bwd_train: dweight, dbias and dx's
 * coefficients coef[3][C] (A, B, C of dx = A g + (B (x - mean) + C)), for a
 * consumer that forms dx itself. */
int hlhgat_bn_bwd_reduce(const float* x, int64_t ldx, const float* y, int64_t ldy,
                         const float* dy, int64_t lddy, int64_t n, const int32_t* n_valid,
                         int64_t C, const float* weight, const float* save_mean,
                         const float* save_invstd, float* coef, float* dweight, float* dbias,
                         void* workspace, int64_t workspace_bytes, void* stream);
int hlhgat_bn_bwd_train(const float* x, int64_t ldx, const float* y, int64_t ldy,
                        const float* dy, int64_t lddy, int64_t n,
                        const int32_t* n_valid, int64_t C,
                        const float* weight, const float* save_mean,
                        const float* save_invstd, float* dx, int64_t lddx,
                        float* dweight, float* dbias, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---- SyncBatchNorm (batch statistics over every data-parallel rank) ----- */
/* torch.nn.SyncBatchNorm semantics for the BatchNorm1d layers of the path
 * (lib/Hodge_ST_Model.py:556-566, lib/Hodge_Cheb_Conv.py:276-289) when the
 * batch is sharded by graph over ranks (parity caveat 1):
 *   1. hlhgat_bn_sums_fwd: this rank's fp64 column sums into
 *      sums[hlhgat_bn_sums_len(C)] = [S0[C] = sum x, S1[C] = sum x^2, n_valid];
 *   2. the caller all-gathers them into gathered[world][2C+1] (RCCL);
 *   3. hlhgat_bn_sync_fwd_apply: every rank totals the gathered sums in rank
 *      order (fp64), finishes mean / invstd / running statistics exactly as
 *      hlhgat_bn_fwd_train does and writes y.
 * Backward: hlhgat_bn_sums_bwd (sum g, sum g (x - mean) with g = dy masked
 * by the ReLU of y; this rank's dweight / dbias, which data-parallel
 * gradient averaging then combines as torch's SyncBatchNorm does), all-gather,
 * hlhgat_bn_sync_bwd_apply (dx with the global sums and count).  y / dx of
 * the _sums_ calls only select the layout (pass the tensors the apply will
 * use): with one rank the results are bitwise those of hlhgat_bn_fwd_train /
 * hlhgat_bn_bwd_train.  The workspace is hlhgat_bn_workspace_bytes' one. */
int64_t hlhgat_bn_sums_len(int64_t C);
int hlhgat_bn_sums_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t n,
                       const int32_t* n_valid, int64_t C, double* sums, void* workspace,
                       int64_t workspace_bytes, void* stream);
int hlhgat_bn_sync_fwd_apply(const float* x, int64_t ldx, int64_t n, const int32_t* n_valid,
                             int64_t C, const double* gathered, int world, const float* weight,
                             const float* bias, float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, float momentum, float eps, int relu,
                             float* y, int64_t ldy, float* save_mean, float* save_invstd,
                             void* stream);
int hlhgat_bn_sums_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy,
                       const float* dy, int64_t lddy, float* dx_layout, int64_t lddx, int64_t n,
                       const int32_t* n_valid, int64_t C, const float* save_mean,
                       const float* save_invstd, double* sums, float* dweight, float* dbias,
                       void* workspace, int64_t workspace_bytes, void* stream);
int hlhgat_bn_sync_bwd_apply(const float* x, int64_t ldx, const float* y, int64_t ldy,
                             const float* dy, int64_t lddy, int64_t n, const int32_t* n_valid,
                             int64_t C, const float* weight, const float* save_mean,
                             const float* save_invstd, const double* gathered, int world,
                             float* dx, int64_t lddx, void* stream);

/* ---- optimizer ------------------------------------------------------------ */
/* torch.optim.Adam (fused, capturable; L2 weight decay added to the gradient)
 * on ONE flat fp32 parameter buffer of n elements (hlhgat.train.TrainStep
 * keeps every parameter there), the reference's optimiser
 * (main_zinc_*.py).  `step` is the device fp32 step count: the update uses
 * step + 1, as torch increments it before the update, and a one-thread
 * launch then stores it.  Same double-precision hyper-parameter arithmetic
 * as torch's fused Adam (up to FMA contraction). */
int hlhgat_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     int64_t n, float* step, double lr, double beta1, double beta2, double eps,
                     double weight_decay, void* stream);
/* The same update split around the step's backward, one launch fewer:
 * hlhgat_adam_prepare (at the start of the step) zeroes the n-element
 * gradient buffer and increments `step`; hlhgat_adam_flat_prepared (after the
 * backward) is hlhgat_adam_flat using `step` as already incremented.  The
 * pair gives the bits of zeroing the gradient + hlhgat_adam_flat. */
int hlhgat_adam_prepare(float* grad, int64_t n, float* step, void* stream);
int hlhgat_adam_flat_prepared(float* param, const float* grad, float* exp_avg,
                              float* exp_avg_sq, int64_t n, const float* step, double lr,
                              double beta1, double beta2, double eps, double weight_decay,
                              void* stream);
/* The two entries above with the learning rate as device state: lr_dev points
 * to ONE fp64 value on the device (8-byte aligned), read by the update's own
 * launch (no extra launch), so a launch captured into a hipGraph follows a
 * scheduler that rewrites the value between replays.  fp64, not torch's fp32
 * tensor-lr convention: the arithmetic is the by-value entries' on the same
 * double, so *lr_dev == lr gives the same bits (float(1e-3) promoted to double
 * is not 1e-3).  Betas, eps and weight decay stay by-value constants. */
int hlhgat_adam_flat_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                         int64_t n, float* step, const double* lr_dev, double beta1,
                         double beta2, double eps, double weight_decay, void* stream);
int hlhgat_adam_flat_dev_prepared(float* param, const float* grad, float* exp_avg,
                                  float* exp_avg_sq, int64_t n, const float* step,
                                  const double* lr_dev, double beta1, double beta2, double eps,
                                  double weight_decay, void* stream);

/* L1 loss, torch.nn.L1Loss(reduction="mean") of the ZINC training loop
 * (torch's sub / abs / mean and its five backward launches):
 *   fwd: loss[0] = sum_i |x_i - y_i| / n   (one workgroup, fixed order);
 *   bwd: dx_i = (gout[0] / n) * sgn(x_i - y_i), torch's MeanBackward then
 *        AbsBackward arithmetic (sgn(0) = sgn(NaN) = 0): bitwise torch's dx.
 * gout is a device scalar (the upstream gradient of the loss). */
int hlhgat_l1_loss_fwd(const float* x, const float* y, int64_t n, float* loss, void* stream);
int hlhgat_l1_loss_bwd(const float* x, const float* y, int64_t n, const float* gout, float* dx,
                       void* stream);

/* BCE with logits, torch.nn.BCEWithLogitsLoss (no weight / pos_weight) of the
 * peptides-func and TSP loops (main_pepfunc...:181-183, main_TSP...:316-321):
 * loss = sum_i ((1 - y_i) x_i - log_sigmoid(x_i)) / div (div = n: "mean",
 * 1: "sum"), one workgroup, fixed summation order; backward
 * dx = (g / div) (sigmoid(x) - y) in ATen's MulBackward + LogSigmoidBackward
 * arithmetic.  One launch each way. */
int hlhgat_bce_logits_fwd(const float* x, const float* y, int64_t n, float div, float* loss,
                          void* stream);
int hlhgat_bce_logits_bwd(const float* x, const float* y, int64_t n, float div,
                          const float* gout, float* dx, void* stream);

/* Mean squared error (csrc/loss.hip), torch.nn.MSELoss of the brain notebook
 * (HL-HGAT-DEMO/OHBM_DEMO.ipynb: `criterion = torch.nn.MSELoss()` in the
 * training cell; its test() accumulates the same sum of squares in the
 * `rmse += ...` line).  The conventions of the two entries above:
 *   fwd: loss[0] = (sum_i (x_i - y_i)^2) / div  (div = n: "mean", 1: "sum");
 *        one launch, one workgroup: thread t adds elements t, t + 256, ... in
 *        order, then one LDS tree.  No floating-point atomics, no host read;
 *   bwd: dx_i = (x_i - y_i) * (2 gout[0] / div), one grid-stride launch, gout
 *        a device scalar.
 * A NaN in x or y gives a NaN loss and a NaN in its own dx element only, as
 * in torch.  n > 0, div > 0 and non-NULL pointers, checked before any launch
 * (HLHGAT_ERR_ARG). */
int hlhgat_mse_loss_fwd(const float* x, const float* y, int64_t n, float div, float* loss,
                        void* stream);
int hlhgat_mse_loss_bwd(const float* x, const float* y, int64_t n, float div, const float* gout,
                        float* dx, void* stream);

/* ---- reduced training losses (csrc/loss.hip) ----------------------------- */
/* Structure shared by the two families below.  No floating-point atomics and
 * no hand-off between workgroups inside a launch: the forward is a grid kernel
 * writing one 32-byte partial record per workgroup into `workspace`, then a
 * one-workgroup finish kernel that sums the records in index order with a
 * fixed tree.  The grid is min(ceil(n / 4096), 256) workgroups, a function of
 * n alone (never of the device), each thread walking its elements in a fixed
 * order; n <= 16384 runs as ONE self-finishing workgroup (one launch, the
 * workspace may be NULL).  Results are therefore a function of the inputs:
 * bitwise equal across runs, streams, pointer alignments, eager or replayed.
 * hlhgat_loss_workspace_bytes(n): the bytes `workspace` must hold (16-byte
 * aligned) for n elements (BCE) or n rows (cross-entropy).
 * Empty selection (cnt == 0): loss = 0 and dx = 0 everywhere.  torch returns
 * NaN for the mean of nothing; one all-missing batch must not poison Adam
 * inside a captured step, so this library differs here on purpose.
 * The backwards are one grid-stride elementwise launch reading the forward's
 * device scalars (sum, stats[0]); gout is a device scalar. */
#define HLHGAT_LOSS_MEAN 0
#define HLHGAT_LOSS_SUM 1
#define HLHGAT_LOSS_FOCAL 2
size_t hlhgat_loss_workspace_bytes(int64_t n);

/* BCE with logits over an on-device selection: the objective of the
 * peptides-func loop, FocalLoss()(out[mask], y[mask]) with mask = ~isnan(y)
 * (main_pepfunc...:179-186,267), of the TSP loop, FocalLoss() on the per-edge
 * logits (main_TSP...:59-71,321,397), and lib/Loss_function.py:14-26, without
 * the data-dependent boolean gather.  Element i is included iff (mask == NULL
 * or mask[i] != 0) and not (ignore_nan and y_i is NaN); the x and y of an
 * excluded element enter no sum.  With I the included set, cnt = |I|:
 *   S = sum_{i in I} ((1 - y_i) x_i - log_sigmoid(x_i)),
 *       log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|));
 *   SUM: loss = S;  MEAN: loss = S / cnt;
 *   FOCAL: b = S / cnt, loss = scale alpha (1 - e^-b)^gamma b, 1 - e^-b taken
 *       as -expm1f(-b); gamma = 0 (loss = scale alpha b) or gamma >= 1.
 *   sum[0] = S; stats[0..3] = cnt, tp, fp, fn over I with prediction x > 0 and
 *       positive label y > 0.5 (the F1 counts of main_TSP...:346-347);
 *       per-workgroup counts are int32, the totals int64.
 *   bwd: dx_i = gout c (sigmoid(x_i) - y_i) for i in I, +0.0 otherwise;
 *       c = 1 (SUM), 1 / cnt (MEAN),
 *       scale alpha ((1-pt)^gamma + gamma (1-pt)^(gamma-1) pt b) / cnt (FOCAL,
 *       pt = e^-b); sigmoid(x) - y in hlhgat_bce_logits_bwd's stable form.
 * 16-byte loads when x, y (dx) are 16-byte and mask 4-byte aligned, a scalar
 * path otherwise, both in the same per-thread order. */
int hlhgat_bce_reduce_fwd(const float* x, const float* y, const unsigned char* mask, int64_t n,
                          int ignore_nan, int reduction, float alpha, float gamma, float scale,
                          void* workspace, size_t workspace_bytes, float* loss, float* sum,
                          int64_t* stats, void* stream);
int hlhgat_bce_reduce_bwd(const float* x, const float* y, const unsigned char* mask, int64_t n,
                          int ignore_nan, int reduction, float alpha, float gamma, float scale,
                          const float* sum, const int64_t* stats, const float* gout, float* dx,
                          void* stream);

/* Cross-entropy over the rows of x [rows, cols] (row stride ldx >= cols: a
 * column block of a wider tensor works), torch.nn.CrossEntropyLoss() of the
 * CIFAR10SP loop (main_cifar10SP...:137,203); 1 <= cols <=
 * HLHGAT_CE_MAX_CLASSES, one thread per row:
 *   loss_r = log sum_j exp(x_rj - m_r) + m_r - x_{r,label_r}, m_r = max_j x_rj;
 *   MEAN: loss = sum_valid loss_r / cnt (torch: the non-ignored rows);
 *   SUM: loss = sum_valid loss_r;
 *   stats[0..1] = cnt, correct (rows whose lowest-index maximum is the label:
 *       the accuracy the loop prints);
 *   bwd: dx_rj = gout / cnt (softmax_rj - [j == label_r]) (SUM: gout) on
 *       valid rows, +0.0 on ignored rows; columns cols..lddx-1 of dx are
 *       never written.
 * A label equal to ignore_index is ignored.  A label that is neither that
 * nor in [0, cols) is ignored too, indexes nothing, and raises
 * HLHGAT_DEVERR_LABEL in the device error word (torch device-asserts). */
#define HLHGAT_CE_MAX_CLASSES 64
int hlhgat_cross_entropy_fwd(const float* x, int64_t ldx, int64_t rows, int64_t cols,
                             const int64_t* label, int64_t ignore_index, int reduction,
                             void* workspace, size_t workspace_bytes, float* loss,
                             int64_t* stats, void* stream);
int hlhgat_cross_entropy_bwd(const float* x, int64_t ldx, int64_t rows, int64_t cols,
                             const int64_t* label, int64_t ignore_index, int reduction,
                             const int64_t* stats, const float* gout, float* dx, int64_t lddx,
                             void* stream);

/* ---- evaluation metrics (csrc/metrics.hip) -------------------------------- */
/* Average precision per class, the reference's eval_ap
 * (lib/Hodge_Dataset.py:73-94: scikit-learn's average_precision_score per
 * column over the rows whose label is not NaN) without the host round trip.
 * pred [n, C] fp32 scores (row stride ldp >= C), label [n, C] fp32 (row
 * stride ldl >= C; NaN = unlabelled).  Per class c:
 *   the rows with a NaN label are dropped; the m others are sorted by score,
 *   descending; rows with equal scores (-0.0 == +0.0) form one threshold
 *   group; tp_k = positives (label == 1) up to the end of group k, r_k = the
 *   1-based index of its last row, P = all positives;
 *   ap[c] = sum_k ((tp_k - tp_{k-1}) / P) * (tp_k / r_k)  in fp64;
 *   counts[c] = {labelled rows m, labels == 1, labels == 0} (int32);
 *   the class is valid iff it has a label == 1 and a label == 0; an invalid
 *   class, or one with a non-finite score in a labelled row (scikit-learn
 *   raises), gets ap[c] = NaN.
 * A non-NaN label other than 0 or 1 counts as a negative (in neither the
 * positives nor the zeros) and raises HLHGAT_DEVERR_METRIC_LABEL.
 * Two launches around one hipcub radix sort of n*C 64-bit keys (class |
 * unlabelled bit | order-preserving image of the score) with a one-byte
 * value: the keys, the sort, then one workgroup per class walks its sorted
 * segment.  No
 * floating-point atomics, a fixed summation order (each thread adds the terms
 * of its rows in row order, then one fixed tree): a function of the inputs,
 * bitwise equal across runs, eager or replayed.  No host synchronisation and
 * no allocation (temporary storage is `workspace`, at least
 * hlhgat_average_precision_workspace_bytes(n, C) bytes, 256-byte aligned), so
 * the call captures into a hipGraph.  n * C < 2^31. */
size_t hlhgat_average_precision_workspace_bytes(int64_t n, int64_t C);
int hlhgat_average_precision(const float* pred, int64_t ldp, const float* label, int64_t ldl,
                             int64_t n, int64_t C, double* ap, int32_t* counts,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The meters of the reference's other test() loops.  Like the average
 * precision: no floating-point atomics, a fixed summation order, no host
 * synchronisation and no allocation, so every call captures into a hipGraph
 * and an eager and a replayed run give the same bits. */

/* The device-side `y_pred.extend(out)` (OHBM_DEMO.ipynb, train / test cells;
 * the torch.cat of y_preds / y_trues, main_pepfunc...:201-225): appends the n
 * rows of x [n, d] (fp32, row stride ldx >= d) to buf [capacity, d] at row
 * *cursor (int64, device memory), then advances *cursor by n on the device, so
 * a replayed launch appends behind the previous replay's rows.  If
 * *cursor + n > capacity nothing is written, the cursor stays, and
 * HLHGAT_DEVERR_METER_FULL is raised.  n == 0 is a no-op; d >= 1.  One launch
 * of one workgroup (an append is one batch's outputs). */
int hlhgat_collect_rows(const float* x, int64_t ldx, int64_t n, int64_t d, float* buf,
                        int64_t capacity, int64_t* cursor, void* stream);

/* torchmetrics' BinaryF1Score() (threshold 0.5) of every graph of a batch: the
 * body of the TSP loop (main_TSP_HL_HGCNN_dense_int3_pyr.py:344-347: unbatch,
 * then one f1() call per graph).  logit [rows] fp32 (element stride ldp),
 * label [rows] fp32 (element stride ldy), seg_ptr [n_graphs + 1] int32 row
 * offsets (graph g owns rows seg_ptr[g] .. seg_ptr[g+1]-1; rows from
 * seg_ptr[n_graphs] on, static-shape padding, belong to no graph; offsets are
 * clamped to [0, rows]).  Per graph:
 *   inside = every logit p of the graph has 0 <= p && p <= 1 (a NaN fails);
 *   pred = p > 0.5f if inside, else 1 / (1 + expf(-p)) > 0.5f in fp32;
 *   tp, fp, fn = integer counts, label == 1 positive, anything else negative;
 *   f1[g] = (float)(2 tp) / (float)(2 tp + fp + fn), one correctly rounded
 *   fp32 division, 0 when the denominator is 0 (a graph of 0 rows too).
 * A label other than 0 or 1 raises HLHGAT_DEVERR_METRIC_LABEL.  One launch,
 * one workgroup per graph. */
int hlhgat_f1_per_graph(const float* logit, int64_t ldp, const float* label, int64_t ldy,
                        const int32_t* seg_ptr, int64_t n_graphs, int64_t rows, float* f1,
                        void* stream);

/* The CIFAR loop's accuracy count (main_cifar10SP_HL_HGCNN_dense_int3_attpool
 * .py:146-161: correct += argmax(out, 1) == y): *correct += the rows of
 * x [n, C] (fp32, row stride ldx >= C) whose argmax is label[r] (int64), and,
 * if seen is not NULL, *seen += n; both int64 in device memory, added by one
 * thread.  The argmax is the first index of the greatest value with NaN
 * greatest (torch's CPU rule).  A label outside [0, C) matches nothing and
 * raises HLHGAT_DEVERR_METRIC_LABEL.  One launch of one workgroup; C >= 1. */
int hlhgat_argmax_correct(const float* x, int64_t ldx, int64_t n, int64_t C,
                          const int64_t* label, int64_t* correct, int64_t* seen, void* stream);

/* The end of a regression epoch over the collected pred / y (fp32, contiguous,
 * N = min(*count, capacity) values each, *count int64 in device memory: the
 * collector's cursor): ZINC's summed |out - y|
 * (main_zinc_HL_HGCNN_dense_int3_pyr.py:165-177) and the notebook's L1, RMSE
 * and standardised correlation (OHBM_DEMO.ipynb, train / test cells).  In
 * fp64, two passes, one workgroup, a fixed tree:
 *   out[0..7] = N, sum |d|, sum d^2 (d = pred - y), mean_p, mean_y,
 *               std_p, std_y (unbiased, torch's .std()),
 *               corr = sum (p - mean_p)(y - mean_y) / (N std_p std_y)
 *                    = mean(z(pred) * z(y)).
 * N == 0: the means are NaN; N < 2 or a zero deviation: corr is NaN, as in
 * torch. */
int hlhgat_regression_summary(const float* pred, const float* y, const int64_t* count,
                              int64_t capacity, double* out, void* stream);

/* ---- workspaces --------------------------------------------------------- */
/* Zero `bytes` (a multiple of 4) at p with a kernel on `stream` (graph-capture
 * safe; used to initialise the BatchNorm workspace counters). */
int hlhgat_zero_fill(void* p, size_t bytes, void* stream);

/* n <= HLHGAT_MAX_COPY_BLOCKS strided fp32 rectangles in ONE launch:
 * dst[b][r*ldd[b] + c] = src[b] ? src[b][r*lds[b] + c] : 0, r < rows[b],
 * c < cols[b].  Packs the NodeEdgeInt first-Linear weights (replaces the
 * torch.cat of lib/Hodge_Cheb_Conv.py:307-308's split weight blocks). */
#define HLHGAT_MAX_COPY_BLOCKS 64
int hlhgat_copy2d_batched(int n, const float* const* src, const int64_t* lds,
                          float* const* dst, const int64_t* ldd, const int64_t* rows,
                          const int64_t* cols, void* stream);

/* ---- device error word ------------------------------------------------- */
/* A host-visible (pinned, mapped) word that kernels raise bits in when they
 * detect a condition whose results must not be used.  Reading it does not
 * synchronise: it shows what kernels that have completed so far reported
 * (callers synchronise first for an exact answer).  hlhgat.ops.
 * check_device_errors / hlhgat.train.TrainStep raise RuntimeError on it. */
/* a BatchNorm arrival counter was found beyond its total (its workspace was
 * written by something else, or shared by concurrent launches): that launch's
 * statistics are not trusted */
#define HLHGAT_DEVERR_BN_STATE 1u
/* hlhgat_hodge_build: a row of L0 / L1 would end past the buffers the caller
 * sized (the row pointers do not describe a simple graph's Laplacians) */
#define HLHGAT_DEVERR_HODGE_SIZE 2u
/* hlhgat_cross_entropy_fwd: a label that is neither ignore_index nor a class
 * index; its row was left out of the loss and the gradient */
#define HLHGAT_DEVERR_LABEL 4u
/* hlhgat_average_precision: a label that is neither NaN, 0 nor 1; its row was
 * counted as a negative.  hlhgat_f1_per_graph: a label other than 0 or 1,
 * counted as a negative.  hlhgat_argmax_correct: a label outside [0, C) */
#define HLHGAT_DEVERR_METRIC_LABEL 8u
/* hlhgat_collect_rows: the rows did not fit the buffer; none was appended */
#define HLHGAT_DEVERR_METER_FULL 16u
/* hlhgat_eig_pe: a graph has more nodes than the caller's max_nodes (which
 * sized its workspace slice); its pe rows are zero and its lmax is 0.
 * hlhgat_eig_pe_edges: more edges than max_edges; its pe rows are zero */
#define HLHGAT_DEVERR_EIGPE_SIZE 32u
/* hlhgat_mlgc_device: an edge end outside its graph's node range, a perm entry
 * outside [0, n), or graph offsets that leave the arrays / the workspace; the
 * offender was treated as absent */
#define HLHGAT_DEVERR_MLGC_RANGE 64u
/* hlhgat_tseries_map: a series length outside [1, t_max], or
 * hlhgat_fc_prepare_windows: a window that is shorter than two samples, longer
 * than t_max or leaves the row; the offender was clamped into range */
#define HLHGAT_DEVERR_TSERIES_LEN 128u
int hlhgat_device_errors(unsigned* out);
int hlhgat_clear_device_errors(void);

/* ---- streams ------------------------------------------------------------ */
/* A HIP stream of the library's own on `device` (the capture, copy and side
 * streams of hlhgat.train.TrainStep / hlhgat.loader.StagedFeed / the node and
 * edge chains: never one of torch's round-robin pool streams, which two
 * unrelated users can be handed at once).  Created by the HIP runtime this
 * library is linked against -- the one torch loaded (same SONAME), so the
 * handle is valid in torch.cuda.ExternalStream.  cu_mask_words > 0: the stream
 * runs only on the CUs whose bits are set (hipExtStreamCreateWithCUMask; bit
 * c of word c/32 = CU c; the words must cover every CU of the device) -- the
 * config-3 per-sample producer's stream (hlhgat.pipeline), so the replayed
 * step keeps the other CUs.  flags: hipStreamNonBlocking (1) etc., unmasked
 * streams only; priority != 0: hipStreamCreateWithPriority (lower = higher
 * priority, hipDeviceGetStreamPriorityRange), unmasked streams only.  The reference has no streams (one implicit CUDA stream,
 * main_*.py); these are plumbing of the drop-in's own training loop. */
int hlhgat_stream_create(int device, unsigned flags, int priority, const uint32_t* cu_mask,
                         int cu_mask_words, void** out);
/* The CU mask a stream runs on (hipExtStreamGetCUMask): all ones for an
 * unmasked stream. */
int hlhgat_stream_cu_mask(void* stream, uint32_t* cu_mask, int cu_mask_words);

/* Test hook: `workgroups` workgroups of 64 threads with lds_bytes of LDS
 * each; the first `hold` of them stay resident for `usec` microseconds (time
 * bounded), the others exit at once -- a kernel that holds most CUs while
 * another stream's kernel runs (tests of the BatchNorm barrier). */
int hlhgat_test_occupy(int workgroups, int hold, int lds_bytes, unsigned usec, void* stream);

/* ---- live kernel timing ------------------------------------------------ */
#define HLHGAT_PROF_POLY 0 /* SpMM / fused polynomial step kernel */
#define HLHGAT_PROF_PROJ 1 /* MFMA projection forward */
#define HLHGAT_PROF_HODGE_NODE 2 /* factored L1, stage 1: Z = B1 X (node rows) */
#define HLHGAT_PROF_HODGE_EDGE 3 /* factored L1, stage 2: k_hodge_edge_step */
#define HLHGAT_PROF_PROJ_BWD 4 /* Linear backward: k_proj_bwd_fused (weight partials + data grad) */
#define HLHGAT_PROF_BN_FWD 5 /* BatchNorm forward: k_bn_fwd_grid / k_bn_stats + k_bn_apply */
#define HLHGAT_PROF_BN_BWD 6 /* BatchNorm backward: k_bn_bwd_reduce + k_bn_bwd_apply */
#define HLHGAT_PROF_PROJ_BN 7 /* projection + BatchNorm forward in one launch: k_proj_bn_fwd */
/* call sites of k_poly_step beside the Laplacian basis (HLHGAT_PROF_POLY):
 * the adjoint recurrence of the basis backward (hlhgat_poly_basis_bwd*), and
 * the |B1| incidence gathers of NodeEdgeInt (hlhgat_incidence_step: node
 * rows gathering edge rows, x_s2t of lib/Hodge_Cheb_Conv.py:294 and the
 * node-side adjoint of x_t2s, :295); k_edge_gather2 (edge rows gathering
 * their two node rows: x_t2s and the adjoint of x_s2t) */
#define HLHGAT_PROF_POLY_ADJ 8
#define HLHGAT_PROF_INCIDENCE 9
#define HLHGAT_PROF_GATHER2 10
#define HLHGAT_PROF_NCLASS 11
/* Enable (1) / disable (0) event timing of the given kernel class. */
int hlhgat_prof_enable(int kernel_class, int enable);
int hlhgat_prof_reset(void);
/* Synchronises the recorded events and returns launch count, summed kernel
 * milliseconds, summed algorithmic bytes and flops for the class. */
int hlhgat_prof_read(int kernel_class, int64_t* launches, double* total_ms,
                     double* total_bytes, double* total_flops);

/* ---- captured-graph introspection (runtime) ----------------------------- */
/* Introspection of a captured graph: its kernel nodes, and those whose
 * kernel name contains name_part (e.g. "ncclDevKernel": RCCL's kernels). */
int hlhgat_graph_kernel_count(void* graph, const char* name_part, int64_t* kernels,
                              int64_t* matching);

/* ---- temporal front end (Inception1D of the DEMO brain model) ----------- */
/* Activations are channels-last: x [n, t, c] row-major, i.e. an [n*t, c]
 * matrix whose rows the BatchNorm entries take unchanged.  taps is odd and at
 * most 5; the zero padding of taps/2 applies per series at both ends. */

/* Packs nb branch weights in nn.Conv1d layout w[b] [cout_b[b]][cin][taps_b[b]]
 * (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:485-487, :490-492: kernel sizes 1, 3, 5
 * on one input) into one weight of `taps` taps with structural zeros, the
 * branches' output channels concatenated (the torch.cat of :505, :509):
 * flip_transpose = 0: wp [taps][Cout][cin] for hlhgat_tconv_fwd;
 * flip_transpose = 1: wp [taps][cin][Cout] with the taps reversed, the weight
 * with which hlhgat_tconv_fwd(dy, cin := Cout, cout := cin) is the data
 * gradient. */
int hlhgat_tconv_pack(int nb, const float* const* w, const int64_t* cout_b,
                      const int32_t* taps_b, int64_t cin, int taps, int flip_transpose,
                      float* wp, void* stream);

/* y[n][t][co] = bias[co] + sum_k sum_ci x[n][t + k - taps/2][ci] * wp[k][co][ci]
 * (F.conv1d with padding taps/2 on the transposed layout, :502-504, :506-508):
 * implicit GEMM on the fp32 MFMA.  bias may be NULL.  Output columns [0, n1)
 * are declared to have only their centre tap non-zero and [n1, n1 + n3) only
 * the centre three (the 1- and 3-tap branches of a packed weight): their
 * 16-column tiles skip the other taps.  n1 = n3 = 0 for a dense weight. */
int hlhgat_tconv_fwd(const float* x, int64_t n, int64_t t, int64_t cin, const float* wp,
                     const float* bias, int64_t cout, int taps, int64_t n1, int64_t n3,
                     float* y, void* stream);

/* The embedding nn.Conv1d(1, c, taps, padding=taps/2) (:483, :501) on
 * x [n, t] with w [c][1][taps]: y [n, t, c]. */
int hlhgat_tconv_embed_fwd(const float* x, int64_t n, int64_t t, const float* w,
                           const float* bias, int64_t c, int taps, float* y, void* stream);

/* Scratch floats needed by hlhgat_tconv_bwd_weight. */
int64_t hlhgat_tconv_bwd_weight_workspace_floats(int64_t n, int64_t t, int64_t cin,
                                                 int64_t cout, int taps);

/* Weight and bias gradient of hlhgat_tconv_fwd (the autograd of :502-508):
 * dW[k][co][ci] = sum_{n,t} dy[n][t][co] * x[n][t + k - taps/2][ci], written
 * to the nb branches' gradients dw[b] in their nn.Conv1d layout (see
 * hlhgat_tconv_pack), and dbias[co] = sum dy (dbias [cout], may be NULL).
 * Per-workgroup partial sums in `workspace`, reduced in a fixed order: no
 * atomics, bitwise reproducible. */
int hlhgat_tconv_bwd_weight(const float* x, const float* dy, int64_t n, int64_t t,
                            int64_t cin, int64_t cout, int taps, int nb, float* const* dw,
                            const int64_t* cout_b, const int32_t* taps_b, float* dbias,
                            float* workspace, int64_t workspace_floats, void* stream);

/* Output length of nn.MaxPool1d(m, stride=m-1, padding=(m-1)/2) (:488). */
int64_t hlhgat_maxpool_time_len(int64_t t, int m);

/* LeakyReLU(slope) then that max-pool over time (:505): y and idx
 * [n, t', c], idx = the time step of the window's first maximum (the padding
 * counts as -inf). */
int hlhgat_leaky_maxpool_time_fwd(const float* x, int64_t n, int64_t t, int64_t c, int m,
                                  float slope, float* y, int32_t* idx, void* stream);
/* dx[n][t][c] = (x > 0 ? 1 : slope) * sum of dy over the windows whose
 * maximum is step t (gather form, fixed order). */
int hlhgat_leaky_maxpool_time_bwd(const float* x, const float* dy, const int32_t* idx,
                                  int64_t n, int64_t t, int64_t c, int m, float slope,
                                  float* dx, void* stream);

/* LeakyReLU(slope) then [max_t | mean_t] (:509-513): y [n, 2c], idx [n, c] the
 * step of the first maximum. */
int hlhgat_time_readout_fwd(const float* x, int64_t n, int64_t t, int64_t c, float slope,
                            float* y, int32_t* idx, void* stream);
int hlhgat_time_readout_bwd(const float* x, const float* dy, const int32_t* idx, int64_t n,
                            int64_t t, int64_t c, float slope, float* dx, void* stream);

/* ---- ragged time layout: series of different lengths in one batch -------- */
/* Brain_MLGC_ALL.get (HL-HGAT-DEMO/lib/Hodge_Dataset.py:131-133) crops every
 * sample to its own window, t_begin in [0, 75) and a length in [250, 300); the
 * reference then runs Inception1D one batch = one length, because rows of
 * different widths do not collate.  Channels-last activations do: series s
 * owns rows [soff[s], soff[s] + len[s]) of a buffer of n_series * t_max rows
 * (a fixed capacity, so no shape depends on the lengths); rows from
 * n_rows = sum len on are dead.  Stage 0 is the layout before the max-pool
 * (lengths len[s], capacity per series t_max[0]), stage 1 the one after it
 * (hlhgat_maxpool_time_len(len[s], pool) and t_max[1] =
 * hlhgat_maxpool_time_len(t_max[0], pool)).  All tables live on the device:
 *   soff[i]  int32 [n_series + 1]  series offsets (soff[i][n_series] = n_rows[i])
 *   tab[i]   int32 [capacity_i][2] per row (step within its series, series
 *                                  length); (0, 0) on a dead row
 *   sid[i]   int32 [capacity_i]    per row its series (0 on a dead row)
 *   n_rows   int32 [2]             the valid-row prefix of either stage: the
 *                                  n_valid of the BatchNorm entries
 * Every *_ragged entry is its dense twin (same tiles, staging, tap skipping,
 * chunking and reduction order: bit for bit the dense result when every
 * length is t_max) with the position predicate read from tab instead of
 * row % T; it never reads an input row >= n_rows and writes zeros to every
 * output row >= n_rows.  Per series the arithmetic is the reference's on that
 * series alone: zero padding at the window's own two ends (:483-492), the
 * pool length of its own length (:488), the mean over its own length (:512). */
typedef struct {
  int64_t n_series;
  int64_t t_max[2];
  int32_t pool; /* the max-pool window m (stride m - 1, padding (m - 1) / 2) */
  int32_t* soff[2];
  int32_t* tab[2];
  int32_t* sid[2];
  int32_t* n_rows;
} hlhgat_tseries_t;

/* Fills every table of `map` from tlen (int32 [n_series], device), in two
 * launches and without a host read: the lengths the reference draws at
 * lib/Hodge_Dataset.py:131-133.  A length outside [1, t_max[0]] is clamped
 * into it and raises HLHGAT_DEVERR_TSERIES_LEN. */
int hlhgat_tseries_map(const int32_t* tlen, const hlhgat_tseries_t* map, void* stream);
/* inverse = 0: the padded time courses src [n_series, ldx] (x[s][len[s]:] is
 * never read) as the compact stage-0 column dst [capacity_0] -- the
 * torch.unsqueeze(x, 1) of lib/Hodge_Cheb_Conv.py:500 on every window at once;
 * inverse = 1: its gradient, compact src -> padded dst, zeros past len[s]. */
int hlhgat_tseries_pack(const float* src, int64_t ldx, const hlhgat_tseries_t* map, int inverse,
                        float* dst, void* stream);
/* hlhgat_tconv_fwd (:502-504, :506-508, and its data gradient) on the rows of
 * `stage`: x [capacity, cin] -> y [capacity, cout]. */
int hlhgat_tconv_fwd_ragged(const float* x, const hlhgat_tseries_t* map, int stage, int64_t cin,
                            const float* wp, const float* bias, int64_t cout, int taps,
                            int64_t n1, int64_t n3, float* y, void* stream);
/* hlhgat_tconv_embed_fwd (:483, :501) on the compact stage-0 column x. */
int hlhgat_tconv_embed_fwd_ragged(const float* x, const hlhgat_tseries_t* map, const float* w,
                                  const float* bias, int64_t c, int taps, float* y,
                                  void* stream);
/* hlhgat_tconv_bwd_weight (the autograd of :501-508) on the rows of `stage`;
 * the workspace is that of (n_series, t_max[stage]).  The partial-sum slot of
 * a row chunk past n_rows is written as zeros, so the reduction is the dense
 * one. */
int hlhgat_tconv_bwd_weight_ragged(const float* x, const float* dy, const hlhgat_tseries_t* map,
                                   int stage, int64_t cin, int64_t cout, int taps, int nb,
                                   float* const* dw, const int64_t* cout_b,
                                   const int32_t* taps_b, float* dbias, float* workspace,
                                   int64_t workspace_floats, void* stream);
/* hlhgat_leaky_maxpool_time_fwd / _bwd (:488, :505): stage-0 rows in, stage-1
 * rows out, idx the step within the series. */
int hlhgat_leaky_maxpool_time_fwd_ragged(const float* x, const hlhgat_tseries_t* map, int64_t c,
                                         float slope, float* y, int32_t* idx, void* stream);
int hlhgat_leaky_maxpool_time_bwd_ragged(const float* x, const float* dy, const int32_t* idx,
                                         const hlhgat_tseries_t* map, int64_t c, float slope,
                                         float* dx, void* stream);
/* hlhgat_time_readout_fwd / _bwd (:509-513) on the stage-1 rows: y
 * [n_series, 2c], the mean divided by the series' own length. */
int hlhgat_time_readout_fwd_ragged(const float* x, const hlhgat_tseries_t* map, int64_t c,
                                   float slope, float* y, int32_t* idx, void* stream);
int hlhgat_time_readout_bwd_ragged(const float* x, const float* dy, const int32_t* idx,
                                   const hlhgat_tseries_t* map, int64_t c, float slope,
                                   float* dx, void* stream);

/* ---- training-mode feature dropout -------------------------------------- */
/* Dropout(p=dropout_ratio), the tail of every HL block (lib/Hodge_ST_Model.py:
 * 556-566; 0.25 in the CIFAR10SP, peptides-func and TSP training scripts),
 * with a counter-based mask instead of a stored one.  Element e = row * d + col
 * (a logical index, independent of ldx / ldy) takes word (e & 3) of
 *   philox4x32-10(counter {g lo, g hi, site, step lo}, key {seed lo, seed hi}),
 *   g = e >> 2,
 * and is kept iff (word >> 8) >= T, T = floor(p * 2^24) <= 2^24:
 *   y = keep ? x * s : 0,  s = float(1 / (1 - p)).
 * state = {seed, step}, two int64 in device memory read by the kernel (a
 * captured launch sees the step advanced between replays); site is the
 * caller's call counter.  The forward copies the {seed, step} it used to
 * snap (two int64, device); x / y are [n, d] with leading dimensions ldx /
 * ldy (y may be a column block of a wider slab).  n * d == 0 is a no-op. */
int hlhgat_dropout_fwd(const float* x, int64_t ldx, int64_t n, int64_t d, uint32_t T, float s,
                       const int64_t* state, uint32_t site, int64_t* snap, float* y,
                       int64_t ldy, void* stream);
/* dx = keep ? dy * s : 0 with the mask regenerated from the forward's snap
 * (no mask is stored); dy may be a column block of a gradient slab. */
int hlhgat_dropout_bwd(const float* dy, int64_t lddy, int64_t n, int64_t d, uint32_t T, float s,
                       const int64_t* snap, uint32_t site, float* dx, int64_t lddx,
                       void* stream);
/* state[1] += 1 (one thread): the next step's masks.  Capturable. */
int hlhgat_dropout_advance(int64_t* state, void* stream);

/* ---- simplex dropout: masked Hodge operators ---------------------------- */
/* The draw of dropout_node (main_TSP_HL_HGCNN_dense_int3_pyr.py:84-92: the
 * per-sample rate p + U/2, prob > rate, logical_or with y_loc) together with
 * the per-sample coin of TSP_EigPE.get (:125-131 == lib/Hodge_Dataset.py:
 * 696-701), for every graph of a batch in one launch, and the mask column
 * the reference appends to x_s (:138 == lib/Hodge_Dataset.py:707).
 * Counter-based like hlhgat_dropout_fwd: state = {seed, step} (two int64,
 * device) is read by the kernel, nothing is stored between steps.
 *   graph g (rows seg_ptr[g] .. seg_ptr[g+1]):
 *     (a0, a1, ., .) = philox4x32-10({g, 0, site, step lo}, {seed lo, seed hi})
 *     aug_g = (a0 >> 8) < Ta;   T_g = Tp + ((uint64(a1 >> 8) * Tj) >> 24)
 *   row e of graph g:
 *     u_e = word (e & 3) of philox({(e>>2) lo, (e>>2) hi, site + 1, step lo},
 *           key) >> 8
 *     keep_e = !aug_g || u_e >= T_g || protect[e * ldp] != 0
 *   rows in no graph (e >= seg_ptr[n_graphs], static-shape padding): 0.
 * Ta = floor(aug_prob 2^24), Tp = floor(p 2^24), Tj = floor(jitter 2^24), all
 * <= 2^24 and Tp + Tj <= 2^24; site = 0x80000000 + 2k (k: the caller's module
 * ordinal; the feature dropout's call counters never reach bit 31).  seg_ptr
 * is int32 [n_graphs + 1], ascending; protect (optional) is read at stride
 * ldp.  mask [n_rows] receives 1.0 / 0.0; col (optional) receives the same
 * values at stride ldc (x_s[:, 1]).  n_rows == 0 is a no-op. */
int hlhgat_simplex_keep(const int32_t* seg_ptr, int64_t n_graphs, int64_t n_rows,
                        const float* protect, int64_t ldp, uint32_t Ta, uint32_t Tp, uint32_t Tj,
                        uint32_t site, const int64_t* state, float* mask, float* col,
                        int64_t ldc, void* stream);
/* subgraph(node_mask, edge_index_s, edge_weight_s) without relabelling
 * (main_TSP_HL_HGCNN_dense_int3_pyr.py:93-95 == lib/Hodge_Dataset.py:163-165)
 * on a CSR operator whose structure stays: val_out[e] = val[e] if mask[row of
 * e] and mask[col[e]] are both non-zero, else 0 -- the values of M A M,
 * M = diag(mask), on A's own rowptr / col.  The SpMM and polynomial-step
 * entry points on (rowptr, col, val_out) return exactly what they return on
 * the filtered operator.  n_rows == 0 or nnz == 0 is a no-op. */
int hlhgat_mask_csr_values(const int32_t* rowptr, const int32_t* col, const float* val,
                           int64_t n_rows, int64_t nnz, const float* mask, float* val_out,
                           void* stream);
/* The same filter (:93-95) on a factored L1 = alpha B1^T B1: sign_out[k] =
 * node_sign[k] if mask[node_edge[k]] != 0 else 0 (incidence order, [2 n_edges])
 * and alpha_out[e] = alpha[e] if mask[e] != 0 else 0; the factor with these
 * two tables in place of node_sign / alpha is M L1 M.  One launch; only
 * node_edge, node_sign, alpha and n_edges of *f are read.  n_edges == 0 is a
 * no-op. */
int hlhgat_mask_hodge_factor(const hlhgat_hodge_factor_t* f, const float* mask, float* sign_out,
                             float* alpha_out, void* stream);

/* ---- PE sign-flip augmentation ------------------------------------------ */
/* The sign draw every stored dataset of the reference applies to the
 * eigenvector positional-encoding columns in get(), per sample and per access
 * (lib/Hodge_Dataset.py:425-440, :500-515, :554-569, :635-650, :869-881):
 *   sign = cat([ones(n_fixed), -1 + 2 * randint(0, 2, (n_flip,))])
 *   x = x[:, :n_fixed + n_flip] * sign
 * Counter-based like hlhgat_dropout_fwd: state = {seed, step} (two int64,
 * device) is read by the kernel, nothing is stored between steps.  Graph g,
 * flipped column j (0-based among the flipped columns):
 *   w    = word (j & 3) of philox4x32-10({g, 0x50450000 + (j >> 2), site,
 *                                         step lo}, {seed lo, seed hi})
 *   sign = (w >> 31) ? -1.0f : +1.0f
 * site < 2^30; the callers use 2k + side (k: the module's ordinal, side 0 = t,
 * 1 = s).  The second counter word lies above every value the feature dropout
 * and the simplex dropout can put there (the high half of an element index
 * >> 2, or 0), so the three draws never share a counter.
 *
 * One side of a flip: y[r][c] = x[r][c] for c < n_fixed and y[r][n_fixed + j]
 * = x[r][n_fixed + j] * sign(g(r), j) for j < n_flip, r < n_rows, where g(r) is
 * the graph with seg_ptr[g] <= r < seg_ptr[g + 1] (int32 [n_graphs + 1],
 * ascending).  Rows in no graph (r >= seg_ptr[n_graphs], static-shape
 * padding) are copied unflipped.  y is [n_rows, n_fixed + n_flip] at pitch
 * ldy; x may be wider (the extra columns are dropped, as x[:, :node_dim]
 * does) and may be a column window of a wider tensor (pitch ldx).  x and y
 * never alias.  n_fixed + n_flip <= 65536. */
typedef struct {
  const float* x;
  int64_t ldx;
  float* y;
  int64_t ldy;
  const int32_t* seg_ptr;
  int64_t n_graphs;
  int64_t n_rows;
  int32_t n_fixed;
  int32_t n_flip;
  uint32_t site;
} hlhgat_pe_side_t;
/* n_sides (1 or 2) sides in ONE launch, the grid partitioned between them.
 * snap (two int64, device) receives the {seed, step} used; snap == state is
 * allowed (a replay from a snapshot: the backward is this entry point on dy
 * with the forward's snap as state).  A side with n_rows == 0 or n_fixed +
 * n_flip == 0 moves nothing; when no side moves anything nothing is launched
 * and snap is left alone.  n_flip == 0 is a copy. */
int hlhgat_pe_flip(const hlhgat_pe_side_t* sides, int n_sides, const int64_t* state,
                   int64_t* snap, void* stream);
/* signs[g][j] (float [n_graphs, n_flip], contiguous) of the same draw at
 * `site`: +1.0 or -1.0.  n_graphs == 0 or n_flip == 0 is a no-op. */
int hlhgat_pe_signs(int64_t n_graphs, int64_t n_flip, uint32_t site, const int64_t* state,
                    float* signs, void* stream);

/* ---- brain input: z-scored series and functional connectivity ----------- */
/* The per-sample arithmetic of Brain_MLGC_ALL.get (HL-HGAT-DEMO/lib/
 * Hodge_Dataset.py:130-145) and of the cohort loop that feeds FC2mask
 * (:148-178; OHBM_DEMO.ipynb, FC[i] = torch.corrcoef(...)), for G graphs of N
 * regions at once.  x holds the series as rows of pitch ldx; graph g owns the
 * N rows from row graph_rows[g] (int64 [G], device) or, with graph_rows NULL,
 * from row g * N; the window is columns [t0, t0 + T).
 *
 * Bytes of the workspace for G graphs (0 when G <= 0, N <= 0 or T < 2): the
 * centred unit-norm rows at pitch roundup(T, 4) and two doubles per row. */
size_t hlhgat_fc_workspace_bytes(int64_t G, int64_t N, int64_t T);
/* The row pass (:136).  Per graph the mean and the UNBIASED std over its N * T
 * window elements, z = (x - mean_g) / std_g written contiguously as [G*N, T]
 * (z may be NULL: not wanted); per row the centred unit-norm row
 * (x_i - mean_i) / ||x_i - mean_i|| into the workspace (16-byte aligned).
 * Correlation is invariant to the graph's z-score, so the rows come from x
 * directly.  A row that is constant over the window (min == max) becomes NaN:
 * the exact-arithmetic 0 / 0 of the reference, whose own float result there is
 * rounding noise.  fp64 accumulators in a fixed order: bitwise reproducible,
 * and a graph's results do not depend on the other graphs of the call. */
int hlhgat_fc_prepare(const float* x, int64_t ldx, const int64_t* graph_rows, int64_t G,
                      int64_t N, int64_t t0, int64_t T, float* z, void* workspace,
                      size_t workspace_bytes, void* stream);
/* hlhgat_fc_prepare with a window per graph, the per-sample crop of
 * Brain_MLGC_ALL.get (lib/Hodge_Dataset.py:131-135: f = f[:, t_begin:t_begin +
 * length], then the z-score and corrcoef of that window): graph g reads
 * columns [t0[g], t0[g] + len[g]) (int32 [G], device), 2 <= len[g] <= t_max
 * and the window inside the ldx columns; a window outside that is clamped
 * into it and raises HLHGAT_DEVERR_TSERIES_LEN.  Mean and unbiased std over
 * the graph's own N x len[g] elements; z is [G*N, t_max] with zeros past
 * len[g], and the workspace rows are zero-padded to t_max, so hlhgat_fc_dense
 * / hlhgat_fc_edges run on it with T = t_max (workspace bytes: those of
 * T = t_max).  Same fp64 fixed-order accumulators: graph g's values are bit
 * for bit those of hlhgat_fc_prepare on that graph alone with (t0[g],
 * len[g]). */
int hlhgat_fc_prepare_windows(const float* x, int64_t ldx, const int64_t* graph_rows, int64_t G,
                              int64_t N, const int32_t* t0, const int32_t* len, int64_t t_max,
                              float* z, void* workspace, size_t workspace_bytes, void* stream);
/* fc[G, N, N] = torch.corrcoef of every graph's window (:137 before the
 * indexing; the FC stack of FC2mask, :148-153) from a prepared workspace:
 * fp32 MFMA on 64 x 64 tiles with row tile <= column tile, each value stored
 * at (i, j) and (j, i) (exactly symmetric), clamped to [-1, 1] as
 * torch.corrcoef clamps; NaN stays NaN. */
int hlhgat_fc_dense(const void* workspace, int64_t G, int64_t N, int64_t T, float* fc,
                    void* stream);
/* The skeleton's entries only (:137, corrcoef(...)[skeleton.indices()]):
 * pair2edge is int32 [N * N], -1 or the edge id (< E) of the pair (i, j),
 * i < j; tiles is int32 [n_tiles][2], the (row tile, column tile) pairs of
 * 64 x 64 tiles that hold an edge.  The value of edge e of graph g goes to
 * out[(g * E + e) * ld], bit for bit the dense entry; the dense stack is
 * never written.  Entries of out that belong to no edge are left alone. */
int hlhgat_fc_edges(const void* workspace, int64_t G, int64_t N, int64_t T,
                    const int32_t* pair2edge, int64_t E, const int32_t* tiles, int64_t n_tiles,
                    float* out, int64_t ld, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* HLHGAT_H_ */
