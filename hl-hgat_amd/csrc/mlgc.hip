// Multi-level graph coarsening (MLGC) for the attention-pooling heads: the
// graclus matching and the fine -> coarse node / edge assignment, as native
// HOST code (host pointers, no stream).  MLGC is dataset preprocessing in the
// reference (lib/Hodge_Dataset.py:241-353, run once per graph before
// training), so it sits beside the other collate-time builders
// (hlhgat_halo_tiles) rather than on the device: one pass over the edges,
// O(E log deg) for the matching and O(E) hashing for the edge map, no Python
// per-edge loops.  Config 3 coarsens every sample of every batch, and the
// brain model's MLGC_Weight adds two pruning passes (hlhgat_mlgc_prune): the
// second half of this file runs all of it for a whole batch in one launch
// (hlhgat_mlgc_device), bit for bit the host results.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <limits>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "common.h"

namespace {

// (lo, hi) coarse-node pair -> one 64-bit key (both < 2^31 by the size check)
inline uint64_t pair_key(int64_t lo, int64_t hi) {
  return ((uint64_t)lo << 32) | (uint64_t)(uint32_t)hi;
}

}  // namespace

// Greedy graclus matching (torch_cluster 1.6.0 graclus_cluster, its weighted
// branch -- the reference always passes a weight, ones_like for MLGC --
// called at lib/Hodge_Dataset.py:252 and :311): self-loops dropped, every
// node's neighbours in ascending column order, nodes visited in perm order;
// an unmatched node u keeps the LAST unmatched neighbour whose weight is >=
// the best so far (best starts at 0, so zero weights match) and both get id
// min(u, v); with no unmatched neighbour u stays alone with id u.  Restated
// from torch_cluster's published graclus_cpu (not in the reference tree):
// parity unpinned.
extern "C" int hlhgat_graclus(const int64_t* edge_index, const double* weight, int64_t n_edges,
                              int64_t n_nodes, const int64_t* perm, int64_t* cluster) {
  HLH_CHECK_ARG(n_edges >= 0 && n_nodes >= 0, "graclus: bad sizes");
  HLH_CHECK_ARG(cluster && (n_nodes == 0 || perm) && (n_edges == 0 || edge_index),
                "graclus: NULL pointer");
  const int64_t* row = edge_index;
  const int64_t* col = edge_index + n_edges;
  std::vector<int64_t> deg((size_t)n_nodes + 1, 0);
  for (int64_t e = 0; e < n_edges; ++e) {
    HLH_CHECK_ARG(row[e] >= 0 && row[e] < n_nodes && col[e] >= 0 && col[e] < n_nodes,
                  "graclus: edge %lld out of range", (long long)e);
    if (row[e] != col[e]) ++deg[(size_t)row[e] + 1];
  }
  std::partial_sum(deg.begin(), deg.end(), deg.begin());
  // CSR with (col, original position) per row, so a stable sort by column
  // reproduces the (row, col) lexsort of the restatement
  std::vector<int64_t> nb((size_t)deg[(size_t)n_nodes]);
  std::vector<double> nw(nb.size());
  {
    std::vector<int64_t> fill(deg.begin(), deg.end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) {
      if (row[e] == col[e]) continue;
      const int64_t p = fill[(size_t)row[e]]++;
      nb[(size_t)p] = e;
    }
    for (int64_t u = 0; u < n_nodes; ++u) {
      const int64_t b = deg[(size_t)u], f = deg[(size_t)u + 1];
      std::stable_sort(nb.begin() + b, nb.begin() + f,
                       [&](int64_t x, int64_t y) { return col[x] < col[y]; });
      for (int64_t p = b; p < f; ++p) {
        const int64_t e = nb[(size_t)p];
        nw[(size_t)p] = weight ? weight[e] : 1.0;
        nb[(size_t)p] = col[e];
      }
    }
  }
  for (int64_t u = 0; u < n_nodes; ++u) cluster[u] = -1;
  for (int64_t i = 0; i < n_nodes; ++i) {
    const int64_t u = perm[i];
    HLH_CHECK_ARG(u >= 0 && u < n_nodes, "graclus: perm[%lld] out of range", (long long)i);
    if (cluster[u] >= 0) continue;
    int64_t best = u;
    double wbest = 0.0;
    for (int64_t p = deg[(size_t)u]; p < deg[(size_t)u + 1]; ++p) {
      const int64_t v = nb[(size_t)p];
      if (cluster[v] >= 0) continue;
      if (nw[(size_t)p] >= wbest) {  // ties: the LAST such neighbour
        best = v;
        wbest = nw[(size_t)p];
      }
    }
    cluster[u] = cluster[best] = std::min(u, best);
  }
  return HLHGAT_OK;
}

// Fine -> coarse assignment of one MLGC level (lib/Hodge_Dataset.py:254-275):
// c_node = rank of the node's cluster id among the distinct ids; an edge whose
// ends share a coarse node gets +inf, the others the index of the coarse edge
// (min, max), numbered in first-seen edge order.
extern "C" int hlhgat_mlgc_map(const int64_t* cluster, int64_t n_nodes, const int64_t* edge_index,
                               int64_t n_edges, int64_t* c_node, float* c_edge,
                               int64_t* coarse_edges, int64_t* n_coarse_nodes,
                               int64_t* n_coarse_edges) {
  HLH_CHECK_ARG(n_edges >= 0 && n_nodes >= 0 && n_nodes < INT32_MAX, "mlgc_map: bad sizes");
  HLH_CHECK_ARG(n_coarse_nodes && n_coarse_edges && (n_nodes == 0 || (cluster && c_node)) &&
                    (n_edges == 0 || (edge_index && c_edge && coarse_edges)),
                "mlgc_map: NULL pointer");
  // cluster ids are node ids: rank = prefix count of the ids present
  std::vector<int64_t> rank((size_t)n_nodes + 1, 0);
  for (int64_t u = 0; u < n_nodes; ++u) {
    HLH_CHECK_ARG(cluster[u] >= 0 && cluster[u] < n_nodes, "mlgc_map: cluster id out of range");
    rank[(size_t)cluster[u] + 1] = 1;
  }
  std::partial_sum(rank.begin(), rank.end(), rank.begin());
  for (int64_t u = 0; u < n_nodes; ++u) c_node[u] = rank[(size_t)cluster[u]];
  const int64_t* row = edge_index;
  const int64_t* col = edge_index + n_edges;
  std::unordered_map<uint64_t, int64_t> key;
  key.reserve((size_t)n_edges);
  int64_t ne = 0;
  for (int64_t i = 0; i < n_edges; ++i) {
    HLH_CHECK_ARG(row[i] >= 0 && row[i] < n_nodes && col[i] >= 0 && col[i] < n_nodes,
                  "mlgc_map: edge %lld out of range", (long long)i);
    const int64_t a = c_node[row[i]], b = c_node[col[i]];
    if (a == b) {
      c_edge[i] = std::numeric_limits<float>::infinity();
      continue;
    }
    const int64_t lo = std::min(a, b), hi = std::max(a, b);
    auto it = key.emplace(pair_key(lo, hi), ne);
    if (it.second) {
      coarse_edges[ne] = lo;
      coarse_edges[n_edges + ne] = hi;
      ++ne;
    }
    c_edge[i] = (float)it.first->second;
  }
  *n_coarse_nodes = rank[(size_t)n_nodes];
  *n_coarse_edges = ne;
  return HLHGAT_OK;
}

// One MLGC level for a whole batch of graphs (SuperpixelPipeline.batch, the
// reference's per-sample get(), main_cifar10SP...:67-125): per graph, graclus
// on L0's pattern (the i<j edge list both ways, unit weights, node order
// perm) and the fine -> coarse map -- hlhgat_graclus + hlhgat_mlgc_map per
// graph, the graphs spread over n_threads host threads.  All indices are
// LOCAL to their graph; graph g's nodes are [node_ptr[g], node_ptr[g+1]) of
// perm / c_node, its edges [edge_ptr[g], edge_ptr[g+1]) of edges ([2][E]) /
// c_edge, and its coarse edges are written from column edge_ptr[g] of
// coarse_edges ([2][E], row stride E), coarse_n[g] / coarse_e[g] sizes.
extern "C" int hlhgat_mlgc_batch(int64_t n_graphs, const int64_t* node_ptr,
                                 const int64_t* edge_ptr, const int64_t* edges,
                                 const int64_t* perm, int n_threads, int64_t* c_node,
                                 float* c_edge, int64_t* coarse_edges, int64_t* coarse_n,
                                 int64_t* coarse_e) {
  HLH_CHECK_ARG(n_graphs >= 0 && node_ptr && edge_ptr && coarse_n && coarse_e,
                "mlgc_batch: bad arguments");
  const int64_t N = n_graphs ? node_ptr[n_graphs] : 0, E = n_graphs ? edge_ptr[n_graphs] : 0;
  HLH_CHECK_ARG(node_ptr[0] == 0 && edge_ptr[0] == 0 && (N == 0 || (perm && c_node)) &&
                    (E == 0 || (edges && c_edge && coarse_edges)),
                "mlgc_batch: bad offsets or NULL arrays");
  for (int64_t g = 0; g < n_graphs; ++g)
    HLH_CHECK_ARG(node_ptr[g + 1] >= node_ptr[g] && edge_ptr[g + 1] >= edge_ptr[g],
                  "mlgc_batch: offsets of graph %lld decrease", (long long)g);
  std::atomic<int64_t> next{0};
  std::atomic<int> rc_first{HLHGAT_OK};
  std::mutex msg_mu;
  std::string msg;
  auto worker = [&]() {
    std::vector<int64_t> both, ei, cl, ce;
    for (;;) {
      const int64_t g = next.fetch_add(1);
      if (g >= n_graphs || rc_first.load() != HLHGAT_OK) return;
      const int64_t n0 = node_ptr[g], n = node_ptr[g + 1] - n0;
      const int64_t e0 = edge_ptr[g], m = edge_ptr[g + 1] - e0;
      ei.resize((size_t)(2 * m));
      both.resize((size_t)(4 * m));
      for (int64_t k = 0; k < m; ++k) {
        const int64_t i = edges[e0 + k], j = edges[E + e0 + k];
        ei[(size_t)k] = i;
        ei[(size_t)(m + k)] = j;
        both[(size_t)k] = i;                // rows: i then j
        both[(size_t)(m + k)] = j;
        both[(size_t)(2 * m + k)] = j;      // cols: j then i
        both[(size_t)(3 * m + k)] = i;
      }
      cl.resize((size_t)n);
      ce.resize((size_t)std::max<int64_t>(2 * m, 2));
      int64_t n1 = 0, ne = 0;
      int rc = hlhgat_graclus(both.data(), nullptr, 2 * m, n, perm + n0, cl.data());
      if (rc == HLHGAT_OK)
        rc = hlhgat_mlgc_map(cl.data(), n, ei.data(), m, c_node + n0, c_edge + e0, ce.data(),
                             &n1, &ne);
      if (rc != HLHGAT_OK) {
        int ok = HLHGAT_OK;
        if (rc_first.compare_exchange_strong(ok, rc)) {
          std::lock_guard<std::mutex> lk(msg_mu);
          msg = std::string("graph ") + std::to_string(g) + ": " + hlhgat_last_error();
        }
        return;
      }
      for (int64_t k = 0; k < ne; ++k) {
        coarse_edges[e0 + k] = ce[(size_t)k];
        coarse_edges[E + e0 + k] = ce[(size_t)(m + k)];
      }
      coarse_n[g] = n1;
      coarse_e[g] = ne;
    }
  };
  const int T = std::max(1, std::min<int>(n_threads, (int)std::min<int64_t>(n_graphs, 64)));
  std::vector<std::thread> pool;
  for (int t = 1; t < T; ++t) pool.emplace_back(worker);
  worker();
  for (auto& th : pool) th.join();
  if (rc_first.load() != HLHGAT_OK) {
    hlhgat::set_error("mlgc_batch: %s", msg.c_str());
    return rc_first.load();
  }
  return HLHGAT_OK;
}

// The two pruning passes of the DEMO's MLGC_Weight (HL-HGAT-DEMO/lib/
// Hodge_Dataset.py:222-241) on hlhgat_mlgc_map's outputs, in place.  The
// reference keys a coarse edge by the float imax + 0.0001 * imin (:207); the
// integer pairs of hlhgat_mlgc_map are equivalent while a level has fewer
// than 10^4 coarse nodes (beyond that the reference's keys collide).
extern "C" int hlhgat_mlgc_prune(int64_t n_nodes, int64_t n_edges, unsigned flags,
                                 const int64_t* c_node_in, float* c_node, float* c_edge,
                                 int64_t* coarse_edges, int64_t* n_coarse_nodes,
                                 int64_t* n_coarse_edges) {
  constexpr int64_t kMax = (int64_t)1 << 24;  // ids stay exact as float32
  HLH_CHECK_ARG(n_nodes >= 0 && n_edges >= 0 && n_nodes < kMax && n_edges < kMax,
                "mlgc_prune: sizes must be in [0, 2^24)");
  HLH_CHECK_ARG((flags & ~(HLHGAT_MLGC_PRUNE_SINGLE | HLHGAT_MLGC_DROP_ISOLATED)) == 0,
                "mlgc_prune: unknown flag bits 0x%x", flags);
  HLH_CHECK_ARG(n_coarse_nodes && n_coarse_edges && (n_nodes == 0 || (c_node_in && c_node)) &&
                    (n_edges == 0 || (c_edge && coarse_edges)),
                "mlgc_prune: NULL pointer");
  int64_t n1 = *n_coarse_nodes, ne = *n_coarse_edges;
  HLH_CHECK_ARG(n1 >= 0 && n1 <= n_nodes && ne >= 0 && ne <= n_edges,
                "mlgc_prune: coarse counts out of range");
  int64_t* lo = coarse_edges;
  int64_t* hi = coarse_edges + n_edges;
  for (int64_t u = 0; u < n_nodes; ++u)
    HLH_CHECK_ARG(c_node_in[u] >= 0 && c_node_in[u] < n1, "mlgc_prune: c_node[%lld] out of range",
                  (long long)u);
  for (int64_t c = 0; c < ne; ++c)
    HLH_CHECK_ARG(lo[c] >= 0 && lo[c] < n1 && hi[c] >= 0 && hi[c] < n1,
                  "mlgc_prune: coarse edge %lld out of range", (long long)c);
  const float inf = std::numeric_limits<float>::infinity();
  for (int64_t i = 0; i < n_edges; ++i)
    HLH_CHECK_ARG(c_edge[i] == inf || (c_edge[i] >= 0.0f && c_edge[i] < (float)ne &&
                                       c_edge[i] == (float)(int64_t)c_edge[i]),
                  "mlgc_prune: c_edge[%lld] is neither +inf nor a coarse edge", (long long)i);
  if (flags & HLHGAT_MLGC_PRUNE_SINGLE) {
    std::vector<int64_t> support((size_t)ne, 0), newid((size_t)ne, -1);
    for (int64_t i = 0; i < n_edges; ++i)
      if (c_edge[i] != inf) ++support[(size_t)c_edge[i]];
    int64_t kept = 0;
    for (int64_t c = 0; c < ne; ++c) {
      if (support[(size_t)c] == 1) continue;
      lo[kept] = lo[c];  // kept <= c: the relative (first-seen) order stays
      hi[kept] = hi[c];
      newid[(size_t)c] = kept++;
    }
    for (int64_t i = 0; i < n_edges; ++i) {
      if (c_edge[i] == inf) continue;
      const int64_t k = newid[(size_t)c_edge[i]];
      c_edge[i] = k < 0 ? inf : (float)k;
    }
    ne = kept;
  }
  if (flags & HLHGAT_MLGC_DROP_ISOLATED) {
    std::vector<int64_t> nmap((size_t)n1 + 1, 0);
    for (int64_t c = 0; c < ne; ++c) nmap[(size_t)lo[c] + 1] = nmap[(size_t)hi[c] + 1] = 1;
    std::vector<char> used((size_t)n1);
    for (int64_t r = 0; r < n1; ++r) used[(size_t)r] = (char)nmap[(size_t)r + 1];
    std::partial_sum(nmap.begin(), nmap.end(), nmap.begin());
    for (int64_t c = 0; c < ne; ++c) {
      lo[c] = nmap[(size_t)lo[c]];
      hi[c] = nmap[(size_t)hi[c]];
    }
    for (int64_t u = 0; u < n_nodes; ++u) {
      const int64_t r = c_node_in[u];
      c_node[u] = used[(size_t)r] ? (float)nmap[(size_t)r] : inf;
    }
    n1 = nmap[(size_t)n1];
  } else {
    for (int64_t u = 0; u < n_nodes; ++u) c_node[u] = (float)c_node_in[u];
  }
  *n_coarse_nodes = n1;
  *n_coarse_edges = ne;
  return HLHGAT_OK;
}

// ---------------------------------------------------------------------------
// MLGC on the device (hlhgat_mlgc_device): hlhgat_mlgc_batch and
// hlhgat_mlgc_prune for a whole batch in one launch, one workgroup per graph.
//
// Phases of a workgroup (barriers between them):
//  1. matching: the visit loop is serial by definition (n dependent steps),
//     so ONE wave walks perm; within a step its 64 lanes stride u's incidence
//     list (the batch's incidence CSR: node -> incident edge ids, the other
//     end from edge_index) and one wave reduction picks the largest (w, id).
//     Every lane stores the step's two cluster ids itself, so what a lane reads
//     in a later step is ordered after its own stores.
//  2. c_node: flag the cluster ids present, exclusive scan = the rank.
//  3. c_edge: each cut edge puts its coarse pair into an open-addressing hash
//     (64-bit compare-and-swap on the key) and atomicMin's its own index into
//     the slot; the edge that owns its slot is the pair's FIRST fine edge, and
//     the exclusive scan of the owner flags in edge order is the first-seen
//     numbering -- deterministic whatever order the atomics land in.
//  4. pruning (flags): support count per coarse edge, scan of the kept ones;
//     coarse nodes touched by a kept edge, scan of those.
//  5. outputs.
// Per-graph state (cluster ids, hash, flags: 12 H + 16 (n + 1) + 24 (m + 1)
// bytes, H = the power of two >= 2 m) lives in LDS when it fits kMgLdsBytes,
// else in the graph's workspace slice at 64 g + 16 node_ptr[g] + 72
// edge_ptr[g] (H <= 4 m bounds it); both routes run the same code.
// ---------------------------------------------------------------------------
namespace {

constexpr int kMgThreads = 256;
constexpr int kMgWaves = kMgThreads / 64;
constexpr int kMgLdsBytes = 64 * 1024;
constexpr int64_t kMgMax = (int64_t)1 << 24;
constexpr unsigned kMgFlags =
    HLHGAT_MLGC_ONE_WAY | HLHGAT_MLGC_PRUNE_SINGLE | HLHGAT_MLGC_DROP_ISOLATED;
constexpr unsigned long long kMgEmpty = ~0ull;

__host__ __device__ inline int64_t mg_hash_size(int64_t m) {
  int64_t h = 2;
  while (h < 2 * m) h <<= 1;
  return h;
}
__host__ __device__ inline int64_t mg_state_bytes(int64_t n, int64_t m) {
  return 12 * mg_hash_size(m) + 16 * (n + 1) + 24 * (m + 1);
}

struct MgArgs {
  const int64_t* node_ptr;
  const int64_t* edge_ptr;
  const int32_t* inc_rowptr;
  const int32_t* inc_edge;
  const int64_t* ei;  // [2][E]
  int64_t E, N;
  const double* weight;
  const int64_t* perm;
  unsigned flags;
  float* c_node;
  float* c_edge;
  int64_t* coarse_edges;
  int64_t* coarse_n;
  int64_t* coarse_e;
  char* ws;
  int64_t ws_bytes;
  unsigned* err;
};

__device__ __forceinline__ void mg_raise(unsigned* err) {
  if (!err) return;
  // host memory without PCIe atomics: load + store keeps the other bits
  const unsigned old = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(err, old | (unsigned)HLHGAT_DEVERR_MLGC_RANGE, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}

// A word other threads updated with atomics (the hash, the support counts):
// read where the atomics landed, whatever a nearer cache still holds.
template <typename T>
__device__ __forceinline__ T mg_ld(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Exclusive scan of a[0, len) in place by the whole workgroup; returns the
// total.  Ends on a barrier (a[] is visible to every thread).
__device__ int mg_scan(int* a, int len, int* red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int carry = 0;
  for (int base = 0; base < len; base += kMgThreads) {
    const int i = base + tid;
    const int v = i < len ? a[i] : 0;
    int s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    if (lane == 63) red[wv] = s;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kMgWaves; ++w) {
      const int r = red[w];
      if (w < wv) off += r;
      tot += r;
    }
    if (i < len) a[i] = carry + off + s - v;
    carry += tot;
    __syncthreads();
  }
  return carry;
}

// One graph: n nodes from n0, m edges from e0, state in st (LDS or workspace).
__device__ void mg_graph(const MgArgs& a, int64_t g, int64_t n0, int n, int64_t e0, int m, char* st,
                         int* red) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int H = (int)mg_hash_size(m);
  int hbits = 0;
  while ((1 << hbits) < H) ++hbits;
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(st);
  unsigned* hval = reinterpret_cast<unsigned*>(st + 8 * (int64_t)H);
  int* cluster = reinterpret_cast<int*>(st + 12 * (int64_t)H);
  int* rank = cluster + (n + 1);
  int* cnode = rank + (n + 1);
  int* used = cnode + (n + 1);
  int* slot = used + (n + 1);
  int* flag = slot + (m + 1);
  int* clo = flag + (m + 1);
  int* chi = clo + (m + 1);
  int* sup = chi + (m + 1);
  int* newid = sup + (m + 1);
  const int64_t* row = a.ei;
  const int64_t* col = a.ei + a.E;
  const bool one_way = (a.flags & HLHGAT_MLGC_ONE_WAY) != 0;
  const bool prune = (a.flags & HLHGAT_MLGC_PRUNE_SINGLE) != 0;
  const bool drop = (a.flags & HLHGAT_MLGC_DROP_ISOLATED) != 0;
  const float inf = __builtin_inff();
  bool err = false;

  for (int u = tid; u <= n; u += kMgThreads) {
    cluster[u] = -1;
    rank[u] = 0;
  }
  for (int h = tid; h < H; h += kMgThreads) {
    keys[h] = kMgEmpty;
    hval[h] = 0xffffffffu;
  }
  __syncthreads();

  // 1. matching, wave 0
  if (tid < 64) {
    for (int i = 0; i < n; ++i) {
      const int64_t u64 = a.perm[n0 + i];
      if (u64 < 0 || u64 >= n) {  // uniform over the wave
        err = true;
        continue;
      }
      const int u = (int)u64;
      if (cluster[u] >= 0) continue;  // uniform: every lane stored the same ids
      double bw = -1.0;
      int bv = -1;
      const int p1 = a.inc_rowptr[n0 + u + 1];
      for (int p = a.inc_rowptr[n0 + u] + lane; p < p1; p += 64) {
        const int64_t e = a.inc_edge[p];
        if (e < e0 || e >= e0 + m) {  // an edge of another graph's slot
          err = true;
          continue;
        }
        const int64_t i_ = row[e] - n0, j_ = col[e] - n0;
        if (i_ < 0 || i_ >= n || j_ < 0 || j_ >= n) continue;  // raised in phase 3
        if (one_way && i_ != u) continue;
        const int v = (int)(i_ == u ? j_ : i_);
        if (v == u || cluster[v] >= 0) continue;
        const double w = a.weight ? a.weight[e] : 1.0;
        if (!(w >= 0.0)) continue;  // negatives and NaN never match
        if (w > bw || (w == bw && v > bv)) {
          bw = w;
          bv = v;
        }
      }
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const double ow = __shfl_xor(bw, d, 64);
        const int ov = __shfl_xor(bv, d, 64);
        if (ow > bw || (ow == bw && ov > bv)) {
          bw = ow;
          bv = ov;
        }
      }
      const int best = bv >= 0 ? bv : u;
      const int id = best < u ? best : u;
      cluster[u] = id;
      cluster[best] = id;
    }
  }
  __syncthreads();

  // 2. c_node = rank of the cluster id among the ids present
  for (int u = tid; u < n; u += kMgThreads) {
    int c = cluster[u];
    if (c < 0) {  // perm was no permutation: u was never visited
      err = true;
      c = u;
      cluster[u] = u;
    }
    rank[c] = 1;
  }
  __syncthreads();
  const int n1 = mg_scan(rank, n, red);
  for (int u = tid; u < n; u += kMgThreads) cnode[u] = rank[cluster[u]];
  __syncthreads();

  // 3. coarse pairs into the hash, the smallest fine-edge index per pair
  for (int k = tid; k < m; k += kMgThreads) {
    const int64_t i_ = row[e0 + k] - n0, j_ = col[e0 + k] - n0;
    int s = -1;
    if (i_ < 0 || i_ >= n || j_ < 0 || j_ >= n) {
      err = true;  // a bad edge is absent
    } else {
      const int ca = cnode[i_], cb = cnode[j_];
      if (ca != cb) {
        const unsigned long long key =
            ((unsigned long long)(ca < cb ? ca : cb) << 32) | (unsigned)(ca < cb ? cb : ca);
        int h = (int)((key * 0x9E3779B97F4A7C15ull) >> (64 - hbits));
        for (int t = 0; t < H; ++t) {  // distinct pairs <= m < H: a slot is found
          const unsigned long long prev = atomicCAS(&keys[h], kMgEmpty, key);
          if (prev == kMgEmpty || prev == key) {
            atomicMin(&hval[h], (unsigned)k);
            s = h;
            break;
          }
          h = (h + 1) & (H - 1);
        }
      }
    }
    slot[k] = s;
  }
  __syncthreads();
  for (int k = tid; k < m; k += kMgThreads)
    flag[k] = slot[k] >= 0 && mg_ld(&hval[slot[k]]) == (unsigned)k;
  __syncthreads();
  const int ne = mg_scan(flag, m, red);
  // flag[owner] is now the pair's first-seen number; hval stays as it is
  for (int k = tid; k < m; k += kMgThreads) {
    const int s = slot[k];
    if (s < 0) continue;
    const int o = (int)mg_ld(&hval[s]);
    const int c = flag[o];
    if (o == k) {
      const unsigned long long key = mg_ld(&keys[s]);
      clo[c] = (int)(key >> 32);
      chi[c] = (int)(key & 0xffffffffu);
      sup[c] = 0;
    }
    slot[k] = c;  // from here: the edge's coarse edge, or -1
  }
  __syncthreads();

  // 4. pruning
  int ne2 = ne;
  if (prune) {
    for (int k = tid; k < m; k += kMgThreads)
      if (slot[k] >= 0) atomicAdd(&sup[slot[k]], 1);
    __syncthreads();
    for (int c = tid; c < ne; c += kMgThreads) newid[c] = mg_ld(&sup[c]) != 1;
    __syncthreads();
    ne2 = mg_scan(newid, ne, red);
  } else {
    for (int c = tid; c < ne; c += kMgThreads) {
      sup[c] = 2;
      newid[c] = c;
    }
    __syncthreads();
  }
  int n2 = n1;
  if (drop) {
    for (int r = tid; r <= n1; r += kMgThreads) used[r] = 0;
    __syncthreads();
    for (int c = tid; c < ne; c += kMgThreads)
      if (mg_ld(&sup[c]) != 1) {
        used[clo[c]] = 1;
        used[chi[c]] = 1;
      }
    __syncthreads();
    n2 = mg_scan(used, n1, red);
    if (tid == 0) used[n1] = n2;  // used[r + 1] - used[r] = 1 where r is kept
    __syncthreads();
  }

  // 5. outputs
  for (int u = tid; u < n; u += kMgThreads) {
    const int r = cnode[u];
    float v = (float)r;
    if (drop) v = used[r + 1] != used[r] ? (float)used[r] : inf;
    a.c_node[n0 + u] = v;
  }
  for (int k = tid; k < m; k += kMgThreads) {
    const int c = slot[k];
    a.c_edge[e0 + k] = (c < 0 || mg_ld(&sup[c]) == 1) ? inf : (float)newid[c];
  }
  for (int c = tid; c < ne; c += kMgThreads) {
    if (mg_ld(&sup[c]) == 1) continue;
    const int q = newid[c];  // q <= c < m: inside the graph's edge slot
    a.coarse_edges[e0 + q] = drop ? used[clo[c]] : clo[c];
    a.coarse_edges[a.E + e0 + q] = drop ? used[chi[c]] : chi[c];
  }
  if (tid == 0) {
    a.coarse_n[g] = n2;
    a.coarse_e[g] = ne2;
  }
  if (err) mg_raise(a.err);
}

__global__ __launch_bounds__(kMgThreads) void k_mlgc(MgArgs a) {
  extern __shared__ __align__(16) char mg_lds[];
  __shared__ int red[kMgWaves];
  const int64_t g = blockIdx.x;
  const int64_t n0 = a.node_ptr[g], n_end = a.node_ptr[g + 1];
  const int64_t e0 = a.edge_ptr[g], e_end = a.edge_ptr[g + 1];
  const int64_t n = n_end - n0, m = e_end - e0;
  // device-side offsets: the host could not check them
  bool bad = n0 < 0 || n < 0 || n_end > a.N || e0 < 0 || m < 0 || e_end > a.E || n >= kMgMax ||
             m >= kMgMax;
  int64_t bytes = 0, off = 0;
  bool lds = false;
  if (!bad) {
    bytes = mg_state_bytes(n, m);
    lds = bytes <= kMgLdsBytes;
    off = 64 * g + 16 * n0 + 72 * e0;
    if (!lds && off + bytes > a.ws_bytes) bad = true;
  }
  if (bad) {
    if (threadIdx.x == 0) {
      a.coarse_n[g] = 0;
      a.coarse_e[g] = 0;
      mg_raise(a.err);
    }
    return;
  }
  if (lds)
    mg_graph(a, g, n0, (int)n, e0, (int)m, mg_lds, red);
  else
    mg_graph(a, g, n0, (int)n, e0, (int)m, a.ws + off, red);
}

}  // namespace

extern "C" size_t hlhgat_mlgc_device_workspace_bytes(int64_t n_nodes, int64_t n_edges,
                                                     int64_t n_graphs) {
  if (n_nodes < 0 || n_edges < 0 || n_graphs < 0) return 0;
  return (size_t)(64 * n_graphs + 16 * n_nodes + 72 * n_edges);
}

extern "C" int hlhgat_mlgc_device(int64_t n_graphs, const int64_t* node_ptr,
                                  const int64_t* edge_ptr, const int32_t* inc_rowptr,
                                  const int32_t* inc_edge, const int64_t* edge_index,
                                  int64_t n_edges, int64_t n_nodes, const double* weight,
                                  const int64_t* perm, unsigned flags, float* c_node,
                                  float* c_edge, int64_t* coarse_edges, int64_t* coarse_n,
                                  int64_t* coarse_e, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  HLH_CHECK_ARG(n_graphs >= 0 && n_nodes >= 0 && n_edges >= 0 && n_edges < INT32_MAX / 2 &&
                    n_nodes < INT32_MAX && n_graphs < INT32_MAX,
                "mlgc_device: bad sizes");
  HLH_CHECK_ARG((flags & ~kMgFlags) == 0, "mlgc_device: unknown flag bits 0x%x", flags);
  if (n_graphs == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(node_ptr && edge_ptr && inc_rowptr && coarse_n && coarse_e && workspace &&
                    (n_nodes == 0 || (perm && c_node)) &&
                    (n_edges == 0 || (edge_index && inc_edge && c_edge && coarse_edges)),
                "mlgc_device: NULL pointer");
  HLH_CHECK_ARG(hlhgat::aligned8(workspace), "mlgc_device: workspace must be 8-byte aligned");
  HLH_CHECK_ARG(workspace_bytes >= hlhgat_mlgc_device_workspace_bytes(n_nodes, n_edges, n_graphs),
                "mlgc_device: workspace too small");
  static bool attr = false;
  if (!attr) {
    HLH_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mlgc),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, kMgLdsBytes));
    attr = true;
  }
  MgArgs a{};
  a.node_ptr = node_ptr;
  a.edge_ptr = edge_ptr;
  a.inc_rowptr = inc_rowptr;
  a.inc_edge = inc_edge;
  a.ei = edge_index;
  a.E = n_edges;
  a.N = n_nodes;
  a.weight = weight;
  a.perm = perm;
  a.flags = flags;
  a.c_node = c_node;
  a.c_edge = c_edge;
  a.coarse_edges = coarse_edges;
  a.coarse_n = coarse_n;
  a.coarse_e = coarse_e;
  a.ws = reinterpret_cast<char*>(workspace);
  a.ws_bytes = (int64_t)workspace_bytes;
  a.err = hlhgat::device_error_word();
  hipLaunchKernelGGL(k_mlgc, dim3((unsigned)n_graphs), dim3(kMgThreads), kMgLdsBytes,
                     hlhgat::as_stream(stream), a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
