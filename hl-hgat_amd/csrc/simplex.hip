// Simplex dropout: the structural augmentation of the TSP training set
// (dropout_node, main_TSP_HL_HGCNN_dense_int3_pyr.py:73-97, applied by
// TSP_EigPE.get, :119-139 == lib/Hodge_Dataset.py:690-708) as a row mask m on a
// Hodge operator whose shape never changes.
//
// The reference filters the COO of L to the entries whose two ends survived
// (subgraph without relabelling): L' = M L M, M = diag(m).  Here the operator
// keeps its rowptr / col and only small tables are rewritten once per step:
//
//   CSR       val'[e]  = m[row(e)] && m[col[e]] ? val[e] : 0
//   factored  sign'[k] = m[node_edge[k]] ? sign[k] : 0    (L1 = alpha B1^T B1)
//             alpha'[e] = m[e] ? alpha[e] : 0
//
// The SpMM / polynomial-step kernels then run unchanged on the masked tables;
// the extra terms add 0 * x into sums taken in the same order.
//
// The mask itself is counter-based like the feature dropout (dropout.hip): a
// function of (seed, step, site, graph, row), nothing stored between steps, and
// a captured launch draws a fresh mask on every replay because {seed, step} are
// read from device memory.  All comparisons are on 24-bit integers:
//
//   graph g:  (a0, a1, ., .) = philox({g, 0, site, step lo}, key)
//             aug_g = (a0 >> 8) < Ta
//             T_g   = Tp + ((uint64(a1 >> 8) * Tj) >> 24)
//   row e:    u_e   = word (e & 3) of philox({(e>>2) lo, (e>>2) hi, site + 1,
//                                             step lo}, key) >> 8
//             keep_e = !aug_g || u_e >= T_g || protect[e] != 0
//   rows outside every graph (static-shape padding): 0
//
// Selects, not multiplies; plain vector stores only; no atomics.
#include "common.h"
#include "philox.h"

namespace hlhgat {
namespace {

struct KeepArgs {
  const int32_t* seg_ptr;  // [G + 1]
  int G;
  int64_t n_rows;
  int64_t groups;  // ceil(n_rows / 4)
  const float* protect;
  int64_t ldp;
  const int64_t* state;  // {seed, step}
  float* mask;
  float* col;
  int64_t ldc;
  uint32_t Ta, Tp, Tj, site;
};

// One thread owns four consecutive rows (one Philox call); the graph of each
// row is found by bisection over seg_ptr and the graph's draw is redone only
// when the graph changes inside the group.  VEC: mask is 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void k_simplex_keep(KeepArgs p) {
  const uint64_t seed = (uint64_t)p.state[0];
  const uint32_t step = (uint32_t)(uint64_t)p.state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.groups; q += stride) {
    const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), p.site + 1u,
                                    step, k0, k1);
    int cur = -1;
    bool aug = false;
    uint32_t Tg = 0;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t e = q * 4 + c;
      if (e >= p.n_rows) break;
      int lo = 0, hi = p.G;  // the first g with seg_ptr[g + 1] > e
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)p.seg_ptr[mid + 1] > e)
          hi = mid;
        else
          lo = mid + 1;
      }
      bool keep = false;
      if (lo < p.G && e >= (int64_t)p.seg_ptr[lo]) {
        if (lo != cur) {
          const Philox4 a = philox4x32_10((uint32_t)lo, 0u, p.site, step, k0, k1);
          aug = (a.w[0] >> 8) < p.Ta;
          Tg = p.Tp + (uint32_t)(((uint64_t)(a.w[1] >> 8) * p.Tj) >> 24);
          cur = lo;
        }
        keep = !aug || (r.w[c] >> 8) >= Tg || (p.protect && p.protect[e * p.ldp] != 0.f);
      }
      vget(v, c) = keep ? 1.f : 0.f;
    }
    const int64_t e0 = q * 4;
    if (VEC && e0 + 4 <= p.n_rows) {
      vstore<4>(p.mask + e0, v);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e0 + c < p.n_rows) p.mask[e0 + c] = vget(v, c);
    }
    if (p.col) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (e0 + c < p.n_rows) p.col[(e0 + c) * p.ldc] = vget(v, c);
    }
  }
}

struct MaskCsrArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  const float* mask;
  float* out;
  int64_t n_rows;
  int64_t nnz;
};

// A group of LPR lanes owns one row (its mask bit is read once) and walks the
// row's entries LPR at a time: coalesced col / val reads and val' stores.
template <int LPR>
__global__ __launch_bounds__(256) void k_mask_csr_values(MaskCsrArgs a) {
  const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR;
  const int sub = threadIdx.x % LPR;
  if (r >= a.n_rows) return;
  int64_t e0 = a.rowptr[r], e1 = a.rowptr[r + 1];
  if (e0 < 0) e0 = 0;
  if (e1 > a.nnz) e1 = a.nnz;
  const bool mr = a.mask[r] != 0.f;
  for (int64_t e = e0 + sub; e < e1; e += LPR) {
    const int64_t c = a.col[e];
    const bool mc = c >= 0 && c < a.n_rows && a.mask[c] != 0.f;
    a.out[e] = (mr && mc) ? a.val[e] : 0.f;
  }
}

struct MaskFactorArgs {
  const int32_t* node_edge;  // [2E]
  const float* node_sign;    // [2E]
  const float* alpha;        // [E]
  const float* mask;         // [E]
  float* sign_out;
  float* alpha_out;
  int64_t E;
};

// One launch for both tables: thread t takes V incidence entries (16-byte
// loads of the edge ids and signs when V == 4) and, while t * V < E, V alphas.
template <int V>
__global__ __launch_bounds__(256) void k_mask_hodge_factor(MaskFactorArgs a) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  const int64_t n2 = 2 * a.E;
  if (i0 >= n2) return;
  if (V > 1 && i0 + V <= n2) {
    const int4 ed = *reinterpret_cast<const int4*>(a.node_edge + i0);
    float4 s = vload<4>(a.node_sign + i0);
    const int e[4] = {ed.x, ed.y, ed.z, ed.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool m = e[c] >= 0 && e[c] < a.E && a.mask[e[c]] != 0.f;
      vget(s, c) = m ? vget(s, c) : 0.f;
    }
    vstore<4>(a.sign_out + i0, s);
  } else {
    for (int64_t i = i0; i < i0 + V && i < n2; ++i) {
      const int64_t e = a.node_edge[i];
      const bool m = e >= 0 && e < a.E && a.mask[e] != 0.f;
      a.sign_out[i] = m ? a.node_sign[i] : 0.f;
    }
  }
  if (i0 >= a.E) return;
  if (V > 1 && i0 + V <= a.E) {
    float4 al = vload<4>(a.alpha + i0);
    const float4 m = vload<4>(a.mask + i0);
    al.x = m.x != 0.f ? al.x : 0.f;
    al.y = m.y != 0.f ? al.y : 0.f;
    al.z = m.z != 0.f ? al.z : 0.f;
    al.w = m.w != 0.f ? al.w : 0.f;
    vstore<4>(a.alpha_out + i0, al);
  } else {
    for (int64_t i = i0; i < i0 + V && i < a.E; ++i)
      a.alpha_out[i] = a.mask[i] != 0.f ? a.alpha[i] : 0.f;
  }
}

constexpr uint32_t kT24 = 1u << 24;

}  // namespace
}  // namespace hlhgat

using namespace hlhgat;

extern "C" int hlhgat_simplex_keep(const int32_t* seg_ptr, int64_t n_graphs, int64_t n_rows,
                                   const float* protect, int64_t ldp, uint32_t Ta, uint32_t Tp,
                                   uint32_t Tj, uint32_t site, const int64_t* state, float* mask,
                                   float* col, int64_t ldc, void* stream) {
  HLH_CHECK_ARG(n_graphs >= 0 && n_graphs < INT32_MAX && n_rows >= 0,
                "simplex_keep: bad sizes (n_graphs, n_rows >= 0)");
  HLH_CHECK_ARG(Ta <= kT24 && Tp <= kT24 && Tj <= kT24, "simplex_keep: a threshold exceeds 2^24");
  HLH_CHECK_ARG(Tp + Tj <= kT24, "simplex_keep: Tp + Tj = %u exceeds 2^24", Tp + Tj);
  HLH_CHECK_ARG((site & 0x80000000u) && !(site & 1u),
                "simplex_keep: site must be 0x80000000 + 2k (got 0x%x)", site);
  HLH_CHECK_ARG((!protect || ldp >= 1) && (!col || ldc >= 1),
                "simplex_keep: bad leading dimension (ld >= 1)");
  if (n_rows == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(seg_ptr && state && mask, "simplex_keep: NULL pointer");
  HLH_CHECK_ARG(aligned8(state), "simplex_keep: state must be 8-byte aligned");
  KeepArgs p{};
  p.seg_ptr = seg_ptr;
  p.G = (int)n_graphs;
  p.n_rows = n_rows;
  p.groups = ceil_div(n_rows, 4);
  p.protect = protect;
  p.ldp = ldp;
  p.state = state;
  p.mask = mask;
  p.col = col;
  p.ldc = ldc;
  p.Ta = Ta;
  p.Tp = Tp;
  p.Tj = Tj;
  p.site = site;
  int64_t blocks = ceil_div(p.groups, 256);
  if (blocks > 2048) blocks = 2048;  // grid-stride beyond
  hipStream_t st = as_stream(stream);
  if (aligned16(mask))
    launch(k_simplex_keep<true>, dim3((unsigned)blocks), dim3(256), 0, st, nullptr, p);
  else
    launch(k_simplex_keep<false>, dim3((unsigned)blocks), dim3(256), 0, st, nullptr, p);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_mask_csr_values(const int32_t* rowptr, const int32_t* col, const float* val,
                                      int64_t n_rows, int64_t nnz, const float* mask,
                                      float* val_out, void* stream) {
  HLH_CHECK_ARG(n_rows >= 0 && nnz >= 0 && n_rows < INT32_MAX && nnz <= INT32_MAX,
                "mask_csr_values: bad sizes (0 <= n_rows, nnz < 2^31)");
  if (n_rows == 0 || nnz == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(rowptr && col && val && mask && val_out, "mask_csr_values: NULL pointer");
  MaskCsrArgs a{rowptr, col, val, mask, val_out, n_rows, nnz};
  const int64_t avg = nnz / n_rows;
  const int lpr = avg >= 24 ? 16 : avg >= 6 ? 8 : 4;
  const dim3 grid((unsigned)ceil_div(n_rows * lpr, 256));
  hipStream_t st = as_stream(stream);
  if (lpr == 16)
    launch(k_mask_csr_values<16>, grid, dim3(256), 0, st, nullptr, a);
  else if (lpr == 8)
    launch(k_mask_csr_values<8>, grid, dim3(256), 0, st, nullptr, a);
  else
    launch(k_mask_csr_values<4>, grid, dim3(256), 0, st, nullptr, a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_mask_hodge_factor(const hlhgat_hodge_factor_t* f, const float* mask,
                                        float* sign_out, float* alpha_out, void* stream) {
  HLH_CHECK_ARG(f, "mask_hodge_factor: NULL factor");
  HLH_CHECK_ARG(f->n_edges >= 0 && f->n_edges <= INT32_MAX / 2,
                "mask_hodge_factor: bad n_edges");
  if (f->n_edges == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(f->node_edge && f->node_sign && f->alpha && mask && sign_out && alpha_out,
                "mask_hodge_factor: NULL pointer");
  MaskFactorArgs a{f->node_edge, f->node_sign, f->alpha, mask, sign_out, alpha_out, f->n_edges};
  const bool vec = aligned16(a.node_edge) && aligned16(a.node_sign) && aligned16(a.alpha) &&
                   aligned16(mask) && aligned16(sign_out) && aligned16(alpha_out);
  hipStream_t st = as_stream(stream);
  if (vec)
    launch(k_mask_hodge_factor<4>, dim3((unsigned)ceil_div(ceil_div(2 * a.E, 4), 256)), dim3(256),
           0, st, nullptr, a);
  else
    launch(k_mask_hodge_factor<1>, dim3((unsigned)ceil_div(2 * a.E, 256)), dim3(256), 0, st,
           nullptr, a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
