// Functional connectivity of the DEMO brain pipeline on the device
// (HL-HGAT-DEMO/lib/Hodge_Dataset.py:130-145 Brain_MLGC_ALL.get, :148-178
// FC2mask's input; OHBM_DEMO.ipynb's FC[i] = torch.corrcoef(...) loop).
//
//   hlhgat_fc_prepare: k_fc_rows  one wave per [N, T] row: fp64 sum, min, max,
//                                 centred sum of squares; the centred
//                                 unit-norm row z^ into the workspace (pitch
//                                 roundup(T, 4), pad zeroed), NaN for a row
//                                 that is constant over the window;
//                      k_fc_z     (only when z is wanted) the graph's mean and
//                                 unbiased std from the row sums, in a fixed
//                                 order, then z = (x - mean) / std.
//   hlhgat_fc_dense /  k_fc_corr  corr(i, j) = z^_i . z^_j: the fp32 MFMA main
//   hlhgat_fc_edges:              loop of gemm_core.h with A = W = z^ of one
//                                 graph (blockIdx.z), 64 x 64 tiles with row
//                                 tile <= column tile, and a dense (mirrored)
//                                 or a skeleton (pair -> edge id) epilogue.
//
// Correlation is invariant to the graph-level z-score, so z^ is formed from x
// directly.  No atomics, no cross-workgroup waits: the launches are ordered by
// the stream and every sum has a fixed order (bitwise reproducible; a graph's
// results do not depend on the other graphs of the call).
#include "gemm_core.h"

#include <cmath>

using namespace hlhgat;

namespace {

constexpr int FC_TN = 4;              // 4 x 16 = 64 output columns per workgroup
constexpr int FC_TILE = 16 * FC_TN;   // and 4 waves x 16 = 64 rows
constexpr int FC_ZROWS = 8;           // rows per workgroup of k_fc_z
constexpr int64_t FC_MAX_GRAPHS = 65535;  // gridDim.z

__host__ __device__ inline int64_t fc_pitch(int64_t T) { return (T + 3) / 4 * 4; }

// workspace: z^ [G*N, pitch] floats (16-byte aligned size), then per row
// {sum, centred sum of squares} as doubles
inline size_t fc_zhat_bytes(int64_t G, int64_t N, int64_t T) {
  return (size_t)((G * N * fc_pitch(T) * 4 + 15) / 16 * 16);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;  // the same butterfly on every lane: one value, a fixed order
}

__device__ __forceinline__ const float* fc_row(const float* x, int64_t ldx,
                                               const int64_t* graph_rows, int64_t g, int64_t N,
                                               int64_t i, int64_t t0) {
  const int64_t r0 = graph_rows ? graph_rows[g] : g * N;
  return x + (r0 + i) * ldx + t0;
}

// Per-graph windows (hlhgat_fc_prepare_windows): graph g reads columns
// [t0[g], t0[g] + len[g]) and everything it writes is padded to t_max columns.
struct FcWindows {
  const int32_t* t0;   // [G]
  const int32_t* len;  // [G]
  int64_t t_max;
  unsigned* err;       // device error word (HLHGAT_DEVERR_TSERIES_LEN)
};

// the window of graph g, clamped to [2, t_max] samples inside the row
__device__ __forceinline__ void fc_window(const FcWindows& w, int64_t g, int64_t ldx, int64_t& t0,
                                          int64_t& T, bool report) {
  const int64_t l = w.len[g], b = w.t0[g];
  T = l < 2 ? 2 : (l > w.t_max ? w.t_max : l);
  t0 = b < 0 ? 0 : (b > ldx - T ? ldx - T : b);
  if (report && (T != l || t0 != b) && w.err) {
    // host memory without PCIe atomics: load + store keeps the other bits
    const unsigned old = __hip_atomic_load(w.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(w.err, old | (unsigned)HLHGAT_DEVERR_TSERIES_LEN, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <bool WIN>
__global__ __launch_bounds__(256) void k_fc_rows(const float* __restrict__ x, int64_t ldx,
                                                 const int64_t* __restrict__ graph_rows,
                                                 int64_t G, int64_t N, int64_t t0, int64_t T,
                                                 float* __restrict__ zhat,
                                                 double* __restrict__ stat, FcWindows w) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= G * N) return;  // whole waves leave: no barrier below
  int64_t P = fc_pitch(T);
  if constexpr (WIN) {
    fc_window(w, row / N, ldx, t0, T, lane == 0 && row % N == 0);
    P = fc_pitch(w.t_max);
  }
  const float* xr = fc_row(x, ldx, graph_rows, row / N, N, row % N, t0);
  double s = 0.0;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t t = lane; t < T; t += 64) {
    const float v = xr[t];
    s += (double)v;
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  const double mean = s / (double)T;
  double ss = 0.0;
  for (int64_t t = lane; t < T; t += 64) {
    const double d = (double)xr[t] - mean;
    ss += d * d;
  }
  ss = wave_sum(ss);
  if (lane == 0) {
    stat[2 * row] = s;
    stat[2 * row + 1] = ss;
  }
  // a row constant over the window: 0 / 0 in exact arithmetic
  const double rn = (lo == hi) ? (double)NAN : 1.0 / sqrt(ss);
  float* zr = zhat + row * P;
  for (int64_t t = lane; t < P; t += 64)
    zr[t] = t < T ? (float)(((double)xr[t] - mean) * rn) : 0.f;
}

// sum of f(row) over the N rows of a graph by all 256 threads of a workgroup,
// in a fixed order; every thread gets the result
template <typename F>
__device__ __forceinline__ double block_sum_rows(int64_t N, double* red, F f) {
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < N; i += 256) v += f(i);
  v = wave_sum(v);
  __syncthreads();  // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool WIN>
__global__ __launch_bounds__(256) void k_fc_z(const float* __restrict__ x, int64_t ldx,
                                              const int64_t* __restrict__ graph_rows, int64_t N,
                                              int64_t t0, int64_t T,
                                              const double* __restrict__ stat,
                                              float* __restrict__ z, FcWindows w) {
  __shared__ double red[4];
  const int64_t g = blockIdx.y;
  int64_t Tz = T;  // the row pitch of z
  if constexpr (WIN) {
    fc_window(w, g, ldx, t0, T, false);
    Tz = w.t_max;
  }
  const double* st = stat + 2 * g * N;
  const double cnt = (double)N * (double)T;
  const double mean = block_sum_rows(N, red, [&](int64_t i) { return st[2 * i]; }) / cnt;
  // sum over the graph of (x - mean)^2, from the rows' centred sums
  const double ssq = block_sum_rows(N, red, [&](int64_t i) {
    const double d = st[2 * i] / (double)T - mean;
    return st[2 * i + 1] + (double)T * d * d;
  });
  const double sd = sqrt(ssq / (cnt - 1.0));  // unbiased, as torch.Tensor.std()
  const int64_t i0 = (int64_t)blockIdx.x * FC_ZROWS;
  const int64_t rows = N - i0 < FC_ZROWS ? N - i0 : FC_ZROWS;
  for (int64_t e = threadIdx.x; e < rows * Tz; e += 256) {
    const int64_t i = i0 + e / Tz, t = e % Tz;
    if (WIN && t >= T) {  // past the graph's own window
      z[(g * N + i) * Tz + t] = 0.f;
      continue;
    }
    const float v = fc_row(x, ldx, graph_rows, g, N, i, t0)[t];
    z[(g * N + i) * Tz + t] = (float)(((double)v - mean) / sd);
  }
}

struct FcArgs {
  const float* zhat;
  int64_t pitch;
  int N;
  int n_tiles_side;          // ceil(N / 64)
  const int32_t* tiles;      // [n][2] (row tile, column tile) or NULL: every rt <= ct
  float* fc;                 // dense epilogue: [G, N, N]
  const int32_t* pair2edge;  // skeleton epilogue: [N * N]
  float* out;
  int64_t E, ld;
};

// keeps NaN, which fminf / fmaxf would drop
__device__ __forceinline__ float clamp1(float v) { return v > 1.f ? 1.f : (v < -1.f ? -1.f : v); }

template <bool DENSE>
__global__ __launch_bounds__(256) void k_fc_corr(FcArgs p) {
  __shared__ float wl[2][FC_TILE][KCP];
  const int64_t g = blockIdx.z;
  int rt, ct;
  if (p.tiles) {
    rt = p.tiles[2 * blockIdx.x];
    ct = p.tiles[2 * blockIdx.x + 1];
  } else {  // blockIdx.x counts the pairs rt <= ct row by row
    int rem = blockIdx.x;
    rt = 0;
    while (rem >= p.n_tiles_side - rt) {
      rem -= p.n_tiles_side - rt;
      ++rt;
    }
    ct = rt + rem;
  }
  // a tile pair outside the triangle computes nothing (the whole workgroup
  // leaves before the main loop's barriers)
  if (rt < 0 || ct < rt || ct >= p.n_tiles_side) return;
  // the main loop indexes its argument blocks at run time: the one-block
  // FwdArgs lives in LDS (a private copy would go to scratch memory)
  __shared__ FwdArgs a;
  if (threadIdx.x == 0) {
    a.nb = 1;
    a.N = p.N;
    a.M = p.N;
    a.A[0] = a.W[0] = p.zhat + g * p.N * p.pitch;
    a.lda[0] = a.ldw[0] = p.pitch;
    a.kb[0] = (int)p.pitch;
  }
  __syncthreads();
  floatx4 acc[FC_TN];
  proj_fwd_lds_mainloop<FC_TN>(a, rt, ct, wl, acc);

  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
#pragma unroll
  for (int tn = 0; tn < FC_TN; ++tn) {
    const int n = ct * FC_TILE + tn * 16 + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = rt * FC_TILE + wave * 16 + 4 * q + r;
      if (n >= p.N || m > n) continue;  // (m < N follows from m <= n)
      const float v = clamp1(acc[tn][r]);
      if constexpr (DENSE) {
        float* f = p.fc + g * p.N * p.N;
        f[(int64_t)m * p.N + n] = v;
        f[(int64_t)n * p.N + m] = v;  // the same value: exactly symmetric
      } else {
        if (m == n) continue;
        const int64_t eid = p.pair2edge[(int64_t)m * p.N + n];
        if (eid >= 0 && eid < p.E) p.out[(g * p.E + eid) * p.ld] = v;
      }
    }
  }
}

int fc_check_ws(const void* workspace, int64_t G, int64_t N, int64_t T, const char* who) {
  HLH_CHECK_ARG(G >= 0, "%s: G = %lld < 0", who, (long long)G);
  HLH_CHECK_ARG(N > 0, "%s: N = %lld must be positive", who, (long long)N);
  HLH_CHECK_ARG(N <= (1 << 24), "%s: N = %lld too large", who, (long long)N);
  HLH_CHECK_ARG(T >= 2, "%s: T = %lld < 2 (a correlation needs two samples)", who, (long long)T);
  HLH_CHECK_ARG(T <= (1 << 28), "%s: T = %lld too large", who, (long long)T);
  HLH_CHECK_ARG(G * N <= INT32_MAX, "%s: G * N = %lld rows in one call", who, (long long)(G * N));
  HLH_CHECK_ARG(G <= FC_MAX_GRAPHS, "%s: G = %lld > %lld graphs in one call", who, (long long)G,
                (long long)FC_MAX_GRAPHS);
  if (G == 0) return 0;
  HLH_CHECK_ARG(workspace != nullptr, "%s: NULL workspace", who);
  HLH_CHECK_ARG(aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" size_t hlhgat_fc_workspace_bytes(int64_t G, int64_t N, int64_t T) {
  if (G <= 0 || N <= 0 || T < 2) return 0;
  return fc_zhat_bytes(G, N, T) + (size_t)(G * N) * 2 * sizeof(double);
}

// win NULL: one window (t0, T) for every graph; else per-graph windows padded
// to T = win->t_max columns
static int fc_prepare_impl(const float* x, int64_t ldx, const int64_t* graph_rows, int64_t G,
                           int64_t N, int64_t t0, int64_t T, float* z, void* workspace,
                           size_t workspace_bytes, const FcWindows* win, void* stream) {
  if (int rc = fc_check_ws(G == 0 ? nullptr : workspace, G, N, T, "fc_prepare")) return rc;
  HLH_CHECK_ARG(t0 >= 0, "fc_prepare: t0 = %lld < 0", (long long)t0);
  HLH_CHECK_ARG(t0 + T <= ldx, "fc_prepare: window t0 + T = %lld exceeds ldx = %lld",
                (long long)(t0 + T), (long long)ldx);
  if (G == 0) return 0;
  HLH_CHECK_ARG(x != nullptr, "fc_prepare: NULL x");
  HLH_CHECK_ARG(workspace_bytes >= hlhgat_fc_workspace_bytes(G, N, T),
                "fc_prepare: workspace of %zu bytes, need %zu", workspace_bytes,
                hlhgat_fc_workspace_bytes(G, N, T));
  hipStream_t s = as_stream(stream);
  float* zhat = static_cast<float*>(workspace);
  double* stat = reinterpret_cast<double*>(static_cast<char*>(workspace) + fc_zhat_bytes(G, N, T));
  const dim3 grows((unsigned)ceil_div(G * N, 4));
  const dim3 gz((unsigned)ceil_div(N, FC_ZROWS), (unsigned)G);
  if (win)
    launch(k_fc_rows<true>, grows, dim3(256), 0, s, nullptr, x, ldx, graph_rows, G, N, t0, T,
           zhat, stat, *win);
  else
    launch(k_fc_rows<false>, grows, dim3(256), 0, s, nullptr, x, ldx, graph_rows, G, N, t0, T,
           zhat, stat, FcWindows{});
  HLH_CHECK_LAUNCH();
  if (z) {
    if (win)
      launch(k_fc_z<true>, gz, dim3(256), 0, s, nullptr, x, ldx, graph_rows, N, t0, T,
             (const double*)stat, z, *win);
    else
      launch(k_fc_z<false>, gz, dim3(256), 0, s, nullptr, x, ldx, graph_rows, N, t0, T,
             (const double*)stat, z, FcWindows{});
    HLH_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int hlhgat_fc_prepare(const float* x, int64_t ldx, const int64_t* graph_rows,
                                 int64_t G, int64_t N, int64_t t0, int64_t T, float* z,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  return fc_prepare_impl(x, ldx, graph_rows, G, N, t0, T, z, workspace, workspace_bytes, nullptr,
                         stream);
}

extern "C" int hlhgat_fc_prepare_windows(const float* x, int64_t ldx, const int64_t* graph_rows,
                                         int64_t G, int64_t N, const int32_t* t0,
                                         const int32_t* len, int64_t t_max, float* z,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  HLH_CHECK_ARG(G <= 0 || (t0 && len), "fc_prepare_windows: NULL window table");
  HLH_CHECK_ARG(t_max >= 1, "fc_prepare_windows: t_max = %lld < 1", (long long)t_max);
  const FcWindows win{t0, len, t_max, device_error_word()};
  return fc_prepare_impl(x, ldx, graph_rows, G, N, 0, t_max, z, workspace, workspace_bytes, &win,
                         stream);
}

extern "C" int hlhgat_fc_dense(const void* workspace, int64_t G, int64_t N, int64_t T, float* fc,
                               void* stream) {
  if (int rc = fc_check_ws(workspace, G, N, T, "fc_dense")) return rc;
  if (G == 0) return 0;
  HLH_CHECK_ARG(fc != nullptr, "fc_dense: NULL fc");
  FcArgs p{};
  p.zhat = static_cast<const float*>(workspace);
  p.pitch = fc_pitch(T);
  p.N = (int)N;
  p.n_tiles_side = (int)ceil_div(N, FC_TILE);
  p.fc = fc;
  const int64_t pairs = (int64_t)p.n_tiles_side * (p.n_tiles_side + 1) / 2;
  HLH_CHECK_ARG(pairs <= INT32_MAX, "fc_dense: N = %lld too large", (long long)N);
  launch(k_fc_corr<true>, dim3((unsigned)pairs, 1, (unsigned)G), dim3(256), 0, as_stream(stream),
         nullptr, p);
  HLH_CHECK_LAUNCH();
  return 0;
}

extern "C" int hlhgat_fc_edges(const void* workspace, int64_t G, int64_t N, int64_t T,
                               const int32_t* pair2edge, int64_t E, const int32_t* tiles,
                               int64_t n_tiles, float* out, int64_t ld, void* stream) {
  if (int rc = fc_check_ws(workspace, G, N, T, "fc_edges")) return rc;
  HLH_CHECK_ARG(pair2edge != nullptr, "fc_edges: NULL pair2edge");
  HLH_CHECK_ARG(E > 0, "fc_edges: E = %lld edges with a pair table", (long long)E);
  HLH_CHECK_ARG(n_tiles >= 0 && n_tiles <= INT32_MAX, "fc_edges: n_tiles = %lld",
                (long long)n_tiles);
  HLH_CHECK_ARG(ld >= 1, "fc_edges: ld = %lld < 1", (long long)ld);
  if (G == 0 || n_tiles == 0) return 0;
  HLH_CHECK_ARG(tiles != nullptr, "fc_edges: NULL tiles");
  HLH_CHECK_ARG(out != nullptr, "fc_edges: NULL out");
  FcArgs p{};
  p.zhat = static_cast<const float*>(workspace);
  p.pitch = fc_pitch(T);
  p.N = (int)N;
  p.n_tiles_side = (int)ceil_div(N, FC_TILE);
  p.tiles = tiles;
  p.pair2edge = pair2edge;
  p.out = out;
  p.E = E;
  p.ld = ld;
  launch(k_fc_corr<false>, dim3((unsigned)n_tiles, 1, (unsigned)G), dim3(256), 0,
         as_stream(stream), nullptr, p);
  HLH_CHECK_LAUNCH();
  return 0;
}
