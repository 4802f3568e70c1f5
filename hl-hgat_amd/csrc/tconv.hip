// Temporal front end of the DEMO brain model (HL-HGAT-DEMO/lib/
// Hodge_Cheb_Conv.py:474-515, Inception1D): 1-D convolutions over time as an
// implicit GEMM on the fp32 MFMA, LeakyReLU + max-pool over time and the
// LeakyReLU + [max_t | mean_t] readout, each with its backward.
//
// Activations are channels-last, [N, T, C] row-major: a batch of series is an
// [N*T, C] matrix (what the BatchNorm entry points take), a convolution tap is
// a row shift of that matrix, and the zero padding at the two ends of every
// series is a per-row mask on the shifted operand -- a row tile that crosses a
// series boundary never multiplies the neighbouring series' rows.
//
// Nothing here uses floating-point atomics: the weight gradient is a set of
// per-workgroup partial sums reduced in a fixed order by a second kernel.
#include "gemm_core.h"

#include <algorithm>

using namespace hlhgat;

namespace {

constexpr int TM = 64;        // output rows of [N*T, C] per workgroup (4 waves x 16)
constexpr int HALO = 2;       // rows staged before and after the tile (taps <= 5)
constexpr int MAXTAPS = 5;
constexpr int MAXBR = 4;      // branches packed into one convolution
constexpr int WG_SUB = 64;    // rows per staging step of the weight gradient
constexpr int WG_PITCH = 80;  // LDS row pitch there: rows q, q+1 on disjoint banks
constexpr int WG_MAX = 512;   // row chunks (workgroups along the rows) at the most

// Ragged time layout (hlhgat_tseries_map): series of different lengths stacked
// compactly in a buffer of fixed capacity.  The position predicate of a row
// then comes from a per-row (step, length) table instead of g % T, and the
// rows from *n_rows on are dead: never read, written as zeros.
struct RowTab {
  const int2* tab;         // [capacity] (step within the series, series length)
  const int32_t* n_rows;   // device scalar: the valid-row prefix
};

__device__ __forceinline__ int64_t live_rows(int64_t cap, const int32_t* n_rows) {
  const int64_t v = (int64_t)*n_rows;
  return v < cap ? (v < 0 ? 0 : v) : cap;
}

// ---------------------------------------------------------------------------
// weight packing: the branches' nn.Conv1d weights [co_b][cin][taps_b] into one
// [taps][Cout][cin] weight with structural zeros (forward), or its flipped
// transpose [taps][cin][Cout] (the data gradient's weight)
// ---------------------------------------------------------------------------
struct PackArgs {
  int nb, taps, flip;
  int64_t cin, cout;
  const float* w[MAXBR];
  int64_t off[MAXBR + 1];
  int tb[MAXBR];
  float* wp;
};

__global__ void k_tconv_pack(PackArgs a) {
  const int64_t total = (int64_t)a.taps * a.cout * a.cin;
  const int half = a.taps >> 1;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(j / (a.cout * a.cin));
    const int64_t rem = j - (int64_t)k * a.cout * a.cin;
    int64_t co, ci;
    if (a.flip) {
      ci = rem / a.cout;
      co = rem - ci * a.cout;
    } else {
      co = rem / a.cin;
      ci = rem - co * a.cin;
    }
    const int kf = a.flip ? a.taps - 1 - k : k;  // the forward tap this entry holds
    int b = 0;
    while (b + 1 < a.nb && co >= a.off[b + 1]) ++b;
    const int kb = kf - half + (a.tb[b] >> 1);
    float v = 0.f;
    if (kb >= 0 && kb < a.tb[b]) v = a.w[b][((co - a.off[b]) * a.cin + ci) * a.tb[b] + kb];
    a.wp[j] = v;
  }
}

// ---------------------------------------------------------------------------
// forward / data gradient: y[g][co] = bias[co] + sum_k sum_ci xs_k[g][ci] W[k][co][ci]
// with xs_k[g] = x[g + k - taps/2] inside the series of row g, else 0.
//
// Workgroup = 4 waves x 16 rows, 64 output columns.  The A tile (TM + 2*HALO
// rows x 64 input channels) is staged once per channel chunk and serves every
// tap; the tap's weight chunk W[k][64 columns][64 channels] is staged beside
// it.  Both use gemm_core.h's 16-B-slot XOR swizzle, so the ds_read_b128 of 16
// consecutive rows touch 16 distinct slots.
// ---------------------------------------------------------------------------
struct ConvArgs {
  const float* x;
  int64_t M;  // N*T rows
  int T, cin, cout, taps;
  const float* w;  // [taps][cout][cin]
  const float* bias;
  float* y;
  int n1, n3;  // columns [0,n1): centre tap only; [n1,n1+n3): the centre three
  int vec_in, vec_out;
  RowTab rt;  // ragged kernels only; M is then the capacity
};

template <bool VEC>
__device__ __forceinline__ void stage_rows(float (*lds)[KC], int nrows, const float* src,
                                           int64_t row_first, int64_t row_lo, int64_t row_hi,
                                           int64_t ld, int c0, int cmax) {
  // lds[r][k] = src[(row_first + r) * ld + c0 + k] for rows in [row_lo, row_hi)
  // and c0 + k < cmax, else 0
  if constexpr (VEC) {
    for (int idx = threadIdx.x; idx < nrows * 16; idx += 256) {
      const int r = idx >> 4, c4 = idx & 15;
      const int64_t g = row_first + r;
      const int k = c0 + 4 * c4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g >= row_lo && g < row_hi && k < cmax)
        v = *reinterpret_cast<const float4*>(src + g * ld + k);
      *reinterpret_cast<float4*>(&lds[r][4 * wswz(r, c4)]) = v;
    }
  } else {
    for (int idx = threadIdx.x; idx < nrows * KC; idx += 256) {
      const int r = idx >> 6, kk = idx & 63;
      const int64_t g = row_first + r;
      const int k = c0 + kk;
      float v = 0.f;
      if (g >= row_lo && g < row_hi && k < cmax) v = src[g * ld + k];
      lds[r][4 * wswz(r, kk >> 2) + (kk & 3)] = v;
    }
  }
}

// rows [lo, hi) x columns [n_base, n_base + ncols) of y := 0 (the dead rows of
// a ragged tile), by one wave
__device__ __forceinline__ void zero_rows(float* y, int64_t ld, int64_t lo, int64_t hi,
                                          int n_base, int ncols) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = lo; r < hi; ++r)
    for (int c = lane; c < ncols; c += 64) y[r * ld + n_base + c] = 0.f;
}

template <bool VEC, bool RAG>
__global__ __launch_bounds__(256) void k_tconv_fwd(ConvArgs a) {
  __shared__ __attribute__((aligned(16))) float xa[TM + 2 * HALO][KC];
  __shared__ __attribute__((aligned(16))) float wl[64][KC];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
  const int64_t row0 = (int64_t)blockIdx.x * TM;
  const int n_base = blockIdx.y * 64;
  const int half = a.taps >> 1;
  const int64_t g = row0 + wave * 16 + i;  // the row this lane feeds as A operand
  int64_t Mv = a.M;
  int tpos, tlen = a.T;
  if constexpr (RAG) {
    Mv = live_rows(a.M, a.rt.n_rows);
    const int64_t w0 = row0 + wave * 16;
    if (row0 >= Mv) {  // a dead tile (the whole workgroup leaves)
      zero_rows(a.y, a.cout, w0, min(w0 + 16, a.M), n_base, min(64, a.cout - n_base));
      return;
    }
    const int2 e = g < Mv ? a.rt.tab[g] : make_int2(0, 0);
    tpos = e.x;
    tlen = e.y;
  } else {
    tpos = g < a.M ? (int)(g % a.T) : -(1 << 20);
  }

  floatx4 acc[4];
#pragma unroll
  for (int tn = 0; tn < 4; ++tn) acc[tn] = floatx4{0.f, 0.f, 0.f, 0.f};

  for (int c0 = 0; c0 < a.cin; c0 += KC) {
    __syncthreads();  // the previous chunk's readers are done with xa
    stage_rows<VEC>(xa, TM + 2 * HALO, a.x, row0 - HALO, 0, Mv, a.cin, c0, a.cin);
    const int ns = min(4, (a.cin - c0 + 15) >> 4);
    for (int k = 0; k < a.taps; ++k) {
      __syncthreads();  // the previous tap's readers are done with wl
      stage_rows<VEC>(wl, 64, a.w + (int64_t)k * a.cout * a.cin, n_base, 0, a.cout, a.cin, c0,
                      a.cin);
      __syncthreads();
      const int d = k > half ? k - half : half - k;
      const bool av = (unsigned)(tpos + k - half) < (unsigned)tlen;
      const int ar = wave * 16 + i + k - half + HALO;
      bool on[4];
#pragma unroll
      for (int tn = 0; tn < 4; ++tn) {
        const int cend = n_base + tn * 16 + 16;
        on[tn] = n_base + tn * 16 < a.cout && !(d >= 1 && cend <= a.n1) &&
                 !(d >= 2 && cend <= a.n1 + a.n3);
      }
      for (int s = 0; s < ns; ++s) {
        float4 af = *reinterpret_cast<const float4*>(&xa[ar][4 * wswz(ar, 4 * s + q)]);
        if (!av) af = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int tn = 0; tn < 4; ++tn) {
          if (on[tn]) {
            const float4 bf =
                *reinterpret_cast<const float4*>(&wl[tn * 16 + i][4 * wswz(i, 4 * s + q)]);
            acc[tn] = mfma16(af.x, bf.x, acc[tn]);
            acc[tn] = mfma16(af.y, bf.y, acc[tn]);
            acc[tn] = mfma16(af.z, bf.z, acc[tn]);
            acc[tn] = mfma16(af.w, bf.w, acc[tn]);
          }
        }
      }
    }
  }
  __syncthreads();  // xa becomes the epilogue's transpose scratch
  float* scratch = &xa[0][0] + wave * (16 * (64 + 4));
  store_tile_rows<4>(acc, scratch, row0 + wave * 16, Mv, a.y + n_base, a.cout,
                     a.cout - n_base, a.bias ? a.bias + n_base : nullptr, 0, a.vec_out != 0);
  if constexpr (RAG) {
    const int64_t w0 = row0 + wave * 16;
    zero_rows(a.y, a.cout, max(w0, Mv), min(w0 + 16, a.M), n_base, min(64, a.cout - n_base));
  }
}

// The Cin = 1 embedding (nn.Conv1d(1, C, taps, padding=taps/2), :483): VALU
// work.  A thread owns V output channels of EMB_R consecutive rows: its
// V x taps weights stay in registers, and each row costs it `taps` loads of
// x (shared by the lanes of the row) and one 4*V-byte store.  w is in the
// module's [C][1][taps] layout.
constexpr int EMB_R = 8;

template <int V, typename IdxT, bool RAG>
__global__ void k_tconv_embed_fwd(const float* __restrict__ x, int64_t M, int T,
                                  const float* __restrict__ w, const float* __restrict__ bias,
                                  int C, int taps, float* __restrict__ y, RowTab rt) {
  const int half = taps >> 1;
  int64_t Mv = M;
  if constexpr (RAG) Mv = live_rows(M, rt.n_rows);
  const IdxT cv = (IdxT)(C / V);
  const IdxT total = (IdxT)((M + EMB_R - 1) / EMB_R) * cv;
  for (IdxT j = (IdxT)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (IdxT)gridDim.x * blockDim.x) {
    const IdxT rb = j / cv;
    const int c = (int)(j - rb * cv) * V;
    const int64_t g0 = (int64_t)rb * EMB_R;
    float wr[V][MAXTAPS], bv[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      bv[u] = bias ? bias[c + u] : 0.f;
#pragma unroll
      for (int k = 0; k < MAXTAPS; ++k) wr[u][k] = k < taps ? w[(c + u) * taps + k] : 0.f;
    }
    int t = RAG ? 0 : (int)(g0 % T);
#pragma unroll
    for (int r = 0; r < EMB_R; ++r) {
      const int64_t g = g0 + r;
      if (g < M) {
        typename VecT<V>::type v;
        if constexpr (RAG) {
          if (g >= Mv) {  // a dead row
#pragma unroll
            for (int u = 0; u < V; ++u) vget(v, u) = 0.f;
            vstore<V>(y + g * C + c, v);
            continue;
          }
          const int2 e = rt.tab[g];
          t = e.x;
          T = e.y;
        }
#pragma unroll
        for (int u = 0; u < V; ++u) vget(v, u) = bv[u];
        // every tap's load is issued unconditionally (clamped address, masked value)
#pragma unroll
        for (int k = 0; k < MAXTAPS; ++k) {
          const int tt = t + k - half;
          const bool ok = k < taps && tt >= 0 && tt < T;
          const float ld = x[ok ? g + k - half : g];
          const float xv = ok ? ld : 0.f;
#pragma unroll
          for (int u = 0; u < V; ++u) vget(v, u) += xv * wr[u][k];
        }
        vstore<V>(y + g * C + c, v);
      }
      if constexpr (!RAG)
        if (++t == T) t = 0;
    }
  }
}

// ---------------------------------------------------------------------------
// weight gradient: dW[k][co][ci] = sum_g dy[g][co] * xs_k[g][ci], db[co] =
// sum_g dy[g][co].  Workgroup (bx, by, bz) owns a chunk of rows, 64 output
// channels (wave w: 16 of them) and 64 input channels, all taps: 5 x 4
// accumulator tiles per wave.  Its partial sums go to workspace slot bx; the
// reduction kernel adds the slots in order and writes the branches' gradients
// in their own [co_b][cin][taps_b] layout.
// ---------------------------------------------------------------------------
struct WgradArgs {
  const float* x;
  const float* dy;
  int64_t M, rows_per_wg;
  int T, cin, cout, taps;
  float* ws;   // [n_wg][taps][cout][cin]
  float* wsb;  // [n_wg][cout]
  RowTab rt;   // ragged kernels only; M is then the capacity
};

template <bool VEC, bool RAG>
__global__ __launch_bounds__(256) void k_tconv_wgrad(WgradArgs a) {
  __shared__ __attribute__((aligned(16))) float dyl[WG_SUB][WG_PITCH];
  __shared__ __attribute__((aligned(16))) float xl[WG_SUB + 2 * HALO][WG_PITCH];
  __shared__ int tp[WG_SUB];
  __shared__ int tl[RAG ? WG_SUB : 1];  // ragged: the series length of the row
  __shared__ float bred[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
  const int co_base = blockIdx.y * 64, ci_base = blockIdx.z * 64;
  const int half = a.taps >> 1;
  const int64_t r_lo = (int64_t)blockIdx.x * a.rows_per_wg;
  int64_t Mv = a.M;
  if constexpr (RAG) Mv = live_rows(a.M, a.rt.n_rows);
  // a chunk past the live rows runs no step and writes a slot of zeros
  const int64_t r_hi = min(Mv, r_lo + a.rows_per_wg);

  floatx4 acc[MAXTAPS][4];
#pragma unroll
  for (int k = 0; k < MAXTAPS; ++k)
#pragma unroll
    for (int cj = 0; cj < 4; ++cj) acc[k][cj] = floatx4{0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  const int sc = threadIdx.x & 63, sr = threadIdx.x >> 6;

  for (int64_t g0 = r_lo; g0 < r_hi; g0 += WG_SUB) {
    __syncthreads();
    if constexpr (VEC) {  // cin, cout multiples of 4 and 16-B aligned: whole float4s
      const int c4 = 4 * (threadIdx.x & 15), vr = threadIdx.x >> 4;
      for (int r = vr; r < WG_SUB; r += 16) {
        const int64_t g = g0 + r;
        const int co = co_base + c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g < r_hi && co < a.cout) v = *reinterpret_cast<const float4*>(a.dy + g * a.cout + co);
        *reinterpret_cast<float4*>(&dyl[r][c4]) = v;
      }
      for (int r = vr; r < WG_SUB + 2 * HALO; r += 16) {
        const int64_t g = g0 - HALO + r;
        const int ci = ci_base + c4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g >= 0 && g < Mv && ci < a.cin)
          v = *reinterpret_cast<const float4*>(a.x + g * a.cin + ci);
        *reinterpret_cast<float4*>(&xl[r][c4]) = v;
      }
    } else {
      for (int r = sr; r < WG_SUB; r += 4) {
        const int64_t g = g0 + r;
        const int co = co_base + sc;
        dyl[r][sc] = (g < r_hi && co < a.cout) ? a.dy[g * a.cout + co] : 0.f;
      }
      for (int r = sr; r < WG_SUB + 2 * HALO; r += 4) {
        const int64_t g = g0 - HALO + r;
        const int ci = ci_base + sc;
        xl[r][sc] = (g >= 0 && g < Mv && ci < a.cin) ? a.x[g * a.cin + ci] : 0.f;
      }
    }
    if (threadIdx.x < WG_SUB) {
      const int64_t g = g0 + threadIdx.x;
      if constexpr (RAG) {
        const int2 e = g < r_hi ? a.rt.tab[g] : make_int2(0, 0);
        tp[threadIdx.x] = e.x;
        tl[threadIdx.x] = e.y;
      } else {
        tp[threadIdx.x] = g < r_hi ? (int)(g % a.T) : -(1 << 20);
      }
    }
    __syncthreads();
    if (blockIdx.z == 0) {
#pragma unroll 4
      for (int r = 0; r < 16; ++r) bsum += dyl[sr * 16 + r][sc];
    }
    for (int s = 0; s < WG_SUB / 4; ++s) {
      const int gl = 4 * s + q;
      const float av = dyl[gl][wave * 16 + i];
      const int t = tp[gl];
      const int tT = RAG ? tl[gl] : a.T;
#pragma unroll
      for (int k = 0; k < MAXTAPS; ++k) {
        if (k < a.taps) {
          const bool ok = (unsigned)(t + k - half) < (unsigned)tT;
#pragma unroll
          for (int cj = 0; cj < 4; ++cj) {
            if (ci_base + cj * 16 < a.cin) {
              float bv = xl[gl + k - half + HALO][cj * 16 + i];
              if (!ok) bv = 0.f;
              acc[k][cj] = mfma16(av, bv, acc[k][cj]);
            }
          }
        }
      }
    }
  }

  float* ws = a.ws + (int64_t)blockIdx.x * a.taps * a.cout * a.cin;
#pragma unroll
  for (int k = 0; k < MAXTAPS; ++k) {
    if (k < a.taps) {
#pragma unroll
      for (int cj = 0; cj < 4; ++cj) {
        const int ci = ci_base + cj * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = co_base + wave * 16 + 4 * q + r;
          if (co < a.cout && ci < a.cin)
            ws[((int64_t)k * a.cout + co) * a.cin + ci] = acc[k][cj][r];
        }
      }
    }
  }
  if (blockIdx.z == 0) {
    bred[sr][sc] = bsum;
    __syncthreads();
    if (threadIdx.x < 64 && co_base + sc < a.cout)
      a.wsb[(int64_t)blockIdx.x * a.cout + co_base + sc] =
          ((bred[0][sc] + bred[1][sc]) + bred[2][sc]) + bred[3][sc];
  }
}

struct WreduceArgs {
  const float* ws;
  const float* wsb;
  int n_wg, taps, nb;
  int64_t cin, cout;
  float* dw[MAXBR];
  int64_t off[MAXBR + 1];
  int tb[MAXBR];
  float* dbias;
};

// sum_p base[p * stride] in the order p = 0, 1, ...: few threads run this with
// one dependent add per partial, so the loads are issued 16 at a time
__device__ __forceinline__ float ordered_sum(const float* base, int64_t stride, int n) {
  float s = 0.f;
  int p = 0;
  for (; p + 16 <= n; p += 16) {
    float v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) v[u] = base[(int64_t)(p + u) * stride];
#pragma unroll
    for (int u = 0; u < 16; ++u) s += v[u];
  }
  for (; p < n; ++p) s += base[(int64_t)p * stride];
  return s;
}

__global__ void k_tconv_wreduce(WreduceArgs a) {
  const int64_t nw = (int64_t)a.taps * a.cout * a.cin;
  const int64_t total = nw + (a.dbias ? a.cout : 0);
  const int half = a.taps >> 1;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    if (j >= nw) {
      const int64_t co = j - nw;
      a.dbias[co] = ordered_sum(a.wsb + co, a.cout, a.n_wg);
      continue;
    }
    const int k = (int)(j / (a.cout * a.cin));
    const int64_t rem = j - (int64_t)k * a.cout * a.cin;
    const int64_t co = rem / a.cin, ci = rem - co * a.cin;
    int b = 0;
    while (b + 1 < a.nb && co >= a.off[b + 1]) ++b;
    const int kb = k - half + (a.tb[b] >> 1);
    if (kb < 0 || kb >= a.tb[b]) continue;  // a structural zero of the packed weight
    const float s = ordered_sum(a.ws + j, nw, a.n_wg);
    a.dw[b][((co - a.off[b]) * a.cin + ci) * a.tb[b] + kb] = s;
  }
}

// ---------------------------------------------------------------------------
// LeakyReLU + MaxPool1d(m, stride m-1, padding (m-1)/2) over time (:488, :505)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : v * slope; }

// Ragged pool / readout: where a row's series lives in the stage before (in)
// and after (out) the pool (hlhgat_tseries_map)
struct SeriesTab {
  const int32_t* soff_in;   // [S + 1] series offsets of the kernel's input rows
  const int32_t* soff_out;  // [S + 1] of its output rows
  const int2* tab;          // (step, length) of the rows the kernel's threads own
  const int32_t* sid;       // series of those rows
  const int32_t* n_rows;    // their valid prefix
};

template <bool RAG>
__global__ void k_leaky_maxpool_fwd(const float* __restrict__ x, int64_t N, int T, int C, int m,
                                    int To, float slope, float* __restrict__ y,
                                    int32_t* __restrict__ idx, SeriesTab st) {
  const int s = m - 1, p = (m - 1) / 2;
  const int64_t total = N * To * C;
  int64_t Mv = N * To;
  if constexpr (RAG) Mv = live_rows(Mv, st.n_rows);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(j % C);
    const int64_t no = j / C;
    int o;
    int64_t base;  // the first input row of the series
    if constexpr (RAG) {
      if (no >= Mv) {
        y[j] = 0.f;
        idx[j] = 0;
        continue;
      }
      const int n = st.sid[no];
      o = st.tab[no].x;
      base = st.soff_in[n];
      T = st.soff_in[n + 1] - (int)base;
    } else {
      o = (int)(no % To);
      base = (no / To) * T;
    }
    const int t0 = max(o * s - p, 0), t1 = min(o * s - p + m, T);
    float best = -INFINITY;
    int bi = t0;
    for (int t = t0; t < t1; ++t) {
      const float v = leaky(x[(base + t) * C + c], slope);
      if (v > best || v != v) {
        best = v;
        bi = t;
      }
    }
    y[j] = best;
    idx[j] = bi;
  }
}

template <bool RAG>
__global__ void k_leaky_maxpool_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                    const int32_t* __restrict__ idx, int64_t N, int T, int C,
                                    int m, int To, float slope, float* __restrict__ dx,
                                    SeriesTab st) {
  const int s = m - 1, p = (m - 1) / 2;
  const int64_t total = N * T * C;
  int64_t Mv = N * T;
  if constexpr (RAG) Mv = live_rows(Mv, st.n_rows);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(j % C);
    const int64_t nt = j / C;
    int t;
    int64_t base;  // the first pooled row of the series
    if constexpr (RAG) {
      if (nt >= Mv) {
        dx[j] = 0.f;
        continue;
      }
      const int n = st.sid[nt];
      t = st.tab[nt].x;
      base = st.soff_out[n];
      To = st.soff_out[n + 1] - (int)base;
    } else {
      t = (int)(nt % T);
      base = (nt / T) * To;
    }
    // windows o with o*s - p <= t <= o*s - p + m - 1
    const int num = t + p - m + 1;
    int o_lo = num <= 0 ? 0 : (num + s - 1) / s;
    int o_hi = min((t + p) / s, To - 1);
    float gsum = 0.f;
    for (int o = o_lo; o <= o_hi; ++o) {
      const int64_t jo = (base + o) * C + c;
      if (idx[jo] == t) gsum += dy[jo];
    }
    dx[j] = x[j] > 0.f ? gsum : gsum * slope;
  }
}

// ---------------------------------------------------------------------------
// LeakyReLU + [max_t | mean_t] readout (:509-513): y [N, 2C]
// ---------------------------------------------------------------------------
template <bool RAG>
__global__ void k_time_readout_fwd(const float* __restrict__ x, int64_t N, int T, int C,
                                   float slope, float* __restrict__ y,
                                   int32_t* __restrict__ idx, SeriesTab st) {
  const int64_t total = N * C;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t n = j / C;
    const int c = (int)(j - n * C);
    int64_t base = n * T;
    if constexpr (RAG) {
      base = st.soff_in[n];
      T = st.soff_in[n + 1] - (int)base;
    }
    float best = -INFINITY, sum = 0.f;
    int bi = 0;
    for (int t = 0; t < T; ++t) {
      const float v = leaky(x[(base + t) * C + c], slope);
      if (v > best || v != v) {
        best = v;
        bi = t;
      }
      sum += v;
    }
    y[n * 2 * C + c] = best;
    y[n * 2 * C + C + c] = sum / (float)T;
    idx[j] = bi;
  }
}

template <bool RAG>
__global__ void k_time_readout_bwd(const float* __restrict__ x, const float* __restrict__ dy,
                                   const int32_t* __restrict__ idx, int64_t N, int T, int C,
                                   float slope, float* __restrict__ dx, SeriesTab st) {
  const int64_t total = N * T * C;
  int64_t Mv = N * T;
  if constexpr (RAG) Mv = live_rows(Mv, st.n_rows);
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(j % C);
    const int64_t nt = j / C;
    int t;
    int64_t n;
    if constexpr (RAG) {
      if (nt >= Mv) {
        dx[j] = 0.f;
        continue;
      }
      n = st.sid[nt];
      const int2 e = st.tab[nt];
      t = e.x;
      T = e.y;
    } else {
      t = (int)(nt % T);
      n = nt / T;
    }
    float g = dy[n * 2 * C + C + c] / (float)T;
    if (idx[n * C + c] == t) g += dy[n * 2 * C + c];
    dx[j] = x[j] > 0.f ? g : g * slope;
  }
}

inline unsigned flat_grid(int64_t total) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(total, 256), 1 << 20));
}

struct WgPlan {
  int64_t rows_per_wg;
  int n_wg;
};
inline WgPlan wg_plan(int64_t M) {
  const int64_t subs = std::max<int64_t>(1, ceil_div(M, WG_SUB));
  const int64_t rows = WG_SUB * ceil_div(subs, WG_MAX);
  return WgPlan{rows, (int)std::max<int64_t>(1, ceil_div(M, rows))};
}

inline bool taps_ok(int taps) { return taps >= 1 && taps <= MAXTAPS && (taps & 1); }

// sizes every entry shares: N series of T >= 1 steps, N*T*C within int32 rows
inline const char* shape_err(int64_t n, int64_t t, int64_t c) {
  if (n < 0) return "n < 0";
  if (t < 1 || t > (1 << 20)) return "T must be in [1, 2^20]";
  if (c < 1 || c > (1 << 20)) return "C must be in [1, 2^20]";
  if (n * t > ((int64_t)1 << 31) - 1024) return "N*T too large";
  return nullptr;
}

// ---------------------------------------------------------------------------
// hlhgat_tseries_map: the tables of the ragged layout, from tlen alone
// ---------------------------------------------------------------------------
__device__ __forceinline__ int pool_len(int t, int m) {  // hlhgat_maxpool_time_len
  const int s = m - 1, p = (m - 1) / 2;
  const int v = t + 2 * p - m;
  return v < 0 ? 0 : v / s + 1;
}

constexpr int SCAN_T = 1024;

// One workgroup: the exclusive prefix sums of the (clamped) lengths of both
// stages.  Thread i owns a contiguous run of series; the runs' totals are
// scanned in LDS.  Integer sums: any order gives the same result.
__global__ __launch_bounds__(SCAN_T) void k_tseries_scan(const int32_t* __restrict__ tlen, int S,
                                                         int t_max, int m,
                                                         int32_t* __restrict__ soff0,
                                                         int32_t* __restrict__ soff1,
                                                         int32_t* __restrict__ n_rows,
                                                         unsigned* err) {
  __shared__ int p0[SCAN_T], p1[SCAN_T];
  const int tid = threadIdx.x;
  const int per = (S + SCAN_T - 1) / SCAN_T;
  const int lo = min(S, tid * per), hi = min(S, lo + per);
  int a0 = 0, a1 = 0;
  bool bad = false;
  for (int s = lo; s < hi; ++s) {
    int l = tlen[s];
    if (l < 1 || l > t_max) {
      bad = true;
      l = l < 1 ? 1 : t_max;
    }
    a0 += l;
    a1 += pool_len(l, m);
  }
  p0[tid] = a0;
  p1[tid] = a1;
  __syncthreads();
  for (int d = 1; d < SCAN_T; d <<= 1) {  // inclusive scan of the runs' totals
    const int v0 = tid >= d ? p0[tid - d] : 0, v1 = tid >= d ? p1[tid - d] : 0;
    __syncthreads();
    p0[tid] += v0;
    p1[tid] += v1;
    __syncthreads();
  }
  int b0 = p0[tid] - a0, b1 = p1[tid] - a1;
  for (int s = lo; s < hi; ++s) {
    int l = tlen[s];
    l = l < 1 ? 1 : (l > t_max ? t_max : l);
    soff0[s] = b0;
    soff1[s] = b1;
    b0 += l;
    b1 += pool_len(l, m);
  }
  if (tid == SCAN_T - 1) {
    soff0[S] = p0[tid];
    soff1[S] = p1[tid];
    n_rows[0] = p0[tid];
    n_rows[1] = p1[tid];
  }
  if (bad && err) {
    // host memory without PCIe atomics: load + store keeps the other bits
    const unsigned old = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(err, old | (unsigned)HLHGAT_DEVERR_TSERIES_LEN, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Thread j = s * t_max + t writes the table entry of step t of series s (both
// stages) and, as row j, the dead entry of a row past the valid prefix: every
// row of both tables is written exactly once.
__global__ void k_tseries_rows(int S, int t_max, int t_max1, const int32_t* __restrict__ soff0,
                               const int32_t* __restrict__ soff1, int2* __restrict__ tab0,
                               int32_t* __restrict__ sid0, int2* __restrict__ tab1,
                               int32_t* __restrict__ sid1) {
  const int64_t cap0 = (int64_t)S * t_max, cap1 = (int64_t)S * t_max1;
  const int64_t n0 = soff0[S], n1 = soff1[S];
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < cap0;
       j += (int64_t)gridDim.x * blockDim.x) {
    const int s = (int)(j / t_max), t = (int)(j - (int64_t)s * t_max);
    const int o0 = soff0[s], l0 = soff0[s + 1] - o0;
    if (t < l0) {
      tab0[o0 + t] = make_int2(t, l0);
      sid0[o0 + t] = s;
    }
    const int o1 = soff1[s], l1 = soff1[s + 1] - o1;
    if (t < l1) {
      tab1[o1 + t] = make_int2(t, l1);
      sid1[o1 + t] = s;
    }
    if (j >= n0) {
      tab0[j] = make_int2(0, 0);
      sid0[j] = 0;
    }
    if (j >= n1 && j < cap1) {
      tab1[j] = make_int2(0, 0);
      sid1[j] = 0;
    }
  }
}

// padded [S, ldx] -> compact [cap] (dead rows 0), or (inverse) compact ->
// padded with zeros past each series' length: the gradient of the former
__global__ void k_tseries_pack(const float* __restrict__ src, int64_t ldx, int S, int t_max,
                               SeriesTab st, int inverse, float* __restrict__ dst) {
  if (inverse) {
    const int64_t total = (int64_t)S * ldx;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
         j += (int64_t)gridDim.x * blockDim.x) {
      const int s = (int)(j / ldx), t = (int)(j - (int64_t)s * ldx);
      const int o = st.soff_in[s], l = st.soff_in[s + 1] - o;
      dst[j] = t < l ? src[o + t] : 0.f;
    }
  } else {
    const int64_t cap = (int64_t)S * t_max;
    const int64_t Mv = live_rows(cap, st.n_rows);
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < cap;
         j += (int64_t)gridDim.x * blockDim.x)
      dst[j] = j < Mv ? src[(int64_t)st.sid[j] * ldx + st.tab[j].x] : 0.f;
  }
}

// what every ragged entry asks of its map; stage 0: before the pool, 1: after
inline const char* map_err(const hlhgat_tseries_t* mp, int stage) {
  if (!mp) return "NULL map";
  if (stage < 0 || stage > 1) return "stage must be 0 or 1";
  if (mp->n_series < 0) return "S < 0";
  if (mp->t_max[0] < 1 || mp->t_max[0] > (1 << 20)) return "t_max must be in [1, 2^20]";
  if (mp->pool < 2 || mp->pool > 64) return "pool window must be in [2, 64]";
  if (mp->t_max[1] != hlhgat_maxpool_time_len(mp->t_max[0], mp->pool) || mp->t_max[1] < 1 ||
      hlhgat_maxpool_time_len(1, mp->pool) < 1)
    return "t_max[1] is not the pooled length of t_max[0] (or a series of one step pools to "
           "nothing)";
  if (mp->n_series * mp->t_max[0] > ((int64_t)1 << 31) - 1024) return "S * t_max too large";
  for (int i = 0; i < 2; ++i)
    if (!mp->soff[i] || !mp->tab[i] || !mp->sid[i]) return "NULL table";
  if (!mp->n_rows) return "NULL table";
  return nullptr;
}

inline RowTab row_tab(const hlhgat_tseries_t* mp, int stage) {
  return RowTab{reinterpret_cast<const int2*>(mp->tab[stage]), mp->n_rows + stage};
}

// the tables of a kernel whose threads own rows of `own` and whose series
// offsets before / after are those of stages `in` / `out`
inline SeriesTab series_tab(const hlhgat_tseries_t* mp, int in, int out, int own) {
  return SeriesTab{mp->soff[in], mp->soff[out], reinterpret_cast<const int2*>(mp->tab[own]),
                   mp->sid[own], mp->n_rows + own};
}

}  // namespace

extern "C" int hlhgat_tconv_pack(int nb, const float* const* w, const int64_t* cout_b,
                                 const int32_t* taps_b, int64_t cin, int taps,
                                 int flip_transpose, float* wp, void* stream) {
  HLH_CHECK_ARG(taps_ok(taps), "tconv_pack: taps=%d must be odd and <= %d", taps, MAXTAPS);
  HLH_CHECK_ARG(nb >= 1 && nb <= MAXBR, "tconv_pack: nb=%d", nb);
  HLH_CHECK_ARG(cin >= 1 && cin <= (1 << 20), "tconv_pack: C (cin=%lld) must be >= 1",
                (long long)cin);
  HLH_CHECK_ARG(w && cout_b && taps_b && wp, "tconv_pack: NULL pointer");
  PackArgs a{};
  a.nb = nb;
  a.taps = taps;
  a.flip = flip_transpose != 0;
  a.cin = cin;
  a.off[0] = 0;
  for (int b = 0; b < nb; ++b) {
    HLH_CHECK_ARG(w[b], "tconv_pack: NULL pointer (branch %d)", b);
    HLH_CHECK_ARG(cout_b[b] >= 1, "tconv_pack: branch %d has C=%lld < 1", b,
                  (long long)cout_b[b]);
    HLH_CHECK_ARG(taps_ok(taps_b[b]) && taps_b[b] <= taps,
                  "tconv_pack: branch %d taps=%d must be odd and <= %d", b, taps_b[b], taps);
    a.w[b] = w[b];
    a.tb[b] = taps_b[b];
    a.off[b + 1] = a.off[b] + cout_b[b];
  }
  a.cout = a.off[nb];
  HLH_CHECK_ARG(a.cout <= (1 << 20), "tconv_pack: Cout too large");
  a.wp = wp;
  hipLaunchKernelGGL(k_tconv_pack, dim3(flat_grid(taps * a.cout * cin)), dim3(256), 0,
                     as_stream(stream), a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

// The entries below come in pairs: the dense one, and the ragged one that
// passes its map's row table (rt); n and t are then the map's series count
// and capacity per series.
static int tconv_fwd_impl(const float* x, int64_t n, int64_t t, int64_t cin, const float* wp,
                          const float* bias, int64_t cout, int taps, int64_t n1, int64_t n3,
                          float* y, const RowTab* rt, void* stream) {
  HLH_CHECK_ARG(taps_ok(taps), "tconv_fwd: taps=%d must be odd and <= %d", taps, MAXTAPS);
  const char* e = shape_err(n, t, cin);
  HLH_CHECK_ARG(!e, "tconv_fwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n, (long long)t,
                (long long)cin);
  HLH_CHECK_ARG(cout >= 1 && cout <= (1 << 20), "tconv_fwd: C (cout=%lld) must be >= 1",
                (long long)cout);
  HLH_CHECK_ARG(n1 >= 0 && n3 >= 0 && n1 + n3 <= cout, "tconv_fwd: bad n1/n3");
  HLH_CHECK_ARG(x && wp && y, "tconv_fwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  ConvArgs a{x, n * t, (int)t, (int)cin, (int)cout, taps, wp, bias, y, (int)n1, (int)n3, 0, 0,
             rt ? *rt : RowTab{}};
  a.vec_in = (cin % 4) == 0 && aligned16(x) && aligned16(wp);
  a.vec_out = (cout % 4) == 0 && aligned16(y);
  const dim3 grid((unsigned)ceil_div(a.M, TM), (unsigned)ceil_div(cout, 64));
  if (rt && a.vec_in)
    hipLaunchKernelGGL((k_tconv_fwd<true, true>), grid, dim3(256), 0, as_stream(stream), a);
  else if (rt)
    hipLaunchKernelGGL((k_tconv_fwd<false, true>), grid, dim3(256), 0, as_stream(stream), a);
  else if (a.vec_in)
    hipLaunchKernelGGL((k_tconv_fwd<true, false>), grid, dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL((k_tconv_fwd<false, false>), grid, dim3(256), 0, as_stream(stream), a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_tconv_fwd(const float* x, int64_t n, int64_t t, int64_t cin,
                                const float* wp, const float* bias, int64_t cout, int taps,
                                int64_t n1, int64_t n3, float* y, void* stream) {
  return tconv_fwd_impl(x, n, t, cin, wp, bias, cout, taps, n1, n3, y, nullptr, stream);
}

extern "C" int hlhgat_tconv_fwd_ragged(const float* x, const hlhgat_tseries_t* map, int stage,
                                       int64_t cin, const float* wp, const float* bias,
                                       int64_t cout, int taps, int64_t n1, int64_t n3, float* y,
                                       void* stream) {
  const char* e = map_err(map, stage);
  HLH_CHECK_ARG(!e, "tconv_fwd_ragged: %s", e);
  const RowTab rt = row_tab(map, stage);
  return tconv_fwd_impl(x, map->n_series, map->t_max[stage], cin, wp, bias, cout, taps, n1, n3, y,
                        &rt, stream);
}

static int tconv_embed_impl(const float* x, int64_t n, int64_t t, const float* w,
                            const float* bias, int64_t c, int taps, float* y, const RowTab* rt,
                            void* stream) {
  HLH_CHECK_ARG(taps_ok(taps), "tconv_embed_fwd: taps=%d must be odd and <= %d", taps, MAXTAPS);
  const char* e = shape_err(n, t, c);
  HLH_CHECK_ARG(!e, "tconv_embed_fwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)c);
  HLH_CHECK_ARG(x && w && y, "tconv_embed_fwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  const int64_t M = n * t;
  const bool v4 = (c % 4) == 0 && aligned16(y);
  const int64_t total = ceil_div(M, EMB_R) * (v4 ? c / 4 : c);
  const dim3 grid(flat_grid(total));
  const bool small = total < ((int64_t)1 << 31) - ((int64_t)1 << 28);  // 32-bit index math
#define HLH_EMBED(V, I)                                                                     \
  do {                                                                                      \
    if (rt)                                                                                 \
      hipLaunchKernelGGL((k_tconv_embed_fwd<V, I, true>), grid, dim3(256), 0,               \
                         as_stream(stream), x, M, (int)t, w, bias, (int)c, taps, y, *rt);   \
    else                                                                                    \
      hipLaunchKernelGGL((k_tconv_embed_fwd<V, I, false>), grid, dim3(256), 0,              \
                         as_stream(stream), x, M, (int)t, w, bias, (int)c, taps, y, RowTab{}); \
  } while (0)
  if (v4 && small)
    HLH_EMBED(4, uint32_t);
  else if (v4)
    HLH_EMBED(4, int64_t);
  else if (small)
    HLH_EMBED(1, uint32_t);
  else
    HLH_EMBED(1, int64_t);
#undef HLH_EMBED
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_tconv_embed_fwd(const float* x, int64_t n, int64_t t, const float* w,
                                      const float* bias, int64_t c, int taps, float* y,
                                      void* stream) {
  return tconv_embed_impl(x, n, t, w, bias, c, taps, y, nullptr, stream);
}

extern "C" int hlhgat_tconv_embed_fwd_ragged(const float* x, const hlhgat_tseries_t* map,
                                             const float* w, const float* bias, int64_t c,
                                             int taps, float* y, void* stream) {
  const char* e = map_err(map, 0);
  HLH_CHECK_ARG(!e, "tconv_embed_fwd_ragged: %s", e);
  const RowTab rt = row_tab(map, 0);
  return tconv_embed_impl(x, map->n_series, map->t_max[0], w, bias, c, taps, y, &rt, stream);
}

extern "C" int64_t hlhgat_tconv_bwd_weight_workspace_floats(int64_t n, int64_t t, int64_t cin,
                                                            int64_t cout, int taps) {
  if (!taps_ok(taps) || shape_err(n, t, cin) || cout < 1) return 0;
  const WgPlan p = wg_plan(n * t);
  return (int64_t)p.n_wg * (taps * cout * cin + cout);
}

static int tconv_bwd_weight_impl(const float* x, const float* dy, int64_t n, int64_t t,
                                 int64_t cin, int64_t cout, int taps, int nb, float* const* dw,
                                 const int64_t* cout_b, const int32_t* taps_b, float* dbias,
                                 float* workspace, int64_t workspace_floats, const RowTab* rt,
                                 void* stream) {
  HLH_CHECK_ARG(taps_ok(taps), "tconv_bwd_weight: taps=%d must be odd and <= %d", taps,
                MAXTAPS);
  const char* e = shape_err(n, t, cin);
  HLH_CHECK_ARG(!e, "tconv_bwd_weight: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)cin);
  HLH_CHECK_ARG(cout >= 1 && cout <= (1 << 20), "tconv_bwd_weight: C (cout=%lld) must be >= 1",
                (long long)cout);
  HLH_CHECK_ARG(nb >= 1 && nb <= MAXBR, "tconv_bwd_weight: nb=%d", nb);
  HLH_CHECK_ARG(x && dy && dw && cout_b && taps_b && workspace,
                "tconv_bwd_weight: NULL pointer");
  WreduceArgs r{};
  r.off[0] = 0;
  for (int b = 0; b < nb; ++b) {
    HLH_CHECK_ARG(dw[b], "tconv_bwd_weight: NULL pointer (branch %d)", b);
    HLH_CHECK_ARG(cout_b[b] >= 1 && taps_ok(taps_b[b]) && taps_b[b] <= taps,
                  "tconv_bwd_weight: branch %d: C=%lld taps=%d", b, (long long)cout_b[b],
                  taps_b[b]);
    r.dw[b] = dw[b];
    r.tb[b] = taps_b[b];
    r.off[b + 1] = r.off[b] + cout_b[b];
  }
  HLH_CHECK_ARG(r.off[nb] == cout, "tconv_bwd_weight: branches sum to %lld, cout=%lld",
                (long long)r.off[nb], (long long)cout);
  const int64_t need = hlhgat_tconv_bwd_weight_workspace_floats(n, t, cin, cout, taps);
  HLH_CHECK_ARG(workspace_floats >= need, "tconv_bwd_weight: workspace %lld < %lld floats",
                (long long)workspace_floats, (long long)need);
  const int64_t M = n * t;
  const WgPlan p = wg_plan(M);
  const int64_t nw = taps * cout * cin;
  WgradArgs a{x, dy, M, p.rows_per_wg, (int)t, (int)cin, (int)cout, taps, workspace,
              workspace + (int64_t)p.n_wg * nw, rt ? *rt : RowTab{}};
  const unsigned gy = (unsigned)ceil_div(cout, 64), gz = (unsigned)ceil_div(cin, 64);
  HLH_CHECK_ARG(gy <= 65535 && gz <= 65535, "tconv_bwd_weight: too many channel tiles");
  const bool vec = (cin % 4) == 0 && (cout % 4) == 0 && aligned16(x) && aligned16(dy);
  const dim3 wgrid((unsigned)p.n_wg, gy, gz);
  if (rt && vec)
    hipLaunchKernelGGL((k_tconv_wgrad<true, true>), wgrid, dim3(256), 0, as_stream(stream), a);
  else if (rt)
    hipLaunchKernelGGL((k_tconv_wgrad<false, true>), wgrid, dim3(256), 0, as_stream(stream), a);
  else if (vec)
    hipLaunchKernelGGL((k_tconv_wgrad<true, false>), wgrid, dim3(256), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL((k_tconv_wgrad<false, false>), wgrid, dim3(256), 0, as_stream(stream), a);
  HLH_CHECK_LAUNCH();
  r.ws = a.ws;
  r.wsb = a.wsb;
  r.n_wg = p.n_wg;
  r.taps = taps;
  r.nb = nb;
  r.cin = cin;
  r.cout = cout;
  r.dbias = dbias;
  hipLaunchKernelGGL(k_tconv_wreduce, dim3(flat_grid(nw + cout)), dim3(256), 0,
                     as_stream(stream), r);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_tconv_bwd_weight(const float* x, const float* dy, int64_t n, int64_t t,
                                       int64_t cin, int64_t cout, int taps, int nb,
                                       float* const* dw, const int64_t* cout_b,
                                       const int32_t* taps_b, float* dbias, float* workspace,
                                       int64_t workspace_floats, void* stream) {
  return tconv_bwd_weight_impl(x, dy, n, t, cin, cout, taps, nb, dw, cout_b, taps_b, dbias,
                               workspace, workspace_floats, nullptr, stream);
}

extern "C" int hlhgat_tconv_bwd_weight_ragged(const float* x, const float* dy,
                                              const hlhgat_tseries_t* map, int stage,
                                              int64_t cin, int64_t cout, int taps, int nb,
                                              float* const* dw, const int64_t* cout_b,
                                              const int32_t* taps_b, float* dbias,
                                              float* workspace, int64_t workspace_floats,
                                              void* stream) {
  const char* e = map_err(map, stage);
  HLH_CHECK_ARG(!e, "tconv_bwd_weight_ragged: %s", e);
  const RowTab rt = row_tab(map, stage);
  return tconv_bwd_weight_impl(x, dy, map->n_series, map->t_max[stage], cin, cout, taps, nb, dw,
                               cout_b, taps_b, dbias, workspace, workspace_floats, &rt, stream);
}

extern "C" int64_t hlhgat_maxpool_time_len(int64_t t, int m) {
  if (t < 1 || m < 2) return 0;
  const int64_t s = m - 1, p = (m - 1) / 2;
  const int64_t v = t + 2 * p - m;
  return v < 0 ? 0 : v / s + 1;
}

static int maxpool_fwd_impl(const float* x, int64_t n, int64_t t, int64_t c, int m, float slope,
                            float* y, int32_t* idx, const SeriesTab* st, void* stream) {
  const char* e = shape_err(n, t, c);
  HLH_CHECK_ARG(!e, "leaky_maxpool_time_fwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)c);
  HLH_CHECK_ARG(m >= 2 && m <= 64, "leaky_maxpool_time_fwd: window m=%d", m);
  const int64_t to = hlhgat_maxpool_time_len(t, m);
  HLH_CHECK_ARG(to >= 1, "leaky_maxpool_time_fwd: T=%lld shorter than the window", (long long)t);
  HLH_CHECK_ARG(x && y && idx, "leaky_maxpool_time_fwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  if (st)
    hipLaunchKernelGGL(k_leaky_maxpool_fwd<true>, dim3(flat_grid(n * to * c)), dim3(256), 0,
                       as_stream(stream), x, n, (int)t, (int)c, m, (int)to, slope, y, idx, *st);
  else
    hipLaunchKernelGGL(k_leaky_maxpool_fwd<false>, dim3(flat_grid(n * to * c)), dim3(256), 0,
                       as_stream(stream), x, n, (int)t, (int)c, m, (int)to, slope, y, idx,
                       SeriesTab{});
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_leaky_maxpool_time_fwd(const float* x, int64_t n, int64_t t, int64_t c,
                                             int m, float slope, float* y, int32_t* idx,
                                             void* stream) {
  return maxpool_fwd_impl(x, n, t, c, m, slope, y, idx, nullptr, stream);
}

extern "C" int hlhgat_leaky_maxpool_time_fwd_ragged(const float* x, const hlhgat_tseries_t* map,
                                                    int64_t c, float slope, float* y,
                                                    int32_t* idx, void* stream) {
  const char* e = map_err(map, 0);
  HLH_CHECK_ARG(!e, "leaky_maxpool_time_fwd_ragged: %s", e);
  const SeriesTab st = series_tab(map, 0, 1, 1);
  return maxpool_fwd_impl(x, map->n_series, map->t_max[0], c, map->pool, slope, y, idx, &st,
                          stream);
}

static int maxpool_bwd_impl(const float* x, const float* dy, const int32_t* idx, int64_t n,
                            int64_t t, int64_t c, int m, float slope, float* dx,
                            const SeriesTab* st, void* stream) {
  const char* e = shape_err(n, t, c);
  HLH_CHECK_ARG(!e, "leaky_maxpool_time_bwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)c);
  HLH_CHECK_ARG(m >= 2 && m <= 64, "leaky_maxpool_time_bwd: window m=%d", m);
  const int64_t to = hlhgat_maxpool_time_len(t, m);
  HLH_CHECK_ARG(to >= 1, "leaky_maxpool_time_bwd: T=%lld shorter than the window", (long long)t);
  HLH_CHECK_ARG(x && dy && idx && dx, "leaky_maxpool_time_bwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  if (st)
    hipLaunchKernelGGL(k_leaky_maxpool_bwd<true>, dim3(flat_grid(n * t * c)), dim3(256), 0,
                       as_stream(stream), x, dy, idx, n, (int)t, (int)c, m, (int)to, slope, dx,
                       *st);
  else
    hipLaunchKernelGGL(k_leaky_maxpool_bwd<false>, dim3(flat_grid(n * t * c)), dim3(256), 0,
                       as_stream(stream), x, dy, idx, n, (int)t, (int)c, m, (int)to, slope, dx,
                       SeriesTab{});
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_leaky_maxpool_time_bwd(const float* x, const float* dy,
                                             const int32_t* idx, int64_t n, int64_t t,
                                             int64_t c, int m, float slope, float* dx,
                                             void* stream) {
  return maxpool_bwd_impl(x, dy, idx, n, t, c, m, slope, dx, nullptr, stream);
}

extern "C" int hlhgat_leaky_maxpool_time_bwd_ragged(const float* x, const float* dy,
                                                    const int32_t* idx,
                                                    const hlhgat_tseries_t* map, int64_t c,
                                                    float slope, float* dx, void* stream) {
  const char* e = map_err(map, 0);
  HLH_CHECK_ARG(!e, "leaky_maxpool_time_bwd_ragged: %s", e);
  const SeriesTab st = series_tab(map, 0, 1, 0);
  return maxpool_bwd_impl(x, dy, idx, map->n_series, map->t_max[0], c, map->pool, slope, dx, &st,
                          stream);
}

static int readout_fwd_impl(const float* x, int64_t n, int64_t t, int64_t c, float slope,
                            float* y, int32_t* idx, const SeriesTab* st, void* stream) {
  const char* e = shape_err(n, t, c);
  HLH_CHECK_ARG(!e, "time_readout_fwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)c);
  HLH_CHECK_ARG(x && y && idx, "time_readout_fwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  if (st)
    hipLaunchKernelGGL(k_time_readout_fwd<true>, dim3(flat_grid(n * c)), dim3(256), 0,
                       as_stream(stream), x, n, (int)t, (int)c, slope, y, idx, *st);
  else
    hipLaunchKernelGGL(k_time_readout_fwd<false>, dim3(flat_grid(n * c)), dim3(256), 0,
                       as_stream(stream), x, n, (int)t, (int)c, slope, y, idx, SeriesTab{});
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_time_readout_fwd(const float* x, int64_t n, int64_t t, int64_t c,
                                       float slope, float* y, int32_t* idx, void* stream) {
  return readout_fwd_impl(x, n, t, c, slope, y, idx, nullptr, stream);
}

extern "C" int hlhgat_time_readout_fwd_ragged(const float* x, const hlhgat_tseries_t* map,
                                              int64_t c, float slope, float* y, int32_t* idx,
                                              void* stream) {
  const char* e = map_err(map, 1);
  HLH_CHECK_ARG(!e, "time_readout_fwd_ragged: %s", e);
  const SeriesTab st = series_tab(map, 1, 1, 1);
  return readout_fwd_impl(x, map->n_series, map->t_max[1], c, slope, y, idx, &st, stream);
}

static int readout_bwd_impl(const float* x, const float* dy, const int32_t* idx, int64_t n,
                            int64_t t, int64_t c, float slope, float* dx, const SeriesTab* st,
                            void* stream) {
  const char* e = shape_err(n, t, c);
  HLH_CHECK_ARG(!e, "time_readout_bwd: %s (n=%lld T=%lld C=%lld)", e, (long long)n,
                (long long)t, (long long)c);
  HLH_CHECK_ARG(x && dy && idx && dx, "time_readout_bwd: NULL pointer");
  if (n == 0) return HLHGAT_OK;
  if (st)
    hipLaunchKernelGGL(k_time_readout_bwd<true>, dim3(flat_grid(n * t * c)), dim3(256), 0,
                       as_stream(stream), x, dy, idx, n, (int)t, (int)c, slope, dx, *st);
  else
    hipLaunchKernelGGL(k_time_readout_bwd<false>, dim3(flat_grid(n * t * c)), dim3(256), 0,
                       as_stream(stream), x, dy, idx, n, (int)t, (int)c, slope, dx, SeriesTab{});
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_time_readout_bwd(const float* x, const float* dy, const int32_t* idx,
                                       int64_t n, int64_t t, int64_t c, float slope, float* dx,
                                       void* stream) {
  return readout_bwd_impl(x, dy, idx, n, t, c, slope, dx, nullptr, stream);
}

extern "C" int hlhgat_time_readout_bwd_ragged(const float* x, const float* dy,
                                              const int32_t* idx, const hlhgat_tseries_t* map,
                                              int64_t c, float slope, float* dx, void* stream) {
  const char* e = map_err(map, 1);
  HLH_CHECK_ARG(!e, "time_readout_bwd_ragged: %s", e);
  const SeriesTab st = series_tab(map, 1, 1, 1);
  return readout_bwd_impl(x, dy, idx, map->n_series, map->t_max[1], c, slope, dx, &st, stream);
}

// ---------------------------------------------------------------------------
// the ragged layout's tables
// ---------------------------------------------------------------------------
extern "C" int hlhgat_tseries_map(const int32_t* tlen, const hlhgat_tseries_t* map,
                                  void* stream) {
  const char* e = map_err(map, 0);
  HLH_CHECK_ARG(!e, "tseries_map: %s", e);
  HLH_CHECK_ARG(tlen, "tseries_map: NULL tlen");
  const int S = (int)map->n_series;
  hipLaunchKernelGGL(k_tseries_scan, dim3(1), dim3(SCAN_T), 0, as_stream(stream), tlen, S,
                     (int)map->t_max[0], (int)map->pool, map->soff[0], map->soff[1], map->n_rows,
                     device_error_word());
  HLH_CHECK_LAUNCH();
  if (S == 0) return HLHGAT_OK;
  hipLaunchKernelGGL(k_tseries_rows, dim3(flat_grid(map->n_series * map->t_max[0])), dim3(256), 0,
                     as_stream(stream), S, (int)map->t_max[0], (int)map->t_max[1], map->soff[0],
                     map->soff[1], reinterpret_cast<int2*>(map->tab[0]), map->sid[0],
                     reinterpret_cast<int2*>(map->tab[1]), map->sid[1]);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_tseries_pack(const float* src, int64_t ldx, const hlhgat_tseries_t* map,
                                   int inverse, float* dst, void* stream) {
  const char* e = map_err(map, 0);
  HLH_CHECK_ARG(!e, "tseries_pack: %s", e);
  HLH_CHECK_ARG(ldx >= map->t_max[0], "tseries_pack: ldx=%lld < t_max=%lld", (long long)ldx,
                (long long)map->t_max[0]);
  HLH_CHECK_ARG(map->n_series * ldx <= ((int64_t)1 << 40), "tseries_pack: S * ldx too large");
  HLH_CHECK_ARG(src && dst, "tseries_pack: NULL pointer");
  if (map->n_series == 0) return HLHGAT_OK;
  const SeriesTab st = series_tab(map, 0, 0, 0);
  const int64_t total = inverse ? map->n_series * ldx : map->n_series * map->t_max[0];
  hipLaunchKernelGGL(k_tseries_pack, dim3(flat_grid(total)), dim3(256), 0, as_stream(stream), src,
                     ldx, (int)map->n_series, (int)map->t_max[0], st, inverse, dst);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
