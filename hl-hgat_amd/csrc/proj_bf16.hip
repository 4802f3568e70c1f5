// Dense projections with bf16 operands and fp32 accumulation on the gfx950
// matrix cores: the opt-in family beside the fp32 kernels of proj.hip
// (hlhgat_set_gemm_precision).  Storage stays fp32 everywhere: operands are
// rounded to bf16 (v_cvt_pk_bf16_f32, round to nearest even) on their way into
// registers or LDS, the products of two bf16 values are exact in fp32, and
// bias, accumulate adds, the bias gradient and the split reduction are fp32.
//
// MFMA: v_mfma_f32_16x16x32_bf16.  Lane l = 16*q + i supplies A[row i][k =
// 8q + j] and B[k = 8q + j][col i] (j = 0..7: one 16-byte fragment each);
// accumulator register r holds C[4q + r][i] -- the C/D map of the fp32
// 16x16x4 instruction, so the geometry (4 waves x 16 rows, TN x 16 columns)
// and the row-store epilogue of gemm_core.h carry over.
//
// LDS image of every staged operand tile: rows of 64 bf16 (128 B, eight 16-B
// slots), slot s of row r stored at slot s ^ ((r >> 1) & 7).  The ds_read_b128
// of a fragment (lanes (q, i): row i, slot 4h + q) then puts each of the
// instruction's four 16-lane groups on 16 distinct 16-B slots of the 256-B
// bank row; an unswizzled 128-B row would be 8-way conflicted.  The
// transposing ds_write_b32 of the gradients (32 lanes: one row, 32
// consecutive words up to the slot permutation) are conflict-free too.
#include "gemm_core.h"
#include "proj_args.h"
#include "proj_bf16.h"

#include <atomic>

using namespace hlhgat;

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

// two fp32 -> one dword of two bf16, round to nearest even; lo is element 0
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
  const bf16x2 v = {(__bf16)lo, (__bf16)hi};
  return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ u32x4 pack8(const float4& x, const float4& y) {
  return u32x4{pack2(x.x, x.y), pack2(x.z, x.w), pack2(y.x, y.y), pack2(y.z, y.w)};
}
// element j of the result pairs x[j] (even reduction index) with y[j] (odd)
__device__ __forceinline__ u32x4 pack_pairs(const float4& x, const float4& y) {
  return u32x4{pack2(x.x, y.x), pack2(x.y, y.y), pack2(x.z, y.z), pack2(x.w, y.w)};
}
__device__ __forceinline__ floatx4 mfma_bf16(const u32x4& a, const u32x4& b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                 __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

constexpr int kRowB = 128;  // bytes of one LDS tile row: 64 bf16
__device__ __forceinline__ int tile_off(int row, int slot) {
  return row * kRowB + 16 * (slot ^ ((row >> 1) & 7));
}
__device__ __forceinline__ u32x4 read_frag(const unsigned char* tile, int row, int slot) {
  return *reinterpret_cast<const u32x4*>(tile + tile_off(row, slot));
}

// A lane's two fragments of a 64-wide chunk of its fp32 row: elements
// k0 + 32h + 8q + (0..7), h = 0, 1; zero past `lim` (lim % 4 == 0).
__device__ __forceinline__ void load_row_frags(const float* row, bool valid, int k0, int lim,
                                               int q, u32x4 (&o)[2]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int k = k0 + 32 * h + 8 * q;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
    if (valid && k < lim) x = *reinterpret_cast<const float4*>(row + k);
    if (valid && k + 4 < lim) y = *reinterpret_cast<const float4*>(row + k + 4);
    o[h] = pack8(x, y);
  }
}

// workgroups are dealt round-robin over the 8 XCDs: item w of linear id L
// makes each XCD walk one contiguous range of the items
__device__ __forceinline__ unsigned xcd_item(unsigned L, unsigned total) {
  const unsigned x = L & 7u, k = L >> 3, per = total >> 3, extra = total & 7u;
  return x * per + (x < extra ? x : extra) + k;
}

// ---------------------------------------------------------------------------
// forward: C = sum_b A_b W_b^T + bias.  The W chunk W_b[n_tile][k0:k0+64] is
// converted once per workgroup and staged in LDS (double buffered) for its 4
// waves; each lane streams its A row chunk into two fragments one chunk ahead.
// Two MFMAs per 16-column tile and 64-wide chunk.
// ---------------------------------------------------------------------------
template <int TN>
__global__ __launch_bounds__(256) void k_proj_fwd_bf16(FwdArgs a) {
  constexpr int kTile = TN * 16 * kRowB;
  constexpr int kScratch = 4 * 16 * (TN * 16 + 4) * (int)sizeof(float);
  constexpr int kLds = 2 * kTile > kScratch ? 2 * kTile : kScratch;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLds];
  constexpr int U = (TN + 1) / 2;  // staging items per thread: TN*16 rows x 8 slots

  unsigned bx = blockIdx.x, by = blockIdx.y;
  if (a.xcd_map && gridDim.y > 1) {  // the column tiles of one row block on one XCD
    const unsigned w = xcd_item(blockIdx.x + blockIdx.y * gridDim.x, gridDim.x * gridDim.y);
    bx = w / gridDim.y;
    by = w % gridDim.y;
  }
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
  const int64_t m_base = ((int64_t)bx * 4 + wave) * 16;
  const int n_base = (int)by * (TN * 16);
  const int64_t row = m_base + i;
  const bool aval = row < a.M;

  auto load_w = [&](int b, int k0, u32x4 (&st)[U]) {
    const float* W = a.W[b];
    const int kb = a.kb[b];
    const int64_t ldw = a.ldw[b];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int r = idx >> 3, c8 = idx & 7;
      const int n = n_base + r, k = k0 + 8 * c8;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (r < TN * 16 && n < a.N && k < kb) {  // kb % 8 == 0: k + 7 < kb
        x = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + k);
        y = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + k + 4);
      }
      st[u] = pack8(x, y);
    }
  };
  auto store_w = [&](unsigned char* tile, const u32x4 (&st)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int r = idx >> 3, c8 = idx & 7;
      if (r < TN * 16) *reinterpret_cast<u32x4*>(tile + tile_off(r, c8)) = st[u];
    }
  };

  floatx4 acc[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) acc[tn] = floatx4{0.f, 0.f, 0.f, 0.f};

  int b = 0, k0 = 0;
  u32x4 wst[U], ac[2];
  load_w(b, k0, wst);
  load_row_frags(a.A[b] + (aval ? row : 0) * a.lda[b], aval, k0, a.kb[b], q, ac);
  store_w(lds, wst);
  __syncthreads();
  int buf = 0;
  while (b < a.nb) {
    int nbk = b, nk = k0 + KC;
    if (nk >= a.kb[b]) {
      nbk = b + 1;
      nk = 0;
    }
    const bool has_next = nbk < a.nb;
    u32x4 an[2];
    if (has_next) {
      load_w(nbk, nk, wst);
      load_row_frags(a.A[nbk] + (aval ? row : 0) * a.lda[nbk], aval, nk, a.kb[nbk], q, an);
    }
    const unsigned char* tile = lds + buf * kTile;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 bf[TN];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) bf[tn] = read_frag(tile, tn * 16 + i, 4 * h + q);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) acc[tn] = mfma_bf16(ac[h], bf[tn], acc[tn]);
    }
    if (has_next) {
      store_w(lds + (buf ^ 1) * kTile, wst);
      ac[0] = an[0];
      ac[1] = an[1];
    }
    __syncthreads();
    buf ^= 1;
    b = nbk;
    k0 = nk;
  }

  // every wave is past the loop's last barrier: the tiles are free
  float* scratch = reinterpret_cast<float*>(lds) + wave * 16 * (TN * 16 + 4);
  const int ncols = a.N - n_base < TN * 16 ? a.N - n_base : TN * 16;
  const bool vec_ok = (a.N % 4) == 0 && (a.ldc % 4) == 0 &&
                      (reinterpret_cast<uintptr_t>(a.C) & 15) == 0;
  store_tile_rows<TN>(acc, scratch, m_base, a.M, a.C + n_base, a.ldc, ncols,
                      a.bias ? a.bias + n_base : nullptr, a.accumulate, vec_ok);
}

// ---------------------------------------------------------------------------
// data gradient: dA_b (+)= dC W_b (reduction over N).  W_b[n0:n0+64][c_tile]
// is staged TRANSPOSED (tile row = output column c, 64 n along the row): a
// thread loads W[n][c..c+3] and W[n+1][c..c+3], packs the (n, n+1) pairs and
// writes one dword to each of the four rows, so a lane's B fragment (8
// consecutive n of one column) is again one ds_read_b128.  dC rows stream into
// fragments one chunk ahead.  One workgroup per (row block, column tile); the
// column tiles of a row block run on one XCD (its dC rows hit that L2).
// ---------------------------------------------------------------------------
template <int TN>
__global__ __launch_bounds__(256) void k_proj_bwd_data_bf16(BwdDataArgs a) {
  constexpr int kTile = TN * 16 * kRowB;
  constexpr int kScratch = 4 * 16 * (TN * 16 + 4) * (int)sizeof(float);
  constexpr int kLds = 2 * kTile > kScratch ? 2 * kTile : kScratch;
  __shared__ __attribute__((aligned(16))) unsigned char lds[kLds];
  constexpr int U = (TN + 1) / 2;  // staging items per thread: TN*4 column quads x 32 n pairs

  const int tiles = a.tile_start[a.nb];
  const unsigned w = xcd_item(blockIdx.x, gridDim.x);
  const int by = (int)(w % (unsigned)tiles);
  const int64_t bx = w / (unsigned)tiles;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
  const int64_t m_base = (bx * 4 + wave) * 16;
  int b = 0;
  while (b + 1 < a.nb && by >= a.tile_start[b + 1]) ++b;
  const int kb = a.kb[b];
  const int c_base = (by - a.tile_start[b]) * (TN * 16);
  const float* __restrict__ W = a.W[b];
  const int64_t ldw = a.ldw[b];
  const int64_t row = m_base + i;
  const bool gval = row < a.M;
  const float* grow = a.G + (gval ? row : 0) * a.ldg;

  auto load_w = [&](int n0, u32x4 (&st)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int p = idx & 31, c4 = idx >> 5;
      const int n = n0 + 2 * p, c = c_base + 4 * c4;
      float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
      if (c4 < TN * 4 && c < kb) {  // kb % 8 == 0: c + 3 < kb
        if (n < a.N) x = *reinterpret_cast<const float4*>(W + (int64_t)n * ldw + c);
        if (n + 1 < a.N) y = *reinterpret_cast<const float4*>(W + (int64_t)(n + 1) * ldw + c);
      }
      st[u] = pack_pairs(x, y);
    }
  };
  auto store_w = [&](unsigned char* tile, const u32x4 (&st)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int p = idx & 31, c4 = idx >> 5;
      if (c4 < TN * 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<unsigned*>(tile + tile_off(4 * c4 + j, p >> 2) + 4 * (p & 3)) = st[u][j];
      }
    }
  };

  floatx4 acc[TN];
#pragma unroll
  for (int tn = 0; tn < TN; ++tn) acc[tn] = floatx4{0.f, 0.f, 0.f, 0.f};
  u32x4 wst[U], gc[2];
  load_w(0, wst);
  load_row_frags(grow, gval, 0, a.N, q, gc);
  store_w(lds, wst);
  __syncthreads();
  int buf = 0;
  for (int n0 = 0; n0 < a.N; n0 += KC) {
    const bool has_next = n0 + KC < a.N;
    u32x4 gn[2];
    if (has_next) {
      load_w(n0 + KC, wst);
      load_row_frags(grow, gval, n0 + KC, a.N, q, gn);
    }
    const unsigned char* tile = lds + buf * kTile;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 bf[TN];
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) bf[tn] = read_frag(tile, tn * 16 + i, 4 * h + q);
#pragma unroll
      for (int tn = 0; tn < TN; ++tn) acc[tn] = mfma_bf16(gc[h], bf[tn], acc[tn]);
    }
    if (has_next) {
      store_w(lds + (buf ^ 1) * kTile, wst);
      gc[0] = gn[0];
      gc[1] = gn[1];
    }
    __syncthreads();
    buf ^= 1;
  }
  float* scratch = reinterpret_cast<float*>(lds) + wave * 16 * (TN * 16 + 4);
  const int ncols = kb - c_base < TN * 16 ? kb - c_base : TN * 16;
  const bool vec_ok = (a.ldo[b] % 4) == 0 && (reinterpret_cast<uintptr_t>(a.O[b]) & 15) == 0;
  store_tile_rows<TN>(acc, scratch, m_base, a.M, a.O[b] + c_base, a.ldo[b], ncols, nullptr,
                      a.accumulate, vec_ok);
}

// ---------------------------------------------------------------------------
// weight gradient: dW_b = dC^T A_b, db = sum_m dC (reduction over M).  The
// deterministic split-M scheme of the fp32 kernels: a workgroup owns a 64 (n)
// x 64 (k) tile of one block and one slice of M and writes fp32 partials to
// the split slab, which k_reduce_splits sums in order.  64-row chunks of dC
// and A_b are staged TRANSPOSED (tile row = n resp. k, 64 m along the row,
// (m, m+1) pairs packed as in the data gradient), so both MFMA operands are
// one ds_read_b128 per fragment; each wave accumulates a 32 x 32 quadrant as
// 2 x 2 accumulators.  db rides along in the k_base == 0 tiles of block 0,
// summed in fp32 from the unrounded dC, per thread over its rows and then over
// the 32 row-pair owners in fixed order.
// ---------------------------------------------------------------------------
constexpr int WCH = 64;          // rows of M per staged chunk
constexpr int kWFlushChunks = 4;  // the MFMA accumulators chain at most 256 rows

__global__ __launch_bounds__(256) void k_proj_bwd_weight_bf16(BwdWeightArgs a) {
  constexpr int kTile = 64 * kRowB;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][kTile];  // [buffer][dC, A]
  int by = (int)blockIdx.y, bz = (int)blockIdx.z;
  if (a.xcd_map) {
    const unsigned w = xcd_item(blockIdx.y + blockIdx.z * gridDim.y, gridDim.y * gridDim.z);
    by = (int)(w % gridDim.y);
    bz = (int)(w / gridDim.y);
  }
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int q = lane >> 4, i = lane & 15;
  const int wn = wave >> 1, wk = wave & 1;
  int b = 0;
  while (b + 1 < a.nb && by >= a.tile_start[b + 1]) ++b;
  const int t = by - a.tile_start[b];
  const int n_base = (t % a.tiles_n) * 64;
  const int k_base = (t / a.tiles_n) * 64;
  const int kb = a.kb[b];
  const float* __restrict__ A = a.A[b];
  const int64_t lda = a.lda[b];
  const bool do_bias = a.bias_off >= 0 && b == 0 && k_base == 0;
  const int64_t m_lo = (int64_t)bz * a.rows_per_split;
  int64_t m_hi = m_lo + a.rows_per_split;
  if (m_hi > a.M) m_hi = a.M;

  // staging: 16 column quads x 32 row pairs per operand, two items per thread
  float4 bsum[2];
  bsum[0] = bsum[1] = make_float4(0.f, 0.f, 0.f, 0.f);
  struct Stage {
    u32x4 g[2], x[2];
  };
  auto load = [&](int64_t m0, Stage& st) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int p = idx & 31, c4 = idx >> 5;
      const int64_t m = m0 + 2 * p;
      const bool v0 = m < m_hi, v1 = m + 1 < m_hi;
      const int n = n_base + 4 * c4, k = k_base + 4 * c4;
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 g0 = z, g1 = z, x0 = z, x1 = z;
      if (n < a.N) {  // N % 4 == 0: n + 3 < N
        if (v0) g0 = *reinterpret_cast<const float4*>(a.G + m * a.ldg + n);
        if (v1) g1 = *reinterpret_cast<const float4*>(a.G + (m + 1) * a.ldg + n);
      }
      if (k < kb) {
        if (v0) x0 = *reinterpret_cast<const float4*>(A + m * lda + k);
        if (v1) x1 = *reinterpret_cast<const float4*>(A + (m + 1) * lda + k);
      }
      if (do_bias) {
        bsum[u].x = (bsum[u].x + g0.x) + g1.x;
        bsum[u].y = (bsum[u].y + g0.y) + g1.y;
        bsum[u].z = (bsum[u].z + g0.z) + g1.z;
        bsum[u].w = (bsum[u].w + g0.w) + g1.w;
      }
      st.g[u] = pack_pairs(g0, g1);
      st.x[u] = pack_pairs(x0, x1);
    }
  };
  auto store = [&](int buf, const Stage& st) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int p = idx & 31, c4 = idx >> 5;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int off = tile_off(4 * c4 + j, p >> 2) + 4 * (p & 3);
        *reinterpret_cast<unsigned*>(&lds[buf][0][off]) = st.g[u][j];
        *reinterpret_cast<unsigned*>(&lds[buf][1][off]) = st.x[u][j];
      }
    }
  };

  floatx4 acc[2][2], outer[2][2];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = outer[tm][tn] = floatx4{0.f, 0.f, 0.f, 0.f};

  const int64_t nchunk = m_hi > m_lo ? (m_hi - m_lo + WCH - 1) / WCH : 0;
  Stage st;
  if (nchunk > 0) {
    load(m_lo, st);
    store(0, st);
  }
  __syncthreads();
  int buf = 0;
  for (int64_t c = 0; c < nchunk; ++c) {
    const bool has_next = c + 1 < nchunk;
    if (has_next) load(m_lo + (c + 1) * WCH, st);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      u32x4 ga[2], xb[2];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        ga[tt] = read_frag(lds[buf][0], 32 * wn + 16 * tt + i, 4 * h + q);
        xb[tt] = read_frag(lds[buf][1], 32 * wk + 16 * tt + i, 4 * h + q);
      }
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) acc[tm][tn] = mfma_bf16(ga[tm], xb[tn], acc[tm][tn]);
    }
    if ((c + 1) % kWFlushChunks == 0 && has_next) {
#pragma unroll
      for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
          outer[tm][tn] = outer[tm][tn] + acc[tm][tn];
          acc[tm][tn] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
    }
    if (has_next) store(buf ^ 1, st);
    __syncthreads();
    buf ^= 1;
  }

  float* slab = a.part + (int64_t)bz * a.part_stride + a.part_off[b];
#pragma unroll
  for (int tm = 0; tm < 2; ++tm)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
      const int k = k_base + 32 * wk + 16 * tn + i;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n_base + 32 * wn + 16 * tm + 4 * q + r;
        if (n < a.N && k < kb) slab[(int64_t)n * kb + k] = outer[tm][tn][r] + acc[tm][tn][r];
      }
    }
  if (do_bias) {  // every wave is past the last barrier: the tiles are free
    float* br = reinterpret_cast<float*>(&lds[0][0][0]);  // [32 row pairs][64 n]
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = threadIdx.x + 256 * u;
      const int p = idx & 31, c4 = idx >> 5;
      *reinterpret_cast<float4*>(br + p * 64 + 4 * c4) = bsum[u];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
      float v = 0.f;
      for (int p = 0; p < 32; ++p) v = v + br[p * 64 + threadIdx.x];
      const int n = n_base + (int)threadIdx.x;
      if (n < a.N) a.part[(int64_t)bz * a.part_stride + a.bias_off + n] = v;
    }
  }
}

std::atomic<int> g_precision{HLHGAT_GEMM_FP32};
std::atomic<int64_t> g_bf16_calls{0}, g_fallback_calls{0};

}  // namespace

namespace hlhgat {

int gemm_precision() { return g_precision.load(std::memory_order_relaxed); }

bool gemm_bf16_shape_ok(int nblocks, const int64_t* kb, const int64_t* ld, int64_t N) {
  if (nblocks < 1 || nblocks > MAXB || !kb || N <= 0 || N % 4 != 0) return false;
  for (int b = 0; b < nblocks; ++b) {
    if (kb[b] <= 0 || kb[b] % 8 != 0) return false;
    if (ld && (ld[b] < kb[b] || ld[b] % 4 != 0)) return false;
  }
  return true;
}

bool gemm_bf16_operands_ok(int nblocks, const float* const* P, const int64_t* ld,
                           const int64_t* kb, int64_t N) {
  if (!P || !ld || !gemm_bf16_shape_ok(nblocks, kb, ld, N)) return false;
  for (int b = 0; b < nblocks; ++b)
    if (!P[b] || !aligned16(P[b])) return false;
  return true;
}

bool gemm_bf16_route(bool eligible) {
  if (gemm_precision() != HLHGAT_GEMM_BF16) return false;
  (eligible ? g_bf16_calls : g_fallback_calls).fetch_add(1, std::memory_order_relaxed);
  return eligible;
}

int launch_proj_fwd_bf16(const void* fwd_args, int tn, hipStream_t s, const ProfScope* prof) {
  const FwdArgs& a = *static_cast<const FwdArgs*>(fwd_args);
  const dim3 g((unsigned)ceil_div(a.M, 64), (unsigned)ceil_div(a.N, tn * 16));
  if (tn == 1)
    launch(k_proj_fwd_bf16<1>, g, dim3(256), 0, s, prof, a);
  else if (tn == 2)
    launch(k_proj_fwd_bf16<2>, g, dim3(256), 0, s, prof, a);
  else
    launch(k_proj_fwd_bf16<4>, g, dim3(256), 0, s, prof, a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

int launch_proj_bwd_data_bf16(const void* data_args, int tnd, hipStream_t s) {
  const BwdDataArgs& a = *static_cast<const BwdDataArgs*>(data_args);
  const int64_t nblk = ceil_div(a.M, 64) * a.tile_start[a.nb];
  HLH_CHECK_ARG(nblk > 0 && nblk < (int64_t)INT32_MAX, "proj_bwd_data: grid too large");
  const dim3 g((unsigned)nblk);
  if (tnd == 1)
    launch(k_proj_bwd_data_bf16<1>, g, dim3(256), 0, s, nullptr, a);
  else if (tnd == 2)
    launch(k_proj_bwd_data_bf16<2>, g, dim3(256), 0, s, nullptr, a);
  else
    launch(k_proj_bwd_data_bf16<4>, g, dim3(256), 0, s, nullptr, a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

int launch_proj_bwd_weight_bf16(const void* weight_args, int tiles_total, int splits,
                                hipStream_t s) {
  const BwdWeightArgs& a = *static_cast<const BwdWeightArgs*>(weight_args);
  launch(k_proj_bwd_weight_bf16, dim3(1, (unsigned)tiles_total, (unsigned)splits), dim3(256), 0, s,
         nullptr, a);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

}  // namespace hlhgat

extern "C" int hlhgat_set_gemm_precision(int mode) {
  HLH_CHECK_ARG(mode == HLHGAT_GEMM_FP32 || mode == HLHGAT_GEMM_BF16,
                "set_gemm_precision: mode must be HLHGAT_GEMM_FP32 or HLHGAT_GEMM_BF16");
  g_precision.store(mode, std::memory_order_relaxed);
  return HLHGAT_OK;
}

extern "C" int hlhgat_get_gemm_precision(void) { return gemm_precision(); }

extern "C" int hlhgat_gemm_bf16_eligible(int nblocks, const int64_t* kb, const int64_t* ld,
                                         int64_t N, int aligned16) {
  return (aligned16 != 0 && gemm_bf16_shape_ok(nblocks, kb, ld, N)) ? 1 : 0;
}

extern "C" int hlhgat_gemm_precision_stats(int64_t out[2], int reset) {
  HLH_CHECK_ARG(out, "gemm_precision_stats: out is NULL");
  if (reset) {
    out[0] = g_bf16_calls.exchange(0);
    out[1] = g_fallback_calls.exchange(0);
  } else {
    out[0] = g_bf16_calls.load();
    out[1] = g_fallback_calls.load();
  }
  return HLHGAT_OK;
}
