// Training objectives of the reference's main_*.py loops that reduce to one
// scalar: BCE-with-logits over an on-device selection (mean / sum / the focal
// form of lib/Loss_function.py:14-26) and row-wise cross-entropy
// (torch.nn.CrossEntropyLoss, main_cifar10SP...:137,203); and, in the simpler
// one-workgroup form of the L1 / BCE entries of runtime.hip, the brain
// notebook's mean squared error (section (c) below).
//
// Reduction structure (both families).  No floating-point atomics and no
// hand-off between workgroups inside a launch.  The forward is a grid kernel
// that writes one 32-byte partial record per workgroup into the caller's
// workspace, followed by a one-workgroup finish kernel that sums the records
// in index order with a fixed tree and writes the results.  Problems of up to
// kOneWG elements (rows) run as ONE workgroup that finishes itself: one
// launch, no workspace traffic.  The grid is min(ceil(n / 4096), 256)
// workgroups -- a function of the problem size alone, never of the device --
// and every thread walks its elements in a fixed order, so a result is a
// function of the inputs: bitwise equal across runs, streams, eager or
// replayed, and across pointer alignments (the 16-byte and the scalar load
// paths give every thread the same elements in the same order).
//
// Empty selection (cnt == 0): loss = 0 and dx = 0.  torch returns NaN for the
// mean of nothing; one all-missing batch must not poison Adam inside a
// captured step, so this library does not.
//
// The backward of either family is one grid-stride elementwise launch that
// reads the forward's device scalars (sum, count); nothing returns to the host.
#include "common.h"

#include <cmath>

namespace hlhgat {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kOneWG = 16384;  // up to here: one self-finishing workgroup
constexpr int64_t kPerWG = 4096;   // elements (rows) per workgroup beyond it
constexpr int kMaxWG = 256;
constexpr int64_t kMaxN = (int64_t)1 << 38;  // per-workgroup counts stay in int32

inline int loss_grid(int64_t n) {
  if (n <= kOneWG) return 1;
  const int64_t g = ceil_div(n, kPerWG);
  return (int)(g < kMaxWG ? g : kMaxWG);
}

struct Partial {  // one workgroup's sums (32 bytes)
  float s;
  int c[4];
  int pad[3];
};

struct LossMode {
  int red;  // HLHGAT_LOSS_*
  float alpha, gamma, scale;
};

// Fixed tree: the 64 lanes of a wave by halving, then the four waves in order.
// Every thread returns the workgroup's sum.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = (lds[0] + lds[1]) + (lds[2] + lds[3]);
  __syncthreads();
  return r;
}

// om^g for g >= 0 (the exponents the entries admit and g - 1 of them)
__device__ __forceinline__ float powg(float om, float g) {
  if (g == 0.f) return 1.f;
  if (g == 1.f) return om;
  if (g == 2.f) return om * om;
  return powf(om, g);
}

__device__ __forceinline__ float loss_value(float S, long long cnt, LossMode m) {
  if (cnt == 0) return 0.f;
  if (m.red == HLHGAT_LOSS_SUM) return S;
  const float b = S / (float)cnt;
  if (m.red == HLHGAT_LOSS_MEAN) return b;
  const float om = -expm1f(-b);  // 1 - pt, pt = exp(-b)
  return m.scale * m.alpha * powg(om, m.gamma) * b;
}

// d loss / d S
__device__ __forceinline__ float loss_coeff(float S, long long cnt, LossMode m) {
  if (cnt == 0) return 0.f;
  if (m.red == HLHGAT_LOSS_SUM) return 1.f;
  const float n = (float)cnt;
  if (m.red == HLHGAT_LOSS_MEAN) return 1.f / n;
  if (m.gamma == 0.f) return m.scale * m.alpha / n;
  const float b = S / n;
  const float pt = expf(-b), om = -expm1f(-b);
  return m.scale * m.alpha * (powg(om, m.gamma) + m.gamma * powg(om, m.gamma - 1.f) * pt * b) / n;
}

struct Results {
  float* loss;     // [1]
  float* sum;      // [1] S, for the backward (NULL: cross-entropy)
  int64_t* stats;  // [nstats]
  int nstats;
};

__device__ __forceinline__ void write_results(const Results& r, LossMode m, float S,
                                              const long long* c) {
  r.loss[0] = loss_value(S, c[0], m);
  if (r.sum) r.sum[0] = S;
  for (int i = 0; i < r.nstats; ++i) r.stats[i] = (int64_t)c[i];
}

// One workgroup: the partial records in index order, fixed tree.
__global__ __launch_bounds__(kThreads) void k_loss_finish(const Partial* __restrict__ part,
                                                          int nparts, LossMode m, Results r) {
  __shared__ float lf[4];
  __shared__ long long li[4];
  float s = 0.f;
  long long c[4] = {0, 0, 0, 0};
  if ((int)threadIdx.x < nparts) {
    const Partial p = part[threadIdx.x];
    s = p.s;
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = p.c[i];
  }
  s = block_sum(s, lf);
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = block_sum(c[i], li);
  if (threadIdx.x == 0) write_results(r, m, s, c);
}

// The end of a grid kernel: workgroup sums, then the record or (one workgroup)
// the results themselves.
__device__ __forceinline__ void wg_finish(float s, const int* cnt, Partial* part, LossMode m,
                                          const Results& r) {
  __shared__ float lf[4];
  __shared__ int li[4];
  s = block_sum(s, lf);
  int c[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) c[i] = block_sum(cnt[i], li);
  if (threadIdx.x != 0) return;
  if (gridDim.x == 1) {
    const long long cl[4] = {c[0], c[1], c[2], c[3]};
    write_results(r, m, s, cl);
  } else {
    Partial p{};
    p.s = s;
#pragma unroll
    for (int i = 0; i < 4; ++i) p.c[i] = c[i];
    part[blockIdx.x] = p;
  }
}

// --- (a) BCE with logits over an on-device selection -------------------------
struct BceArgs {
  const float* x;
  const float* y;
  const unsigned char* mask;  // NULL: all
  int64_t n;
  int64_t groups;  // ceil(n / 4)
  int ignore_nan;
  LossMode m;
};

__device__ __forceinline__ bool bce_included(bool mask, float y, int ignore_nan) {
  return mask && !(ignore_nan && y != y);
}

struct BceAcc {
  float s = 0.f;
  int c[4] = {0, 0, 0, 0};  // cnt, tp, fp, fn
};

__device__ __forceinline__ void bce_fwd_elem(BceAcc& a, float x, float y, bool mask,
                                             int ignore_nan) {
  const bool inc = bce_included(mask, y, ignore_nan);
  const float ls = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));  // log_sigmoid
  const float t = (1.f - y) * x - ls;
  a.s += inc ? t : 0.f;  // an excluded element's x and y never enter the sum
  const bool p = x > 0.f, l = y > 0.5f;
  a.c[0] += inc;
  a.c[1] += inc && p && l;
  a.c[2] += inc && p && !l;
  a.c[3] += inc && !p && l;
}

// Thread t of workgroup b takes the 4-element groups b * 256 + t + k * grid * 256,
// k = 0, 1, ...; VEC loads a whole group with one 16-byte load per operand.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_bce_reduce_fwd(BceArgs p, Partial* part,
                                                             Results r) {
  BceAcc a;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < p.groups; g += stride) {
    const int64_t e0 = g * 4;
    if (VEC && e0 + 4 <= p.n) {
      float4 xv = vload<4>(p.x + e0), yv = vload<4>(p.y + e0);
      const uint32_t mw =
          p.mask ? *reinterpret_cast<const uint32_t*>(p.mask + e0) : 0x01010101u;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        bce_fwd_elem(a, vget(xv, c), vget(yv, c), ((mw >> (8 * c)) & 0xffu) != 0u, p.ignore_nan);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t e = e0 + c;
        if (e >= p.n) break;
        bce_fwd_elem(a, p.x[e], p.y[e], p.mask ? p.mask[e] != 0 : true, p.ignore_nan);
      }
    }
  }
  wg_finish(a.s, a.c, part, p.m, r);
}

// sigmoid(x) - y in the arithmetic of k_bce_logits_bwd (runtime.hip)
__device__ __forceinline__ float bce_bwd_elem(float q, float x, float y, bool mask,
                                              int ignore_nan) {
  if (!bce_included(mask, y, ignore_nan)) return 0.f;
  const bool neg = x < 0.f;
  const float m = neg ? 1.f : 0.f, sg = neg ? 1.f : -1.f;
  const float z = expf(-fabsf(x));
  return q * ((1.f - y) - (m - sg * (z / (1.f + z))));
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_bce_reduce_bwd(BceArgs p,
                                                             const float* __restrict__ sum,
                                                             const int64_t* __restrict__ stats,
                                                             const float* __restrict__ gout,
                                                             float* __restrict__ dx) {
  const float q = gout[0] * loss_coeff(sum[0], (long long)stats[0], p.m);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x; g < p.groups; g += stride) {
    const int64_t e0 = g * 4;
    if (VEC && e0 + 4 <= p.n) {
      float4 xv = vload<4>(p.x + e0), yv = vload<4>(p.y + e0), d;
      const uint32_t mw =
          p.mask ? *reinterpret_cast<const uint32_t*>(p.mask + e0) : 0x01010101u;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        vget(d, c) = bce_bwd_elem(q, vget(xv, c), vget(yv, c), ((mw >> (8 * c)) & 0xffu) != 0u,
                                  p.ignore_nan);
      vstore<4>(dx + e0, d);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t e = e0 + c;
        if (e >= p.n) break;
        dx[e] = bce_bwd_elem(q, p.x[e], p.y[e], p.mask ? p.mask[e] != 0 : true, p.ignore_nan);
      }
    }
  }
}

// --- (b) cross-entropy over rows ----------------------------------------------
struct CeArgs {
  const float* x;
  int64_t ld;
  int64_t rows;
  int cols;
  const int64_t* label;
  int64_t ignore_index;
  LossMode m;
};

// 0: the row counts; 1: ignore_index; 2: a label outside [0, C) (ignored too)
__device__ __forceinline__ int ce_row_kind(int64_t lab, const CeArgs& p) {
  if (lab == p.ignore_index) return 1;
  return lab >= 0 && lab < p.cols ? 0 : 2;
}

// One thread per row: max (lowest index wins), sum of exp, the label's logit.
__global__ __launch_bounds__(kThreads) void k_cross_entropy_fwd(CeArgs p, Partial* part,
                                                                Results r, unsigned* err) {
  float s = 0.f;
  int c[4] = {0, 0, 0, 0};  // cnt, correct
  bool bad = false;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < p.rows; i += stride) {
    const int64_t lab = p.label[i];
    const int kind = ce_row_kind(lab, p);
    if (kind != 0) {
      bad = bad || kind == 2;
      continue;
    }
    const float* row = p.x + i * p.ld;
    float mx = row[0];
    int am = 0;
    for (int j = 1; j < p.cols; ++j) {
      const float v = row[j];
      if (v > mx) {
        mx = v;
        am = j;
      }
    }
    float se = 0.f;
    for (int j = 0; j < p.cols; ++j) se += expf(row[j] - mx);
    s += (logf(se) + mx) - row[lab];
    c[0] += 1;
    c[1] += am == (int)lab;
  }
  if (bad && err)
    __hip_atomic_store(err, (unsigned)HLHGAT_DEVERR_LABEL, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  wg_finish(s, c, part, p.m, r);
}

__global__ __launch_bounds__(kThreads) void k_cross_entropy_bwd(CeArgs p,
                                                                const int64_t* __restrict__ stats,
                                                                const float* __restrict__ gout,
                                                                float* __restrict__ dx,
                                                                int64_t lddx) {
  const long long cnt = (long long)stats[0];
  const float q = cnt == 0 ? 0.f
                           : (p.m.red == HLHGAT_LOSS_SUM ? gout[0] : gout[0] / (float)cnt);
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < p.rows; i += stride) {
    float* d = dx + i * lddx;
    const int64_t lab = p.label[i];
    if (ce_row_kind(lab, p) != 0) {
      for (int j = 0; j < p.cols; ++j) d[j] = 0.f;
      continue;
    }
    const float* row = p.x + i * p.ld;
    float mx = row[0];
    for (int j = 1; j < p.cols; ++j) mx = fmaxf(mx, row[j]);
    float se = 0.f;
    for (int j = 0; j < p.cols; ++j) se += expf(row[j] - mx);
    for (int j = 0; j < p.cols; ++j)
      d[j] = q * (expf(row[j] - mx) / se - (j == (int)lab ? 1.f : 0.f));
  }
}

bool gamma_ok(float g) { return g == 0.f || g >= 1.f; }  // false for NaN

// --- (c) mean squared error (torch.nn.MSELoss) ---------------------------------
// The regression loss of the brain notebook (OHBM_DEMO.ipynb: criterion =
// torch.nn.MSELoss(); its test() accumulates the same sum as `rmse +=`).  The
// conventions of the L1 and BCE-with-logits entries (runtime.hip): one launch
// each way, a device scalar upstream gradient, nothing returns to the host.
//   forward  loss = (sum_i (x_i - y_i)^2) / div  (div = n: "mean", 1: "sum");
//            one workgroup, thread t sums elements t, t + 256, ... in order,
//            then one LDS tree.
//   backward dx_i = (x_i - y_i) * (2 g / div).
// A NaN in x or y reaches the loss and its own dx element, as in torch.
__global__ __launch_bounds__(kThreads) void k_mse_loss_fwd(const float* __restrict__ x,
                                                           const float* __restrict__ y,
                                                           int64_t n, float div,
                                                           float* __restrict__ loss) {
  __shared__ float red[kThreads];
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < n; i += kThreads) {
    const float d = x[i] - y[i];
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / div;
}

__global__ __launch_bounds__(kThreads) void k_mse_loss_bwd(const float* __restrict__ x,
                                                           const float* __restrict__ y,
                                                           int64_t n, float div,
                                                           const float* __restrict__ gout,
                                                           float* __restrict__ dx) {
  const float q = (2.f * gout[0]) / div;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kThreads)
    dx[i] = (x[i] - y[i]) * q;
}

}  // namespace
}  // namespace hlhgat

using namespace hlhgat;

extern "C" size_t hlhgat_loss_workspace_bytes(int64_t n) {
  if (n <= 0) return 0;
  return (size_t)loss_grid(n) * sizeof(Partial);
}

extern "C" int hlhgat_bce_reduce_fwd(const float* x, const float* y, const unsigned char* mask,
                                     int64_t n, int ignore_nan, int reduction, float alpha,
                                     float gamma, float scale, void* workspace,
                                     size_t workspace_bytes, float* loss, float* sum,
                                     int64_t* stats, void* stream) {
  HLH_CHECK_ARG(n > 0 && n <= kMaxN, "bce_reduce_fwd: n = %lld outside [1, 2^38]", (long long)n);
  HLH_CHECK_ARG(x && y && loss && sum && stats, "bce_reduce_fwd: NULL pointer");
  HLH_CHECK_ARG(aligned8(stats), "bce_reduce_fwd: stats must be 8-byte aligned");
  HLH_CHECK_ARG(reduction == HLHGAT_LOSS_MEAN || reduction == HLHGAT_LOSS_SUM ||
                    reduction == HLHGAT_LOSS_FOCAL,
                "bce_reduce_fwd: unknown reduction %d", reduction);
  HLH_CHECK_ARG(reduction != HLHGAT_LOSS_FOCAL || gamma_ok(gamma),
                "bce_reduce_fwd: focal gamma = %g unsupported (0 or >= 1)", (double)gamma);
  const int grid = loss_grid(n);
  HLH_CHECK_ARG(grid == 1 || (workspace && aligned16(workspace) &&
                              workspace_bytes >= (size_t)grid * sizeof(Partial)),
                "bce_reduce_fwd: workspace NULL, misaligned or smaller than "
                "hlhgat_loss_workspace_bytes(n) = %zu", (size_t)grid * sizeof(Partial));
  BceArgs p{x, y, mask, n, ceil_div(n, 4), ignore_nan != 0, {reduction, alpha, gamma, scale}};
  Results r{loss, sum, stats, 4};
  Partial* part = static_cast<Partial*>(workspace);
  const bool vec = aligned16(x) && aligned16(y) && (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
  hipStream_t st = as_stream(stream);
  if (vec)
    launch(k_bce_reduce_fwd<true>, dim3((unsigned)grid), dim3(kThreads), 0, st, nullptr, p, part,
           r);
  else
    launch(k_bce_reduce_fwd<false>, dim3((unsigned)grid), dim3(kThreads), 0, st, nullptr, p, part,
           r);
  HLH_CHECK_LAUNCH();
  if (grid > 1) {
    launch(k_loss_finish, dim3(1), dim3(kThreads), 0, st, nullptr, (const Partial*)part, grid,
           p.m, r);
    HLH_CHECK_LAUNCH();
  }
  return HLHGAT_OK;
}

extern "C" int hlhgat_bce_reduce_bwd(const float* x, const float* y, const unsigned char* mask,
                                     int64_t n, int ignore_nan, int reduction, float alpha,
                                     float gamma, float scale, const float* sum,
                                     const int64_t* stats, const float* gout, float* dx,
                                     void* stream) {
  HLH_CHECK_ARG(n > 0 && n <= kMaxN, "bce_reduce_bwd: n = %lld outside [1, 2^38]", (long long)n);
  HLH_CHECK_ARG(x && y && sum && stats && gout && dx, "bce_reduce_bwd: NULL pointer");
  HLH_CHECK_ARG(aligned8(stats), "bce_reduce_bwd: stats must be 8-byte aligned");
  HLH_CHECK_ARG(reduction == HLHGAT_LOSS_MEAN || reduction == HLHGAT_LOSS_SUM ||
                    reduction == HLHGAT_LOSS_FOCAL,
                "bce_reduce_bwd: unknown reduction %d", reduction);
  HLH_CHECK_ARG(reduction != HLHGAT_LOSS_FOCAL || gamma_ok(gamma),
                "bce_reduce_bwd: focal gamma = %g unsupported (0 or >= 1)", (double)gamma);
  BceArgs p{x, y, mask, n, ceil_div(n, 4), ignore_nan != 0, {reduction, alpha, gamma, scale}};
  int64_t grid = ceil_div(p.groups, kThreads);
  if (grid > 2048) grid = 2048;
  const bool vec = aligned16(x) && aligned16(y) && aligned16(dx) &&
                   (reinterpret_cast<uintptr_t>(mask) & 3u) == 0;
  hipStream_t st = as_stream(stream);
  if (vec)
    launch(k_bce_reduce_bwd<true>, dim3((unsigned)grid), dim3(kThreads), 0, st, nullptr, p, sum,
           stats, gout, dx);
  else
    launch(k_bce_reduce_bwd<false>, dim3((unsigned)grid), dim3(kThreads), 0, st, nullptr, p, sum,
           stats, gout, dx);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

namespace {
int ce_check(const char* what, const float* x, int64_t ldx, int64_t rows, int64_t cols,
             const int64_t* label, int reduction, const int64_t* stats) {
  HLH_CHECK_ARG(rows > 0 && rows <= kMaxN, "%s: rows = %lld outside [1, 2^38]", what,
                (long long)rows);
  HLH_CHECK_ARG(cols >= 1 && cols <= HLHGAT_CE_MAX_CLASSES, "%s: C = %lld outside [1, %d]", what,
                (long long)cols, HLHGAT_CE_MAX_CLASSES);
  HLH_CHECK_ARG(ldx >= cols, "%s: ld = %lld < C = %lld", what, (long long)ldx, (long long)cols);
  HLH_CHECK_ARG(x && label && stats, "%s: NULL pointer", what);
  HLH_CHECK_ARG(aligned8(label) && aligned8(stats), "%s: label / stats must be 8-byte aligned",
                what);
  HLH_CHECK_ARG(reduction == HLHGAT_LOSS_MEAN || reduction == HLHGAT_LOSS_SUM,
                "%s: unknown reduction %d (mean or sum)", what, reduction);
  return HLHGAT_OK;
}
}  // namespace

extern "C" int hlhgat_cross_entropy_fwd(const float* x, int64_t ldx, int64_t rows, int64_t cols,
                                        const int64_t* label, int64_t ignore_index,
                                        int reduction, void* workspace, size_t workspace_bytes,
                                        float* loss, int64_t* stats, void* stream) {
  if (int rc = ce_check("cross_entropy_fwd", x, ldx, rows, cols, label, reduction, stats))
    return rc;
  HLH_CHECK_ARG(loss, "cross_entropy_fwd: NULL pointer");
  const int grid = loss_grid(rows);
  HLH_CHECK_ARG(grid == 1 || (workspace && aligned16(workspace) &&
                              workspace_bytes >= (size_t)grid * sizeof(Partial)),
                "cross_entropy_fwd: workspace NULL, misaligned or smaller than "
                "hlhgat_loss_workspace_bytes(rows) = %zu", (size_t)grid * sizeof(Partial));
  CeArgs p{x, ldx, rows, (int)cols, label, ignore_index, {reduction, 0.f, 0.f, 0.f}};
  Results r{loss, nullptr, stats, 2};
  Partial* part = static_cast<Partial*>(workspace);
  hipStream_t st = as_stream(stream);
  launch(k_cross_entropy_fwd, dim3((unsigned)grid), dim3(kThreads), 0, st, nullptr, p, part, r,
         device_error_word());
  HLH_CHECK_LAUNCH();
  if (grid > 1) {
    launch(k_loss_finish, dim3(1), dim3(kThreads), 0, st, nullptr, (const Partial*)part, grid,
           p.m, r);
    HLH_CHECK_LAUNCH();
  }
  return HLHGAT_OK;
}

extern "C" int hlhgat_cross_entropy_bwd(const float* x, int64_t ldx, int64_t rows, int64_t cols,
                                        const int64_t* label, int64_t ignore_index,
                                        int reduction, const int64_t* stats, const float* gout,
                                        float* dx, int64_t lddx, void* stream) {
  if (int rc = ce_check("cross_entropy_bwd", x, ldx, rows, cols, label, reduction, stats))
    return rc;
  HLH_CHECK_ARG(gout && dx, "cross_entropy_bwd: NULL pointer");
  HLH_CHECK_ARG(lddx >= cols, "cross_entropy_bwd: lddx = %lld < C = %lld", (long long)lddx,
                (long long)cols);
  CeArgs p{x, ldx, rows, (int)cols, label, ignore_index, {reduction, 0.f, 0.f, 0.f}};
  int64_t grid = ceil_div(rows, kThreads);
  if (grid > 2048) grid = 2048;
  launch(k_cross_entropy_bwd, dim3((unsigned)grid), dim3(kThreads), 0, as_stream(stream), nullptr,
         p, stats, gout, dx, lddx);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_mse_loss_fwd(const float* x, const float* y, int64_t n, float div,
                                   float* loss, void* stream) {
  HLH_CHECK_ARG(n > 0 && x && y && loss && div > 0.f,
                "mse_loss_fwd: NULL pointer, n <= 0 or div <= 0");
  launch(k_mse_loss_fwd, dim3(1), dim3(kThreads), 0, as_stream(stream), nullptr, x, y, n, div,
         loss);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_mse_loss_bwd(const float* x, const float* y, int64_t n, float div,
                                   const float* gout, float* dx, void* stream) {
  HLH_CHECK_ARG(n > 0 && x && y && gout && dx && div > 0.f,
                "mse_loss_bwd: NULL pointer, n <= 0 or div <= 0");
  int64_t g = ceil_div(n, kThreads);
  if (g > 1024) g = 1024;
  launch(k_mse_loss_bwd, dim3((unsigned)g), dim3(kThreads), 0, as_stream(stream), nullptr, x, y,
         n, div, gout, dx);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
