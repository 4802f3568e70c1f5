// Evaluation metrics on the device (include/hlhgat.h, "evaluation metrics").
//
// hlhgat_average_precision: the per-class average precision of the
// reference's eval_ap (scikit-learn's average_precision_score over the rows
// whose label is not NaN).
//   k_ap_keys   one 64-bit key and one byte per (row, class):
//                 key  = class << 33 | unlabelled << 32 | ~image(score)
//                 byte = 1 (label == 1), 2 (label == 0), 0 (anything else)
//               image() is the order-preserving unsigned image of the fp32
//               score with the sign of zero removed, complemented so that an
//               ascending sort puts the highest score first; the unlabelled
//               bit sends NaN-label rows behind the class's labelled rows.
//   hipcub::DeviceRadixSort::SortPairs over the 33 + bits(C - 1) key bits.
//               Every class owns exactly n consecutive sorted items; rows with equal
//               keys are one threshold group, so their order is immaterial.
//   k_ap_walk   one workgroup per class: a counting pass (labelled, positives,
//               zeros, non-finite scores), then 256 rows at a time a block
//               scan of the positives (tp) and a block max-scan of tp at
//               group ends (tp of the previous group), carried across chunks.
//               Each thread adds the fp64 terms of its rows in row order; one
//               fixed LDS tree sums the 256 partial sums.  No atomics.
//
// The meters of the other test() loops (hlhgat.metrics), each one launch:
//   k_collect_rows        append rows at a device-side cursor, then advance it
//   k_f1_per_graph        BinaryF1Score of every graph of a batch
//   k_argmax_correct      the argmax(out, 1) == y count
//   k_regression_summary  sums, means, deviations and correlation, in fp64
// Integer counts or a fixed summation order, no atomics, no synchronisation.
#include "common.h"

#include <hipcub/hipcub.hpp>

#include <map>
#include <mutex>
#include <utility>

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t score_image_desc(float s) {
  uint32_t u = __float_as_uint(s);
  if ((u << 1) == 0u) u = 0u;  // -0.0 == +0.0
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

// the bits of the score behind a key's low word (zero's sign is gone)
__device__ __forceinline__ uint32_t score_bits_of(uint32_t low) {
  const uint32_t asc = ~low;
  return (asc & 0x80000000u) ? (asc & 0x7fffffffu) : ~asc;
}

__global__ __launch_bounds__(kThreads) void k_ap_keys(const float* __restrict__ pred, int64_t ldp,
                                                      const float* __restrict__ label,
                                                      int64_t ldl, int64_t n, int64_t C,
                                                      uint64_t* __restrict__ keys,
                                                      unsigned char* __restrict__ vals,
                                                      unsigned* err) {
  const int64_t total = n * C;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * kThreads) {
    const int64_t i = e / C, c = e - i * C;
    const float y = label[i * ldl + c];
    const float s = pred[i * ldp + c];
    const bool unl = y != y;
    unsigned char v = 0;
    if (y == 1.0f) v = 1;
    else if (y == 0.0f) v = 2;
    else if (!unl) bad = true;
    keys[e] = ((uint64_t)c << 33) | ((uint64_t)(unl ? 1u : 0u) << 32) | score_image_desc(s);
    vals[e] = v;
  }
  if (bad && err) {
    // the word is host memory without PCIe atomics: a load and a store keep
    // the bits other kernels raised before (a reporter racing with this one
    // may still overwrite it; any nonzero value means "do not use")
    const unsigned old = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(err, old | (unsigned)HLHGAT_DEVERR_METRIC_LABEL, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

struct OpAdd {
  __device__ __forceinline__ int operator()(int a, int b) const { return a + b; }
};
struct OpMax {
  __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; }
};

// Inclusive scan of v over the 256 threads of the block (identity 0, values
// >= 0); *total = the scan of all 256.  sh holds kWaves ints; two barriers.
template <class Op>
__device__ __forceinline__ int block_scan_incl(int v, Op op, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v = op(v, o);
  }
  __syncthreads();  // sh free again (the previous scan's readers are done)
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  int pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int t = sh[w];
    if (w < wave) pre = op(pre, t);
    tot = op(tot, t);
  }
  *total = tot;
  return op(pre, v);
}

__global__ __launch_bounds__(kThreads) void k_ap_walk(const uint64_t* __restrict__ keys,
                                                      const unsigned char* __restrict__ vals,
                                                      int64_t n, double* __restrict__ ap,
                                                      int32_t* __restrict__ counts) {
  __shared__ int sh_scan[kWaves];
  __shared__ int sh_cnt[4][kThreads];
  __shared__ double sh_sum[kThreads];
  const int tid = threadIdx.x;
  const int64_t c = blockIdx.x;
  const uint64_t* k = keys + c * n;
  const unsigned char* v = vals + c * n;

  // pass 1: the class's counts (integers: any order gives the same result)
  int lab = 0, pos = 0, zer = 0, nonfin = 0;
  for (int64_t j = tid; j < n; j += kThreads) {
    const uint64_t key = k[j];
    if ((key >> 32) & 1u) continue;
    const unsigned char b = v[j];
    lab += 1;
    pos += b == 1;
    zer += b == 2;
    nonfin += (score_bits_of((uint32_t)key) & 0x7f800000u) == 0x7f800000u;
  }
  sh_cnt[0][tid] = lab;
  sh_cnt[1][tid] = pos;
  sh_cnt[2][tid] = zer;
  sh_cnt[3][tid] = nonfin;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sh_cnt[q][tid] += sh_cnt[q][tid + w];
    }
    __syncthreads();
  }
  const int64_t m = sh_cnt[0][0];
  const int P = sh_cnt[1][0];
  const int Z = sh_cnt[2][0];
  const bool valid = P > 0 && Z > 0 && sh_cnt[3][0] == 0;
  if (tid == 0) {
    counts[3 * c + 0] = (int32_t)m;
    counts[3 * c + 1] = P;
    counts[3 * c + 2] = Z;
  }
  if (!valid) {  // uniform over the block
    if (tid == 0) ap[c] = __longlong_as_double(0x7ff8000000000000LL);
    return;
  }

  // pass 2: the labelled rows are the first m of the segment
  const double dP = (double)P;
  double acc = 0.0;
  int carry_tp = 0, carry_prev = 0;
  for (int64_t base = 0; base < m; base += kThreads) {
    const int64_t j = base + tid;
    const bool in = j < m;
    uint64_t key = 0, next = 1;
    int p = 0;
    if (in) {
      key = k[j];
      next = (j + 1 < m) ? k[j + 1] : ~key;
      p = v[j] == 1;
    }
    int chunk_tp, chunk_end;
    const int tp = carry_tp + block_scan_incl(p, OpAdd(), sh_scan, &chunk_tp);
    const bool end = in && next != key;
    const int e = end ? tp : 0;
    const int incl = block_scan_incl(e, OpMax(), sh_scan, &chunk_end);
    // tp is non-decreasing, so the largest group-end tp before this row is the
    // previous group's; an end row's own e is >= every earlier one
    int prev = __shfl_up(incl, 1, 64);
    if ((tid & 63) == 0) {
      prev = 0;
      for (int w = 0; w < (tid >> 6); ++w) prev = sh_scan[w] > prev ? sh_scan[w] : prev;
    }
    if (carry_prev > prev) prev = carry_prev;
    if (end && tp > prev)
      acc += ((double)(tp - prev) / dP) * ((double)tp / (double)(j + 1));
    carry_tp += chunk_tp;
    if (chunk_end > carry_prev) carry_prev = chunk_end;
  }
  sh_sum[tid] = acc;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (tid < w) sh_sum[tid] = sh_sum[tid] + sh_sum[tid + w];
    __syncthreads();
  }
  if (tid == 0) ap[c] = sh_sum[0];
}

// Raise `bit` in the device error word: a load and a store (k_ap_keys).
__device__ __forceinline__ void raise_error(unsigned* err, unsigned bit) {
  if (!err) return;
  const unsigned old = __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(err, old | bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Sum of v over the 256 threads of the block, in every thread (integers: any
// order gives the same result).  sh holds kWaves ints; two barriers.
__device__ __forceinline__ int block_sum_int(int v, int* sh) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  __syncthreads();  // sh free again
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) t += sh[w];
  return t;
}

// ---- collect_rows -----------------------------------------------------------
// One workgroup: the appends of an evaluation loop are a batch's outputs (a few
// thousand floats at most), and one workgroup can advance the cursor after its
// own copy behind a barrier, with no protocol between workgroups.
__global__ __launch_bounds__(kThreads) void k_collect_rows(const float* __restrict__ x,
                                                           int64_t ldx, int64_t n, int64_t d,
                                                           float* __restrict__ buf,
                                                           int64_t capacity, int64_t* cursor,
                                                           unsigned* err) {
  const int64_t cur = *cursor;  // every thread reads it before thread 0 may write it
  const bool fits = cur >= 0 && cur <= capacity && n <= capacity - cur;
  if (fits) {
    float* dst = buf + cur * d;
    const int64_t total = n * d;
    if (d == 1) {
      for (int64_t e = threadIdx.x; e < total; e += kThreads) dst[e] = x[e * ldx];
    } else {
      for (int64_t e = threadIdx.x; e < total; e += kThreads) {
        const int64_t r = e / d;
        dst[e] = x[r * ldx + (e - r * d)];
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (fits) *cursor = cur + n;
    else raise_error(err, (unsigned)HLHGAT_DEVERR_METER_FULL);
  }
}

// ---- f1_per_graph -----------------------------------------------------------
// One workgroup per graph, one pass over its rows: the counts under both
// formatting rules (raw threshold, sigmoid threshold) and the number of logits
// outside [0, 1], which picks the rule once the block knows it.
__global__ __launch_bounds__(kThreads) void k_f1_per_graph(const float* __restrict__ logit,
                                                           int64_t ldp,
                                                           const float* __restrict__ label,
                                                           int64_t ldy,
                                                           const int32_t* __restrict__ seg_ptr,
                                                           int64_t rows, float* __restrict__ f1,
                                                           unsigned* err) {
  __shared__ int sh[kWaves];
  const int g = blockIdx.x;
  int64_t lo = seg_ptr[g], hi = seg_ptr[g + 1];
  if (lo < 0) lo = 0;
  if (hi > rows) hi = rows;  // never past the tensors, whatever seg_ptr holds
  int outside = 0, pos = 0, tp_raw = 0, pp_raw = 0, tp_sig = 0, pp_sig = 0;
  bool bad = false;
  for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
    const float p = logit[i * ldp];
    const float y = label[i * ldy];
    const bool is_pos = y == 1.0f;
    if (!is_pos && !(y == 0.0f)) bad = true;
    outside += !(0.0f <= p && p <= 1.0f);  // a NaN is outside
    const bool raw = p > 0.5f;
    const bool sig = __fdiv_rn(1.0f, 1.0f + expf(-p)) > 0.5f;
    pos += is_pos;
    pp_raw += raw;
    tp_raw += raw && is_pos;
    pp_sig += sig;
    tp_sig += sig && is_pos;
  }
  outside = block_sum_int(outside, sh);
  pos = block_sum_int(pos, sh);
  const int tp = block_sum_int(outside ? tp_sig : tp_raw, sh);  // outside: block-uniform
  const int pp = block_sum_int(outside ? pp_sig : pp_raw, sh);
  if (bad) raise_error(err, (unsigned)HLHGAT_DEVERR_METRIC_LABEL);
  if (threadIdx.x == 0) {
    // 2tp + fp + fn with fp = pp - tp, fn = pos - tp
    const int64_t den = (int64_t)pp + (int64_t)pos;
    f1[g] = den > 0 ? __fdiv_rn((float)(2 * (int64_t)tp), (float)den) : 0.0f;
  }
}

// ---- argmax_correct ---------------------------------------------------------
// One workgroup, one thread per row (the batch's graphs: a few hundred rows).
__global__ __launch_bounds__(kThreads) void k_argmax_correct(const float* __restrict__ x,
                                                             int64_t ldx, int64_t n, int64_t C,
                                                             const int64_t* __restrict__ label,
                                                             int64_t* correct, int64_t* seen,
                                                             unsigned* err) {
  __shared__ int sh[kWaves];
  int hit = 0;
  bool bad = false;
  for (int64_t r = threadIdx.x; r < n; r += kThreads) {
    const float* row = x + r * ldx;
    float best = row[0];
    int64_t arg = 0;
    // torch's CPU rule: the first index of the greatest value, NaN greatest
    for (int64_t j = 1; j < C && best == best; ++j) {
      const float v = row[j];
      if (v > best || v != v) {
        best = v;
        arg = j;
      }
    }
    const int64_t y = label[r];
    if (y < 0 || y >= C) bad = true;
    hit += y == arg;
  }
  hit = block_sum_int(hit, sh);
  if (bad) raise_error(err, (unsigned)HLHGAT_DEVERR_METRIC_LABEL);
  if (threadIdx.x == 0) {
    *correct += hit;
    if (seen) *seen += n;
  }
}

// ---- regression_summary -----------------------------------------------------
constexpr int kSumThreads = 1024;

// Sums of v[0..3] over the block in one fixed tree; the result in every thread.
__device__ __forceinline__ void block_sum4(double (&v)[4], double (*sh)[kSumThreads]) {
  const int tid = threadIdx.x;
  __syncthreads();  // sh free again
#pragma unroll
  for (int q = 0; q < 4; ++q) sh[q][tid] = v[q];
  __syncthreads();
  for (int w = kSumThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sh[q][tid] = sh[q][tid] + sh[q][tid + w];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = sh[q][0];
}

// One workgroup, two passes in fp64: N is a dataset's size (1e4 - 1e5 values,
// 100 per thread), so the launch is latency-bound either way and a single
// workgroup keeps the summation order a function of N alone.
__global__ __launch_bounds__(kSumThreads) void k_regression_summary(
    const float* __restrict__ pred, const float* __restrict__ y, const int64_t* __restrict__ count,
    int64_t capacity, double* __restrict__ out) {
  __shared__ double sh[4][kSumThreads];
  const int tid = threadIdx.x;
  int64_t N = *count;
  if (N < 0) N = 0;
  if (N > capacity) N = capacity;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double dn = (double)N;
  double s1[4] = {0.0, 0.0, 0.0, 0.0};  // sum p, sum y, sum |d|, sum d^2
  for (int64_t i = tid; i < N; i += kSumThreads) {
    const double p = (double)pred[i], t = (double)y[i];
    const double d = p - t;
    s1[0] += p;
    s1[1] += t;
    s1[2] += fabs(d);
    s1[3] += d * d;
  }
  block_sum4(s1, sh);
  const double mp = N > 0 ? s1[0] / dn : nan, my = N > 0 ? s1[1] / dn : nan;
  double s2[4] = {0.0, 0.0, 0.0, 0.0};  // centred: sum a^2, sum b^2, sum a b, unused
  for (int64_t i = tid; i < N; i += kSumThreads) {
    const double a = (double)pred[i] - mp, b = (double)y[i] - my;
    s2[0] += a * a;
    s2[1] += b * b;
    s2[2] += a * b;
  }
  block_sum4(s2, sh);
  if (tid == 0) {
    const double sdp = N > 1 ? sqrt(s2[0] / (dn - 1.0)) : nan;
    const double sdy = N > 1 ? sqrt(s2[1] / (dn - 1.0)) : nan;
    out[0] = dn;
    out[1] = s1[2];
    out[2] = s1[3];
    out[3] = mp;
    out[4] = my;
    out[5] = sdp;
    out[6] = sdy;
    out[7] = N > 1 ? s2[2] / (dn * (sdp * sdy)) : nan;  // a zero deviation: 0 / 0
  }
}

int bits_of(uint64_t v) {  // bits needed to represent the value v (at least 1)
  int b = 1;
  while (b < 64 && (v >> b) > 0) ++b;
  return b;
}

// sorted key bits: 32 of the score, the unlabelled bit, the class index (< C)
inline int key_bits(int64_t C) { return 33 + bits_of((uint64_t)(C > 0 ? C - 1 : 0)); }

inline size_t align_up(size_t v) { return (v + 255) & ~size_t(255); }

// hipcub's temporary bytes for `items` pairs over `bits` key bits: a host-side
// query, made once per (items, bits)
size_t cub_temp_bytes(int64_t items, int bits) {
  static std::mutex mu;
  static std::map<std::pair<int64_t, int>, size_t> known;
  std::lock_guard<std::mutex> lk(mu);
  auto it = known.find({items, bits});
  if (it != known.end()) return it->second;
  size_t t = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, t, (uint64_t*)nullptr, (uint64_t*)nullptr,
                                           (unsigned char*)nullptr, (unsigned char*)nullptr,
                                           (int)items, 0, bits);
  if (known.size() >= 64) known.clear();
  known[{items, bits}] = t;
  return t;
}

// workspace layout as byte offsets: keys in / out, values in / out, hipcub temp
struct ApLayout {
  size_t keys_in, keys_out, vals_in, vals_out, temp, temp_bytes, total;
};

ApLayout layout(int64_t items, int64_t C) {
  const size_t t = (size_t)(items > 0 ? items : 1);
  ApLayout l;
  l.keys_in = 0;
  l.keys_out = l.keys_in + align_up(t * 8);
  l.vals_in = l.keys_out + align_up(t * 8);
  l.vals_out = l.vals_in + align_up(t);
  l.temp = l.vals_out + align_up(t);
  l.temp_bytes = align_up(cub_temp_bytes((int64_t)t, key_bits(C)));
  l.total = l.temp + l.temp_bytes;
  return l;
}

inline bool items_ok(int64_t n, int64_t C) {
  return n >= 0 && C >= 0 && (C == 0 || n < (int64_t)INT32_MAX / C);
}

}  // namespace

using namespace hlhgat;

extern "C" size_t hlhgat_average_precision_workspace_bytes(int64_t n, int64_t C) {
  if (!items_ok(n, C)) return 0;
  return layout(n * C, C).total;
}

extern "C" int hlhgat_average_precision(const float* pred, int64_t ldp, const float* label,
                                        int64_t ldl, int64_t n, int64_t C, double* ap,
                                        int32_t* counts, void* workspace, size_t workspace_bytes,
                                        void* stream) {
  HLH_CHECK_ARG(n >= 0 && C >= 0, "average_precision: n=%lld or C=%lld < 0", (long long)n,
                (long long)C);
  HLH_CHECK_ARG(items_ok(n, C), "average_precision: n * C = %lld * %lld out of int32 range",
                (long long)n, (long long)C);
  if (C == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(ap && counts, "average_precision: NULL output pointer");
  HLH_CHECK_ARG(aligned8(ap), "average_precision: ap must be 8-byte aligned");
  hipStream_t s = as_stream(stream);
  const int64_t items = n * C;
  if (items == 0) {  // n == 0: every class is empty (invalid); the walk reads nothing
    launch(k_ap_walk, dim3((unsigned)C), dim3(kThreads), 0, s, nullptr, (const uint64_t*)nullptr,
           (const unsigned char*)nullptr, n, ap, counts);
    HLH_CHECK_LAUNCH();
    return HLHGAT_OK;
  }
  HLH_CHECK_ARG(pred && label, "average_precision: NULL input pointer");
  HLH_CHECK_ARG(ldp >= C && ldl >= C, "average_precision: row stride below C");
  HLH_CHECK_ARG(workspace, "average_precision: NULL workspace");
  HLH_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                "average_precision: workspace must be 256-byte aligned");
  const ApLayout l = layout(items, C);
  HLH_CHECK_ARG(workspace_bytes >= l.total, "average_precision: workspace too small (%zu < %zu)",
                workspace_bytes, l.total);
  unsigned* err = device_error_word();
  HLH_CHECK_ARG(err, "average_precision: %s", hlhgat_last_error());
  char* w = static_cast<char*>(workspace);
  uint64_t* keys_in = reinterpret_cast<uint64_t*>(w + l.keys_in);
  uint64_t* keys_out = reinterpret_cast<uint64_t*>(w + l.keys_out);
  unsigned char* vals_in = reinterpret_cast<unsigned char*>(w + l.vals_in);
  unsigned char* vals_out = reinterpret_cast<unsigned char*>(w + l.vals_out);
  int64_t g = ceil_div(items, kThreads);
  if (g > 2048) g = 2048;
  launch(k_ap_keys, dim3((unsigned)g), dim3(kThreads), 0, s, nullptr, pred, ldp, label, ldl, n, C,
         keys_in, vals_in, err);
  HLH_CHECK_LAUNCH();
  size_t temp = l.temp_bytes;
  HLH_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(w + l.temp, temp, keys_in, keys_out, vals_in,
                                                   vals_out, (int)items, 0, key_bits(C), s));
  launch(k_ap_walk, dim3((unsigned)C), dim3(kThreads), 0, s, nullptr, (const uint64_t*)keys_out,
         (const unsigned char*)vals_out, n, ap, counts);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_collect_rows(const float* x, int64_t ldx, int64_t n, int64_t d, float* buf,
                                   int64_t capacity, int64_t* cursor, void* stream) {
  HLH_CHECK_ARG(n >= 0 && capacity >= 0, "collect_rows: n=%lld or capacity=%lld < 0",
                (long long)n, (long long)capacity);
  HLH_CHECK_ARG(d > 0, "collect_rows: d=%lld must be positive", (long long)d);
  if (n == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(x && buf && cursor, "collect_rows: NULL pointer");
  HLH_CHECK_ARG(ldx >= d || n == 1, "collect_rows: row stride %lld below d=%lld", (long long)ldx,
                (long long)d);
  HLH_CHECK_ARG(n <= INT64_MAX / d && capacity <= INT64_MAX / d / 4,
                "collect_rows: n * d or capacity * d out of range");
  HLH_CHECK_ARG(aligned8(cursor), "collect_rows: cursor must be 8-byte aligned");
  unsigned* err = device_error_word();
  HLH_CHECK_ARG(err, "collect_rows: %s", hlhgat_last_error());
  launch(k_collect_rows, dim3(1), dim3(kThreads), 0, as_stream(stream), nullptr, x, ldx, n, d, buf,
         capacity, cursor, err);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_f1_per_graph(const float* logit, int64_t ldp, const float* label,
                                   int64_t ldy, const int32_t* seg_ptr, int64_t n_graphs,
                                   int64_t rows, float* f1, void* stream) {
  HLH_CHECK_ARG(n_graphs >= 0 && rows >= 0, "f1_per_graph: n_graphs=%lld or rows=%lld < 0",
                (long long)n_graphs, (long long)rows);
  HLH_CHECK_ARG(n_graphs < INT32_MAX && rows <= INT32_MAX,
                "f1_per_graph: n_graphs or rows out of int32 range");
  if (n_graphs == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(seg_ptr && f1, "f1_per_graph: NULL seg_ptr or output pointer");
  HLH_CHECK_ARG(rows == 0 || (logit && label), "f1_per_graph: NULL input pointer");
  HLH_CHECK_ARG(ldp >= 1 && ldy >= 1, "f1_per_graph: stride below 1");
  unsigned* err = device_error_word();
  HLH_CHECK_ARG(err, "f1_per_graph: %s", hlhgat_last_error());
  launch(k_f1_per_graph, dim3((unsigned)n_graphs), dim3(kThreads), 0, as_stream(stream), nullptr,
         logit, ldp, label, ldy, seg_ptr, rows, f1, err);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_argmax_correct(const float* x, int64_t ldx, int64_t n, int64_t C,
                                     const int64_t* label, int64_t* correct, int64_t* seen,
                                     void* stream) {
  HLH_CHECK_ARG(n >= 0, "argmax_correct: n=%lld < 0", (long long)n);
  HLH_CHECK_ARG(C > 0, "argmax_correct: C=%lld must be positive", (long long)C);
  if (n == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(x && label && correct, "argmax_correct: NULL pointer");
  HLH_CHECK_ARG(ldx >= C || n == 1, "argmax_correct: row stride %lld below C=%lld",
                (long long)ldx, (long long)C);
  HLH_CHECK_ARG(n <= INT32_MAX, "argmax_correct: n out of int32 range");
  HLH_CHECK_ARG(aligned8(correct) && aligned8(seen) && aligned8(label),
                "argmax_correct: int64 pointers must be 8-byte aligned");
  unsigned* err = device_error_word();
  HLH_CHECK_ARG(err, "argmax_correct: %s", hlhgat_last_error());
  launch(k_argmax_correct, dim3(1), dim3(kThreads), 0, as_stream(stream), nullptr, x, ldx, n, C,
         label, correct, seen, err);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_regression_summary(const float* pred, const float* y, const int64_t* count,
                                         int64_t capacity, double* out, void* stream) {
  HLH_CHECK_ARG(capacity >= 0, "regression_summary: capacity=%lld < 0", (long long)capacity);
  HLH_CHECK_ARG(count && out, "regression_summary: NULL count or output pointer");
  HLH_CHECK_ARG(capacity == 0 || (pred && y), "regression_summary: NULL input pointer");
  HLH_CHECK_ARG(aligned8(count) && aligned8(out),
                "regression_summary: count and out must be 8-byte aligned");
  launch(k_regression_summary, dim3(1), dim3(kSumThreads), 0, as_stream(stream), nullptr, pred, y,
         count, capacity, out);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
