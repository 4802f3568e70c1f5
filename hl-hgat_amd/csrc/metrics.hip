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
