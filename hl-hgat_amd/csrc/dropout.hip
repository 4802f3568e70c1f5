// Training-mode feature dropout (the Dropout(p=dropout_ratio) that ends every
// HL block, lib/Hodge_ST_Model.py:556-566) with a counter-based mask: nothing
// is stored between the forward and the backward, and a captured step draws a
// fresh mask on every replay.
//
// Mask rule.  Element e = row * d + col (a LOGICAL index: it does not depend
// on any leading dimension) belongs to group g = e >> 2 and takes word e & 3 of
//
//   philox4x32-10(counter = {g & 0xffffffff, g >> 32, site, step & 0xffffffff},
//                 key     = {seed & 0xffffffff, seed >> 32})
//
// and is kept iff (word >> 8) >= T, T = floor(p * 2^24).  y = keep ? x * s : 0
// with s = float(1 / (1 - p)).  {seed, step} live in a two-word int64 device
// state that the kernel reads (so a graph replay sees the advanced step);
// `site` is a host-side call counter baked into the launch.  The forward
// copies the {seed, step} it used into `snap`, and the backward regenerates
// the mask from that snapshot.
//
// One Philox call per four consecutive elements; 16-byte accesses when every
// group lies inside one row and is aligned (d % 4 == 0, 16-byte aligned
// pointers and leading dimensions), a scalar path otherwise.  No atomics;
// plain vector stores only.
#include "common.h"
#include "philox.h"

namespace hlhgat {
namespace {

struct DropArgs {
  const float* src;  // fwd: x; bwd: dy
  int64_t lds;
  float* dst;  // fwd: y; bwd: dx
  int64_t ldd;
  int64_t d;
  int64_t total;           // n * d
  int64_t groups;          // ceil(total / 4)
  const int64_t* state;    // {seed, step}: the live state (fwd) or the snapshot (bwd)
  int64_t* snap;           // fwd: receives the {seed, step} used; bwd: NULL
  uint32_t T;
  uint32_t site;
  float s;
};

// VEC: every group is four consecutive columns of one row, 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void k_dropout(DropArgs p) {
  const uint64_t seed = (uint64_t)p.state[0];
  const uint32_t step = (uint32_t)(uint64_t)p.state[1];
  if (p.snap && blockIdx.x == 0 && threadIdx.x == 0) {
    p.snap[0] = p.state[0];
    p.snap[1] = p.state[1];
  }
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const bool small = p.total <= 0xffffffffll;  // 32-bit row / column arithmetic
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < p.groups; g += stride) {
    const Philox4 r = philox4x32_10((uint32_t)g, (uint32_t)((uint64_t)g >> 32), p.site, step,
                                    k0, k1);
    const int64_t e0 = g * 4;
    if constexpr (VEC) {
      int64_t row, col;
      if (small) {
        row = (uint32_t)e0 / (uint32_t)p.d;
        col = (uint32_t)e0 - (uint32_t)row * (uint32_t)p.d;
      } else {
        row = e0 / p.d;
        col = e0 - row * p.d;
      }
      float4 v = vload<4>(p.src + row * p.lds + col);
#pragma unroll
      for (int c = 0; c < 4; ++c)
        vget(v, c) = (r.w[c] >> 8) >= p.T ? vget(v, c) * p.s : 0.f;
      vstore<4>(p.dst + row * p.ldd + col, v);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int64_t e = e0 + c;
        if (e >= p.total) break;
        int64_t row, col;
        if (small) {
          row = (uint32_t)e / (uint32_t)p.d;
          col = (uint32_t)e - (uint32_t)row * (uint32_t)p.d;
        } else {
          row = e / p.d;
          col = e - row * p.d;
        }
        const float x = p.src[row * p.lds + col];
        p.dst[row * p.ldd + col] = (r.w[c] >> 8) >= p.T ? x * p.s : 0.f;
      }
    }
  }
}

__global__ void k_dropout_advance(int64_t* state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) state[1] = state[1] + 1;
}

// Workgroups for a grid-stride pass: 8 per CU of the current device (cached
// per device; no device query after the first call, so launches capture).
int grid_cap() {
  static int cap[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 2048;
  if (cap[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
      cus = 256;
    cap[dev] = cus * 8;
  }
  return cap[dev];
}

int run(const char* what, const float* src, int64_t lds, int64_t n, int64_t d, uint32_t T,
        float s, const int64_t* state, uint32_t site, int64_t* snap, bool need_snap, float* dst,
        int64_t ldd, void* stream) {
  HLH_CHECK_ARG(n >= 0 && d >= 0 && lds >= d && ldd >= d, "%s: bad sizes (n, d >= 0, ld >= d)",
                what);
  HLH_CHECK_ARG(T <= (1u << 24), "%s: T = %u exceeds 2^24", what, T);
  if (n == 0 || d == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(src && dst && state && (snap || !need_snap), "%s: NULL pointer", what);
  HLH_CHECK_ARG(aligned8(state) && (!snap || aligned8(snap)), "%s: state must be 8-byte aligned",
                what);
  HLH_CHECK_ARG(n <= INT64_MAX / 4 / d, "%s: n * d overflows", what);
  DropArgs p{};
  p.src = src;
  p.lds = lds;
  p.dst = dst;
  p.ldd = ldd;
  p.d = d;
  p.total = n * d;
  p.groups = ceil_div(p.total, 4);
  p.state = state;
  p.snap = need_snap ? snap : nullptr;
  p.T = T;
  p.site = site;
  p.s = s;
  const bool vec = d % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && aligned16(src) && aligned16(dst);
  int64_t blocks = ceil_div(p.groups, 256);
  const int cap = grid_cap();
  if (blocks > cap) blocks = cap;
  hipStream_t st = as_stream(stream);
  if (vec)
    launch(k_dropout<true>, dim3((unsigned)blocks), dim3(256), 0, st, nullptr, p);
  else
    launch(k_dropout<false>, dim3((unsigned)blocks), dim3(256), 0, st, nullptr, p);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

}  // namespace
}  // namespace hlhgat

using namespace hlhgat;

extern "C" int hlhgat_dropout_fwd(const float* x, int64_t ldx, int64_t n, int64_t d, uint32_t T,
                                  float s, const int64_t* state, uint32_t site, int64_t* snap,
                                  float* y, int64_t ldy, void* stream) {
  return run("dropout_fwd", x, ldx, n, d, T, s, state, site, snap, true, y, ldy, stream);
}

extern "C" int hlhgat_dropout_bwd(const float* dy, int64_t lddy, int64_t n, int64_t d, uint32_t T,
                                  float s, const int64_t* snap, uint32_t site, float* dx,
                                  int64_t lddx, void* stream) {
  return run("dropout_bwd", dy, lddy, n, d, T, s, snap, site, nullptr, false, dx, lddx, stream);
}

extern "C" int hlhgat_dropout_advance(int64_t* state, void* stream) {
  HLH_CHECK_ARG(state && aligned8(state), "dropout_advance: NULL or misaligned state");
  launch(k_dropout_advance, dim3(1), dim3(64), 0, as_stream(stream), nullptr, state);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
