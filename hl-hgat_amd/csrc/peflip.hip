// PE sign-flip augmentation: the per-sample, per-access sign draw on the
// eigenvector positional-encoding columns that every stored dataset of the
// reference applies in get() (lib/Hodge_Dataset.py:425-440 ZINC, :500-515,
// :554-569 and :635-650 peptides, :869-881 CIFAR10SP):
//
//   sign = cat([ones(n_fixed), -1 + 2 * randint(0, 2, (n_flip,))])
//   x    = x[:, :n_fixed + n_flip] * sign          (once for x_t, once for x_s)
//
// as one out-of-place pass over both sides of a batch.  The draw is
// counter-based like the feature dropout (dropout.hip) and the simplex dropout
// (simplex.hip): a function of (seed, step, site, graph, column), nothing
// stored between the forward and the backward, and a captured launch draws
// fresh signs on every replay because {seed, step} are read from device
// memory.  Graph g, flipped column j (0-based among the flipped columns):
//
//   w    = word (j & 3) of philox({g, 0x50450000 + (j >> 2), site, step lo},
//                                 {seed lo, seed hi})
//   sign = (w >> 31) ? -1.0f : +1.0f
//
// Counter disjointness.  The second counter word of every other draw of the
// library is the high half of a 4-element group index or 0: dropout.hip forms
// {g lo, g hi, site, step} with g = e >> 2 < 2^59 (run() bounds n * d by
// INT64_MAX / 4), so g hi < 2^27; simplex.hip forms {graph, 0, site, step} and
// {q lo, q hi, site + 1, step} with q = row >> 2 < 2^61, so q hi < 2^29.  Here
// it lies in [0x50450000, 0x50450000 + 2^14) (n_flip <= 2^16), above both
// ranges, so no counter of this file can equal one of theirs whatever the
// sites are.
//
// A group of kLanes lanes owns one row: the lanes share the row's graph lookup
// (a bisection over seg_ptr on the same addresses), copy the fixed columns
// lane-strided, and each lane then owns whole groups of four flipped columns:
// one Philox call per (row, group), its four words used.  Rows are 18 to 37
// floats at odd pitches, so accesses are dwords.  Multiplies by +-1 (the
// reference's `* sign`, -0.0 from zeros included); rows outside every graph
// (static-shape padding) are copied.  No atomics, no LDS; plain vector stores.
#include "common.h"
#include "philox.h"

namespace hlhgat {
namespace {

constexpr int kLanes = 8;             // lanes per row
constexpr int kRows = 256 / kLanes;   // rows per workgroup and pass
constexpr uint32_t kPeCounter = 0x50450000u;
constexpr int64_t kMaxWidth = 65536;  // n_fixed + n_flip
constexpr unsigned kMaxBlocks = 2048; // per side; grid-stride beyond

struct FlipSide {
  const float* x;
  int64_t ldx;
  float* y;
  int64_t ldy;
  const int32_t* seg_ptr;  // [G + 1]
  int G;
  int64_t n_rows;
  int n_fixed, n_flip;
  uint32_t site;
  unsigned blocks;  // workgroups of the grid that serve this side
};

struct FlipArgs {
  FlipSide side[2];
  const int64_t* state;  // {seed, step}: the live state, or a snapshot
  int64_t* snap;         // receives the {seed, step} used; NULL when snap == state
};

// The first g with seg_ptr[g + 1] > r, or -1 when r lies in no graph.
__device__ __forceinline__ int graph_of(const int32_t* seg_ptr, int G, int64_t r) {
  int lo = 0, hi = G;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)seg_ptr[mid + 1] > r)
      hi = mid;
    else
      lo = mid + 1;
  }
  return (lo < G && r >= (int64_t)seg_ptr[lo]) ? lo : -1;
}

// Workgroups [0, side[0].blocks) serve side 0, the rest side 1.
__global__ __launch_bounds__(256) void k_pe_flip(FlipArgs p) {
  const uint64_t seed = (uint64_t)p.state[0];
  const uint32_t step = (uint32_t)(uint64_t)p.state[1];
  if (p.snap && blockIdx.x == 0 && threadIdx.x == 0) {
    p.snap[0] = p.state[0];
    p.snap[1] = p.state[1];
  }
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const bool second = blockIdx.x >= p.side[0].blocks;
  const FlipSide a = second ? p.side[1] : p.side[0];
  const unsigned b = second ? blockIdx.x - p.side[0].blocks : blockIdx.x;
  const int sub = threadIdx.x % kLanes;
  const int64_t stride = (int64_t)a.blocks * kRows;
  for (int64_t r = (int64_t)b * kRows + threadIdx.x / kLanes; r < a.n_rows; r += stride) {
    const float* xr = a.x + r * a.ldx;
    float* yr = a.y + r * a.ldy;
    for (int c = sub; c < a.n_fixed; c += kLanes) yr[c] = xr[c];
    if (a.n_flip == 0) continue;
    const int g = graph_of(a.seg_ptr, a.G, r);
    xr += a.n_fixed;
    yr += a.n_fixed;
    for (int q = sub; q * 4 < a.n_flip; q += kLanes) {
      Philox4 w = {{0u, 0u, 0u, 0u}};
      if (g >= 0) w = philox4x32_10((uint32_t)g, kPeCounter + (uint32_t)q, a.site, step, k0, k1);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int j = q * 4 + c;
        if (j >= a.n_flip) break;
        const float v = xr[j];
        yr[j] = g >= 0 ? v * ((w.w[c] >> 31) ? -1.0f : 1.0f) : v;
      }
    }
  }
}

struct SignArgs {
  float* signs;  // [G, n_flip]
  int64_t G;
  int n_flip;
  int groups;  // ceil(n_flip / 4)
  const int64_t* state;
  uint32_t site;
};

// One thread per (graph, group of four columns).
__global__ __launch_bounds__(256) void k_pe_signs(SignArgs p) {
  const uint64_t seed = (uint64_t)p.state[0];
  const uint32_t step = (uint32_t)(uint64_t)p.state[1];
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const int64_t total = p.G * p.groups;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t g = i / p.groups;
    const int q = (int)(i - g * p.groups);
    const Philox4 w = philox4x32_10((uint32_t)g, kPeCounter + (uint32_t)q, p.site, step, k0, k1);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = q * 4 + c;
      if (j >= p.n_flip) break;
      p.signs[g * p.n_flip + j] = (w.w[c] >> 31) ? -1.0f : 1.0f;
    }
  }
}

}  // namespace
}  // namespace hlhgat

using namespace hlhgat;

extern "C" int hlhgat_pe_flip(const hlhgat_pe_side_t* sides, int n_sides, const int64_t* state,
                              int64_t* snap, void* stream) {
  HLH_CHECK_ARG(n_sides == 1 || n_sides == 2, "pe_flip: n_sides = %d (1 or 2)", n_sides);
  HLH_CHECK_ARG(sides, "pe_flip: NULL pointer (sides)");
  FlipArgs p{};
  unsigned total = 0;
  for (int i = 0; i < n_sides; ++i) {
    const hlhgat_pe_side_t& s = sides[i];
    const int64_t width = (int64_t)s.n_fixed + (int64_t)s.n_flip;
    HLH_CHECK_ARG(s.n_rows >= 0 && s.n_graphs >= 0 && s.n_graphs < INT32_MAX && s.n_fixed >= 0 &&
                      s.n_flip >= 0 && width <= kMaxWidth,
                  "pe_flip: bad sizes (n_rows, n_graphs, n_fixed, n_flip >= 0, n_fixed + n_flip "
                  "<= 65536) on side %d", i);
    HLH_CHECK_ARG(s.ldx >= width && s.ldy >= width,
                  "pe_flip: bad leading dimension (ld >= n_fixed + n_flip) on side %d", i);
    HLH_CHECK_ARG(s.site < (1u << 30), "pe_flip: site 0x%x out of range (< 2^30) on side %d",
                  s.site, i);
    FlipSide& a = p.side[i];
    if (s.n_rows == 0 || width == 0) continue;  // blocks = 0: nothing to move
    HLH_CHECK_ARG(s.x && s.y && (s.seg_ptr || s.n_graphs == 0 || s.n_flip == 0),
                  "pe_flip: NULL pointer on side %d", i);
    HLH_CHECK_ARG(s.x != s.y, "pe_flip: x and y alias on side %d (out of place only)", i);
    a.x = s.x;
    a.ldx = s.ldx;
    a.y = s.y;
    a.ldy = s.ldy;
    a.seg_ptr = s.seg_ptr;
    a.G = (int)s.n_graphs;
    a.n_rows = s.n_rows;
    a.n_fixed = s.n_fixed;
    a.n_flip = s.n_flip;
    a.site = s.site;
    const int64_t blocks = ceil_div(s.n_rows, kRows);
    a.blocks = blocks > (int64_t)kMaxBlocks ? kMaxBlocks : (unsigned)blocks;
    total += a.blocks;
  }
  if (total == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(state && snap, "pe_flip: NULL pointer (state, snap)");
  HLH_CHECK_ARG(aligned8(state) && aligned8(snap), "pe_flip: state must be 8-byte aligned");
  p.state = state;
  p.snap = snap == state ? nullptr : snap;
  launch(k_pe_flip, dim3(total), dim3(256), 0, as_stream(stream), nullptr, p);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}

extern "C" int hlhgat_pe_signs(int64_t n_graphs, int64_t n_flip, uint32_t site,
                               const int64_t* state, float* signs, void* stream) {
  HLH_CHECK_ARG(n_graphs >= 0 && n_graphs < INT32_MAX && n_flip >= 0 && n_flip <= kMaxWidth,
                "pe_signs: bad sizes (n_graphs >= 0, 0 <= n_flip <= 65536)");
  HLH_CHECK_ARG(site < (1u << 30), "pe_signs: site 0x%x out of range (< 2^30)", site);
  if (n_graphs == 0 || n_flip == 0) return HLHGAT_OK;
  HLH_CHECK_ARG(state && signs, "pe_signs: NULL pointer");
  HLH_CHECK_ARG(aligned8(state), "pe_signs: state must be 8-byte aligned");
  SignArgs p{};
  p.signs = signs;
  p.G = n_graphs;
  p.n_flip = (int)n_flip;
  p.groups = (int)ceil_div(n_flip, 4);
  p.state = state;
  p.site = site;
  int64_t blocks = ceil_div(n_graphs * p.groups, 256);
  if (blocks > (int64_t)kMaxBlocks) blocks = kMaxBlocks;
  launch(k_pe_signs, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), nullptr, p);
  HLH_CHECK_LAUNCH();
  return HLHGAT_OK;
}
