// Argument blocks of the projection gradients, shared by the fp32 kernels
// (proj.hip) and the bf16-operand kernels (proj_bf16.hip).  Like FwdArgs in
// gemm_core.h they have internal linkage: each including file gets its own,
// identical copy.
#pragma once
#include "gemm_core.h"

namespace {

// data gradient: dA_b = dC W_b   (reduction over N)
struct BwdDataArgs {
  int nb;
  int N;
  int64_t M;
  const float* G;
  int64_t ldg;
  const float* W[MAXB];
  float* O[MAXB];
  int64_t ldw[MAXB];
  int64_t ldo[MAXB];
  int kb[MAXB];
  int tile_start[MAXB + 1];
  int accumulate;
};

// weight gradient: dW_b = dC^T A_b  (reduction over M, split over workgroups)
struct BwdWeightArgs {
  int nb;
  int N;
  int64_t M;
  const float* G;
  int64_t ldg;
  const float* A[MAXB];
  int64_t lda[MAXB];
  int kb[MAXB];
  int tile_start[MAXB + 1];
  int64_t part_off[MAXB];
  int64_t bias_off;  // -1: no bias gradient
  int64_t part_stride;
  float* part;
  int64_t rows_per_split;
  int tiles_n;
  int xcd_map;  // remap (tile, split) so each XCD walks one contiguous range of them
};

}  // namespace
