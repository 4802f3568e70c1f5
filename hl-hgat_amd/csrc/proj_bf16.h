// Host interface of the bf16-operand projection kernels (proj_bf16.hip): the
// process-wide matmul precision, the eligibility rule of one GEMM call and the
// three launchers.  The argument blocks are passed as untyped pointers because
// FwdArgs / BwdDataArgs / BwdWeightArgs have internal linkage (gemm_core.h,
// proj_args.h): caller and callee each include the one definition.
#pragma once
#include "common.h"

namespace hlhgat {

// HLHGAT_GEMM_FP32 or HLHGAT_GEMM_BF16 (hlhgat_set_gemm_precision)
int gemm_precision();

// The rule of hlhgat_gemm_bf16_eligible over one operand family: every
// kb % 8 == 0, every stride in ld % 4 == 0, N % 4 == 0.
bool gemm_bf16_shape_ok(int nblocks, const int64_t* kb, const int64_t* ld, int64_t N);

// gemm_bf16_shape_ok plus 16-B alignment of every operand block P[b].
bool gemm_bf16_operands_ok(int nblocks, const float* const* P, const int64_t* ld,
                           const int64_t* kb, int64_t N);

// Books one GEMM call made in bf16 mode: `eligible` calls go to the bf16
// kernels (returns true), the others fall back to fp32 (returns false).
// In fp32 mode it books nothing and returns false.
bool gemm_bf16_route(bool eligible);

// fwd_args: FwdArgs; tn: 16-column tiles per wave (1, 2 or 4)
int launch_proj_fwd_bf16(const void* fwd_args, int tn, hipStream_t s, const ProfScope* prof);
// data_args: BwdDataArgs with tile_start in units of tnd * 16 columns
int launch_proj_bwd_data_bf16(const void* data_args, int tnd, hipStream_t s);
// weight_args: BwdWeightArgs planned with 64 x 64 tiles; the caller reduces
// the split slab (k_reduce_splits) afterwards
int launch_proj_bwd_weight_bf16(const void* weight_args, int tiles_total, int splits,
                                hipStream_t s);

}  // namespace hlhgat
