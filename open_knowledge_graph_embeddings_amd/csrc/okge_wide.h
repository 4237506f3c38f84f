// Launchers of the wide path (okge_wide.hip): slot sizes 513 .. 4096.  Shapes, plans and workspace layouts: okge_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "okge_kernels.h"

namespace okge {

// wide_tile_kernel<mode> over (row_blocks x tiles) 128 x 128 score blocks; mode: MODE_SCORE / _STATS / _TRAIN_BCE / _TRAIN_KL.
// a.N = candidates of the launch, a.cand_col0 = position of its first candidate in the call's list, a.tile_ptr / a.loss_partial
// / a.stats already moved to its first tile; a.G = [Bpad][a.ldg]
hipError_t launch_wide_tile(int mode, const FusedArgs &a, int row_blocks, int tiles, hipStream_t st);
// Cm[n][ldc] = dropout(E[candidate n]), n < n; pos0 = position of candidate 0 in the call's list (the mask's key)
hipError_t launch_wide_gather(const float *E, const int32_t *cand_ids, int cand_first, int pos0, int n, int d, int64_t ldc,
                              const DropDev &drop, int64_t table_rows, float *Cm, hipStream_t st);
// dE[candidate n] (+)= mask(n) * dC[n]
hipError_t launch_wide_dc_scatter(const float *dC, int64_t ldc, const int32_t *cand_ids, int cand_first, int pos0, int n, int d,
                                  const DropDev &drop, int exclusive, int grads_zero, float *dE, int64_t table_rows, hipStream_t st);
// dQ[b][k] = (accumulate ? dQ[b][k] : 0) + slab[0][b][k] + slab[1][b][k] + ...
hipError_t launch_wide_dq_reduce(const float *slab, int splits, int64_t slab_stride, int B, int d, int ldq, int accumulate, float *dQ,
                                 hipStream_t st);
// gemm_f32_kernel (okge_gemm.hip): C[M][N] = op(A) . B; A = [M][K] (ta = false) or [K][M] (ta = true), B = [K][N], all row-major.
// splits > 1: K is cut into `splits` pieces of k_per_split, piece z written to C + z * slab_stride (added up by the caller)
hipError_t launch_gemm_f32(bool ta, const float *A, int64_t lda, const float *B, int64_t ldb, float *C, int64_t ldc, int M, int N, int K,
                           int splits, int k_per_split, int64_t slab_stride, hipStream_t st);

}  // namespace okge
