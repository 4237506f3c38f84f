// Evaluation's rank kernels (gfx950):
//   ranks_kernel          filtered ranks of a materialised score block, exact integer counts (rank_sweep / rank_sweep_regs);
//                         also the two phases of the candidate-sharded evaluation            dataset.py:423-446
//   rank_metrics_kernel   the meters of compute_metrics, kept on the device                   dataset.py:447-452
//   eval_side_kernel      the fused evaluation's point scores and ranks-from-counts in one launch (okge_eval_device.h)
#include "okge_kernels.h"
#include "okge_eval_device.h"

namespace okge {

constexpr int RANK_GROUPS = 8;

// Count, for NG answer groups of one row at once, how many (filter-corrected) scores are greater than / equal to
// each group's true score.  NG is the compile-time number of live groups (1, 2, 4 or 8): the sweep is VALU-bound
// on the compares, and most rows have one or two groups.
template <int NG>
__device__ __forceinline__ void rank_sweep(const float *__restrict__ row, int64_t ld_is_vec, int N,
                                           const int32_t *__restrict__ filt_col, int64_t f_lo, int64_t f_hi, int col0,
                                           const float *tv, int tid, int (&gt)[RANK_GROUPS], int (&eq)[RANK_GROUPS])
{
    float t[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) t[j] = tv[j];
    int g[NG], e[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) { g[j] = 0; e[j] = 0; }
    const int n4 = ld_is_vec ? (N >> 2) : 0;
    const float4 *row4 = reinterpret_cast<const float4 *>(row);
    // 16-byte loads, four in flight per thread: a row is 58 KB at the FB15k-237 size and the sweep is a chain of memory
    // round trips, not compares
    for (int i = tid; i < n4; i += 1024) {
        float4 xv[4];
        bool has[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            has[u] = i + 256 * u < n4;
            xv[u] = has[u] ? row4[i + 256 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (!has[u]) continue;
            const float xs[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma unroll
                for (int j = 0; j < NG; ++j) { g[j] += xs[k] > t[j]; e[j] += xs[k] == t[j]; }
            }
        }
    }
    for (int n = 4 * n4 + tid; n < N; n += 256) {
        const float x = row[n];
#pragma unroll
        for (int j = 0; j < NG; ++j) { g[j] += x > t[j]; e[j] += x == t[j]; }
    }
    // filtered positions count as -1e8 instead of their score (dataset.py:441)
    for (int64_t f = f_lo + tid; f < f_hi; f += 256) {
        const int col = filt_col[f] - col0;                     // a shard only sees its own candidate columns
        if (col < 0 || col >= N) continue;
        const float x = row[col];
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            g[j] += (-1e8f > t[j]) - (x > t[j]);
            e[j] += (-1e8f == t[j]) - (x == t[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < RANK_GROUPS; ++j) { gt[j] = j < NG ? g[j < NG ? j : 0] : 0; eq[j] = j < NG ? e[j < NG ? j : 0] : 0; }
}

// The same counts with the thread's part of the row already in registers (rows up to RANK_REG_ROW floats): the row
// loads are issued at kernel entry and overlap the dependent-load chain that finds the true scores
// (row_ptr -> grp_ptr -> ids -> score), and several group chunks reuse them.
constexpr int RANK_REG_F4 = 16, RANK_REG_ROW = 256 * 4 * RANK_REG_F4;

template <int NG>
__device__ __forceinline__ void rank_sweep_regs(const float4 (&rv)[RANK_REG_F4], int n4, float tail_x, bool has_tail, float filt_x,
                                                bool has_filt, const float *__restrict__ row, int N,
                                                const int32_t *__restrict__ filt_col, int64_t f_lo, int64_t f_hi, int col0,
                                                const float *tv, int tid, int (&gt)[RANK_GROUPS], int (&eq)[RANK_GROUPS])
{
    float t[NG];
    int g[NG], e[NG];
#pragma unroll
    for (int j = 0; j < NG; ++j) { t[j] = tv[j]; g[j] = 0; e[j] = 0; }
#pragma unroll
    for (int u = 0; u < RANK_REG_F4; ++u) {
        if (tid + 256 * u >= n4) continue;
        const float xs[4] = {rv[u].x, rv[u].y, rv[u].z, rv[u].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int j = 0; j < NG; ++j) { g[j] += xs[k] > t[j]; e[j] += xs[k] == t[j]; }
        }
    }
    if (has_tail) {
#pragma unroll
        for (int j = 0; j < NG; ++j) { g[j] += tail_x > t[j]; e[j] += tail_x == t[j]; }
    }
    // filtered positions count as -1e8 instead of their score (dataset.py:441); the first 256 were fetched at entry
    if (has_filt) {
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            g[j] += (-1e8f > t[j]) - (filt_x > t[j]);
            e[j] += (-1e8f == t[j]) - (filt_x == t[j]);
        }
    }
    for (int64_t f = f_lo + 256 + tid; f < f_hi; f += 256) {
        const int col = filt_col[f] - col0;
        if (col < 0 || col >= N) continue;
        const float x = row[col];
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            g[j] += (-1e8f > t[j]) - (x > t[j]);
            e[j] += (-1e8f == t[j]) - (x == t[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < RANK_GROUPS; ++j) { gt[j] = j < NG ? g[j < NG ? j : 0] : 0; eq[j] = j < NG ? e[j < NG ? j : 0] : 0; }
}

__global__ __launch_bounds__(256) void ranks_kernel(const float *__restrict__ scores, int64_t ld, int N,
                                                    const int64_t *__restrict__ filt_ptr,
                                                    const int32_t *__restrict__ filt_col,
                                                    const int64_t *__restrict__ row_ptr,
                                                    const int64_t *__restrict__ grp_ptr, const int32_t *__restrict__ ids,
                                                    int64_t *__restrict__ ranks, int col0,
                                                    const float *__restrict__ true_in, float *__restrict__ true_out,
                                                    int64_t *__restrict__ counts_out)
{
    // Whole candidate list (col0 = 0, true_in = true_out = counts_out = null): ranks.
    // Candidate-sharded evaluation runs it twice around two tiny all-reduces:
    //   true_out   : the shard's maximum over each group's ids that fall in [col0, col0 + N)   -> all-reduce(max)
    //   true_in    : global true scores in, counts_out[g] = {#greater, #equal} of this shard   -> all-reduce(sum)
    // blockIdx.y strides over the row's chunks of 8 answer groups: rows with many answers (they set the kernel's
    // duration) are spread over gridDim.y workgroups, the others leave at once
    __shared__ float tv[RANK_GROUPS];
    __shared__ int cnt[4][2 * RANK_GROUPS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t g_lo = row_ptr[b] + (int64_t)RANK_GROUPS * blockIdx.y, g_hi = row_ptr[b + 1];
    if (g_lo >= g_hi) return;
    const float *row = scores + (size_t)b * ld;
    const int64_t f_lo = filt_ptr[b], f_hi = filt_ptr[b + 1];
    const int64_t vec = ((ld & 3) == 0) && ((reinterpret_cast<uintptr_t>(scores) & 15) == 0);
    const bool in_regs = vec && N <= RANK_REG_ROW && !true_out;
    const int n4 = N >> 2;
    float4 rv[RANK_REG_F4];
    float tail_x = 0.f, filt_x = 0.f;
    bool has_tail = false, has_filt = false;
    if (in_regs) {
        // everything that does not depend on the true scores is requested now: the row, its (< 4) tail elements and
        // the scores under the first 256 filter entries
#pragma unroll
        for (int u = 0; u < RANK_REG_F4; ++u)
            rv[u] = tid + 256 * u < n4 ? reinterpret_cast<const float4 *>(row)[tid + 256 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
        has_tail = 4 * n4 + tid < N;
        if (has_tail) tail_x = row[4 * n4 + tid];
        if (f_lo + tid < f_hi) {
            const int col = filt_col[f_lo + tid] - col0;
            has_filt = col >= 0 && col < N;
            if (has_filt) filt_x = row[col];
        }
    }
    for (int64_t g0 = g_lo; g0 < g_hi; g0 += (int64_t)RANK_GROUPS * gridDim.y) {
        const int ng = (int)min((int64_t)RANK_GROUPS, g_hi - g0);
        if (tid < RANK_GROUPS) {
            float t = __builtin_nanf("");                       // unused slots never compare true
            if (tid < ng) {
                if (true_in) {
                    t = true_in[g0 + tid];
                } else {
                    t = -INFINITY;
                    for (int64_t j = grp_ptr[g0 + tid]; j < grp_ptr[g0 + tid + 1]; ++j) {
                        const int col = ids[j] - col0;
                        if (col >= 0 && col < N) t = fmaxf(t, row[col]);
                    }
                    if (true_out) true_out[g0 + tid] = t;
                }
            }
            tv[tid] = t;
        }
        if (true_out) continue;                                 // uniform: phase 1 of the sharded evaluation
        __syncthreads();
        int gt[RANK_GROUPS], eq[RANK_GROUPS];
        if (in_regs) {
            if (ng == 1)      rank_sweep_regs<1>(rv, n4, tail_x, has_tail, filt_x, has_filt, row, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
            else if (ng == 2) rank_sweep_regs<2>(rv, n4, tail_x, has_tail, filt_x, has_filt, row, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
            else if (ng <= 4) rank_sweep_regs<4>(rv, n4, tail_x, has_tail, filt_x, has_filt, row, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
            else              rank_sweep_regs<8>(rv, n4, tail_x, has_tail, filt_x, has_filt, row, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
        } else if (ng == 1)   rank_sweep<1>(row, vec, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
        else if (ng == 2)     rank_sweep<2>(row, vec, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
        else if (ng <= 4)     rank_sweep<4>(row, vec, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
        else                  rank_sweep<8>(row, vec, N, filt_col, f_lo, f_hi, col0, tv, tid, gt, eq);
#pragma unroll
        for (int j = 0; j < RANK_GROUPS; ++j) {
            const int a = wave_sum(gt[j]), e = wave_sum(eq[j]);
            if ((tid & 63) == 0) { cnt[tid >> 6][2 * j] = a; cnt[tid >> 6][2 * j + 1] = e; }
        }
        __syncthreads();
        if (tid < ng) {
            const int64_t a = (int64_t)cnt[0][2 * tid] + cnt[1][2 * tid] + cnt[2][2 * tid] + cnt[3][2 * tid];
            const int64_t e = (int64_t)cnt[0][2 * tid + 1] + cnt[1][2 * tid + 1] + cnt[2][2 * tid + 1] + cnt[3][2 * tid + 1];
            if (counts_out) {
                counts_out[2 * (g0 + tid)] = a;
                counts_out[2 * (g0 + tid) + 1] = e;
            } else {
                ranks[g0 + tid] = a + e / 2;
            }
        }
        __syncthreads();
    }
}

// acc[0..6] += {#groups, sum 1/(rank+1), sum rank, #rank<1, #rank<3, #rank<10, #rank<50}: the meters of compute_metrics
// (dataset.py:447-452) kept on the device, so that evaluation batches need no host round trip
__global__ __launch_bounds__(256) void rank_metrics_kernel(const int64_t *__restrict__ ranks, int64_t n, double *__restrict__ acc)
{
    __shared__ double red[4][7];
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int64_t r = ranks[i];
        v[0] += 1.0;
        v[1] += (double)(1.0f / (float)(r + 1));       // fp32 reciprocal like the reference's (1/(rank+1).float())
        v[2] += (double)r;
        v[3] += r < 1; v[4] += r < 3; v[5] += r < 10; v[6] += r < 50;
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double t = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = t;
    }
    __syncthreads();
    // atomic: launches of independent stream chains may share one `acc` (PipelinedEvaluator hands every chain its own
    // and sums them after the join, which also keeps the double sums order-deterministic)
    if (threadIdx.x < 7)
        atomicAdd(acc + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// ---- fused evaluation (okge_evaluate_fused): the side work (okge_eval_device.h) ------------------------------------
// The two small kernels of the fused evaluation in ONE launch: workgroups [0, n_points) take the rows of `pts`, the rest
// the groups of `rk`.  In a run of batches the points of batch i+1 ride with the ranks of batch i (independent work of
// two batches; either part may be empty).
__global__ __launch_bounds__(256) void eval_side_kernel(const EvalPointsArgs pts, const EvalRanksArgs rk, int n_points)
{
    if ((int)blockIdx.x < n_points) eval_points_block(pts, blockIdx.x);
    else eval_ranks_block(rk, (int)blockIdx.x - n_points);
}

// ---- launchers -----------------------------------------------------------------------------------------
hipError_t launch_rank_metrics(const int64_t *ranks, int64_t n, double *acc, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(rank_metrics_kernel, dim3(1), dim3(256), 0, st, ranks, n, acc);
    return hipGetLastError();
}

hipError_t launch_ranks(const float *scores, int64_t ld, int B, int N, const int64_t *filt_ptr,
                        const int32_t *filt_col, const int64_t *row_ptr, const int64_t *grp_ptr, const int32_t *ids,
                        int64_t *ranks, int col0, const float *true_in, float *true_out, int64_t *counts_out,
                        hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(ranks_kernel, dim3(B, 4), dim3(256), 0, st, scores, ld, N, filt_ptr, filt_col, row_ptr, grp_ptr,
                       ids, ranks, col0, true_in, true_out, counts_out);
    return hipGetLastError();
}

hipError_t launch_eval_side(const EvalPointsArgs *pts, const EvalRanksArgs *rk, hipStream_t st)
{
    const int n_points = pts ? pts->Bpad : 0;
    const int n_ranks = rk && rk->n_groups > 0 ? (int)((rk->n_groups + 3) / 4) : 0;
    if (n_points + n_ranks <= 0) return hipSuccess;
    static const EvalPointsArgs no_pts = {};
    static const EvalRanksArgs no_rk = {};
    hipLaunchKernelGGL(eval_side_kernel, dim3(n_points + n_ranks), dim3(256), 0, st, pts ? *pts : no_pts, rk ? *rk : no_rk, n_points);
    return hipGetLastError();
}

}  // namespace okge
