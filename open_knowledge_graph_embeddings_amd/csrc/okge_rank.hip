// Evaluation's rank kernels (gfx950):
//   ranks_kernel          filtered ranks of a materialised score block, exact integer counts (rank_sweep / rank_sweep_regs);
//                         also the two phases of the candidate-sharded evaluation            dataset.py:423-446
//   rank_metrics_kernel   the meters of compute_metrics, kept on the device                   dataset.py:447-452
//   eval_side_kernel      the fused evaluation's point scores and ranks-from-counts in one launch (okge_eval_device.h)
//   eval_side_loss_kernel, eval_loss_rows_kernel, eval_loss_reduce_kernel, block_loss_rows_kernel
//                         the validation loss of an evaluation batch (trainer.py:93-106, :263-271), fused and from a score block
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
    if ((int)blockIdx.x < n_points) eval_points_block<false>(pts, blockIdx.x, EvalLossPoints{});
    else eval_ranks_block(rk, (int)blockIdx.x - n_points);
}
// ... and with the validation loss' label term from the points part
__global__ __launch_bounds__(256) void eval_side_loss_kernel(const EvalPointsArgs pts, const EvalLossPoints el, const EvalRanksArgs rk,
                                                             int n_points)
{
    if ((int)blockIdx.x < n_points) eval_points_block<true>(pts, blockIdx.x, el);
    else eval_ranks_block(rk, (int)blockIdx.x - n_points);
}

// ---- the validation loss of an evaluation batch (trainer.py:93-106 in eval mode, unfiltered scores) ---------------------------
// A row's loss from its label-free sums and its label term.  BCE (smoothing eps): S - (1 - eps) (P + X / N), S - P at eps = 0,
// S = sum softplus(x), X = sum x, P = sum of x over the row's positives.  KL (unnormalised labels): npos lse - P; a row without
// positives adds 0.
__device__ __forceinline__ double eval_row_loss(int kind, double s_or_lse, double xsum, double pos_sum, int npos, int N, double eps)
{
    if (kind == LOSS_BCE) return eps > 0.0 ? s_or_lse - (1.0 - eps) * (pos_sum + xsum / (double)N) : s_or_lse - pos_sum;
    return npos > 0 ? (double)npos * s_or_lse - pos_sum : 0.0;
}

// The rows' losses of a fused batch: thread b takes row b (the batch's sorted position: the sum below runs over all rows) and
// merges the tiles' partials in tile order -- BCE in double; KL as a running (max, sum-exp) like kl_row_lse_kernel.  One
// wave per workgroup, the loads of EVAL_LOSS_UNROLL tiles in flight ahead of their (ordered) adds: the merge is a chain of
// memory round trips, not arithmetic.
constexpr int EVAL_LOSS_UNROLL = 16;
__global__ __launch_bounds__(64) void eval_loss_rows_kernel(const EvalLossReduce a)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= a.B) return;
    double S = 0.0, X = 0.0;
    float m = -INFINITY, se = 0.f;
    for (int t0 = 0; t0 < a.tiles; t0 += EVAL_LOSS_UNROLL) {
        float2 p[EVAL_LOSS_UNROLL];
#pragma unroll
        for (int u = 0; u < EVAL_LOSS_UNROLL; ++u)
            p[u] = t0 + u < a.tiles ? a.part[(size_t)(t0 + u) * a.Bpad + b] : make_float2(a.kind == LOSS_BCE ? 0.f : -INFINITY, 0.f);
#pragma unroll
        for (int u = 0; u < EVAL_LOSS_UNROLL; ++u) {
            if (t0 + u >= a.tiles) {
                // (past the last tile: nothing to merge)
            } else if (a.kind == LOSS_BCE) {
                S += (double)p[u].x;
                X += (double)p[u].y;
            } else {
                const float mn = fmaxf(m, p[u].x);
                se = (m > -INFINITY ? se * __expf(m - mn) : 0.f) + (p[u].x > -INFINITY ? p[u].y * __expf(p[u].x - mn) : 0.f);
                m = mn;
            }
        }
    }
    a.rows[b] = a.kind == LOSS_BCE ? eval_row_loss(LOSS_BCE, S, X, a.pos_sum[b], 0, a.N, a.smoothing)
                                   : eval_row_loss(LOSS_KL, (double)m + log((double)se), 0.0, a.pos_sum[b], a.npos[b], a.N, 0.0);
}

// rows[0 .. B) added in row order into *out by ONE thread, from LDS (the workgroup stages 1024 rows at a time: the sum is a
// chain of dependent adds, the loads must not be).  No atomics: the value is the same bits on every run.
__global__ __launch_bounds__(256) void eval_loss_reduce_kernel(const EvalLossReduce a)
{
    constexpr int CH = 1024;
    __shared__ double rs[CH];
    double tot = 0.0;
    for (int b0 = 0; b0 < a.B; b0 += CH) {
        const int n = min(CH, a.B - b0);
        for (int i = threadIdx.x; i < n; i += 256) rs[i] = a.rows[b0 + i];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i) tot += rs[i];
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.out = tot;
}

// The same row losses from a materialised score block: one workgroup per row.  Thread t sums columns t, t + 256, ... (double),
// the threads are added lanes first, then the four waves: a fixed order.  Positives: the union of the row's group ids, an id
// counted where it first occurs in the row's id range.
__device__ __forceinline__ double block_sum256(double v, double *red)
{
    v = wave_sum(v);
    __syncthreads();                                         // (red is reused)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__global__ __launch_bounds__(256) void block_loss_rows_kernel(const float *__restrict__ scores, int64_t ld, int N,
                                                              const int64_t *__restrict__ row_ptr, const int64_t *__restrict__ grp_ptr,
                                                              const int32_t *__restrict__ ids, int kind, double smoothing,
                                                              double *__restrict__ rows)
{
    __shared__ double red[4];
    __shared__ float redm[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *row = scores + (size_t)b * ld;
    const int64_t g_lo = row_ptr[b], g_hi = row_ptr[b + 1];
    const int64_t j_lo = g_lo < g_hi ? grp_ptr[g_lo] : 0, j_hi = g_lo < g_hi ? grp_ptr[g_hi] : 0;
    double pos = 0.0, np = 0.0;
    for (int64_t j = j_lo + tid; j < j_hi; j += 256) {
        const int col = ids[j];
        if (col < 0 || col >= N) continue;                   // (ids are positions in the candidate list)
        bool first = true;
        for (int64_t jj = j_lo; jj < j; ++jj) first = first && ids[jj] != col;
        if (first) { pos += (double)row[col]; np += 1.0; }
    }
    pos = block_sum256(pos, red);
    np = block_sum256(np, red);
    double v;
    if (kind == LOSS_BCE) {
        double S = 0.0, X = 0.0;
        for (int n = tid; n < N; n += 256) {
            const float x = row[n];
            S += (double)(fmaxf(x, 0.f) + __builtin_amdgcn_logf(bce_terms(x).ope) * TILE_LN2);
            X += (double)x;
        }
        S = block_sum256(S, red);
        X = block_sum256(X, red);
        v = eval_row_loss(LOSS_BCE, S, X, pos, 0, N, smoothing);
    } else {
        float m = -INFINITY;
        for (int n = tid; n < N; n += 256) m = fmaxf(m, row[n]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) redm[tid >> 6] = m;
        __syncthreads();
        m = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
        double se = 0.0;
        for (int n = tid; n < N; n += 256) se += (double)__expf(row[n] - m);
        se = block_sum256(se, red);
        v = eval_row_loss(LOSS_KL, (double)m + log(se), 0.0, pos, (int)np, N, 0.0);
    }
    if (tid == 0) rows[b] = v;
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

hipError_t launch_eval_side_loss(const EvalPointsArgs *pts, const EvalLossPoints *el, const EvalRanksArgs *rk, hipStream_t st)
{
    const int n_points = pts && el ? pts->Bpad : 0;
    const int n_ranks = rk && rk->n_groups > 0 ? (int)((rk->n_groups + 3) / 4) : 0;
    if (n_points + n_ranks <= 0) return hipSuccess;
    static const EvalPointsArgs no_pts = {};
    static const EvalLossPoints no_el = {};
    static const EvalRanksArgs no_rk = {};
    hipLaunchKernelGGL(eval_side_loss_kernel, dim3(n_points + n_ranks), dim3(256), 0, st, n_points ? *pts : no_pts, n_points ? *el : no_el,
                       rk ? *rk : no_rk, n_points);
    return hipGetLastError();
}

hipError_t launch_eval_loss_reduce(const EvalLossReduce &a, hipStream_t st)
{
    if (a.part && a.B > 0) {
        hipLaunchKernelGGL(eval_loss_rows_kernel, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(eval_loss_reduce_kernel, dim3(1), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_block_loss_rows(const float *scores, int64_t ld, int B, int N, const int64_t *row_ptr, const int64_t *grp_ptr,
                                  const int32_t *ids, int kind, double smoothing, double *rows, hipStream_t st)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(block_loss_rows_kernel, dim3(B), dim3(256), 0, st, scores, ld, N, row_ptr, grp_ptr, ids, kind, smoothing, rows);
    return hipGetLastError();
}

}  // namespace okge
