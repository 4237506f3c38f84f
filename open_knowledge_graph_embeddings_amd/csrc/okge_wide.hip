// The wide path: slot sizes 513 .. 4096.
//
// Both tile kernels of the step (okge_train64.hip, okge_train64k.hip) keep a whole query row block resident across the
// contraction, which is what stops them at d = 512.  wide_tile_kernel<MODE> contracts over d in a LOOP instead:
//   workgroup = 4 waves = a 128 (batch rows) x 128 (candidates) block of scores, wave (wm, wn) a 64 x 64 quarter = 4 x 4 blocks
//   of v_mfma_f32_16x16x4_f32 (exact fp32); d in chunks of 16 columns staged through LDS, the next chunk's global loads in
//   registers while the current one is multiplied (as gemm_f32_kernel does).  A thread stages 8 consecutive columns of one query
//   row and of one candidate row: one Philox call gives the candidate's eight keep flags (the mask documented in okge.h, keyed
//   by candidate POSITION and column / 8: bit-identical to what the d <= 512 kernels draw).
// Every score is ONE accumulation chain over the ldq = ceil16(d) columns in ascending order, whatever tile, row block or
// candidate range it lands in: its bits depend on the operands and on d alone.
//   MODE_SCORE                   stores X[B][ldx]
//   MODE_STATS                   (max, sum-exp) per (tile, row) for the KL loss' row log-sum-exp (merged by kl_row_lse_kernel)
//   MODE_TRAIN_BCE / _TRAIN_KL   loss epilogue in registers (okge_tile.h's loss_element), one double loss partial per (tile, row
//                                block), G = dLoss/dScore / normalizer stored row-major to G[Bpad][ldg] for the two products
//                                dC = G^T . Q and dQ = G . Cm, which run on gemm_f32_kernel (okge_gemm.hip): with d a free
//                                dimension of both, a generic GEMM serves every width.
// Also here: the gather of a range's masked candidate rows (the dQ product's operand when the range is not a plain table
// slice), the masked scatter of its gradient rows into dE, and the ordered reduction of the dQ product's split-K slabs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "okge_device.h"
#include "okge_kernels.h"
#include "okge_plan.h"
#include "okge_tile.h"
#include "okge_wide.h"

namespace okge {

namespace {

constexpr int WIDE_THREADS = 256;
constexpr int WLD = WIDE_KC + 4;      // leading dimension of the [128][16] LDS tiles: 4 * odd, 16-byte aligned rows

template <int MODE>
__global__ __launch_bounds__(WIDE_THREADS, 2) void wide_tile_kernel(const FusedArgs a)
{
    constexpr bool TRAIN = MODE == MODE_TRAIN_BCE || MODE == MODE_TRAIN_KL;
    __shared__ __attribute__((aligned(16))) float Qs[WIDE_TM * WLD];
    __shared__ __attribute__((aligned(16))) float Cs[WIDE_TN * WLD];
    __shared__ uint32_t ybits[TRAIN ? WIDE_TM * (WIDE_TN / 32) : 1];      // label bit of (row, candidate) of the block
    __shared__ float2 part[MODE == MODE_STATS ? 2 * WIDE_TM : 1];         // (max, sum-exp) of the two candidate halves
    __shared__ double red[WIDE_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int b0 = blockIdx.x * WIDE_TM, t = blockIdx.y, n0 = t * WIDE_TN;
    const int d = a.d;

    if (TRAIN) {
        for (int i = tid; i < WIDE_TM * (WIDE_TN / 32); i += WIDE_THREADS) ybits[i] = 0u;
        __syncthreads();
        // the tile's positives (column-sorted coordinates, offsets per 128-candidate tile from the encode launch); rows of
        // other row blocks, and padding entries (row < 0), fall outside [0, 128)
        const int pos_lo = a.tile_ptr[t], pos_hi = a.tile_ptr[t + 1];
        for (int q = pos_lo + tid; q < pos_hi; q += WIDE_THREADS) {
            const int row = a.pos_row[q] - b0, col = a.pos_col[q] - a.cand_col0 - n0;
            if (row >= 0 && row < WIDE_TM && col >= 0 && col < WIDE_TN) atomicOr(&ybits[row * (WIDE_TN / 32) + (col >> 5)], 1u << (col & 31));
        }
        // (the main loop's barriers order these before the epilogue reads them)
    }

    // staging role: row `srow` of both operands, columns k0 + 8 * soct .. + 7 of every chunk
    const int srow = tid >> 1, soct = tid & 1;
    const float *qrow = a.Q + (size_t)(b0 + srow) * a.ldq;                // (Bpad rows: always inside the block)
    const int sn = n0 + srow;
    const bool snvalid = sn < a.N;
    const int64_t crow = snvalid ? cand_table_row(a.cand_ids, a.cand_first, sn, a.n_table_rows, (soct == 0 && blockIdx.x == 0) ? a.id_err : nullptr) : 0;
    const float *cptr = a.E + crow * d;
    const bool cvec = (d & 3) == 0 && (reinterpret_cast<uintptr_t>(a.E) & 15) == 0;
    const bool dropping = a.drop_c.enabled != 0;
    const uint32_t dstep = (dropping && !a.drop_c.keep) ? drop_step(a.drop_c) : 0u;
    v4f rq[2], rc[2];
    auto load = [&](int k0) {
        const int k = k0 + 8 * soct;                                      // k + 8 <= ldq
        rq[0] = *reinterpret_cast<const v4f *>(qrow + k);
        rq[1] = *reinterpret_cast<const v4f *>(qrow + k + 4);
        rc[0] = v4f{0.f, 0.f, 0.f, 0.f};
        rc[1] = v4f{0.f, 0.f, 0.f, 0.f};
        if (!snvalid || k >= d) return;
        if (cvec) {                                                       // d % 4 == 0: a quad is inside the row or past it
            rc[0] = *reinterpret_cast<const v4f *>(cptr + k);
            if (k + 4 < d) rc[1] = *reinterpret_cast<const v4f *>(cptr + k + 4);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k + e < d) rc[0][e] = cptr[k + e];
                if (k + 4 + e < d) rc[1][e] = cptr[k + 4 + e];
            }
        }
        if (dropping) {
            const uint32_t bits = drop_keep8(a.drop_c, (uint32_t)(a.cand_col0 + sn), k >> 3, d, dstep);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                rc[0][e] *= (bits >> e & 1u) ? a.drop_c.scale : 0.f;
                rc[1][e] *= (bits >> (4 + e) & 1u) ? a.drop_c.scale : 0.f;
            }
        }
    };
    auto stage = [&]() {
        float *qd = Qs + srow * WLD + 8 * soct, *cd = Cs + srow * WLD + 8 * soct;
        *reinterpret_cast<v4f *>(qd) = rq[0];
        *reinterpret_cast<v4f *>(qd + 4) = rq[1];
        *reinterpret_cast<v4f *>(cd) = rc[0];
        *reinterpret_cast<v4f *>(cd + 4) = rc[1];
    };

    v4f acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    const int K = a.ldq;
    load(0);
    for (int k0 = 0; k0 < K; k0 += WIDE_KC) {
        __syncthreads();                                                  // the previous chunk has been multiplied
        stage();
        __syncthreads();
        if (k0 + WIDE_KC < K) load(k0 + WIDE_KC);
#pragma unroll
        for (int k4 = 0; k4 < WIDE_KC; k4 += 4) {
            float qa[4], cb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                qa[i] = Qs[(64 * wm + 16 * i + (lane & 15)) * WLD + k4 + (lane >> 4)];
                cb[i] = Cs[(64 * wn + 16 * i + (lane & 15)) * WLD + k4 + (lane >> 4)];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(qa[i], cb[j], acc[i][j]);
        }
    }

    // result register r of acc[i][j] in lane l: batch row ml = 64 wm + 16 i + 4 (l >> 4) + r, candidate cl = 64 wn + 16 j + (l & 15)
    const int ml0 = 64 * wm + 4 * (lane >> 4), cl0 = 64 * wn + (lane & 15);
    if (MODE == MODE_SCORE) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = b0 + ml0 + 16 * i + r;
                if (m >= a.B) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = n0 + cl0 + 16 * j;
                    if (n < a.N) a.X[(size_t)m * a.ldx + n] = acc[i][j][r];
                }
            }
        return;
    }
    if (MODE == MODE_STATS) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n0 + cl0 + 16 * j < a.N) mx = fmaxf(mx, acc[i][j][r]);
                mx = row16_max(mx);
                float se = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n0 + cl0 + 16 * j < a.N) se += __builtin_amdgcn_exp2f((acc[i][j][r] - mx) * TILE_LOG2E);
                se = row16_sum(se);
                if ((lane & 15) == 0) part[wn * WIDE_TM + ml0 + 16 * i + r] = make_float2(mx, se);
            }
        __syncthreads();
        if (tid < WIDE_TM) {                                              // the two candidate halves, in order
            const float2 p0 = part[tid], p1 = part[WIDE_TM + tid];
            const float m2 = fmaxf(p0.x, p1.x);
            float s2 = 0.f;
            if (p0.x > -INFINITY) s2 += p0.y * __builtin_amdgcn_exp2f((p0.x - m2) * TILE_LOG2E);
            if (p1.x > -INFINITY) s2 += p1.y * __builtin_amdgcn_exp2f((p1.x - m2) * TILE_LOG2E);
            reinterpret_cast<float2 *>(a.stats)[(size_t)t * a.Bpad + b0 + tid] = make_float2(m2, s2);
        }
        return;
    }
    if (TRAIN) {
        float lsum = 0.f;
        // rows / candidates of this lane inside the batch / the launch: 16 i + r < mlim, 16 j < nlim (lane data, compared where
        // it is used: sixteen row predicates and their combinations held in scalar registers spilled some of them)
        const int mlim = a.B - (b0 + ml0), nlim = a.N - (n0 + cl0);
        float *grow = a.G + (size_t)(b0 + ml0) * a.ldg + n0 + cl0;       // row (i, r) is 16 i + r rows further down
        const uint32_t *yrow = ybits + ml0 * (WIDE_TN / 32) + 2 * wn;     // the wave's candidate half: two 32-bit words per row
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int lim = mlim;
                asm volatile("" : "+v"(lim));                             // (keeps the compare inside this iteration)
                const bool mvalid = 16 * i + r < lim;
                const int m = b0 + ml0 + 16 * i + r;
                const uint32_t y0 = yrow[(16 * i + r) * (WIDE_TN / 32)], y1 = yrow[(16 * i + r) * (WIDE_TN / 32) + 1];
                float *gp = grow + (size_t)(16 * i + r) * a.ldg;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool pos = ((j < 2 ? y0 : y1) >> (16 * (j & 1) + (lane & 15))) & 1u;
                    const bool valid = mvalid && 16 * j < nlim;
                    const LossTerm lt = loss_element<TRAIN ? MODE : MODE_TRAIN_BCE>(a, acc[i][j][r], pos, m, false, true, a.B);
                    lsum += valid ? lt.l : 0.f;
                    // padding rows / candidates carry a zero gradient: the products may read the whole block
                    // (stored under OKGE_TRAIN_LOSS_ONLY too: the block is in the workspace anyway, and a uniform branch
                    //  around each store cut the epilogue into sixty-four basic blocks)
                    gp[16 * j] = valid ? lt.g : 0.f;
                }
                __builtin_amdgcn_sched_barrier(0);       // one row of four elements at a time: the unrolled epilogue is not interleaved
            }
        const double ls = wave_sum((double)lsum);
        if (lane == 0) red[w] = ls;
        __syncthreads();
        if (tid == 0) a.loss_partial[(size_t)t * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

// Cm[n][0 .. d) = dropout(E[candidate n of the range]): the dQ product's operand when the range is not a plain table slice.
// One workgroup per candidate, one thread per column octet (= one Philox call).  pos0: position of the range's first candidate
// in the call's candidate list (the mask's key).
__global__ __launch_bounds__(128) void wide_gather_kernel(const float *__restrict__ E, const int32_t *__restrict__ cand_ids, int cand_first,
                                                          int pos0, int d, int64_t ldc, const DropDev drop, int64_t table_rows,
                                                          float *__restrict__ Cm)
{
    const int n = blockIdx.x;
    const int64_t row = cand_table_row(cand_ids, cand_first, n, table_rows, nullptr);      // (counted by the tile kernel)
    const float *src = E + row * d;
    float *dst = Cm + (size_t)n * ldc;
    const uint32_t step = (drop.enabled && !drop.keep) ? drop_step(drop) : 0u;
    for (int o = threadIdx.x; 8 * o < d; o += blockDim.x) {
        const uint32_t bits = drop.enabled ? drop_keep8(drop, (uint32_t)(pos0 + n), o, d, step) : 0xFFu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * o + e;
            if (k < d) dst[k] = src[k] * ((bits >> e & 1u) ? drop.scale : 0.f);
        }
    }
}

// dE[candidate n] (+)= mask(n) * dC[n]: stored when the rows are exclusive and the gradients zero, read-modify-written when
// exclusive, float atomics for an id list that may repeat
__global__ __launch_bounds__(128) void wide_dc_scatter_kernel(const float *__restrict__ dC, int64_t ldc, const int32_t *__restrict__ cand_ids,
                                                              int cand_first, int pos0, int d, const DropDev drop, int exclusive,
                                                              int grads_zero, float *__restrict__ dE, int64_t table_rows)
{
    const int n = blockIdx.x;
    const int64_t row = cand_table_row(cand_ids, cand_first, n, table_rows, nullptr);
    const float *src = dC + (size_t)n * ldc;
    float *dst = dE + row * d;
    const uint32_t step = (drop.enabled && !drop.keep) ? drop_step(drop) : 0u;
    for (int o = threadIdx.x; 8 * o < d; o += blockDim.x) {
        const uint32_t bits = drop.enabled ? drop_keep8(drop, (uint32_t)(pos0 + n), o, d, step) : 0xFFu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = 8 * o + e;
            if (k >= d) continue;
            const float v = src[k] * ((bits >> e & 1u) ? drop.scale : 0.f);
            if (!exclusive) atomicAdd(dst + k, v);
            else dst[k] = grads_zero ? v : dst[k] + v;
        }
    }
}

// dQ[b][k] (+)= the dQ product's split-K slabs, added in split order; later candidate ranges accumulate
__global__ __launch_bounds__(256) void wide_dq_reduce_kernel(const float *__restrict__ slab, int splits, int64_t slab_stride, int B, int d,
                                                             int ldq, int accumulate, float *__restrict__ dQ)
{
    const int64_t total = (int64_t)B * d, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t at = (size_t)(i / d) * ldq + (size_t)(i % d);
        float v = accumulate ? dQ[at] : 0.f;
        for (int s = 0; s < splits; ++s) v += slab[(size_t)s * slab_stride + at];
        dQ[at] = v;
    }
}

}  // namespace

hipError_t launch_wide_tile(int mode, const FusedArgs &a, int row_blocks, int tiles, hipStream_t st)
{
    if (row_blocks <= 0 || tiles <= 0) return hipSuccess;
    if (tiles > 65535) return hipErrorInvalidValue;
    const dim3 grid(row_blocks, tiles), block(WIDE_THREADS);
    switch (mode) {
    case MODE_SCORE: hipLaunchKernelGGL(wide_tile_kernel<MODE_SCORE>, grid, block, 0, st, a); break;
    case MODE_STATS: hipLaunchKernelGGL(wide_tile_kernel<MODE_STATS>, grid, block, 0, st, a); break;
    case MODE_TRAIN_BCE: hipLaunchKernelGGL(wide_tile_kernel<MODE_TRAIN_BCE>, grid, block, 0, st, a); break;
    case MODE_TRAIN_KL: hipLaunchKernelGGL(wide_tile_kernel<MODE_TRAIN_KL>, grid, block, 0, st, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_wide_gather(const float *E, const int32_t *cand_ids, int cand_first, int pos0, int n, int d, int64_t ldc,
                              const DropDev &drop, int64_t table_rows, float *Cm, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(wide_gather_kernel, dim3(n), dim3(128), 0, st, E, cand_ids, cand_first, pos0, d, ldc, drop, table_rows, Cm);
    return hipGetLastError();
}

hipError_t launch_wide_dc_scatter(const float *dC, int64_t ldc, const int32_t *cand_ids, int cand_first, int pos0, int n, int d,
                                  const DropDev &drop, int exclusive, int grads_zero, float *dE, int64_t table_rows, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(wide_dc_scatter_kernel, dim3(n), dim3(128), 0, st, dC, ldc, cand_ids, cand_first, pos0, d, drop, exclusive,
                       grads_zero, dE, table_rows);
    return hipGetLastError();
}

hipError_t launch_wide_dq_reduce(const float *slab, int splits, int64_t slab_stride, int B, int d, int ldq, int accumulate, float *dQ,
                                 hipStream_t st)
{
    const int64_t total = (int64_t)B * d;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(wide_dq_reduce_kernel, dim3((unsigned)std::min<int64_t>(2048, (total + 255) / 256)), dim3(256), 0, st, slab, splits,
                       slab_stride, B, d, ldq, accumulate, dQ);
    return hipGetLastError();
}

}  // namespace okge
