// Top-k link prediction, the small kernels around the score sweep (order, keys and the per-tile selection: okge_topk.h).
//
//   topk_cut_kernel    slot sizes above 256: fused_tile_kernel has no instance there, so the sweep runs MODE_SCORE of ONE candidate
//                      range into workspace (fused_tile64k_kernel, the bits of okge_score_prefixes) and this kernel cuts the same
//                      per-(tile, row) records out of that block.
//   topk_merge_kernel  per row, L sorted lists of kq records + the running (B, k) list -> the running list.  One wave per row:
//                      lane i holds the i-th best record so far; the lists stream through 64 records at a time (the loads of
//                      four such batches in flight together), and only records that beat the current k-th best are inserted
//                      (a ballot finds them, a shift by one lane makes room).  Latency-bound and small; after the first few
//                      tiles of a row hardly any record passes the threshold.
#include "okge_kernels.h"

namespace okge {

__global__ __launch_bounds__(FUSED_THREADS) void topk_cut_kernel(const float *__restrict__ X, int64_t ldx, int B, int Bpad, int N,
                                                                 int cand_col0, const int64_t *__restrict__ filt_ptr,
                                                                 const int32_t *__restrict__ filt_col, int kq, TopkRec *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) float Xs[BC * LDG];
    const int tid = threadIdx.x, r = tid >> 3, j8 = 8 * (tid & 7);
    const int n0 = blockIdx.x * NT, b = blockIdx.y * BC + r;
    uint64_t mask = 0;
    if (filt_ptr && b < B) mask = topk_filter_mask(filt_ptr, filt_col, b, cand_col0 + n0);
    uint32_t elig8 = 0;
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const bool in = b < B && n0 + j8 + m < N;
        Xs[r * LDG + j8 + m] = in ? X[(size_t)b * ldx + n0 + j8 + m] : 0.f;
        elig8 |= (in && !((mask >> (j8 + m)) & 1ull)) ? 1u << m : 0u;
    }
    // (every thread reads back only what it wrote itself before the barrier inside)
    topk_select_rows<LDG>(Xs, tid, elig8, kq, cand_col0 + n0, b < B ? part + ((size_t)blockIdx.x * Bpad + b) * kq : nullptr);
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v)
{
    return ((uint64_t)(uint32_t)__shfl_up((int)(v >> 32), 1) << 32) | (uint32_t)__shfl_up((int)(uint32_t)v, 1);
}

__global__ __launch_bounds__(256) void topk_merge_kernel(const TopkMergeArgs a)
{
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.B) return;                                  // a whole wave leaves: no barrier below
    float rs = -INFINITY;
    int32_t rc = -1;
    if (!a.first && lane < a.k) {
        rs = a.out_sc[(size_t)row * a.k + lane];
        rc = a.out_cl[(size_t)row * a.k + lane];
    }
    uint64_t rkey = topk_key64(rs, rc);                      // descending over the lanes; 0 = empty
    uint64_t kth = shfl64(rkey, a.k - 1);
    const int T = a.L * a.kq;
    constexpr int NB = 4;                                    // batches of 64 records whose loads are in flight together
    for (int base = 0; base < T; base += 64 * NB) {
        float s[NB];
        int32_t cc[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int idx = base + 64 * u + lane;
            s[u] = -INFINITY;
            cc[u] = -1;
            if (idx < T) {
                const int l = idx / a.kq, sl = idx - l * a.kq;
                const size_t e = (((size_t)l * a.rows_ld + row) * a.kq + sl) * a.elem_stride;
                s[u] = a.sc[e];
                cc[u] = a.cl[e];
            }
        }
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const uint64_t key = topk_key64(s[u], cc[u]);
            uint64_t pend = __ballot(key > kth);
            while (pend) {
                const int src = __ffsll((unsigned long long)pend) - 1;
                pend &= pend - 1;
                const uint64_t nk = shfl64(key, src);
                if (nk <= kth) continue;                     // (uniform: the threshold rose since the ballot)
                const float ns = __shfl(s[u], src);
                const int32_t nc = __shfl(cc[u], src);
                const int pos = __popcll(__ballot(rkey > nk));   // the records that stay in front of the new one
                const uint64_t upk = shfl_up64(rkey);
                const float ups = __shfl_up(rs, 1);
                const int32_t upc = __shfl_up(rc, 1);
                if (lane == pos) { rkey = nk; rs = ns; rc = nc; }
                else if (lane > pos) { rkey = upk; rs = ups; rc = upc; }
                kth = shfl64(rkey, a.k - 1);
            }
        }
    }
    if (lane < a.k) {
        a.out_sc[(size_t)row * a.k + lane] = rs;
        a.out_cl[(size_t)row * a.k + lane] = rc;
        if (a.out_id) a.out_id[(size_t)row * a.k + lane] = rc < 0 ? -1 : a.cand_ids ? a.cand_ids[rc] : a.cand_first + rc;
    }
}

hipError_t launch_topk_cut(const float *X, int64_t ldx, int B, int Bpad, int N, int cand_col0, const int64_t *filt_ptr,
                           const int32_t *filt_col, int kq, TopkRec *part, hipStream_t st)
{
    hipLaunchKernelGGL(topk_cut_kernel, dim3((N + NT - 1) / NT, Bpad / BC), dim3(FUSED_THREADS), 0, st, X, ldx, B, Bpad, N,
                       cand_col0, filt_ptr, filt_col, kq, part);
    return hipGetLastError();
}

hipError_t launch_topk_merge(const TopkMergeArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(topk_merge_kernel, dim3((a.B + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace okge
