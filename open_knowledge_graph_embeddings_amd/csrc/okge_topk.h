// Top-k link prediction: the total order of include/okge.h ("top-k link prediction") as integer keys, and the per-tile selection
// shared by fused_tile_kernel<KB, MODE_TOPK> (okge_train.hip) and topk_cut_kernel (okge_topk.hip).
//
// Order: higher score first; equal scores (float comparison, -0.0 == +0.0) by the smaller candidate column; NaN as -inf;
// filtered columns and padding take no part.  key32 maps a score to a uint32 that compares like the score does (never 0, so 0
// marks "not eligible"); key64 appends the column, descending, so that ONE unsigned comparison decides the whole order.  The
// keys only order: the records carry the score's own bits (a NaN stays a NaN, a -0.0 a -0.0).
#pragma once
#include "okge_device.h"

namespace okge {

struct __attribute__((aligned(8))) TopkRec { float score; int32_t col; };   // padding: (-inf, -1)

__device__ __forceinline__ uint32_t topk_key32(float x)
{
    if (x != x) x = -INFINITY;
    if (x == 0.f) x = 0.f;                                   // -0.0 -> +0.0
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);      // -inf -> 0x007FFFFF: the smallest key of a real candidate
}

__device__ __forceinline__ uint64_t topk_key64(float x, int32_t col)
{
    return col < 0 ? 0ull : ((uint64_t)topk_key32(x) << 32) | (uint32_t)(0x7FFFFFFF - col);
}

// bit c set <=> global column c0 + c is in row b's filter list (ascending columns, CSR): binary search for the window's first
// column, then a walk through the window
__device__ __forceinline__ uint64_t topk_filter_mask(const int64_t *__restrict__ filt_ptr, const int32_t *__restrict__ filt_col, int b, int c0)
{
    const int64_t hi = filt_ptr[b + 1];
    int64_t l = filt_ptr[b], h = hi;
    while (l < h) {
        const int64_t mid = (l + h) >> 1;
        if (filt_col[mid] < c0) l = mid + 1; else h = mid;
    }
    uint64_t m = 0;
    for (; l < hi; ++l) {
        const int64_t c = (int64_t)filt_col[l] - c0;
        if (c >= 64) break;
        m |= 1ull << c;
    }
    return m;
}

// Selection over one staged 64 x 64 score tile Xs[row][LDX] by 512 threads: thread (row r = tid / 8, j = tid % 8) owns the
// row's candidates 8j .. 8j + 7 (bit m of elig8: candidate 8j + m is eligible).  It replaces them in LDS by their keys (0 when
// not eligible), and after the barrier counts for each how many of the row's 64 keys precede it: an element of rank r < kq is
// record r of dst; the records past the row's eligible count are padding.  Exact and stable, no atomics, no overflow case.
//   "o precedes e"  <=>  key_o > key_e, or key_o == key_e and o < e  <=>  key_o > key_e - (o < e)   (keys of eligibles are > 0)
// The caller passes the barrier that makes Xs complete before, and one more before Xs is written again.
template <int LDX>
__device__ __forceinline__ void topk_select_rows(float *Xs, int tid, uint32_t elig8, int kq, int gcol0, TopkRec *dst)
{
    const int r = tid >> 3, j = tid & 7;
    uint32_t *U = reinterpret_cast<uint32_t *>(Xs) + r * LDX;
    float xf[8];
    uint32_t u[8];
    {
        const v4f x0 = *reinterpret_cast<const v4f *>(Xs + r * LDX + 8 * j), x1 = *reinterpret_cast<const v4f *>(Xs + r * LDX + 8 * j + 4);
#pragma unroll
        for (int m = 0; m < 4; ++m) { xf[m] = x0[m]; xf[4 + m] = x1[m]; }
#pragma unroll
        for (int m = 0; m < 8; ++m) u[m] = (elig8 >> m) & 1u ? topk_key32(xf[m]) : 0u;
        *reinterpret_cast<uint4 *>(U + 8 * j) = make_uint4(u[0], u[1], u[2], u[3]);
        *reinterpret_cast<uint4 *>(U + 8 * j + 4) = make_uint4(u[4], u[5], u[6], u[7]);
    }
    __syncthreads();
    int rk[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) rk[m] = 0;
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        const uint4 o0 = *reinterpret_cast<const uint4 *>(U + 8 * g), o1 = *reinterpret_cast<const uint4 *>(U + 8 * g + 4);
        const uint32_t uo[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
        const uint32_t dl = g < j ? 1u : 0u, dle = g <= j ? 1u : 0u;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const uint32_t tl = u[m] - dl, te = u[m] - dle;   // thresholds against the group's elements at / after and before position m
#pragma unroll
            for (int mo = 0; mo < 8; ++mo) rk[m] += uo[mo] > (mo < m ? te : tl) ? 1 : 0;
        }
    }
    int n_elig = __builtin_popcount(elig8 & 0xFFu);
    n_elig += __shfl_xor(n_elig, 1);
    n_elig += __shfl_xor(n_elig, 2);
    n_elig += __shfl_xor(n_elig, 4);
    if (dst) {
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (((elig8 >> m) & 1u) && rk[m] < kq) dst[rk[m]] = TopkRec{xf[m], gcol0 + 8 * j + m};
        for (int sl = n_elig + j; sl < kq; sl += 8) dst[sl] = TopkRec{-INFINITY, -1};
    }
}

}  // namespace okge
