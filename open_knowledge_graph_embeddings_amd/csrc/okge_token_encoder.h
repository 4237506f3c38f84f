// Host and device code shared by the encoders that run on the virtual-table step: the LSTM (okge_lstm.hip), the bigram
// convolution (okge_bigram.hip) and the lookup embedder's variants (okge_lookup_encode.hip: the call list, the column sum, the
// parameter-gradient sum, the split-K choice and the GEMM tile).  ONE definition of the call list of a pass, the workspace
// carving, the split-K choice, the batch-norm column sum and parameter-gradient sum, the token-gradient scatter and the 64 x 128
// exact-fp32 GEMM tile, so that a further encoder brings only what is its own: its operand fetches, its epilogues, its
// statistics.  Everything here has internal linkage (three translation units include it); nothing branches on which encoder it
// runs in.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "okge_kernels.h"

namespace okge {

namespace {

constexpr int ENC_MAX_CALLS = 8;         // calls of one pass
constexpr int TM = 64, TN = 128, TK = 16;
constexpr int LDA = TK + 4;              // A tile [64 m][16 k]
constexpr int LDB = TN + 16;             // [16 k][128 n] tiles: rows 16 banks apart, 4 rows x 16 columns hit 64 banks
constexpr int LDAT = TM + 16;            // A tile of the transposed product [16 k][64 m]
constexpr int BN_COLS = 16, BN_LANES = 16;   // batch-norm workgroup: 16 columns x 16 row lanes

// ---- the calls of a pass: rows row0[k] .. row0[k + 1] - 1 are call k's, named by an id list or a range ---------------------
struct EncCalls {
    const int32_t *ids[ENC_MAX_CALLS];
    int32_t        first_id[ENC_MAX_CALLS], row0[ENC_MAX_CALLS + 1];
    int32_t        n_calls;
};

__device__ __forceinline__ int call_of(const EncCalls &c, int r)
{
    int k = 0;
    while (k + 1 < c.n_calls && r >= c.row0[k + 1]) ++k;
    return k;
}

// Call: okge_lstm_call / okge_bigram_call (one layout); what: "LSTM" / "bigram" for the message; -> c, R = rows of the pass
template <class Call>
int check_calls(const Call *calls, int32_t n_calls, int32_t n_ids, int32_t max_len, const char *what, EncCalls &c, int &R)
{
    c = EncCalls{};
    c.n_calls = n_calls;
    int64_t rows = 0;
    for (int i = 0; i < n_calls; ++i) {
        if (calls[i].n < 0) return report_error(OKGE_ERR_INVALID, "negative row count");
        if (!calls[i].ids && (calls[i].first_id < 0 || (int64_t)calls[i].first_id + calls[i].n > n_ids))
            return report_error(OKGE_ERR_INVALID, "row range outside the token-id matrix");
        c.ids[i] = calls[i].ids;
        c.first_id[i] = calls[i].first_id;
        c.row0[i] = (int32_t)rows;
        rows += calls[i].n;
    }
    c.row0[n_calls] = (int32_t)rows;
    if (rows <= 0 || rows * max_len > INT32_MAX / 4)
        return report_error(OKGE_ERR_INVALID, std::string(what) + " pass of 1 .. 2^29 / max_len rows");
    R = (int)rows;
    return OKGE_OK;
}

// ---- small host helpers ---------------------------------------------------------------------------------------------------
// A workspace cut into 256-byte aligned pieces in the order asked for; base == nullptr: only the size (bytes) is wanted
struct Carver {
    char  *base;
    size_t bytes = 0;
    template <class T> T *take(size_t count)
    {
        char *q = base ? base + bytes : nullptr;
        bytes += (sizeof(T) * count + 255) / 256 * 256;
        return reinterpret_cast<T *>(q);
    }
};

inline int64_t tiles_of(int M, int N) { return (int64_t)((M + TM - 1) / TM) * ((N + TN - 1) / TN); }

// split-K slabs of a weight-gradient product: about 1024 workgroups in all, at most 16 slabs, at least 256 terms per slab
inline int dw_splits(int64_t contraction, int64_t tiles)
{
    const int64_t s = std::max<int64_t>(1, std::min<int64_t>(16, 1024 / std::max<int64_t>(tiles, 1)));
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, contraction / 256));
}

inline unsigned grid1(int64_t n, int per, int cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, (n + per - 1) / per)); }

// dW (vocab x d) += the position gradients dX [n][d], summed per token in the order of pos_order (no dropout; token 0 skipped)
inline hipError_t scatter_token_grads(const float *dX, int d, const int32_t *pos_tok, const int32_t *pos_order, int n, float *dW,
                                      int vocab, int *err, hipStream_t st)
{
    DropDev none;
    std::memset(&none, 0, sizeof(none));
    none.scale = 1.f;
    const hipError_t e = launch_scatter_rows(dX, d, pos_tok, pos_order, 0, n, d, none, dW, vocab, err, st);
    return e == hipSuccess ? hipGetLastError() : e;
}

// ---- batch-norm pieces ----------------------------------------------------------------------------------------------------
// sum over the 16 lanes of a column, added in lane order; red: BN_LANES * BN_COLS doubles of LDS
__device__ __forceinline__ double bn_colsum(double v, double *red)
{
    const int col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    __syncthreads();
    red[ln * BN_COLS + col] = v;
    __syncthreads();
    double s = 0.0;
    for (int j = 0; j < BN_LANES; ++j) s += red[j * BN_COLS + col];
    return s;
}

// (d weight, d bias) = the calls' saved[call][2d ..] / [3d ..], added in call order
__global__ __launch_bounds__(256) void enc_bn_grad_kernel(int n_calls, int d, const float *__restrict__ saved, float *__restrict__ d_w,
                                                          float *__restrict__ d_b)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d) return;
    float gw = 0.f, gb = 0.f;
    for (int c = 0; c < n_calls; ++c) {
        gw += saved[(size_t)c * 4 * d + 2 * d + k];
        gb += saved[(size_t)c * 4 * d + 3 * d + k];
    }
    d_w[k] = gw;
    d_b[k] = gb;
}

// ---- C[m][n] = sum_k A(m, k) B(k, n) on a 64 x 128 tile (blockIdx.x, blockIdx.y) of a 256-thread workgroup -----------------
// 4 waves, wave (wm, wn) = 32 rows x 64 columns = 2 x 4 MFMA blocks; K = [k_lo, K) in chunks of 16 through LDS (the next
// chunk's global loads in registers while the current one is multiplied).  The caller says how an element is fetched:
//   a_elem(j, k)   TA = false: A(m0 + (tid >> 4) + 16 j, k), the thread's load slot j;  TA = true (A is stored [k][m]): A(m0 + (tid & 63), k)
//   b_elem(k, n)   B(k, n); asked only for k < K, n < N
// (a_elem is asked only for k < K; rows past M are the caller's to zero.)  Blocked summation: the chunk's 16 products are a
// fresh MFMA chain, then one add into the running sum (one k-ordered chain over all of K -- up to 10^5 terms in the weight
// gradients -- lost a factor 3-4 in accuracy to a blocked sgemm).
// Result register r of lane l in acc[i][j]: row 32 wm + 16 i + 4 (l >> 4) + r, column 64 wn + 16 j + (l & 15) of the tile.
template <bool TA, class FA, class FB>
__device__ __forceinline__ void enc_gemm_tile(int k_lo, int K, int N, FA a_elem, FB b_elem, v4f (&acc)[2][4])
{
    __shared__ float As[TA ? TK * LDAT : TM * LDA];
    __shared__ float Bs[TK * LDB];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int n0 = blockIdx.y * TN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[8];
    auto load = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k0 + (TA ? (tid >> 6) + 4 * j : (tid & 15));
            ra[j] = kk < K ? a_elem(j, kk) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kk = k0 + (tid >> 7) + 2 * j, n = n0 + (tid & 127);
            rb[j] = (kk < K && n < N) ? b_elem(kk, n) : 0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (TA) As[((tid >> 6) + 4 * j) * LDAT + (tid & 63)] = ra[j];
            else As[((tid >> 4) + 16 * j) * LDA + (tid & 15)] = ra[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[((tid >> 7) + 2 * j) * LDB + (tid & 127)] = rb[j];
    };
    if (k_lo < K) load(k_lo);
    for (int k0 = k_lo; k0 < K; k0 += TK) {
        __syncthreads();                                 // the previous chunk has been multiplied
        stage();
        __syncthreads();
        if (k0 + TK < K) load(k0 + TK);
        v4f part[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) part[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k4 = 0; k4 < TK; k4 += 4) {
            float av[2], bv[4];
            const int kk = k4 + (lane >> 4);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = 32 * wm + 16 * i + (lane & 15);
                av[i] = TA ? As[kk * LDAT + m] : As[m * LDA + kk];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = Bs[kk * LDB + 64 * wn + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) part[i][j] = mfma16(av[i], bv[j], part[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += part[i][j];
    }
}

// the tile's part of out[M][N]
__device__ __forceinline__ void enc_store_tile(const v4f (&acc)[2][4], float *out, int M, int N)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wm = w >> 1, wn = w & 1;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 32 * wm + 16 * i + 4 * (lane >> 4) + r, n = n0 + 64 * wn + 16 * j + (lane & 15);
                if (m < M && n < N) out[(size_t)m * N + n] = acc[i][j][r];
            }
}

}  // namespace

}  // namespace okge
