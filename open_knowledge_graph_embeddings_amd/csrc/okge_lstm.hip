// LSTM token encoder (LSTMRelationEmbedder, openkge/model.py:912-998) for the LSTM{Complex,Distmult}RelationModel classes
// (:1026-1034): id -> the row's (last max_len) token ids -> embedding rows -> one-layer torch.nn.LSTM (gates i, f, g, o;
// h0 = c0 = 0) -> h at last = count(tokens > 0) - 1 (-1 wraps to max_len - 1) -> [BatchNorm1d per call] -> rows.
// Forward and backward through time, fp32 throughout, products on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// One PASS encodes the rows of up to ENC_MAX_CALLS calls of one slot (the LSTM is row-independent; batch-norm stays per call):
//   1 lstm_rank_kernel    len = last + 1 of every row (ids behind the id guard), its rank among the rows of its 256-row block
//                         with the same len, and the block's count per len
//   2 lstm_scan_kernel    counting sort by len, DESCENDING (block order inside a len: stable): n_t = rows still live at step t,
//                         off_t = first packed position of step t, P = off_L = the positions the LSTM steps through
//   3 lstm_pack_kernel    sorted row s of original row r; packed position p = off_t + s of (s, t): its token id (guarded against the
//                         vocabulary) and the position of (s, t - 1)
//   4 lstm_gemm_kernel<FWD>, one launch per step t: gates = [x_t | h_{t-1}] . [W_ih | W_hh]^T for the n_t live rows (a prefix of
//                         the sorted rows: finished rows cost nothing); the token-row gather is the A-operand load.  A workgroup owns
//                         64 rows x 32 hidden units and computes all four gate blocks of them, so the gate nonlinearities and the
//                         c / h update are an epilogue in registers: it stores c_t, h_t (and, training, the activated gates)
//   5 batch-norm per call (training: this call's statistics, running statistics updated in call order; evaluation: running ones)
// Backward of a pass:
//   1 batch-norm backward per call -> dY (gradient of the LSTM output rows), parameter gradients summed in call order
//   2 lstm_gemm_kernel<BWD>, t = L-1 .. 0: dh_t = dG_{t+1} . W_hh (+ dY at the row's last step), the gate-gradient epilogue
//                         fused (dc carried per (row, unit)); dG_t overwrites the saved gates of step t
//   3 lstm_gemm_kernel<DW> [dW_ih | dW_hh | db] = dG^T . [x | h_{t-1} | 1] over the P positions (split-K slabs, summed in split order)
//   4 lstm_gemm_kernel<DX> dx = dG . W_ih, then okge_gemm.hip's sorted-id scatter into the token table's gradient (token 0 skipped)
// No float atomics: two runs on the same inputs give bit-identical results.  Grids are sized by the upper bound rows x max_len and
// read n_t / off_t / P from the device (no host synchronisation); workgroups past the live rows end at once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/okge.h"
#include "okge_token_encoder.h"

namespace okge {

namespace {

constexpr int LSTM_MAX_LEN = 64;
constexpr int RB = 256;                  // rows per block of the counting sort
constexpr int GRID_CAP = 4096;           // workgroups of a grid-stride launch

enum { G_FWD = 0, G_BWD = 1, G_DX = 2, G_DW = 3 };

using CallsDev = EncCalls;

// workspace of a pass (carved in this order; sizes from rows R, max_len L, slot size d)
struct LstmWs {
    int32_t *lens, *rank, *cnt, *base, *meta, *order, *slen, *pprev;
    float   *wt, *gates, *C, *H, *bn, *dc, *dY, *slab, *dX;
    int32_t  splits;
    size_t   bytes;
};

__host__ __device__ inline int d32_of(int d) { return (d + 31) / 32 * 32; }

LstmWs carve(char *p, int R, int L, int d, bool training)
{
    LstmWs w;
    std::memset(&w, 0, sizeof(w));
    const size_t pm = (size_t)R * L, nblk = (R + RB - 1) / RB;
    Carver cv{p};
    w.lens = cv.take<int32_t>(R);
    w.rank = cv.take<int32_t>(R);
    w.cnt = cv.take<int32_t>(nblk * L);
    w.base = cv.take<int32_t>(nblk * L);
    w.meta = cv.take<int32_t>(2 * L + 2);
    w.order = cv.take<int32_t>(R);
    w.slen = cv.take<int32_t>(R);
    w.pprev = cv.take<int32_t>(pm);
    w.wt = cv.take<float>((size_t)2 * d * 4 * d32_of(d));
    w.C = cv.take<float>(pm * d);
    w.H = cv.take<float>(pm * d);
    w.bn = cv.take<float>((size_t)ENC_MAX_CALLS * 4 * d);
    if (training) {
        w.splits = dw_splits((int64_t)pm, tiles_of(4 * d, 2 * d + 1));
        w.gates = cv.take<float>(pm * 4 * d);
        w.dc = cv.take<float>((size_t)R * d);
        w.dY = cv.take<float>((size_t)R * d);
        w.slab = cv.take<float>((size_t)w.splits * 4 * d * (2 * d + 1));
        w.dX = cv.take<float>(pm * d);
    }
    w.bytes = cv.bytes;
    return w;
}

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// ---- 1-3: counting sort of the rows by len (descending), packed positions ------------------------------------------
__global__ __launch_bounds__(RB) void lstm_rank_kernel(const CallsDev c, const int32_t *__restrict__ tok, int n_ids, int L, int R,
                                                       int32_t *__restrict__ lens, int32_t *__restrict__ rank, int32_t *__restrict__ cnt,
                                                       int *id_err)
{
    __shared__ int32_t sl[RB];
    const int r = blockIdx.x * RB + threadIdx.x;
    int len = 0;
    if (r < R) {
        const int k = call_of(c, r);
        const int id = c.ids[k] ? c.ids[k][r - c.row0[k]] : c.first_id[k] + (r - c.row0[k]);
        const int64_t row = checked_row(id, n_ids, id_err);
        int live = 0;
        for (int t = 0; t < L; ++t) live += tok[row * L + t] > 0;
        len = live > 0 ? live : L;                   // last = live - 1; -1 wraps to L - 1 (output[range(n), -1])
        lens[r] = len;
    }
    sl[threadIdx.x] = len;
    __syncthreads();
    int rk = 0;
    for (int j = 0; j < (int)threadIdx.x; ++j) rk += sl[j] == len;
    if (r < R) rank[r] = rk;
    for (int v = threadIdx.x; v < L; v += RB) {      // count of len v + 1
        int n = 0;
        for (int j = 0; j < RB; ++j) n += sl[j] == v + 1;
        cnt[(size_t)blockIdx.x * L + v] = n;
    }
}

// one workgroup: base[b][len - 1] = rows of larger len + rows of the same len in earlier blocks; meta = {n_0..n_{L-1}, off_0..off_L}
__global__ __launch_bounds__(1024) void lstm_scan_kernel(const int32_t *__restrict__ cnt, int nblk, int L, int32_t *__restrict__ base,
                                                         int32_t *__restrict__ meta)
{
    __shared__ int32_t sc[1024];
    __shared__ int32_t run;
    if (threadIdx.x == 0) run = 0;
    for (int v = L - 1; v >= 0; --v) {               // len = v + 1, descending
        for (int b0 = 0; b0 < nblk; b0 += 1024) {
            const int b = b0 + threadIdx.x;
            const int x = b < nblk ? cnt[(size_t)b * L + v] : 0;
            __syncthreads();
            sc[threadIdx.x] = x;
            __syncthreads();
            for (int s = 1; s < 1024; s <<= 1) {     // inclusive scan (Hillis-Steele)
                const int y = threadIdx.x >= (unsigned)s ? sc[threadIdx.x - s] : 0;
                __syncthreads();
                sc[threadIdx.x] += y;
                __syncthreads();
            }
            if (b < nblk) base[(size_t)b * L + v] = run + sc[threadIdx.x] - x;
            __syncthreads();
            if (threadIdx.x == 0) run += sc[1023];
        }
        __syncthreads();
        if (threadIdx.x == 0) meta[v] = run;         // n_v = rows with len > v
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int o = 0;
        for (int t = 0; t < L; ++t) {
            meta[L + t] = o;
            o += meta[t];
        }
        meta[2 * L] = o;                             // P
    }
}

__global__ __launch_bounds__(RB) void lstm_pack_kernel(const CallsDev c, const int32_t *__restrict__ tok, int n_ids, int vocab, int L, int R,
                                                       const int32_t *__restrict__ lens, const int32_t *__restrict__ rank,
                                                       const int32_t *__restrict__ base, const int32_t *__restrict__ meta,
                                                       int32_t *__restrict__ order, int32_t *__restrict__ slen, int32_t *__restrict__ pos_tok,
                                                       int32_t *__restrict__ pprev, int *id_err)
{
    const int r = blockIdx.x * RB + threadIdx.x;
    if (r >= R) return;
    const int len = lens[r];
    const int s = base[(size_t)blockIdx.x * L + len - 1] + rank[r];
    order[s] = r;
    slen[s] = len;
    const int k = call_of(c, r);
    const int id = c.ids[k] ? c.ids[k][r - c.row0[k]] : c.first_id[k] + (r - c.row0[k]);
    const int64_t row = checked_row(id, n_ids, nullptr);          // (counted once, by lstm_rank_kernel)
    for (int t = 0; t < len; ++t) {
        const int p = meta[L + t] + s;
        pos_tok[p] = (int32_t)checked_row(tok[row * L + t], vocab, id_err);
        pprev[p] = t > 0 ? meta[L + t - 1] + s : -1;
    }
}

// B operand of the forward: wt[k][n] = [W_ih | W_hh][gate row of n][k], columns in tile order (per 32 units: wave half
// wn = 16 units, gate, unit) so that a lane's four accumulators of one row block are the four gates of ONE unit
__global__ __launch_bounds__(256) void lstm_wt_kernel(const float *__restrict__ w_ih, const float *__restrict__ w_hh, int d,
                                                      float *__restrict__ wt)
{
    const int ncol = 4 * d32_of(d);
    const int64_t total = (int64_t)2 * d * ncol;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / ncol), n = (int)(i % ncol);
        const int blk = n / TN, c = n % TN, wn = c / 64, gate = (c / 16) & 3, jj = c & 15;
        const int unit = blk * 32 + 16 * wn + jj;
        float v = 0.f;
        if (unit < d) {
            const int64_t g = (int64_t)gate * d + unit;
            v = k < d ? w_ih[g * d + k] : w_hh[g * d + (k - d)];
        }
        wt[i] = v;
    }
}

struct GemmArgs {
    const float   *W;            // token table (vocab x d)
    const float   *wt;           // FWD: [2d][4 d32]
    const float   *w_ih, *w_hh, *b_ih, *b_hh;
    const int32_t *meta, *pos_tok, *pprev, *order, *slen;
    float         *gates, *C, *H;
    float         *raw;          // FWD: output rows [R][ld]
    const float   *dY;           // BWD: gradient of the output rows [R][ld_dy]
    float         *dc, *dX, *slab;
    int64_t        ld, ld_dy;
    int32_t        d, L, t, training, k_per_split;
};

// One 64 x 128 tile of a product of the pass (enc_gemm_tile: 4 waves, K in chunks of 16 through LDS):
//   FWD  gates_t = [x_t | h_{t-1}] . wt for the n_t live rows      BWD  dh_t = dG_{t+1} . W_hh
//   DX   dx = dG . W_ih over the P positions                       DW   dG^T . [x | h_{t-1} | 1] over this split's positions
template <int MODE>
__global__ __launch_bounds__(256) void lstm_gemm_kernel(const GemmArgs a)
{
    constexpr bool TA = MODE == G_DW;
    const int d = a.d, L = a.L, t = a.t;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * TN;
    // rows (M), contraction (K) and columns (N) of this product
    int M, K, N, k_lo = 0;
    int rows_a = 0;                  // BWD: rows of dG_{t+1} (A rows past it are zero)
    if (MODE == G_FWD) { M = a.meta[t]; K = t > 0 ? 2 * d : d; N = 4 * d32_of(d); }
    else if (MODE == G_BWD) { M = a.meta[t]; rows_a = t + 1 < L ? a.meta[t + 1] : 0; K = t + 1 < L ? 4 * d : 0; N = d; }
    else if (MODE == G_DX) { M = a.meta[2 * L]; K = 4 * d; N = d; }
    else { M = 4 * d; N = 2 * d + 1; k_lo = blockIdx.z * a.k_per_split; K = min(a.meta[2 * L], k_lo + a.k_per_split); }
    if (m0 >= M) return;             // (whole workgroup: before any barrier)
    const int off_t = (MODE == G_FWD || MODE == G_BWD) ? a.meta[L + t] : 0;
    const int off_p = (MODE == G_FWD && t > 0) ? a.meta[L + t - 1] : 0;              // FWD: positions of step t - 1
    const int off_n = (MODE == G_BWD && t + 1 < L) ? a.meta[L + t + 1] : 0;          // BWD: positions of step t + 1

    // the A rows this thread loads (non-transposed: rows (tid >> 4) + 16 j, 16 consecutive k)
    const float *xr[4], *hr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (tid >> 4) + 16 * j;
        xr[j] = hr[j] = nullptr;
        if (MODE == G_FWD) {
            if (m < M) {
                xr[j] = a.W + (size_t)a.pos_tok[off_t + m] * d;
                if (t > 0) hr[j] = a.H + (size_t)(off_p + m) * d;
            }
        } else if (MODE == G_BWD) {
            if (m < rows_a) xr[j] = a.gates + (size_t)(off_n + m) * 4 * d;
        } else if (MODE == G_DX) {
            if (m < M) xr[j] = a.gates + (size_t)m * 4 * d;
        }
    }
    v4f acc[2][4];
    enc_gemm_tile<TA>(
        k_lo, K, N,
        [&](int j, int kk) -> float {
            if (TA) {                                    // A[k][m] = dG[position k][gate row m]
                const int m = m0 + (tid & 63);
                return m < M ? a.gates[(size_t)kk * 4 * d + m] : 0.f;
            }
            if (MODE == G_FWD) return kk < d ? (xr[j] ? xr[j][kk] : 0.f) : (hr[j] ? hr[j][kk - d] : 0.f);
            return xr[j] ? xr[j][kk] : 0.f;
        },
        [&](int kk, int n) -> float {
            if (MODE == G_FWD) return a.wt[(size_t)kk * N + n];
            if (MODE == G_BWD) return a.w_hh[(size_t)kk * d + n];
            if (MODE == G_DX) return a.w_ih[(size_t)kk * d + n];
            if (n < d) return a.W[(size_t)a.pos_tok[kk] * d + n];            // [x | h_{t-1} | 1] of position kk
            if (n < 2 * d) { const int pp = a.pprev[kk]; return pp >= 0 ? a.H[(size_t)pp * d + (n - d)] : 0.f; }
            return 1.f;
        },
        acc);
    // result register r of lane l in block (i, j): row 32 wm + 16 i + 4 (l >> 4) + r, column 64 wn + 16 j + (l & 15)
    if (MODE == G_FWD) {
        const int unit = blockIdx.y * 32 + 16 * wn + (lane & 15);
        if (unit >= d) return;
        const float bi = a.b_ih[unit] + a.b_hh[unit], bf = a.b_ih[d + unit] + a.b_hh[d + unit];
        const float bg = a.b_ih[2 * d + unit] + a.b_hh[2 * d + unit], bo = a.b_ih[3 * d + unit] + a.b_hh[3 * d + unit];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s = m0 + 32 * wm + 16 * i + 4 * (lane >> 4) + r;
                if (s >= M) continue;
                const float ig = sigm(acc[i][0][r] + bi), fg = sigm(acc[i][1][r] + bf);
                const float gg = tanhf(acc[i][2][r] + bg), og = sigm(acc[i][3][r] + bo);
                const float cp = t > 0 ? a.C[(size_t)(off_p + s) * d + unit] : 0.f;
                const float c = fg * cp + ig * gg, h = og * tanhf(c);
                const size_t p = (size_t)(off_t + s);
                a.C[p * d + unit] = c;
                a.H[p * d + unit] = h;
                if (a.training) {
                    float *g = a.gates + p * 4 * d + unit;
                    g[0] = ig; g[d] = fg; g[2 * d] = gg; g[3 * d] = og;
                }
                if (a.slen[s] == t + 1) a.raw[(size_t)a.order[s] * a.ld + unit] = h;
            }
    } else if (MODE == G_BWD) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int unit = n0 + 64 * wn + 16 * j + (lane & 15);
            if (unit >= d) continue;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int s = m0 + 32 * wm + 16 * i + 4 * (lane >> 4) + r;
                    if (s >= M) continue;
                    float dh = acc[i][j][r];
                    if (a.slen[s] == t + 1) dh += a.dY[(size_t)a.order[s] * a.ld_dy + unit];
                    const size_t p = (size_t)(off_t + s);
                    float *g = a.gates + p * 4 * d + unit;
                    const float ig = g[0], fg = g[d], gg = g[2 * d], og = g[3 * d];
                    const float c = a.C[p * d + unit], cp = t > 0 ? a.C[(size_t)(a.meta[L + t - 1] + s) * d + unit] : 0.f;
                    const float tc = tanhf(c);
                    float *dcp = a.dc + (size_t)s * d + unit;
                    const float dct = *dcp + dh * og * (1.f - tc * tc);
                    g[0] = dct * gg * ig * (1.f - ig);
                    g[d] = dct * cp * fg * (1.f - fg);
                    g[2 * d] = dct * ig * (1.f - gg * gg);
                    g[3 * d] = dh * tc * og * (1.f - og);
                    *dcp = dct * fg;
                }
        }
    } else {
        enc_store_tile(acc, MODE == G_DX ? a.dX : a.slab + (size_t)blockIdx.z * M * N, M, N);
    }
}

// [dW_ih | dW_hh | db] from the split-K slabs, added in split order
__global__ __launch_bounds__(256) void lstm_dw_finish_kernel(const float *__restrict__ slab, int splits, int d, float *__restrict__ d_w_ih,
                                                             float *__restrict__ d_w_hh, float *__restrict__ d_b_ih, float *__restrict__ d_b_hh)
{
    const int N = 2 * d + 1;
    const int64_t total = (int64_t)4 * d * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += slab[(size_t)s * total + i];
        const int m = (int)(i / N), n = (int)(i % N);
        if (n < d) d_w_ih[(size_t)m * d + n] = v;
        else if (n < 2 * d) d_w_hh[(size_t)m * d + n - d] = v;
        else { d_b_ih[m] = v; d_b_hh[m] = v; }
    }
}

// ---- batch-norm over the output rows of each call (BatchNorm1d(momentum 0.1, eps 1e-5), model.py:611-612, :985-986) ----------
// Workgroup = (16 columns, one call), 16 row lanes per column; column sums in double, the 16 lanes added in a fixed order
// (bn_colsum).

struct BnDev {
    const float *w, *b;
    float       *run_mean, *run_var;
    float        eps, momentum;
};

// training: saved[call] = {mean, rstd, unbiased var} of the call's rows, out = normalised rows; evaluation: running statistics
__global__ __launch_bounds__(256) void lstm_bn_fwd_kernel(const CallsDev c, const BnDev bn, int training, const float *__restrict__ raw,
                                                          float *__restrict__ out, int64_t ld, int d, float *__restrict__ saved)
{
    __shared__ double red[BN_LANES * BN_COLS];
    const int call = blockIdx.y, col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    const int k = blockIdx.x * BN_COLS + col;
    const int r0 = c.row0[call], n = c.row0[call + 1] - r0;
    const bool ok = k < d;
    float mean, rstd;
    if (training) {
        double s = 0.0;
        for (int i = ln; i < n; i += BN_LANES) s += ok ? raw[(size_t)(r0 + i) * ld + k] : 0.f;
        const double mu = bn_colsum(s, red) / n;
        double q = 0.0;
        for (int i = ln; i < n; i += BN_LANES) {
            const double x = ok ? raw[(size_t)(r0 + i) * ld + k] - mu : 0.0;
            q += x * x;
        }
        const double m2 = bn_colsum(q, red);
        mean = (float)mu;
        rstd = (float)(1.0 / sqrt(m2 / n + (double)bn.eps));
        if (ok && ln == 0) {
            float *sv = saved + (size_t)call * 4 * d;
            sv[k] = mean;
            sv[d + k] = rstd;
            sv[2 * d + k] = (float)(m2 / (n - 1));
        }
    } else {
        if (!ok) return;
        mean = bn.run_mean[k];
        rstd = 1.f / sqrtf(bn.run_var[k] + bn.eps);
    }
    if (!ok) return;
    const float wk = bn.w[k], bk = bn.b[k];
    for (int i = ln; i < n; i += BN_LANES) {
        const size_t o = (size_t)(r0 + i) * ld + k;
        out[o] = (raw[o] - mean) * rstd * wk + bk;
    }
}

// running statistics, call after call in the order given (the reference's _encode calls update one module in sequence)
__global__ __launch_bounds__(256) void lstm_bn_running_kernel(const BnDev bn, int n_calls, int d, const float *__restrict__ saved)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d) return;
    float m = bn.run_mean[k], v = bn.run_var[k];
    for (int c = 0; c < n_calls; ++c) {
        const float *sv = saved + (size_t)c * 4 * d;
        m = (1.f - bn.momentum) * m + bn.momentum * sv[k];
        v = (1.f - bn.momentum) * v + bn.momentum * sv[2 * d + k];
    }
    bn.run_mean[k] = m;
    bn.run_var[k] = v;
}

// dx = w rstd (dy - sum(dy)/n - xhat sum(dy xhat)/n); this call's (dbias, dweight) -> saved[call][3d ..] / [2d ..] scratch
__global__ __launch_bounds__(256) void lstm_bn_bwd_kernel(const CallsDev c, const BnDev bn, const float *__restrict__ raw,
                                                          const float *__restrict__ dout, int64_t ld, int d, float *__restrict__ saved,
                                                          float *__restrict__ dY)
{
    __shared__ double red[BN_LANES * BN_COLS];
    const int call = blockIdx.y, col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    const int k = blockIdx.x * BN_COLS + col;
    const int r0 = c.row0[call], n = c.row0[call + 1] - r0;
    const bool ok = k < d;
    float *sv = saved + (size_t)call * 4 * d;
    const float mean = ok ? sv[k] : 0.f, rstd = ok ? sv[d + k] : 0.f;
    double s = 0.0, q = 0.0;
    for (int i = ln; i < n; i += BN_LANES) {
        if (!ok) break;
        const size_t o = (size_t)(r0 + i) * ld + k;
        const float g = dout[o], xh = (raw[o] - mean) * rstd;
        s += g;
        q += (double)g * xh;
    }
    const double sdy = bn_colsum(s, red), sdx = bn_colsum(q, red);
    if (!ok) return;
    const float fdb = (float)sdy, fdw = (float)sdx;
    if (ln == 0) { sv[2 * d + k] = fdw; sv[3 * d + k] = fdb; }
    const float wk = bn.w[k], mb = fdb / n, mw = fdw / n;
    for (int i = ln; i < n; i += BN_LANES) {
        const size_t o = (size_t)(r0 + i) * ld + k;
        const float xh = (raw[o] - mean) * rstd;
        dY[(size_t)(r0 + i) * d + k] = wk * rstd * (dout[o] - mb - xh * mw);
    }
}

int check_slot(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, CallsDev &c, int &R)
{
    if (!s || !calls || n_calls <= 0 || n_calls > ENC_MAX_CALLS) return report_error(OKGE_ERR_INVALID, "1 to 8 LSTM calls per pass");
    if (!s->W || !s->token_ids || !s->w_ih || !s->w_hh || !s->b_ih || !s->b_hh || s->d <= 0 || s->vocab <= 0 || s->n_ids <= 0)
        return report_error(OKGE_ERR_INVALID, "bad LSTM slot");
    if (s->max_len <= 0 || s->max_len > LSTM_MAX_LEN) return report_error(OKGE_ERR_UNSUPPORTED, "LSTM max_len must lie in 1..64");
    if (s->d > 512) return report_error(OKGE_ERR_UNSUPPORTED, "LSTM slot sizes above 512");
    return check_calls(calls, n_calls, s->n_ids, s->max_len, "LSTM", c, R);
}

BnDev bn_of(const okge_lstm_slot *s)
{
    BnDev b;
    b.w = s->bn_weight; b.b = s->bn_bias; b.run_mean = s->bn_running_mean; b.run_var = s->bn_running_var;
    b.eps = s->bn_eps; b.momentum = s->bn_momentum;
    return b;
}

}  // namespace

// the C ABI's okge_lstm_* (okge_api.hip) with the device's id-error word
size_t lstm_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    if (rows <= 0 || max_len <= 0 || d <= 0) return 0;
    return carve(nullptr, rows, max_len, d, training != 0).bytes;
}

int lstm_encode_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, int32_t training, float *raw, float *out,
                      int64_t ld, int32_t *pos_tok, void *workspace, size_t workspace_bytes, int *err, void *stream)
{
    CallsDev c;
    int R = 0;
    if (int rc = check_slot(s, calls, n_calls, c, R)) return rc;
    const int d = s->d, L = s->max_len;
    const bool bn = s->bn_weight != nullptr;
    if (!raw || !pos_tok || ld < d || (bn && (!out || !s->bn_bias || !s->bn_running_mean || !s->bn_running_var)))
        return report_error(OKGE_ERR_INVALID, "bad LSTM encode arguments");
    if (bn && training)
        for (int i = 0; i < n_calls; ++i)
            if (calls[i].n == 1) return report_error(OKGE_ERR_INVALID, "batch-norm in training needs more than 1 row per call");
    LstmWs w = carve(static_cast<char *>(workspace), R, L, d, training != 0);
    if (!workspace || workspace_bytes < w.bytes) return report_error(OKGE_ERR_WORKSPACE, "LSTM workspace too small");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nblk = (R + RB - 1) / RB;
    const int64_t pm = (int64_t)R * L;
    hipError_t e = hipMemsetAsync(pos_tok, 0, sizeof(int32_t) * pm, st);
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lstm: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(lstm_rank_kernel, dim3(nblk), dim3(RB), 0, st, c, s->token_ids, s->n_ids, L, R, w.lens, w.rank, w.cnt, err);
    hipLaunchKernelGGL(lstm_scan_kernel, dim3(1), dim3(1024), 0, st, w.cnt, nblk, L, w.base, w.meta);
    hipLaunchKernelGGL(lstm_pack_kernel, dim3(nblk), dim3(RB), 0, st, c, s->token_ids, s->n_ids, s->vocab, L, R, w.lens, w.rank, w.base,
                       w.meta, w.order, w.slen, pos_tok, w.pprev, err);
    hipLaunchKernelGGL(lstm_wt_kernel, dim3(grid1((int64_t)2 * d * 4 * d32_of(d), 256, GRID_CAP)), dim3(256), 0, st, s->w_ih, s->w_hh, d, w.wt);
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = s->W; a.wt = w.wt; a.w_ih = s->w_ih; a.w_hh = s->w_hh; a.b_ih = s->b_ih; a.b_hh = s->b_hh;
    a.meta = w.meta; a.pos_tok = pos_tok; a.pprev = w.pprev; a.order = w.order; a.slen = w.slen;
    a.gates = w.gates; a.C = w.C; a.H = w.H; a.raw = raw; a.ld = ld; a.d = d; a.L = L; a.training = training != 0;
    for (int t = 0; t < L; ++t) {
        a.t = t;
        hipLaunchKernelGGL(lstm_gemm_kernel<G_FWD>, dim3((R + TM - 1) / TM, d32_of(d) / 32), dim3(256), 0, st, a);
    }
    if (bn) {
        hipLaunchKernelGGL(lstm_bn_fwd_kernel, dim3((d + BN_COLS - 1) / BN_COLS, n_calls), dim3(256), 0, st, c, bn_of(s), training != 0,
                           (const float *)raw, out, ld, d, w.bn);
        if (training) hipLaunchKernelGGL(lstm_bn_running_kernel, dim3((d + 255) / 256), dim3(256), 0, st, bn_of(s), n_calls, d, (const float *)w.bn);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lstm_encode: ") + hipGetErrorString(e));
    return OKGE_OK;
}

int lstm_backward_calls(const okge_lstm_slot *s, const okge_lstm_call *calls, int32_t n_calls, const float *raw, const float *d_out,
                        int64_t ld, const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_w_ih, float *d_w_hh,
                        float *d_b_ih, float *d_b_hh, float *d_bn_weight, float *d_bn_bias, void *workspace, size_t workspace_bytes,
                        int *err, void *stream)
{
    CallsDev c;
    int R = 0;
    if (int rc = check_slot(s, calls, n_calls, c, R)) return rc;
    const int d = s->d, L = s->max_len;
    const bool bn = s->bn_weight != nullptr;
    if (!raw || !d_out || ld < d || !pos_tok || !pos_order || !dW || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh ||
        (bn && (!d_bn_weight || !d_bn_bias)))
        return report_error(OKGE_ERR_INVALID, "bad LSTM backward arguments");
    LstmWs w = carve(static_cast<char *>(workspace), R, L, d, true);
    if (!workspace || workspace_bytes < w.bytes) return report_error(OKGE_ERR_WORKSPACE, "LSTM workspace too small (training size)");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t pm = (int64_t)R * L;
    const float *dY = d_out;
    int64_t ld_dy = ld;
    if (bn) {
        hipLaunchKernelGGL(lstm_bn_bwd_kernel, dim3((d + BN_COLS - 1) / BN_COLS, n_calls), dim3(256), 0, st, c, bn_of(s), raw, d_out, ld, d,
                           w.bn, w.dY);
        hipLaunchKernelGGL(enc_bn_grad_kernel, dim3((d + 255) / 256), dim3(256), 0, st, n_calls, d, (const float *)w.bn, d_bn_weight, d_bn_bias);
        dY = w.dY;
        ld_dy = d;
    }
    hipError_t e = hipMemsetAsync(w.dc, 0, sizeof(float) * (size_t)R * d, st);
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lstm: ") + hipGetErrorString(e));
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = s->W; a.w_ih = s->w_ih; a.w_hh = s->w_hh; a.b_ih = s->b_ih; a.b_hh = s->b_hh;
    a.meta = w.meta; a.pos_tok = pos_tok; a.pprev = w.pprev; a.order = w.order; a.slen = w.slen;
    a.gates = w.gates; a.C = w.C; a.H = w.H; a.dY = dY; a.ld_dy = ld_dy; a.dc = w.dc; a.dX = w.dX; a.slab = w.slab;
    a.d = d; a.L = L; a.training = 1;
    for (int t = L - 1; t >= 0; --t) {
        a.t = t;
        hipLaunchKernelGGL(lstm_gemm_kernel<G_BWD>, dim3((R + TM - 1) / TM, (d + TN - 1) / TN), dim3(256), 0, st, a);
    }
    a.t = 0;
    a.k_per_split = (int)(((pm + w.splits - 1) / w.splits + TK - 1) / TK * TK);
    hipLaunchKernelGGL(lstm_gemm_kernel<G_DW>, dim3((4 * d + TM - 1) / TM, (2 * d + 1 + TN - 1) / TN, w.splits), dim3(256), 0, st, a);
    hipLaunchKernelGGL(lstm_dw_finish_kernel, dim3(grid1((int64_t)4 * d * (2 * d + 1), 256, GRID_CAP)), dim3(256), 0, st, (const float *)w.slab, w.splits, d,
                       d_w_ih, d_w_hh, d_b_ih, d_b_hh);
    hipLaunchKernelGGL(lstm_gemm_kernel<G_DX>, dim3((unsigned)((pm + TM - 1) / TM), (d + TN - 1) / TN), dim3(256), 0, st, a);
    e = scatter_token_grads(w.dX, d, pos_tok, pos_order, (int)pm, dW, s->vocab, err, st);
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lstm_backward: ") + hipGetErrorString(e));
    return OKGE_OK;
}

}  // namespace okge
