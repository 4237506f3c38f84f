// Bigram token encoder (BigramPoolingRelationEmbedder, openkge/model.py:801-909) for the BigramPooling{Complex,Distmult}RelationModel
// classes: id -> the row's token ids (the mapping the reference's encode_* leave out) -> embedding rows x_0 .. x_{L-1} ->
// Conv1d(d, d, kernel_size 2, no bias) over neighbouring pairs: Y[t] = K0 x_t + K1 x_{t+1}, t = 0 .. L-2 -> [BatchNorm1d(momentum
// None) over ALL n (L-1) positions of the call, padded ones included] -> + x_{t+1} -> x mask[t] = token[t+1] > 0 -> sum or max over
// t -> ['mean': / (sum mask + 1e-12)].  Forward and backward, fp32 throughout, products on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
//
// One PASS encodes the rows of up to ENC_MAX_CALLS calls of one slot.  Position p = r (L-1) + t of row r; P = rows (L-1):
//   1 bigram_prep_kernel      token id of every (r, t) behind the id guard (-> pos_tok) and its live flag (token > 0)
//   2 bigram_wt_kernel        [K0 | K1]^T (2d x d), and for the backward [K0 | K1] (d x 2d)
//   3 bigram_gemm_kernel<FWD> Y = [x_t | x_{t+1}] . [K0 | K1]^T over the P positions: one launch, the token-row gather is the
//                             A-operand load (the LSTM tile: 64 x 128, 4 waves, K chunks of 16 as fresh MFMA chains)
//   4 batch-norm statistics per call: column sums of Y and Y^2 in double over chunks of positions, added in chunk order;
//     running mean / unbiased variance as a cumulative average (factor 1 / num_batches_tracked), call after call
//   5 bigram_pool_kernel      normalise, residual, mask, pool, mean: one thread per (row, column)
// Backward of a pass:
//   1 bigram_denc_kernel      pooled-row gradient -> dE[p] (gradient of the masked enc: broadcast, or the saved max position)
//   2 batch-norm backward over all positions -> dY (without batch-norm dY = dE); parameter gradients summed in call order
//   3 bigram_gemm_kernel<DW>  dK = dY^T . [x_t | x_{t+1}] over the positions (split-K slabs, summed in split order)
//   4 bigram_gemm_kernel<DX>  [dY K0 | dY K1], then dx[r, t] = dE[t-1] + (dY K1)[t-1] + (dY K0)[t], then okge_gemm.hip's
//                             sorted-id scatter into the token table's gradient (token 0 skipped)
// No float atomics: two runs on the same inputs give bit-identical results.  No host synchronisation.
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

constexpr int BIGRAM_MAX_LEN = 64;
constexpr int GRID_CAP = 65536;          // workgroups of a grid-stride launch

enum { B_FWD = 0, B_DX = 1, B_DW = 2 };
enum { POOL_SUM = 0, POOL_MAX = 1 };
enum { NORM_NONE = 0, NORM_MEAN = 1, NORM_BATCHNORM = 2 };

struct CallsDev : EncCalls {
    int32_t chunk0[ENC_MAX_CALLS + 1], chunk;      // chunk: positions per batch-norm partial sum; chunk0: first chunk of a call
};

// workspace of a pass (carved in this order; sizes from rows R, max_len L, slot size d)
struct BigramWs {
    uint8_t *live, *amax;
    float   *wt, *wt2, *Y, *bn, *dE, *dYX, *dXc, *slab;
    double  *part;
    int32_t  splits, chunk, max_chunks;
    size_t   bytes;
};

BigramWs carve(char *p, int R, int L, int d, bool training)
{
    BigramWs w;
    std::memset(&w, 0, sizeof(w));
    const int64_t P = (int64_t)R * (L - 1), PT = (int64_t)R * L;
    Carver cv{p};
    w.chunk = (int)std::max<int64_t>(2048, ((P + 4095) / 4096 + 15) / 16 * 16);
    w.max_chunks = (int)((P + w.chunk - 1) / w.chunk);
    w.live = cv.take<uint8_t>((size_t)PT);
    w.wt = cv.take<float>((size_t)2 * d * d);
    w.Y = cv.take<float>((size_t)P * d);
    w.bn = cv.take<float>((size_t)ENC_MAX_CALLS * 4 * d);
    w.part = cv.take<double>((size_t)(w.max_chunks + ENC_MAX_CALLS) * 2 * d);
    if (training) {
        w.splits = dw_splits(P, tiles_of(d, 2 * d));
        w.amax = cv.take<uint8_t>((size_t)R * d);
        w.wt2 = cv.take<float>((size_t)2 * d * d);
        w.dE = cv.take<float>((size_t)P * d);
        w.dYX = cv.take<float>((size_t)PT * d);
        w.dXc = cv.take<float>((size_t)P * 2 * d);
        w.slab = cv.take<float>((size_t)w.splits * d * 2 * d);
    }
    w.bytes = cv.bytes;
    return w;
}

// ---- 1: tokens of the pass ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bigram_prep_kernel(const CallsDev c, const int32_t *__restrict__ tok, int n_ids, int vocab, int L,
                                                          int64_t PT, int32_t *__restrict__ pos_tok, uint8_t *__restrict__ live, int *id_err)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < PT; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / L), t = (int)(i % L);
        const int k = call_of(c, r);
        const int id = c.ids[k] ? c.ids[k][r - c.row0[k]] : c.first_id[k] + (r - c.row0[k]);
        const int64_t row = checked_row(id, n_ids, t == 0 ? id_err : nullptr);        // (counted once per row)
        const int32_t x = tok[row * L + t];
        live[i] = x > 0;
        pos_tok[i] = (int32_t)checked_row(x, vocab, id_err);
    }
}

// ---- 2: wt[k][n] = [K0 | K1][n][k] (2d x d), wt2[m][n] = [K0 | K1][m][n] (d x 2d); conv weight (d out, d in, 2) -------------
__global__ __launch_bounds__(256) void bigram_wt_kernel(const float *__restrict__ conv, int d, float *__restrict__ wt, float *__restrict__ wt2)
{
    const int64_t total = (int64_t)2 * d * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i / d), n = (int)(i % d);
        wt[i] = conv[((size_t)n * d + (k < d ? k : k - d)) * 2 + (k >= d)];
        if (wt2) {
            const int m = (int)(i / (2 * d)), c = (int)(i % (2 * d));
            wt2[i] = conv[((size_t)m * d + (c < d ? c : c - d)) * 2 + (c >= d)];
        }
    }
}

struct GemmArgs {
    const float   *W;            // token table (vocab x d)
    const float   *wt, *wt2;
    const int32_t *pos_tok;
    float         *Y;            // FWD: [P][d]
    const float   *dY;           // DX, DW: [P][d]
    float         *dXc, *slab;
    int32_t        d, L, P, k_per_split;
};

// One 64 x 128 tile of a product of the pass (enc_gemm_tile: 4 waves, K in chunks of 16 through LDS):
//   FWD  M = P, K = 2d, N = d    A(m, k) = [x_t | x_{t+1}] of position m (gathered token rows), B = wt
//   DX   M = P, K = d,  N = 2d   A = dY, B = wt2
//   DW   M = d, K = P (this split's slab), N = 2d   A(m, k) = dY[k][m], B(k, n) = [x_t | x_{t+1}] of position k
template <int MODE>
__global__ __launch_bounds__(256) void bigram_gemm_kernel(const GemmArgs a)
{
    constexpr bool TA = MODE == B_DW;
    const int d = a.d, L = a.L, Lm = a.L - 1;
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * TM;
    int M, K, N, k_lo = 0;
    if (MODE == B_FWD) { M = a.P; K = 2 * d; N = d; }
    else if (MODE == B_DX) { M = a.P; K = d; N = 2 * d; }
    else { M = d; N = 2 * d; k_lo = blockIdx.z * a.k_per_split; K = min(a.P, k_lo + a.k_per_split); }
    if (m0 >= M) return;             // (whole workgroup: before any barrier)

    // the A rows this thread loads (non-transposed: rows (tid >> 4) + 16 j, 16 consecutive k)
    const float *xr[4], *hr[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (tid >> 4) + 16 * j;
        xr[j] = hr[j] = nullptr;
        if (m < M) {
            if (MODE == B_FWD) {
                const size_t i = (size_t)(m / Lm) * L + m % Lm;
                xr[j] = a.W + (size_t)a.pos_tok[i] * d;
                hr[j] = a.W + (size_t)a.pos_tok[i + 1] * d;
            } else if (MODE == B_DX) {
                xr[j] = a.dY + (size_t)m * d;
            }
        }
    }
    v4f acc[2][4];
    enc_gemm_tile<TA>(
        k_lo, K, N,
        [&](int j, int kk) -> float {
            if (TA) {                                    // A[k][m] = dY[position k][channel m]
                const int m = m0 + (tid & 63);
                return m < M ? a.dY[(size_t)kk * d + m] : 0.f;
            }
            if (!xr[j]) return 0.f;
            if (MODE == B_FWD) return kk < d ? xr[j][kk] : hr[j][kk - d];
            return xr[j][kk];
        },
        [&](int kk, int n) -> float {
            if (MODE == B_FWD) return a.wt[(size_t)kk * N + n];
            if (MODE == B_DX) return a.wt2[(size_t)kk * N + n];
            const size_t i = (size_t)(kk / Lm) * L + kk % Lm;               // [x_t | x_{t+1}] of position kk
            return n < d ? a.W[(size_t)a.pos_tok[i] * d + n] : a.W[(size_t)a.pos_tok[i + 1] * d + (n - d)];
        },
        acc);
    enc_store_tile(acc, MODE == B_FWD ? a.Y : MODE == B_DX ? a.dXc : a.slab + (size_t)blockIdx.z * M * N, M, N);
}

// dK (d, d, 2) from the split-K slabs [d][2d], added in split order
__global__ __launch_bounds__(256) void bigram_dw_finish_kernel(const float *__restrict__ slab, int splits, int d, float *__restrict__ d_conv)
{
    const int64_t total = (int64_t)2 * d * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int s = 0; s < splits; ++s) v += slab[(size_t)s * total + i];
        const int m = (int)(i / (2 * d)), c = (int)(i % (2 * d));
        d_conv[((size_t)m * d + (c < d ? c : c - d)) * 2 + (c >= d)] = v;
    }
}

// ---- batch-norm over ALL positions of each call (BatchNorm1d(d, momentum=None, eps 1e-5) inside entity_encoder_in) ----------
// Workgroup = (16 columns, one chunk of positions, one call), 16 position lanes per column; sums in double, the 16 lanes and
// then the chunks added in a fixed order.

struct BnDev {
    const float *w, *b;
    float       *run_mean, *run_var;
    int64_t     *nbt;
    float        eps;
};

// BWD == 0: part = {sum Y, sum Y^2}; BWD == 1: part = {sum dE, sum dE xhat}
template <int BWD>
__global__ __launch_bounds__(256) void bigram_bn_part_kernel(const CallsDev c, int Lm, int d, const float *__restrict__ Y,
                                                             const float *__restrict__ dE, const float *__restrict__ saved,
                                                             double *__restrict__ part)
{
    __shared__ double red[BN_LANES * BN_COLS];
    const int call = blockIdx.z, chunk = blockIdx.y;
    if (chunk >= c.chunk0[call + 1] - c.chunk0[call]) return;           // (whole workgroup: before any barrier)
    const int col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    const int k = blockIdx.x * BN_COLS + col;
    const bool ok = k < d;
    const int64_t p0 = (int64_t)c.row0[call] * Lm + (int64_t)chunk * c.chunk;
    const int64_t p1 = min((int64_t)c.row0[call + 1] * Lm, p0 + c.chunk);
    float mean = 0.f, rstd = 0.f;
    if (BWD && ok) { mean = saved[(size_t)call * 4 * d + k]; rstd = saved[(size_t)call * 4 * d + d + k]; }
    double s = 0.0, q = 0.0;
    if (ok)
        for (int64_t p = p0 + ln; p < p1; p += BN_LANES) {
            const float y = Y[(size_t)p * d + k];
            if (BWD) {
                const float g = dE[(size_t)p * d + k];
                s += g;
                q += (double)g * ((y - mean) * rstd);
            } else {
                s += y;
                q += (double)y * y;
            }
        }
    const double ss = bn_colsum(s, red), qq = bn_colsum(q, red);
    if (ok && ln == 0) {
        double *o = part + (size_t)(c.chunk0[call] + chunk) * 2 * d;
        o[k] = ss;
        o[d + k] = qq;
    }
}

// forward: saved[call] = {mean, rstd, unbiased var}; backward: saved[call][2d ..] = {d weight, d bias} of this call
template <int BWD>
__global__ __launch_bounds__(256) void bigram_bn_finish_kernel(const CallsDev c, int Lm, int d, float eps, const double *__restrict__ part,
                                                               float *__restrict__ saved)
{
    const int call = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= d) return;
    double s = 0.0, q = 0.0;
    for (int ch = c.chunk0[call]; ch < c.chunk0[call + 1]; ++ch) {
        s += part[(size_t)ch * 2 * d + k];
        q += part[(size_t)ch * 2 * d + d + k];
    }
    float *sv = saved + (size_t)call * 4 * d;
    if (BWD) {
        sv[2 * d + k] = (float)q;
        sv[3 * d + k] = (float)s;
    } else {
        const double n = (double)(c.row0[call + 1] - c.row0[call]) * Lm;
        const double mu = s / n, var = fmax(q / n - mu * mu, 0.0);
        sv[k] = (float)mu;
        sv[d + k] = (float)(1.0 / sqrt(var + (double)eps));
        sv[2 * d + k] = (float)(var * n / (n - 1.0));
    }
}

// running statistics: momentum None = cumulative average, factor 1 / num_batches_tracked, one count per call in call order
__global__ __launch_bounds__(512) void bigram_bn_running_kernel(const BnDev bn, int n_calls, int d, const float *__restrict__ saved)
{
    const int k = threadIdx.x;
    const int64_t n0 = *bn.nbt;
    if (k < d) {
        double m = bn.run_mean[k], v = bn.run_var[k];
        for (int c = 0; c < n_calls; ++c) {
            const double f = 1.0 / (double)(n0 + c + 1);
            m = (1.0 - f) * m + f * saved[(size_t)c * 4 * d + k];
            v = (1.0 - f) * v + f * saved[(size_t)c * 4 * d + 2 * d + k];
        }
        bn.run_mean[k] = (float)m;
        bn.run_var[k] = (float)v;
    }
    __syncthreads();                                     // every thread has read the counter
    if (k == 0) *bn.nbt = n0 + n_calls;
}

// ---- 5: normalise, residual, mask, pool ------------------------------------------------------------------------------------
struct PoolArgs {
    const float   *W, *Y, *saved;
    const int32_t *pos_tok;
    const uint8_t *live;
    uint8_t       *amax;         // training, max pooling: the winning position of (row, column)
    float         *out;
    int64_t        ld;
    int32_t        d, L, R, pool, normalize, training;
};

__global__ __launch_bounds__(256) void bigram_pool_kernel(const CallsDev c, const BnDev bn, const PoolArgs a)
{
    const int d = a.d, L = a.L, Lm = a.L - 1;
    const int64_t total = (int64_t)a.R * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / d), k = (int)(i % d);
        float scale = 1.f, shift = 0.f, mean = 0.f;
        if (a.normalize == NORM_BATCHNORM) {
            float rstd;
            if (a.training) {
                const float *sv = a.saved + (size_t)call_of(c, r) * 4 * d;
                mean = sv[k];
                rstd = sv[d + k];
            } else {
                mean = bn.run_mean[k];
                rstd = 1.f / sqrtf(bn.run_var[k] + bn.eps);
            }
            scale = rstd * bn.w[k];
            shift = bn.b[k];
        }
        float acc = 0.f, cnt = 0.f;
        int am = 0;
        for (int t = 0; t < Lm; ++t) {
            const size_t j = (size_t)r * L + t + 1;
            const float m = a.live[j] ? 1.f : 0.f;
            const float y = (a.Y[((size_t)r * Lm + t) * d + k] - mean) * scale + shift;
            const float v = (y + a.W[(size_t)a.pos_tok[j] * d + k]) * m;
            if (a.pool == POOL_MAX) {
                if (t == 0 || v > acc) { acc = v; am = t; }
            } else {
                acc += v;
            }
            cnt += m;
        }
        if (a.normalize == NORM_MEAN) acc = acc / (cnt + 1e-12f);
        a.out[(size_t)r * a.ld + k] = acc;
        if (a.training && a.pool == POOL_MAX) a.amax[i] = (uint8_t)am;
    }
}

// ---- backward 1: dE[p] = gradient of the masked enc at position p -------------------------------------------------------------
__global__ __launch_bounds__(256) void bigram_denc_kernel(const float *__restrict__ d_out, int64_t ld, const uint8_t *__restrict__ live,
                                                          const uint8_t *__restrict__ amax, int R, int d, int L, int pool, int normalize,
                                                          float *__restrict__ dE)
{
    const int Lm = L - 1;
    const int64_t total = (int64_t)R * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(i / d), k = (int)(i % d);
        float g = d_out[(size_t)r * ld + k];
        if (normalize == NORM_MEAN) {
            float cnt = 0.f;
            for (int t = 1; t < L; ++t) cnt += live[(size_t)r * L + t] ? 1.f : 0.f;
            g = g / (cnt + 1e-12f);
        }
        const int am = pool == POOL_MAX ? amax[i] : -1;
        for (int t = 0; t < Lm; ++t) {
            const bool on = live[(size_t)r * L + t + 1] && (pool != POOL_MAX || t == am);
            dE[((size_t)r * Lm + t) * d + k] = on ? g : 0.f;
        }
    }
}

// dY = w rstd (dE - sum(dE)/n - xhat sum(dE xhat)/n) over all positions of the call
__global__ __launch_bounds__(256) void bigram_bn_dy_kernel(const CallsDev c, const BnDev bn, int Lm, int d, int64_t P,
                                                           const float *__restrict__ Y, const float *__restrict__ dE,
                                                           const float *__restrict__ saved, float *__restrict__ dY)
{
    const int64_t total = P * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % d), r = (int)(i / d / Lm);
        const int call = call_of(c, r);
        const float *sv = saved + (size_t)call * 4 * d;
        const float n = (float)(c.row0[call + 1] - c.row0[call]) * Lm;
        const float rstd = sv[d + k], xh = (Y[i] - sv[k]) * rstd;
        dY[i] = bn.w[k] * rstd * (dE[i] - sv[3 * d + k] / n - xh * (sv[2 * d + k] / n));
    }
}

// dx[r, t] = dE[r, t-1] (residual) + (dY K1)[r, t-1] + (dY K0)[r, t]; dXc = [dY K0 | dY K1] per position
__global__ __launch_bounds__(256) void bigram_dx_kernel(const float *__restrict__ dE, const float *__restrict__ dXc, int64_t PT, int d, int L,
                                                        float *__restrict__ dX)
{
    const int Lm = L - 1;
    const int64_t total = PT * d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(i % d);
        const int64_t j = i / d;
        const int t = (int)(j % L);
        const size_t p = (size_t)(j / L) * Lm + t;                      // position (r, t)
        float v = 0.f;
        if (t > 0) v = dE[(p - 1) * d + k] + dXc[(p - 1) * 2 * d + d + k];
        if (t < Lm) v += dXc[p * 2 * d + k];
        dX[i] = v;
    }
}

int check_slot(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, CallsDev &c, int &R)
{
    if (!s || !calls || n_calls <= 0 || n_calls > ENC_MAX_CALLS) return report_error(OKGE_ERR_INVALID, "1 to 8 bigram calls per pass");
    if (!s->W || !s->token_ids || !s->conv_weight || s->d <= 0 || s->vocab <= 0 || s->n_ids <= 0)
        return report_error(OKGE_ERR_INVALID, "bad bigram slot");
    if (s->max_len < 2 || s->max_len > BIGRAM_MAX_LEN) return report_error(OKGE_ERR_UNSUPPORTED, "bigram max_len must lie in 2..64");
    if (s->d > 512) return report_error(OKGE_ERR_UNSUPPORTED, "bigram slot sizes above 512");
    if (s->pool != POOL_SUM && s->pool != POOL_MAX) return report_error(OKGE_ERR_INVALID, "bigram pool: 0 (sum) or 1 (max)");
    if (s->normalize < NORM_NONE || s->normalize > NORM_BATCHNORM) return report_error(OKGE_ERR_INVALID, "bigram normalize: 0, 1 (mean) or 2 (batchnorm)");
    if (s->normalize == NORM_BATCHNORM && (!s->bn_weight || !s->bn_bias || !s->bn_running_mean || !s->bn_running_var || !s->bn_num_batches_tracked))
        return report_error(OKGE_ERR_INVALID, "bigram batch-norm needs weight, bias, running statistics and the counter");
    c = CallsDev{};
    return check_calls(calls, n_calls, s->n_ids, s->max_len, "bigram", c, R);
}

void set_chunks(CallsDev &c, int Lm, int chunk)
{
    c.chunk = chunk;
    for (int i = 0; i < c.n_calls; ++i) {
        const int64_t p = (int64_t)(c.row0[i + 1] - c.row0[i]) * Lm;
        c.chunk0[i + 1] = c.chunk0[i] + (int32_t)((p + chunk - 1) / chunk);
    }
}

BnDev bn_of(const okge_bigram_slot *s)
{
    BnDev b;
    b.w = s->bn_weight; b.b = s->bn_bias; b.run_mean = s->bn_running_mean; b.run_var = s->bn_running_var;
    b.nbt = s->bn_num_batches_tracked; b.eps = s->bn_eps;
    return b;
}

}  // namespace

// the C ABI's okge_bigram_* (okge_api.hip) with the device's id-error word
size_t bigram_workspace_bytes(int32_t rows, int32_t max_len, int32_t d, int32_t training)
{
    if (rows <= 0 || max_len < 2 || d <= 0 || (int64_t)rows * max_len > INT32_MAX / 4) return 0;
    return carve(nullptr, rows, max_len, d, training != 0).bytes;
}

int bigram_encode_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, int32_t training, float *out, int64_t ld,
                        int32_t *pos_tok, void *workspace, size_t workspace_bytes, int *err, void *stream)
{
    CallsDev c;
    int R = 0;
    if (int rc = check_slot(s, calls, n_calls, c, R)) return rc;
    const int d = s->d, L = s->max_len, Lm = L - 1;
    const bool bn = s->normalize == NORM_BATCHNORM;
    if (!out || !pos_tok || ld < d) return report_error(OKGE_ERR_INVALID, "bad bigram encode arguments");
    if (bn && training)
        for (int i = 0; i < n_calls; ++i)
            if ((int64_t)calls[i].n * Lm < 2)
                return report_error(OKGE_ERR_INVALID, "batch-norm in training needs more than 1 position per call");
    BigramWs w = carve(static_cast<char *>(workspace), R, L, d, training != 0);
    if (!workspace || workspace_bytes < w.bytes) return report_error(OKGE_ERR_WORKSPACE, "bigram workspace too small");
    set_chunks(c, Lm, w.chunk);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)R * Lm, PT = (int64_t)R * L;
    hipLaunchKernelGGL(bigram_prep_kernel, dim3(grid1(PT, 256, GRID_CAP)), dim3(256), 0, st, c, s->token_ids, s->n_ids, s->vocab, L, PT, pos_tok, w.live, err);
    hipLaunchKernelGGL(bigram_wt_kernel, dim3(grid1((int64_t)2 * d * d, 256, GRID_CAP)), dim3(256), 0, st, s->conv_weight, d, w.wt, training ? w.wt2 : nullptr);
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = s->W; a.wt = w.wt; a.pos_tok = pos_tok; a.Y = w.Y; a.d = d; a.L = L; a.P = (int32_t)P;
    hipLaunchKernelGGL(bigram_gemm_kernel<B_FWD>, dim3((unsigned)((P + TM - 1) / TM), (d + TN - 1) / TN), dim3(256), 0, st, a);
    BnDev b;
    std::memset(&b, 0, sizeof(b));
    if (bn) b = bn_of(s);
    if (bn && training) {
        int most = 1;
        for (int i = 0; i < n_calls; ++i) most = std::max(most, c.chunk0[i + 1] - c.chunk0[i]);
        hipLaunchKernelGGL(bigram_bn_part_kernel<0>, dim3((d + BN_COLS - 1) / BN_COLS, most, n_calls), dim3(256), 0, st, c, Lm, d,
                           (const float *)w.Y, (const float *)nullptr, (const float *)nullptr, w.part);
        hipLaunchKernelGGL(bigram_bn_finish_kernel<0>, dim3((d + 255) / 256, n_calls), dim3(256), 0, st, c, Lm, d, s->bn_eps,
                           (const double *)w.part, w.bn);
        hipLaunchKernelGGL(bigram_bn_running_kernel, dim3(1), dim3(512), 0, st, b, n_calls, d, (const float *)w.bn);
    }
    PoolArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.W = s->W; pa.Y = w.Y; pa.saved = w.bn; pa.pos_tok = pos_tok; pa.live = w.live; pa.amax = w.amax; pa.out = out; pa.ld = ld;
    pa.d = d; pa.L = L; pa.R = R; pa.pool = s->pool; pa.normalize = s->normalize; pa.training = training != 0;
    hipLaunchKernelGGL(bigram_pool_kernel, dim3(grid1((int64_t)R * d, 256, GRID_CAP)), dim3(256), 0, st, c, b, pa);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("bigram_encode: ") + hipGetErrorString(e));
    return OKGE_OK;
}

int bigram_backward_calls(const okge_bigram_slot *s, const okge_bigram_call *calls, int32_t n_calls, const float *d_out, int64_t ld,
                          const int32_t *pos_tok, const int32_t *pos_order, float *dW, float *d_conv, float *d_bn_weight,
                          float *d_bn_bias, void *workspace, size_t workspace_bytes, int *err, void *stream)
{
    CallsDev c;
    int R = 0;
    if (int rc = check_slot(s, calls, n_calls, c, R)) return rc;
    const int d = s->d, L = s->max_len, Lm = L - 1;
    const bool bn = s->normalize == NORM_BATCHNORM;
    if (!d_out || ld < d || !pos_tok || !pos_order || !dW || !d_conv || (bn && (!d_bn_weight || !d_bn_bias)))
        return report_error(OKGE_ERR_INVALID, "bad bigram backward arguments");
    BigramWs w = carve(static_cast<char *>(workspace), R, L, d, true);
    if (!workspace || workspace_bytes < w.bytes) return report_error(OKGE_ERR_WORKSPACE, "bigram workspace too small (training size)");
    set_chunks(c, Lm, w.chunk);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int64_t P = (int64_t)R * Lm, PT = (int64_t)R * L;
    hipLaunchKernelGGL(bigram_denc_kernel, dim3(grid1((int64_t)R * d, 256, GRID_CAP)), dim3(256), 0, st, d_out, ld, (const uint8_t *)w.live,
                       (const uint8_t *)w.amax, R, d, L, s->pool, s->normalize, w.dE);
    const float *dY = w.dE;
    if (bn) {
        int most = 1;
        for (int i = 0; i < n_calls; ++i) most = std::max(most, c.chunk0[i + 1] - c.chunk0[i]);
        hipLaunchKernelGGL(bigram_bn_part_kernel<1>, dim3((d + BN_COLS - 1) / BN_COLS, most, n_calls), dim3(256), 0, st, c, Lm, d,
                           (const float *)w.Y, (const float *)w.dE, (const float *)w.bn, w.part);
        hipLaunchKernelGGL(bigram_bn_finish_kernel<1>, dim3((d + 255) / 256, n_calls), dim3(256), 0, st, c, Lm, d, s->bn_eps,
                           (const double *)w.part, w.bn);
        hipLaunchKernelGGL(bigram_bn_dy_kernel, dim3(grid1(P * d, 256, GRID_CAP)), dim3(256), 0, st, c, bn_of(s), Lm, d, P, (const float *)w.Y,
                           (const float *)w.dE, (const float *)w.bn, w.dYX);
        hipLaunchKernelGGL(enc_bn_grad_kernel, dim3((d + 255) / 256), dim3(256), 0, st, n_calls, d, (const float *)w.bn, d_bn_weight,
                           d_bn_bias);
        dY = w.dYX;
    }
    GemmArgs a;
    std::memset(&a, 0, sizeof(a));
    a.W = s->W; a.wt = w.wt; a.wt2 = w.wt2; a.pos_tok = pos_tok; a.dY = dY; a.dXc = w.dXc; a.slab = w.slab;
    a.d = d; a.L = L; a.P = (int32_t)P;
    a.k_per_split = (int)(((P + w.splits - 1) / w.splits + TK - 1) / TK * TK);
    hipLaunchKernelGGL(bigram_gemm_kernel<B_DW>, dim3((d + TM - 1) / TM, (2 * d + TN - 1) / TN, w.splits), dim3(256), 0, st, a);
    hipLaunchKernelGGL(bigram_dw_finish_kernel, dim3(grid1((int64_t)2 * d * d, 256, GRID_CAP)), dim3(256), 0, st, (const float *)w.slab, w.splits, d, d_conv);
    hipLaunchKernelGGL(bigram_gemm_kernel<B_DX>, dim3((unsigned)((P + TM - 1) / TM), (2 * d + TN - 1) / TN), dim3(256), 0, st, a);
    // (dX takes the place of dY: the two products have read it)
    hipLaunchKernelGGL(bigram_dx_kernel, dim3(grid1(PT * d, 256, GRID_CAP)), dim3(256), 0, st, (const float *)w.dE, (const float *)w.dXc, PT, d, L, w.dYX);
    const hipError_t e = scatter_token_grads(w.dYX, d, pos_tok, pos_order, (int)PT, dW, s->vocab, err, st);
    if (e != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("bigram_backward: ") + hipGetErrorString(e));
    return OKGE_OK;
}

}  // namespace okge
