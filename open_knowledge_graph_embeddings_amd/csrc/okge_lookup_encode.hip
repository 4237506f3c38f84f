// Encode of the lookup embedder's variants (LookupBaseRelationEmbedder._encode, openkge/model.py:455-480, without its final
// dropout and l2_reg hook) for Lookup{Complex,Distmult}RelationModel: gather -> input dropout -> BatchNorm1d per call ->
// entity projection rows . W^T [-> ReLU] -> F.normalize.  Forward and backward, fp32 throughout, the projection's three products
// on the exact-fp32 MFMA tile of okge_token_encoder.h.
//
// One PASS encodes the rows of up to ENC_MAX_CALLS calls: row r of the pass belongs to call call_of(r); the entity calls are
// numbered first (rows 0 .. Re - 1, the rows of EV), then the relation calls (rows of RV).  With a projection, rows 0 .. Robj - 1
// take W_obj and rows Robj .. Re - 1 W_subj.  Launches of a pass (their number does not depend on the number of calls):
//   1 lookup_gather_kernel       X = table rows behind the id guard, times the input-dropout mask; W_obj^T, W_subj^T
//   2 lookup_bn_part_kernel<0>   training batch-norm: column sums of X and X^2 in double over chunks of 128 rows of one call ...
//   3 lookup_bn_finish_kernel<0> ... added in chunk order: mean and rstd per call (kept in double); running statistics call by call
//   4 lookup_gemm_kernel<FWD>    projection of the entity rows; the batch-norm scale and shift are applied in the A-operand fetch
//                                (training: the fetched rows are kept for the weight gradient)
//   5 lookup_rows_kernel<0>      one wave per row: batch-norm of the rows without projection, row norm, division
// Backward:
//   1 lookup_rows_kernel<1>      G1 = gradient behind the normalisation and the ReLU mask
//   2 lookup_gemm_kernel<DX>     G2 = G1 . W;   3 lookup_gemm_kernel<DW> dW = G1^T . Xbn in split-K slabs;   4 their sum in slab order
//   5 lookup_bn_part_kernel<1>, 6 lookup_bn_finish_kernel<1>: per call sum g, sum g xhat;  7, 8 enc_bn_grad_kernel per batch-norm
//   9 lookup_scatter_range_kernel   dx of an id range, added row for row (one thread per element)
//  10 lookup_scatter_list_kernel    dx of the id lists: the first of a run of equal (table, id) in list_order owns the run
// where dx = w rstd (g - sum g / n - xhat sum g xhat / n) times the forward's input-dropout mask.
// No float atomics: two runs on the same inputs give bit-identical results.  No host synchronisation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/okge.h"
#include "okge_host.h"
#include "okge_plan.h"
#include "okge_token_encoder.h"

namespace okge {

namespace {

static_assert(LOOKUP_MAX_CALLS == ENC_MAX_CALLS, "a pass of the lookup encode is a pass of the token encoders");
static_assert(LOOKUP_BN_CHUNK % BN_LANES == 0, "a chunk is whole rounds of the 16 row lanes");

constexpr int GRID_CAP = 65536;          // workgroups of a grid-stride launch

enum { L_FWD = 0, L_DX = 1, L_DW = 2 };

struct LkCalls : EncCalls {
    DropDev drop[ENC_MAX_CALLS];                   // input dropout of each call
    int32_t chunk0[ENC_MAX_CALLS + 1];             // first batch-norm chunk of a call
    int32_t n_ent_calls, Re, Robj, Rt;             // entity calls, entity rows, entity rows that take W_obj, rows
};

struct LkDev {
    const float *T[2];                             // [0] entity, [1] relation: table, batch-norm parameters
    const float *bnw[2], *bnb[2];
    float       *rm[2], *rv[2];
    int32_t      n_rows[2];
    const float *W[2];                             // W_obj, W_subj
    float       *X, *Xbn, *saved, *Wt, *P, *G1, *G2, *slab;      // Xbn: training, the batch-normed entity rows the projection read
    double      *norm, *part, *stat;                    // stat [call][2 d]: the call's batch mean and rstd
    float       *out[2];                           // EV, RV
    const float *dout[2];
    int64_t      ld[2], ldd[2];
    int32_t      d, bn, proj, relu, normalize, training, splits, k_per_split;
    float        eps, momentum;
    int         *err;
};

__device__ __forceinline__ int slot_of(const LkCalls &c, int call) { return call >= c.n_ent_calls; }

// batch-norm of one element of call `call` (training: the call's statistics; eval: the running statistics).  The statistics
// stay in double and xhat is rounded to fp32 once: an fp32 mean and rstd would each add a rounding to every element.
__device__ __forceinline__ float bn_apply(const LkDev &a, int slot, int call, int k, float x)
{
    if (!a.bn) return x;
    double mean, rstd;
    if (a.training) {
        const double *sd = a.stat + (size_t)call * 2 * a.d;
        mean = sd[k];
        rstd = sd[a.d + k];
    } else {
        mean = a.rm[slot][k];
        rstd = 1.0 / sqrt((double)a.rv[slot][k] + (double)a.eps);
    }
    const float xh = (float)(((double)x - mean) * rstd);
    return xh * a.bnw[slot][k] + a.bnb[slot][k];
}

// ---- 1: gather + input dropout; the transposed projection weights -------------------------------------------------------------
__global__ __launch_bounds__(256) void lookup_gather_kernel(const LkCalls c, const LkDev a)
{
    const int d = a.d;
    const int64_t rows_total = (int64_t)c.Rt * d, total = rows_total + (a.proj ? (int64_t)2 * d * d : 0);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        if (i >= rows_total) {                               // Wt[p][k][n] = W[p][n][k]
            const int64_t j = i - rows_total;
            const int p = (int)(j / ((int64_t)d * d)), k = (int)(j / d % d), n = (int)(j % d);
            a.Wt[j] = a.W[p][(size_t)n * d + k];
            continue;
        }
        const int r = (int)(i / d), k = (int)(i % d);
        const int call = call_of(c, r), pos = r - c.row0[call], slot = slot_of(c, call);
        const int id = c.ids[call] ? c.ids[call][pos] : c.first_id[call] + pos;
        const int64_t row = checked_row(id, a.n_rows[slot], k == 0 ? a.err : nullptr);       // (counted once per row)
        a.X[i] = a.T[slot][row * d + k] * drop_mult1(c.drop[call], (uint32_t)pos, k, d);
    }
}

// the gradient that reaches the batch-norm output of row r: behind the projection for the projected rows
__device__ __forceinline__ float grad_in(const LkCalls &c, const LkDev &a, int r, int k)
{
    return (a.proj && r < c.Re) ? a.G2[(size_t)r * a.d + k] : a.G1[(size_t)r * a.d + k];
}

// ---- 2, 3: batch-norm statistics ---------------------------------------------------------------------------------------------------
// Workgroup = (16 columns, one chunk of rows, one call), 16 row lanes per column; sums in double, the 16 lanes and then the
// chunks added in a fixed order.  BWD == 0: part = {sum x, sum x^2}; BWD == 1: part = {sum g, sum g xhat}
template <int BWD>
__global__ __launch_bounds__(256) void lookup_bn_part_kernel(const LkCalls c, const LkDev a)
{
    __shared__ double red[BN_LANES * BN_COLS];
    const int call = blockIdx.z, chunk = blockIdx.y, d = a.d;
    if (chunk >= c.chunk0[call + 1] - c.chunk0[call]) return;           // (whole workgroup: before any barrier)
    const int col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    const int k = blockIdx.x * BN_COLS + col;
    const bool ok = k < d;
    const int r0 = c.row0[call] + chunk * LOOKUP_BN_CHUNK, r1 = min(c.row0[call + 1], r0 + LOOKUP_BN_CHUNK);
    double mean = 0.0, rstd = 0.0;
    if (BWD && ok) { mean = a.stat[(size_t)call * 2 * d + k]; rstd = a.stat[(size_t)call * 2 * d + d + k]; }
    double s = 0.0, q = 0.0;
    if (ok)
        for (int r = r0 + ln; r < r1; r += BN_LANES) {
            const float x = a.X[(size_t)r * d + k];
            if (BWD) {
                const float g = grad_in(c, a, r, k);
                s += g;
                q += (double)g * (((double)x - mean) * rstd);
            } else {
                s += x;
                q += (double)x * x;
            }
        }
    const double ss = bn_colsum(s, red), qq = bn_colsum(q, red);
    if (ok && ln == 0) {
        double *o = a.part + (size_t)(c.chunk0[call] + chunk) * 2 * d;
        o[k] = ss;
        o[d + k] = qq;
    }
}

// Workgroup = 16 columns x 16 lanes, call after call: lane l adds the chunks l, l + 16, ... of the call, then the 16 lanes are added
// in lane order (a fixed order; one thread walking all chunks was a chain of dependent loads: 36 us at the S-FB shape).
// Forward: stat[call] = {mean, rstd} and the running statistics of the call's batch-norm, moved once per call in call order with
// the unbiased variance; backward: saved[call][2d ..] = {d weight, d bias} of this call (the layout enc_bn_grad_kernel reads)
template <int BWD>
__global__ __launch_bounds__(256) void lookup_bn_finish_kernel(const LkCalls c, const LkDev a)
{
    __shared__ double red[BN_LANES * BN_COLS];
    const int d = a.d, col = threadIdx.x % BN_COLS, ln = threadIdx.x / BN_COLS;
    const int k = blockIdx.x * BN_COLS + col;
    const bool ok = k < d, writer = ok && ln == 0;
    float run_m[2] = {0.f, 0.f}, run_v[2] = {0.f, 0.f};
    if (!BWD && writer)
        for (int s = 0; s < 2; ++s) { run_m[s] = a.rm[s][k]; run_v[s] = a.rv[s][k]; }
    for (int call = 0; call < c.n_calls; ++call) {             // (the same trip for every thread: bn_colsum holds barriers)
        const int n_rows = c.row0[call + 1] - c.row0[call];
        float *sv = a.saved + (size_t)call * 4 * d;
        if (n_rows <= 0) {                                   // an empty call adds nothing to the parameter gradients
            if (BWD && writer) sv[2 * d + k] = sv[3 * d + k] = 0.f;
            continue;
        }
        double s = 0.0, q = 0.0;
        if (ok)
            for (int ch = c.chunk0[call] + ln; ch < c.chunk0[call + 1]; ch += BN_LANES) {
                s += a.part[(size_t)ch * 2 * d + k];
                q += a.part[(size_t)ch * 2 * d + d + k];
            }
        s = bn_colsum(s, red);
        q = bn_colsum(q, red);
        if (!writer) continue;
        if (BWD) {
            sv[2 * d + k] = (float)q;
            sv[3 * d + k] = (float)s;
        } else {
            const double n = (double)n_rows;
            const double mu = s / n, var = fmax(q / n - mu * mu, 0.0);
            const float mean = (float)mu, uvar = (float)(var * n / (n - 1.0));
            a.stat[(size_t)call * 2 * d + k] = mu;
            a.stat[(size_t)call * 2 * d + d + k] = 1.0 / sqrt(var + (double)a.eps);
            const int slot = slot_of(c, call);
            run_m[slot] += a.momentum * (mean - run_m[slot]);
            run_v[slot] += a.momentum * (uvar - run_v[slot]);
        }
    }
    if (!BWD && writer)
        for (int s = 0; s < 2; ++s) { a.rm[s][k] = run_m[s]; a.rv[s][k] = run_v[s]; }
}

// ---- 4: the projection's products on the 64 x 128 tile ----------------------------------------------------------------------------
//   FWD  M = rows of a part, K = d, N = d      A(m, k) = bn(X[m][k]), B = W^T of the part       -> ReLU -> P or EV
//   DX   M = rows of a part, K = d, N = d      A = G1, B = W of the part                         -> G2
//   DW   M = d, K = rows of a part (this split's slab), N = d    A(m, k) = G1[k][m], B(k, n) = Xbn[k][n], the rows FWD read   -> slab
// blockIdx.x (FWD, DX) walks the obj part's row tiles, then the subj part's; blockIdx.z (DW) = part * splits + split.
template <int MODE>
__global__ __launch_bounds__(256) void lookup_gemm_kernel(const LkCalls c, const LkDev a, int tiles_obj)
{
    constexpr bool TA = MODE == L_DW;
    const int d = a.d, tid = threadIdx.x;
    int part, m0, m_end, k_lo = 0, K = d;
    if (MODE == L_DW) {
        part = blockIdx.z / a.splits;
        const int lo = part ? c.Robj : 0, hi = part ? c.Re : c.Robj;
        k_lo = min(hi, lo + (int)(blockIdx.z % a.splits) * a.k_per_split);
        K = min(hi, k_lo + a.k_per_split);
        m0 = blockIdx.x * TM;
        m_end = d;
    } else {
        part = (int)blockIdx.x >= tiles_obj;
        m0 = part ? c.Robj + ((int)blockIdx.x - tiles_obj) * TM : (int)blockIdx.x * TM;
        m_end = part ? c.Re : c.Robj;
    }
    // FWD: the call of each A row this thread loads (rows (tid >> 4) + 16 j)
    int cj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int m = m0 + (tid >> 4) + 16 * j;
        cj[j] = (MODE == L_FWD && m < m_end) ? call_of(c, m) : 0;
    }
    v4f acc[2][4];
    enc_gemm_tile<TA>(
        k_lo, K, d,
        [&](int j, int kk) -> float {
            if (TA) {                                    // A[k][m] = G1[row k][channel m]
                const int m = m0 + (tid & 63);
                return m < m_end ? a.G1[(size_t)kk * d + m] : 0.f;
            }
            const int m = m0 + (tid >> 4) + 16 * j;
            if (m >= m_end) return 0.f;
            if (MODE == L_FWD) {                         // (kept for the weight gradient: every (m, kk) passes here once per column tile)
                const float v = bn_apply(a, 0, cj[j], kk, a.X[(size_t)m * d + kk]);
                if (a.training && blockIdx.y == 0) a.Xbn[(size_t)m * d + kk] = v;
                return v;
            }
            return a.G1[(size_t)m * d + kk];
        },
        [&](int kk, int n) -> float {
            if (MODE == L_FWD) return a.Wt[((size_t)part * d + kk) * d + n];
            if (MODE == L_DX) return a.W[part][(size_t)kk * d + n];
            return a.Xbn[(size_t)kk * d + n];
        },
        acc);
    if (MODE == L_DW) {
        enc_store_tile(acc, a.slab + (size_t)blockIdx.z * d * d, d, d);
        return;
    }
    // the tile's rows m0 .. of this part (enc_store_tile's register layout, rows counted from m0)
    float *dst = MODE == L_DX ? a.G2 : (a.normalize ? a.P : a.out[0]);
    const int64_t ld = (MODE == L_FWD && !a.normalize) ? a.ld[0] : d;
    const int lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, n0 = blockIdx.y * TN;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 32 * wm + 16 * i + 4 * (lane >> 4) + r, n = n0 + 64 * wn + 16 * j + (lane & 15);
                if (m < m_end && n < d) {
                    float v = acc[i][j][r];
                    if (MODE == L_FWD && a.relu) v = fmaxf(v, 0.f);
                    dst[(size_t)m * ld + n] = v;
                }
            }
}

// dW_obj, dW_subj from the split-K slabs [part][split][d][d], added in split order
__global__ __launch_bounds__(256) void lookup_dw_finish_kernel(const LkDev a, float *__restrict__ dW_obj, float *__restrict__ dW_subj)
{
    const int64_t dd = (int64_t)a.d * a.d;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * dd; i += (int64_t)gridDim.x * blockDim.x) {
        const int part = i >= dd;
        const int64_t j = i - part * dd;
        float v = 0.f;
        for (int s = 0; s < a.splits; ++s) v += a.slab[((size_t)part * a.splits + s) * dd + j];
        (part ? dW_subj : dW_obj)[j] = v;
    }
}

// ---- 5 / backward 1: one wave per row -----------------------------------------------------------------------------------------------
// BWD == 0: y = the projected row, or bn(X) -> [norm = ||y||, y / max(norm, 1e-12)] -> EV / RV (projected rows without a
//           normalisation are in place already)
// BWD == 1: G1 = (g - y (y . g)) / max(norm, 1e-12) [x (projected row > 0)], g the row's gradient, y the row in EV / RV
template <int BWD>
__global__ __launch_bounds__(256) void lookup_rows_kernel(const LkCalls c, const LkDev a)
{
    constexpr int PER_LANE = LOOKUP_MAX_D / 64;            // columns lane, lane + 64, ...: the row stays in registers
    const int d = a.d, lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= c.Rt) return;                                 // (whole waves; no barrier below)
    const int call = call_of(c, r), slot = slot_of(c, call);
    const bool projected = a.proj && slot == 0;
    const size_t vrow = (size_t)(slot ? r - c.Re : r);
    float *out = a.out[slot] + vrow * a.ld[slot];
    // the row sums and the division run in double, rounded to fp32 once per element
    if (!BWD) {
        if (projected && !a.normalize) return;
        float y[PER_LANE];
        double sq = 0.0;
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) {
            const int k = lane + 64 * i;
            y[i] = 0.f;
            if (k < d) y[i] = projected ? a.P[(size_t)r * d + k] : bn_apply(a, slot, call, k, a.X[(size_t)r * d + k]);
            sq += (double)y[i] * y[i];
        }
        double nrm = 1.0;
        if (a.normalize) {
            nrm = sqrt(wave_sum(sq));
            if (lane == 0) a.norm[r] = nrm;
            nrm = fmax(nrm, 1e-12);
        }
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) {
            const int k = lane + 64 * i;
            if (k < d) out[k] = a.normalize ? (float)((double)y[i] / nrm) : y[i];
        }
    } else {
        const float *g = a.dout[slot] + vrow * a.ldd[slot];
        double dot = 0.0, nrm = 1.0;
        if (a.normalize) {
            for (int k = lane; k < d; k += 64) dot += (double)out[k] * g[k];
            dot = wave_sum(dot);
            nrm = fmax(a.norm[r], 1e-12);
        }
        const float *p = a.normalize ? a.P + (size_t)r * d : out;       // the projected row behind the activation
        for (int k = lane; k < d; k += 64) {
            float v = a.normalize ? (float)(((double)g[k] - (double)out[k] * dot) / nrm) : g[k];
            if (projected && a.relu && !(p[k] > 0.f)) v = 0.f;
            a.G1[(size_t)r * d + k] = v;
        }
    }
}

// ---- backward 9, 10: dx and its scatter -------------------------------------------------------------------------------------------
__device__ __forceinline__ float lookup_dx(const LkCalls &c, const LkDev &a, int r, int call, int pos, int k)
{
    const int d = a.d;
    float g = grad_in(c, a, r, k);
    if (a.bn) {                                            // (in double from the fp32 sums, rounded once)
        const float *sv = a.saved + (size_t)call * 4 * d;
        const double *sd = a.stat + (size_t)call * 2 * d;
        const double n = (double)(c.row0[call + 1] - c.row0[call]);
        const double rstd = sd[d + k], xh = ((double)a.X[(size_t)r * d + k] - sd[k]) * rstd;
        g = (float)((double)a.bnw[slot_of(c, call)][k] * rstd * ((double)g - (double)sv[3 * d + k] / n - xh * ((double)sv[2 * d + k] / n)));
    }
    return g * drop_mult1(c.drop[call], (uint32_t)pos, k, d);
}

// the id ranges of the pass (at most one per table): every element of the table's gradient has one thread
__global__ __launch_bounds__(256) void lookup_scatter_range_kernel(const LkCalls c, const LkDev a, float *dE, float *dR)
{
    const int d = a.d;
    for (int call = 0; call < c.n_calls; ++call) {
        if (c.ids[call]) continue;
        const int slot = slot_of(c, call);
        float *table = slot ? dR : dE;
        const int64_t total = (int64_t)(c.row0[call + 1] - c.row0[call]) * d;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
            const int pos = (int)(i / d), k = (int)(i % d);
            const int64_t row = checked_row((int64_t)c.first_id[call] + pos, a.n_rows[slot], nullptr);   // (counted by the forward)
            if (row == 0) continue;                          // the padding row: no gradient
            table[row * d + k] += lookup_dx(c, a, c.row0[call] + pos, call, pos, k);
        }
    }
}

// One workgroup per entry of list_order (rows of the pass that an id list names, sorted by (table, id), stable); the first of
// a run of equal (table, id) owns the run and adds its rows' dx in list order.
__global__ __launch_bounds__(128) void lookup_scatter_list_kernel(const LkCalls c, const LkDev a, const int32_t *__restrict__ order, int n,
                                                                   float *dE, float *dR)
{
    const int d = a.d, j0 = blockIdx.x;
    auto row_of = [&](int j) { return min(max(order[j], 0), c.Rt - 1); };
    auto key_of = [&](int j, int &call, int &pos) -> int64_t {
        const int r = row_of(j);
        call = call_of(c, r);
        pos = r - c.row0[call];
        const int id = c.ids[call] ? c.ids[call][pos] : c.first_id[call] + pos;
        return ((int64_t)slot_of(c, call) << 32) | (uint32_t)id;
    };
    int call, pos;
    const int64_t key = key_of(j0, call, pos);
    if (j0 > 0) {
        int c1, p1;
        if (key_of(j0 - 1, c1, p1) == key) return;
    }
    const int slot = slot_of(c, call);
    const int64_t row = checked_row((int64_t)(int32_t)(uint32_t)key, a.n_rows[slot], nullptr);           // (counted by the forward)
    if (row == 0) return;
    int hi = j0 + 1;
    for (int c1, p1; hi < n && key_of(hi, c1, p1) == key;) ++hi;
    float *table = slot ? dR : dE;
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        float acc = 0.f;
        for (int j = j0; j < hi; ++j) {
            int cc, pp;
            key_of(j, cc, pp);
            acc += lookup_dx(c, a, row_of(j), cc, pp, k);
        }
        table[row * d + k] += acc;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct Pass {
    LkCalls      c;
    LkDev        a;
    LookupLayout l;
    int          most_chunks;
};

int make_pass(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, bool training, void *workspace,
              size_t workspace_bytes, int *err, Pass &p)
{
    if (!e || !calls || n_calls <= 0 || n_calls > ENC_MAX_CALLS) return report_error(OKGE_ERR_INVALID, "1 to 8 lookup calls per pass");
    if (!e->E || !e->R || e->d <= 0 || e->n_ent <= 0 || e->n_rel <= 0) return report_error(OKGE_ERR_INVALID, "bad lookup encoder");
    if (e->d > LOOKUP_MAX_D) return report_error(OKGE_ERR_UNSUPPORTED, "lookup encode: slot sizes above 512");
    if (e->normalize < 0 || e->normalize > 1 || e->activation < 0 || e->activation > 1)
        return report_error(OKGE_ERR_INVALID, "lookup encoder: normalize 0 / 1, activation 0 (none) / 1 (ReLU)");
    const bool bn = e->bn_e_weight != nullptr, proj = e->W_obj != nullptr;
    if (bn && (!e->bn_e_bias || !e->bn_e_running_mean || !e->bn_e_running_var || !e->bn_r_weight || !e->bn_r_bias ||
               !e->bn_r_running_mean || !e->bn_r_running_var))
        return report_error(OKGE_ERR_INVALID, "lookup batch-norm needs weight, bias and running statistics of both slots");
    if (proj && !e->W_subj) return report_error(OKGE_ERR_INVALID, "lookup projection needs W_obj and W_subj");
    LkCalls &c = p.c;
    std::memset(&c, 0, sizeof(c));
    // entity calls first, then relation calls, each in the order given
    int order[ENC_MAX_CALLS], n = 0;
    for (int slot = 0; slot < 2; ++slot) {
        for (int i = 0; i < n_calls; ++i)
            if ((calls[i].relation != 0) == (slot != 0)) order[n++] = i;
        if (slot == 0) c.n_ent_calls = n;
    }
    c.n_calls = n_calls;
    int64_t rows = 0;
    bool subj_seen = false, range_seen[2] = {false, false};
    for (int j = 0; j < n_calls; ++j) {
        const okge_lookup_call &q = calls[order[j]];
        const int slot = j >= c.n_ent_calls;
        if (j == c.n_ent_calls) c.Re = (int32_t)rows;
        if (q.n < 0) return report_error(OKGE_ERR_INVALID, "negative row count");
        if (!q.ids && q.n > 0) {
            if (q.first_id < 0 || (int64_t)q.first_id + q.n > (slot ? e->n_rel : e->n_ent))
                return report_error(OKGE_ERR_INVALID, "row range outside the table");
            if (range_seen[slot]) return report_error(OKGE_ERR_INVALID, "at most one id range per table and pass");
            range_seen[slot] = true;
        }
        if (bn && training && q.n == 1)
            return report_error(OKGE_ERR_INVALID, "batch-norm in training needs more than 1 row per call");
        if (!slot && q.n > 0) {
            if (q.subj) subj_seen = true;
            else if (subj_seen && proj) return report_error(OKGE_ERR_INVALID, "obj-projected calls come before subj-projected calls");
            if (!q.subj || !proj) c.Robj = (int32_t)(rows + q.n);
        }
        c.ids[j] = q.ids;
        c.first_id[j] = q.first_id;
        c.row0[j] = (int32_t)rows;
        c.drop[j] = to_dev(q.input_drop);
        if (!training) { c.drop[j].enabled = 0; c.drop[j].scale = 1.f; }
        rows += q.n;
        if (rows * e->d > INT32_MAX) return report_error(OKGE_ERR_UNSUPPORTED, "lookup pass of more than 2^31 elements");
        c.chunk0[j + 1] = c.chunk0[j] + (q.n + LOOKUP_BN_CHUNK - 1) / LOOKUP_BN_CHUNK;
    }
    c.row0[n_calls] = (int32_t)rows;
    if (c.n_ent_calls == n_calls) c.Re = (int32_t)rows;
    if (!proj) c.Robj = c.Re;
    c.Rt = (int32_t)rows;
    if (rows <= 0) return report_error(OKGE_ERR_INVALID, "lookup pass without rows");
    if (!lookup_layout(c.Re, c.Rt - c.Re, e->d, training, p.l)) return report_error(OKGE_ERR_INVALID, "bad lookup pass shape");
    if (!workspace || workspace_bytes < p.l.total) return report_error(OKGE_ERR_WORKSPACE, "lookup workspace too small (okge_lookup_workspace_bytes)");
    p.most_chunks = 1;
    for (int j = 0; j < n_calls; ++j) p.most_chunks = std::max(p.most_chunks, c.chunk0[j + 1] - c.chunk0[j]);
    LkDev &a = p.a;
    std::memset(&a, 0, sizeof(a));
    char *ws = static_cast<char *>(workspace);
    a.T[0] = e->E; a.T[1] = e->R; a.n_rows[0] = e->n_ent; a.n_rows[1] = e->n_rel;
    a.bnw[0] = e->bn_e_weight; a.bnb[0] = e->bn_e_bias; a.rm[0] = e->bn_e_running_mean; a.rv[0] = e->bn_e_running_var;
    a.bnw[1] = e->bn_r_weight; a.bnb[1] = e->bn_r_bias; a.rm[1] = e->bn_r_running_mean; a.rv[1] = e->bn_r_running_var;
    a.W[0] = e->W_obj; a.W[1] = e->W_subj;
    a.X = reinterpret_cast<float *>(ws + p.l.off_X);
    a.saved = reinterpret_cast<float *>(ws + p.l.off_saved);
    a.part = reinterpret_cast<double *>(ws + p.l.off_part);
    a.stat = reinterpret_cast<double *>(ws + p.l.off_stat);
    a.norm = reinterpret_cast<double *>(ws + p.l.off_norm);
    a.Wt = reinterpret_cast<float *>(ws + p.l.off_Wt);
    a.P = reinterpret_cast<float *>(ws + p.l.off_P);
    a.G1 = reinterpret_cast<float *>(ws + p.l.off_G1);
    a.G2 = reinterpret_cast<float *>(ws + p.l.off_G2);
    a.Xbn = reinterpret_cast<float *>(ws + p.l.off_Xbn);
    a.slab = reinterpret_cast<float *>(ws + p.l.off_slab);
    a.d = e->d; a.bn = bn; a.proj = proj; a.relu = e->activation == 1; a.normalize = e->normalize; a.training = training;
    a.eps = e->bn_eps; a.momentum = e->bn_momentum;
    a.err = err;
    return OKGE_OK;
}

int set_tables(Pass &p, const float *EV, int64_t ld_e, const float *RV, int64_t ld_r)
{
    const LkCalls &c = p.c;
    if ((c.Re > 0 && (!EV || ld_e < p.a.d)) || (c.Rt > c.Re && (!RV || ld_r < p.a.d)))
        return report_error(OKGE_ERR_INVALID, "bad lookup row blocks (EV / RV)");
    p.a.out[0] = const_cast<float *>(EV); p.a.out[1] = const_cast<float *>(RV);
    p.a.ld[0] = ld_e; p.a.ld[1] = ld_r;
    return OKGE_OK;
}

}  // namespace

// the C ABI's okge_lookup_* (okge_api_encoders.hip) with the device's id-error word
size_t lookup_workspace_bytes(int32_t ent_rows, int32_t rel_rows, int32_t d, int32_t training)
{
    LookupLayout l;
    return lookup_layout(ent_rows, rel_rows, d, training != 0, l) ? l.total : 0;
}

int lookup_encode_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, int32_t training, float *EV,
                        int64_t ld_e, float *RV, int64_t ld_r, void *workspace, size_t workspace_bytes, int *err, void *stream)
{
    Pass p;
    if (int rc = make_pass(e, calls, n_calls, training != 0, workspace, workspace_bytes, err, p)) return rc;
    if (int rc = set_tables(p, EV, ld_e, RV, ld_r)) return rc;
    const LkCalls &c = p.c;
    const LkDev &a = p.a;
    const int d = a.d;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(lookup_gather_kernel, dim3(grid1((int64_t)c.Rt * d + (a.proj ? (int64_t)2 * d * d : 0), 256, GRID_CAP)), dim3(256), 0, st, c, a);
    if (a.bn && training) {
        hipLaunchKernelGGL(lookup_bn_part_kernel<0>, dim3((d + BN_COLS - 1) / BN_COLS, p.most_chunks, n_calls), dim3(256), 0, st, c, a);
        hipLaunchKernelGGL(lookup_bn_finish_kernel<0>, dim3((d + BN_COLS - 1) / BN_COLS), dim3(256), 0, st, c, a);
    }
    if (a.proj && c.Re > 0) {
        const int tiles_obj = (c.Robj + TM - 1) / TM, tiles_subj = (c.Re - c.Robj + TM - 1) / TM;
        hipLaunchKernelGGL(lookup_gemm_kernel<L_FWD>, dim3(tiles_obj + tiles_subj, (d + TN - 1) / TN), dim3(256), 0, st, c, a, tiles_obj);
    }
    hipLaunchKernelGGL(lookup_rows_kernel<0>, dim3((c.Rt + 3) / 4), dim3(256), 0, st, c, a);
    const hipError_t er = hipGetLastError();
    if (er != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lookup_encode: ") + hipGetErrorString(er));
    return OKGE_OK;
}

int lookup_backward_calls(const okge_lookup_encoder *e, const okge_lookup_call *calls, int32_t n_calls, const float *EV, int64_t ld_e,
                          const float *RV, int64_t ld_r, const float *dEV, int64_t ld_de, const float *dRV, int64_t ld_dr,
                          const int32_t *list_order, int32_t n_list, float *dE, float *dR, float *d_bn_e_weight, float *d_bn_e_bias,
                          float *d_bn_r_weight, float *d_bn_r_bias, float *dW_obj, float *dW_subj, void *workspace,
                          size_t workspace_bytes, int *err, void *stream)
{
    Pass p;
    if (int rc = make_pass(e, calls, n_calls, true, workspace, workspace_bytes, err, p)) return rc;
    if (int rc = set_tables(p, EV, ld_e, RV, ld_r)) return rc;
    const LkCalls &c = p.c;
    LkDev &a = p.a;
    const int d = a.d;
    if ((c.Re > 0 && (!dEV || ld_de < d)) || (c.Rt > c.Re && (!dRV || ld_dr < d)) || !dE || !dR)
        return report_error(OKGE_ERR_INVALID, "bad lookup backward arguments (dEV / dRV, dE / dR)");
    if (a.bn && (!d_bn_e_weight || !d_bn_e_bias || !d_bn_r_weight || !d_bn_r_bias))
        return report_error(OKGE_ERR_INVALID, "lookup batch-norm backward needs the four parameter-gradient buffers");
    if (a.proj && (!dW_obj || !dW_subj)) return report_error(OKGE_ERR_INVALID, "lookup projection backward needs dW_obj and dW_subj");
    int n_list_rows = 0;
    for (int j = 0; j < n_calls; ++j)
        if (c.ids[j]) n_list_rows += c.row0[j + 1] - c.row0[j];
    if (n_list != n_list_rows || (n_list > 0 && !list_order))
        return report_error(OKGE_ERR_INVALID, "list_order: one entry per row of the pass that an id list names");
    a.dout[0] = dEV; a.dout[1] = dRV; a.ldd[0] = ld_de; a.ldd[1] = ld_dr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(lookup_rows_kernel<1>, dim3((c.Rt + 3) / 4), dim3(256), 0, st, c, a);
    if (a.proj) {
        const int most = std::max(c.Robj, c.Re - c.Robj);
        a.splits = std::min(LOOKUP_MAX_SPLITS, dw_splits(most, tiles_of(d, d)));
        a.k_per_split = std::max(TK, ((most + a.splits - 1) / a.splits + TK - 1) / TK * TK);
        if (c.Re > 0) {
            const int tiles_obj = (c.Robj + TM - 1) / TM, tiles_subj = (c.Re - c.Robj + TM - 1) / TM;
            hipLaunchKernelGGL(lookup_gemm_kernel<L_DX>, dim3(tiles_obj + tiles_subj, (d + TN - 1) / TN), dim3(256), 0, st, c, a, tiles_obj);
        }
        hipLaunchKernelGGL(lookup_gemm_kernel<L_DW>, dim3((d + TM - 1) / TM, (d + TN - 1) / TN, 2 * a.splits), dim3(256), 0, st, c, a, 0);
        hipLaunchKernelGGL(lookup_dw_finish_kernel, dim3(grid1((int64_t)2 * d * d, 256, GRID_CAP)), dim3(256), 0, st, a, dW_obj, dW_subj);
    }
    if (a.bn) {
        hipLaunchKernelGGL(lookup_bn_part_kernel<1>, dim3((d + BN_COLS - 1) / BN_COLS, p.most_chunks, n_calls), dim3(256), 0, st, c, a);
        hipLaunchKernelGGL(lookup_bn_finish_kernel<1>, dim3((d + BN_COLS - 1) / BN_COLS), dim3(256), 0, st, c, a);
        const int n_e = c.n_ent_calls, n_r = n_calls - c.n_ent_calls;
        hipLaunchKernelGGL(enc_bn_grad_kernel, dim3((d + 255) / 256), dim3(256), 0, st, n_e, d, (const float *)a.saved, d_bn_e_weight, d_bn_e_bias);
        hipLaunchKernelGGL(enc_bn_grad_kernel, dim3((d + 255) / 256), dim3(256), 0, st, n_r, d, (const float *)(a.saved + (size_t)n_e * 4 * d),
                           d_bn_r_weight, d_bn_r_bias);
    }
    int64_t most_range = 0;
    for (int j = 0; j < n_calls; ++j)
        if (!c.ids[j]) most_range = std::max<int64_t>(most_range, (int64_t)(c.row0[j + 1] - c.row0[j]) * d);
    if (most_range > 0)
        hipLaunchKernelGGL(lookup_scatter_range_kernel, dim3(grid1(most_range, 256, GRID_CAP)), dim3(256), 0, st, c, a, dE, dR);
    if (n_list > 0)
        hipLaunchKernelGGL(lookup_scatter_list_kernel, dim3(n_list), dim3(128), 0, st, c, a, list_order, n_list, dE, dR);
    const hipError_t er = hipGetLastError();
    if (er != hipSuccess) return report_error(OKGE_ERR_HIP, std::string("lookup_backward: ") + hipGetErrorString(er));
    return OKGE_OK;
}

}  // namespace okge
